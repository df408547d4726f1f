// hattention.hip — float16 attention, out[b] = half(softmax_rows(scale * Q[b] K[b]^T) V[b]), in one launch (gfx950).
//
// Reference: the chain BatchedDot / Dot22 / Dot22Scalar -> [Elemwise * or /] -> Softmax{axis=-1} -> BatchedDot / Dot22
// (pytensor/tensor/blas/batched.py:18, blas/gemm.py:248,298, tensor/special.py:26), which attnfuse.py folds into one
// `Attention` node.  The S x T scores never reach memory: they live in the fp32 accumulators of
// v_mfma_f32_32x32x16_f16, the scale is applied there in fp32, the softmax is the online one (running maximum m,
// running sum l, O rescaled by exp(m_old - m_new)) in fp32 with exp through v_exp_f32 (log2 e folded into the scale),
// P is rounded to half only as an operand of the second product, l is summed from the fp32 values, and O / l is rounded
// to half once.  One launch, no scratch, no tickets, a fixed summation order: the bits repeat run to run.
//
// Both products are computed TRANSPOSED (fragment layout: hgemm.hip): S^T = K Q^T (keys x queries) and
// O^T = V^T P^T (dv x queries).  In the 32x32 accumulator layout a lane then holds ONE query (column l & 31) and, per
// 32-key block, the 16 keys (r&3) + 8 (r>>2) + 4 (l>>5): a row's maximum and sum are reductions over the lane's own
// registers plus one exchange between the two lane halves, the rescale factor is a per-lane scalar, and the
// exponentiated S^T registers, packed to half, ARE a B operand of the second product: registers 8g .. 8g+7 of a key
// block are the eight k values of lane half h = l>>5 in k-step g, keys 16g + 4h + {0..3} and 16g + 8 + 4h + {0..3}.
// The A operand agrees by reading V^T from LDS [dv][key] at those two key quads (two ds_read_b64).  P never goes
// through LDS.
//
// Work split: 256 threads = 4 waves own 128 queries of one batch item, each wave 32 of them outright, so m and l never
// cross a wave.  Q (the B operand of the first product) is loaded once into registers, DM/16 fragments of 8 halves.
// K / V tiles of 64 keys are staged global -> registers -> LDS once per workgroup, double-buffered (the loads of tile
// t+1 are issued before the MFMAs of tile t and stored behind them; one barrier per tile), and shared by the four waves.
//   K tile [key][d], d contiguous, pitch DM + 8 halves: (DM + 8) / 2 = 68, 36 or 20 dwords; 16 consecutive rows start
//   at 16 different multiples of 4 dwords mod 64, so a pass of a 128-bit fragment read covers the banks once.
//   V tile [dv][key], pitch 68 halves = 34 dwords: the 32 rows of a 64-bit fragment read start at 32 different even
//   dwords mod 64.  V is dv-contiguous in memory: it is transposed on the way in with the 8 x 4 register transpose of
//   hgemm's row-contiguous staging (a thread loads 8 dv of 4 consecutive keys, writes 8 ds_write_b64).
//   Two buffers of both: 2 * (64 * (DM + 8) + DM * 68) halves = 69632 bytes at DM = 128 (two workgroups per CU).
// DM in {32, 64, 128} is the smallest that holds max(D, Dv); d >= D, dv >= Dv and keys >= T are zero-filled, keys >= T
// get a score of -inf, rows >= S are computed on zeros and never stored.  16-byte loads where pointer, row stride and
// batch stride are multiples of 8 halves (whole tiles without a branch when D = DM and the tile is inside T);
// otherwise bounds-checked 2-byte loads, kept out of line as in hgemm.hip and for the same reason.
// Epilogue: a lane holds a column of O^T, so the 128 x Dv tile is transposed through the (now free) LDS and stored as
// 16-byte rows.
#include "common.h"
#include "mfma_tile_device.h"

namespace {

constexpr int BLOCK = 256;
constexpr int QB = 128;       // queries per workgroup
constexpr int KT = 64;        // keys per tile
constexpr int VLD = KT + 4;   // pitch of the V^T tile in halves
constexpr int MAX_D = 128;

using mfma::float16_t;
using mfma::half8_t;
typedef unsigned short hbits;

union Vec8 {
  uint4 q;
  uint2 d[2];
  unsigned int w[4];
  hbits h[8];
  half8_t f;
};

// g[0 .. min(n, 8) - 1] by 2-byte loads, zeros behind them (n <= 0: no load at all)
__device__ __noinline__ uint4 load8_partial(const hbits* __restrict__ g, long long n) {
  Vec8 r;
#pragma unroll
  for (int e = 0; e < 8; e++) r.h[e] = e < n ? g[e] : (hbits)0;
  return r.q;
}

// 8 halves at g: rows `in` of them inside the operand (0: none), by one 16-byte load where the alignment allows
__device__ __forceinline__ uint4 load8(const hbits* __restrict__ g, long long in, bool vec) {
  if (vec && in >= 8) return *(const uint4*)g;
  return load8_partial(g, in);
}

__device__ __forceinline__ hbits to_half_bits(float x) {
  union { _Float16 h; hbits b; } u;
  u.h = (_Float16)x;
  return u.b;
}

__device__ __forceinline__ float h2f(hbits b) {
  union { hbits b; _Float16 h; } u;
  u.b = b;
  return (float)u.h;
}

template <int DM>
__global__ __launch_bounds__(BLOCK, 2) void hattention_kernel(
    hbits* __restrict__ out, const hbits* __restrict__ Q, const hbits* __restrict__ K, const hbits* __restrict__ V,
    const hbits* __restrict__ scale, int scale_div, long long S, long long T, int D, int Dv, long long sQb, long long sQ0,
    long long sKb, long long sK0, long long sVb, long long sV0, long long qblocks, long long total, int vecQ, int vecK,
    int vecV, int vecO) {
  constexpr int KLD = DM + 8;            // pitch of the K tile (and of the output tile) in halves
  constexpr int KSIZE = KT * KLD, VSIZE = DM * VLD;
  constexpr int NKV = KT * DM / 8 / BLOCK;  // 16-byte vectors of the K tile per thread: 1, 2, 4
  constexpr int VUNITS = DM / 8 * (KT / 4); // (8 dv x 4 keys) units of the V tile: 64, 128, 256
  constexpr int ND = DM / 16;            // k-steps of the first product
  constexpr int NO = DM / 32;            // 32-row blocks of O^T
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  hbits* Ks = (hbits*)smem_raw;   // [2][KSIZE]
  hbits* Vs = Ks + 2 * KSIZE;     // [2][VSIZE]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, c = lane & 31;
  const long long pid = mfma::xcd_band((long long)blockIdx.x, total);  // the query blocks of an item share an XCD's L2
  const long long b = pid / qblocks, q0 = (pid - b * qblocks) * QB;
  const hbits* Qb = Q + b * sQb;
  const hbits* Kb = K + b * sKb;
  const hbits* Vb = V + b * sVb;

  // exp(scale * s - max) = exp2(sl2 * s - max'): one fp32 factor, read from device memory (no host read of a runtime scalar)
  constexpr float LOG2E = 1.44269504088896340736f;
  float sl2 = LOG2E;
  if (scale) {
    const float sc = h2f(*scale);
    sl2 = scale_div ? LOG2E / sc : sc * LOG2E;
  }

  // Q fragments: query q0 + 32 w + c, d = 16 kk + 8 h .. + 7
  half8_t qf[ND];
  {
    const long long q = q0 + w * 32 + c;
#pragma unroll
    for (int kk = 0; kk < ND; kk++) {
      const int d0 = kk * 16 + h * 8;
      Vec8 t;
      t.q = load8(Qb + q * sQ0 + d0, q < S ? (long long)D - d0 : 0, vecQ);
      qf[kk] = t.f;
    }
  }

  Vec8 kv[NKV], vv[4];
  const int vrg = (tid & 3) + 4 * (tid >> 6), vkq = (tid >> 2) & 15;  // V staging: this thread's group of 8 dv and key quad
  auto load_tile = [&](long long key0) {
    const bool whole = key0 + KT <= T;  // workgroup-uniform
    if (vecK && whole && D == DM) {
#pragma unroll
      for (int p = 0; p < NKV; p++) {
        const int id = tid + p * BLOCK;
        kv[p].q = *(const uint4*)(Kb + (key0 + id / (DM / 8)) * sK0 + (id % (DM / 8)) * 8);
      }
    } else {
#pragma unroll
      for (int p = 0; p < NKV; p++) {
        const int id = tid + p * BLOCK, d0 = (id % (DM / 8)) * 8;
        const long long key = key0 + id / (DM / 8);
        kv[p].q = load8(Kb + key * sK0 + d0, key < T ? (long long)D - d0 : 0, vecK);
      }
    }
    if (tid < VUNITS) {
      if (vecV && whole && Dv == DM) {
#pragma unroll
        for (int j = 0; j < 4; j++) vv[j].q = *(const uint4*)(Vb + (key0 + vkq * 4 + j) * sV0 + vrg * 8);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const long long key = key0 + vkq * 4 + j;
          vv[j].q = load8(Vb + key * sV0 + vrg * 8, key < T ? (long long)Dv - vrg * 8 : 0, vecV);
        }
      }
    }
  };
  auto store_tile = [&](int buf) {
    hbits* ks = Ks + buf * KSIZE;
#pragma unroll
    for (int p = 0; p < NKV; p++) {
      const int id = tid + p * BLOCK;
      *(uint4*)(ks + (id / (DM / 8)) * KLD + (id % (DM / 8)) * 8) = kv[p].q;
    }
    if (tid < VUNITS) {
      hbits* d = Vs + buf * VSIZE + vrg * 8 * VLD + vkq * 4;
#pragma unroll
      for (int r = 0; r < 8; r++) {  // dv row r of the 8 x 4 block: half r of each of the four key vectors
        const int sh = (r & 1) * 16;
        uint2 o;
        o.x = ((vv[0].w[r >> 1] >> sh) & 0xffffu) | (((vv[1].w[r >> 1] >> sh) & 0xffffu) << 16);
        o.y = ((vv[2].w[r >> 1] >> sh) & 0xffffu) | (((vv[3].w[r >> 1] >> sh) & 0xffffu) << 16);
        *(uint2*)(d + r * VLD) = o;
      }
    }
  };

  float16_t oacc[NO];
  mfma::zero_acc(oacc);
  float m = -__builtin_huge_valf(), l = 0.f;  // this lane's query: running maximum (both lane halves agree), sum of its own keys

  load_tile(0);
  store_tile(0);
  __syncthreads();
  const long long nt = (T + KT - 1) / KT;
  int buf = 0;
  for (long long t = 0; t < nt; t++) {
    const long long key0 = t * KT;
    const bool more = t + 1 < nt;
    if (more) load_tile(key0 + KT);
    const hbits* ks = Ks + buf * KSIZE;
    const hbits* vs = Vs + buf * VSIZE;
    // S^T (64 keys x 32 queries of this wave) = K Q^T
    float16_t sacc[2];
    mfma::zero_acc(sacc);
#pragma unroll
    for (int kk = 0; kk < ND; kk++) {
      if (kk * 16 < D || kk == 0) {  // (uniform: k-steps of zero fill only are skipped)
#pragma unroll
        for (int kb = 0; kb < 2; kb++) {
          Vec8 a;
          a.q = *(const uint4*)(ks + (kb * 32 + c) * KLD + kk * 16 + h * 8);
          sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.f, qf[kk], sacc[kb], 0, 0, 0);
        }
      }
    }
    // scale, mask the keys behind T, this tile's maximum
    const bool tail = key0 + KT > T;
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float s = sacc[kb][r] * sl2;
        if (tail && mfma::acc32_row(key0 + kb * 32, r, lane) >= T) s = -__builtin_huge_valf();
        sacc[kb][r] = s;
        mx = fmaxf(mx, s);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);  // finite from the first tile on: every tile holds a key < T
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float p = __builtin_amdgcn_exp2f(sacc[kb][r] - mn);
        sacc[kb][r] = p;
        rs += p;
      }
    l = l * alpha + rs;
#pragma unroll
    for (int i = 0; i < NO; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) oacc[i][r] *= alpha;
    // O^T += V^T P^T: the P registers of a key block, eight at a time, are the B fragment as they are
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int g = 0; g < 2; g++) {
        half8_t pf;
#pragma unroll
        for (int e = 0; e < 8; e++) pf[e] = (_Float16)sacc[kb][g * 8 + e];
#pragma unroll
        for (int i = 0; i < NO; i++) {
          if (i * 32 < Dv || i == 0) {
            const hbits* a0 = vs + (i * 32 + c) * VLD + kb * 32 + g * 16 + h * 4;
            Vec8 a;
            a.d[0] = *(const uint2*)a0;
            a.d[1] = *(const uint2*)(a0 + 8);
            oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.f, pf, oacc[i], 0, 0, 0);
          }
        }
      }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: O / l, one rounding, transposed through LDS (every wave is behind the loop's last barrier)
  const float inv = 1.f / (l + __shfl_xor(l, 32));
  hbits* Os = (hbits*)smem_raw;  // [QB][KLD]
#pragma unroll
  for (int i = 0; i < NO; i++)
#pragma unroll
    for (int rq = 0; rq < 4; rq++) {  // registers 4 rq .. 4 rq + 3: dv = 32 i + 8 rq + 4 h + {0..3}
      uint2 o;
      o.x = to_half_bits(oacc[i][rq * 4] * inv) | ((unsigned)to_half_bits(oacc[i][rq * 4 + 1] * inv) << 16);
      o.y = to_half_bits(oacc[i][rq * 4 + 2] * inv) | ((unsigned)to_half_bits(oacc[i][rq * 4 + 3] * inv) << 16);
      *(uint2*)(Os + (w * 32 + c) * KLD + i * 32 + rq * 8 + h * 4) = o;
    }
  __syncthreads();
  hbits* ob = out + (b * S + q0) * Dv;
#pragma unroll
  for (int p = 0; p < QB * DM / 8 / BLOCK; p++) {
    const int id = tid + p * BLOCK, row = id / (DM / 8), d0 = (id % (DM / 8)) * 8;
    if (q0 + row >= S || d0 >= Dv) continue;
    Vec8 o;
    o.q = *(const uint4*)(Os + row * KLD + d0);
    hbits* g = ob + (long long)row * Dv + d0;
    if (vecO) {  // Dv is a multiple of 8: the vector is inside the row
      *(uint4*)g = o.q;
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (d0 + e < Dv) g[e] = o.h[e];
    }
  }
}

template <int DM>
int hattention_launch(long long batch, long long S, long long T, int D, int Dv, const hbits* Q, long long sQb, long long sQ0,
                      const hbits* K, long long sKb, long long sK0, const hbits* V, long long sVb, long long sV0,
                      const hbits* scale, int scale_div, hbits* out) {
  const size_t shmem = (size_t)2 * (KT * (DM + 8) + DM * VLD) * sizeof(hbits);  // (the output tile, QB x (DM + 8), is smaller)
  if (int r = pthip::lds_opt_in((const void*)hattention_kernel<DM>, shmem)) return r;
  const long long qblocks = (S + QB - 1) / QB, total = qblocks * batch;
  auto vec = [](const void* p, long long s0, long long sb) { return (int)(((uintptr_t)p) % 16 == 0 && s0 % 8 == 0 && sb % 8 == 0); };
  const int vecQ = vec(Q, sQ0, sQb), vecK = vec(K, sK0, sKb), vecV = vec(V, sV0, sVb), vecO = vec(out, Dv, 0);
  PTHIP_KLAUNCH((hattention_kernel<DM>), dim3((unsigned)total), dim3(BLOCK), shmem, pthip::ctx().stream, out, Q, K, V, scale, scale_div,
                S, T, D, Dv, sQb, sQ0, sKb, sK0, sVb, sV0, qblocks, total, vecQ, vecK, vecV, vecO);
  return pthip::post_launch("hattention");
}

}  // namespace

extern "C" int64_t pthip_hattention_max_d(void) { return MAX_D; }

extern "C" int pthip_hattention(int64_t batch, int64_t S, int64_t T, int64_t D, int64_t Dv, const void* Q, int64_t sQb,
                                int64_t sQ0, const void* K, int64_t sKb, int64_t sK0, const void* V, int64_t sVb,
                                int64_t sV0, const void* scale, int scale_div, void* out) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || S <= 0 || Dv <= 0) return 0;
  if (T <= 0) return pthip::set_error("pthip_hattention: no keys (T = %lld): the softmax of an empty row is undefined", (long long)T);
  if (D < 0 || D > MAX_D || Dv > MAX_D)
    return pthip::set_error("pthip_hattention: D = %lld, Dv = %lld beyond %d", (long long)D, (long long)Dv, MAX_D);
  if (sQb < 0 || sQ0 < 0 || sKb < 0 || sK0 < 0 || sVb < 0 || sV0 < 0) return pthip::set_error("pthip_hattention: negative strides are not supported");
  if (((S + QB - 1) / QB) * batch > 0x7fffffffLL) return pthip::set_error("pthip_hattention: too many query blocks");
  const hbits* q = (const hbits*)Q;
  const hbits* k = (const hbits*)K;
  const hbits* v = (const hbits*)V;
  const hbits* sc = (const hbits*)scale;
  hbits* o = (hbits*)out;
  const int dm = (int)(D > Dv ? D : Dv);
#define GO(DM) return hattention_launch<DM>(batch, S, T, (int)D, (int)Dv, q, sQb, sQ0, k, sKb, sK0, v, sVb, sV0, sc, scale_div, o)
  if (dm <= 32) GO(32);
  if (dm <= 64) GO(64);
  GO(128);
#undef GO
}
