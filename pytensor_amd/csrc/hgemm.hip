// hgemm.hip — float16 Dot / matmul / BatchedDot on the matrix cores (gfx950), and the float16 matrix-vector product.
//
// Reference: Dot.perform on float16 operands is np.dot (pytensor/tensor/math.py:3041), which accumulates every output
// element in a float and rounds it to half once.  Here: products of two halves are exact in fp32, the sum over k is
// carried in the fp32 accumulators of v_mfma_f32_32x32x16_f16, and the one conversion to half (round to nearest even,
// overflow to inf, gradual underflow) happens in registers in the epilogue.
//
// MFMA 32x32x16 f16: lane l passes 8 halves of A (row l&31, k = 8(l>>5) .. +7) and 8 of B (the same k, column l&31);
// the accumulator layout is the one of the fp32 32x32x2 form (mfma_tile_device.h: acc32_row, acc32_col).
// The sum over k is order-free, so all the kernel has to guarantee is that the A and the B fragment of a lane hold the
// SAME eight k values: both are read from LDS at k = 16 kk + 8 (l>>5).
//
// Tiling: 256 threads = 4 waves; block tile 128 x 128 (wave tile 64 x 64 = 2 x 2 MFMA blocks, 64 accumulator
// registers), or for M <= 64 the skinny tile 64 x 128 (wave tile 64 x 32: no MFMA on padding rows beyond 64).  A
// K stage is HK = 64 deep: 4 MFMA k-steps = 16 (8) MFMAs per wave between two barriers.
//
// LDS: both operand tiles are stored [row][k], k contiguous, whatever their orientation in global memory, so every
// fragment is one ds_read_b128.  A row is 64 halves = 32 dwords; it is padded to HLD = 72 halves = 36 dwords: 16
// consecutive rows then start at dwords 36 i mod 64 = {0,36,8,44,16,52,24,60,32,4,40,12,48,20,56,28}, sixteen
// different multiples of 4, so the 16 lanes x 4 dwords of one pass of a 128-bit read cover the 64 banks exactly once
// (and any 8 of them the 32 banks of a half).  72 halves = 144 bytes keeps every row 16-byte aligned.
//
// Staging (global -> registers -> LDS, double-buffered; the loads of stage t+1 are issued before the MFMAs of stage t
// and stored behind them; the first stage of a workgroup's NEXT tile rides behind the last stage of the current one):
//   K-contiguous operand (A row-major, B stored N x K): 16-byte loads along k, 16-byte LDS stores.
//   row-contiguous operand (A stored K x M, B row-major — `x @ W`): a thread loads four 16-byte vectors of 8 rows at
//   4 consecutive k, transposes the 8 x 4 halves in registers and writes 8 ds_write_b64, one per row.  A wave covers
//   4 row groups x 16 k-quads: for one store instruction the 64 lanes hit dwords 288 g + 2 q (+ const), g the row
//   group, q the k-quad: 32 banks by q, the other 32 by the parity of g — 128 dwords over 64 banks in the minimal
//   two passes.  (Lanes along the row groups alone would coalesce the global loads better and put 8 lanes on a bank.)
//   Without 16-byte alignment (pointer, leading dimension or batch stride), and on tiles that cross M, N or K, the
//   same registers are filled by 2-byte loads with bounds checks and zero fill.
//
// Split-K (few tiles, deep K): the walk runs over UNITS (batch item, tile, split s of S) instead of tiles; a unit is a
// contiguous range of K stages (balanced: the ranges differ by at most one stage, none is empty, the partial stage is
// in the last one).  A unit stores its fp32 accumulators to a slab of its own in accumulator-register order (register
// (i, j, r) of thread t at [(i*NJ + j)*16 + r][t]: every store instruction of a workgroup writes 256 consecutive
// floats, no LDS transpose), fences at device scope and takes a ticket of its tile.  The workgroup that draws S - 1
// puts the ticket back to 0, reads the S slabs back with the same mapping, adds them in ascending s — whoever arrived
// last, so the bits do not depend on the arrival order — rounds once and stores through the epilogue.  Nobody waits:
// a workgroup that is not last goes on to its next unit.  hgemm_splits() holds the rule for S.
#include "common.h"
#include "mfma_tile_device.h"
#include "wave_device.h"

namespace {

constexpr int BLOCK = 256;
constexpr int HN = 128;         // tile columns
constexpr int HK = 64;          // k per stage
constexpr int HLD = HK + 8;     // LDS row pitch in halves (see above)

using mfma::float16_t;
using mfma::half8_t;
typedef unsigned short hbits;  // a half moved as bits

union Vec8 {
  uint4 q;
  unsigned int w[4];
  hbits h[8];
};

// g[0 .. min(n, 8) - 1] by 2-byte loads, zeros behind them: the staging of misaligned operands and of edge tiles.  Not
// inlined: 64 predicated loads with their addresses, unrolled into each of the kernel's load sites, spilled its registers.
__device__ __noinline__ uint4 load8_partial(const hbits* __restrict__ g, long long n) {
  Vec8 r;
#pragma unroll
  for (int e = 0; e < 8; e++) r.h[e] = e < n ? g[e] : (hbits)0;
  return r.q;
}

// One operand tile of ROWS x HK halves on its way from global memory to the [row][k] LDS image.
// KC: element (row, k) at base + row * ld + k; otherwise at base + k * ld + row.
template <bool KC, int ROWS> struct HStage {
  static constexpr int SIZE = ROWS * HLD;                 // halves per LDS buffer
  static constexpr int NV = KC ? ROWS * HK / 8 / BLOCK : 4;  // 16-byte vectors per thread
  static constexpr int UNITS = ROWS / 8 * (HK / 4);       // !KC: (8 rows x 4 k) units: 256 or 128
  Vec8 v[NV];

  // !KC: row group and k-quad of this thread
  static __device__ __forceinline__ int rg() { return (threadIdx.x & 3) + 4 * (threadIdx.x >> 6); }
  static __device__ __forceinline__ int kq() { return (threadIdx.x >> 2) & 15; }
  static __device__ __forceinline__ bool active() { return KC || threadIdx.x < UNITS; }

  __device__ __forceinline__ void load(const hbits* __restrict__ base, long long ld, long long row0, long long k0,
                                       long long rows, long long K, bool vec_ok) {
    if (!active()) return;
    const bool interior = vec_ok && row0 + ROWS <= rows && k0 + HK <= K;  // workgroup-uniform
    if constexpr (KC) {
#pragma unroll
      for (int p = 0; p < NV; p++) {
        const int id = threadIdx.x + p * BLOCK;
        const long long row = row0 + (id >> 3), k = k0 + (id & 7) * 8;
        const hbits* g = base + row * ld + k;
        if (interior) { v[p].q = *(const uint4*)g; continue; }
        v[p].q = load8_partial(g, row < rows ? K - k : 0);
      }
    } else {
      const long long row = row0 + rg() * 8;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const long long k = k0 + kq() * 4 + j;
        const hbits* g = base + k * ld + row;
        if (interior) { v[j].q = *(const uint4*)g; continue; }
        v[j].q = load8_partial(g, k < K ? rows - row : 0);
      }
    }
  }

  __device__ __forceinline__ void store(hbits* __restrict__ s) const {
    if (!active()) return;
    if constexpr (KC) {
#pragma unroll
      for (int p = 0; p < NV; p++) {
        const int id = threadIdx.x + p * BLOCK;
        *(uint4*)(s + (id >> 3) * HLD + (id & 7) * 8) = v[p].q;
      }
    } else {
      hbits* d = s + rg() * 8 * HLD + kq() * 4;
#pragma unroll
      for (int r = 0; r < 8; r++) {
        // row r of the 8 x 4 block: half r of each of the four vectors
        const int sh = (r & 1) * 16;
        uint2 o;
        o.x = ((v[0].w[r >> 1] >> sh) & 0xffffu) | (((v[1].w[r >> 1] >> sh) & 0xffffu) << 16);
        o.y = ((v[2].w[r >> 1] >> sh) & 0xffffu) | (((v[3].w[r >> 1] >> sh) & 0xffffu) << 16);
        *(uint2*)(d + r * HLD) = o;
      }
    }
  }
};

// the 8 halves of a lane for MFMA k-step kk of the stage: row r0 + (l&31), k = 16 kk + 8 (l>>5)
__device__ __forceinline__ half8_t hfrag(const hbits* __restrict__ s, int r0, int kk, int lane) {
  union { uint4 q; half8_t h; } u;
  u.q = *(const uint4*)(s + (r0 + (lane & 31)) * HLD + kk * 16 + (lane >> 5) * 8);
  return u.h;
}

// fp32 -> half, round to nearest even, overflow to inf, subnormal results kept (v_cvt_f16_f32)
__device__ __forceinline__ hbits to_half_bits(float x) {
  union { _Float16 h; hbits b; } u;
  u.h = (_Float16)x;
  return u.b;
}

// What the split kernel is given beyond the unsplit one (whose arguments stay what they were): S > 1 splits per tile,
// one TM x HN fp32 slab per unit, one ticket word per tile.
template <bool SPLIT> struct HSplitArgs {};
template <> struct HSplitArgs<true> {
  int S;
  float* slabs;
  int* tickets;
};

// Workgroups walk the (batch x tile x split) space with stride gridDim.x.  SKINNY: tile 64 x 128, the four waves side
// by side.
template <bool AKC, bool BKC, bool SKINNY, bool SPLIT>
__global__ __launch_bounds__(BLOCK, 2) void hgemm_kernel(
    hbits* __restrict__ out, const hbits* __restrict__ A, const hbits* __restrict__ B, long long M, long long N,
    long long K, long long lda, long long ldb, long long sAb, long long sBb, long long tiles_m, long long tiles_n,
    long long batch, int vecA, int vecB, HSplitArgs<SPLIT> sp) {
  constexpr int TM = SKINNY ? 64 : 128;
  constexpr int NJ = SKINNY ? 1 : 2;
  using SA = HStage<AKC, TM>;
  using SB = HStage<BKC, HN>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  hbits* As = (hbits*)smem_raw;   // [2][SA::SIZE]
  hbits* Bs = As + 2 * SA::SIZE;  // [2][SB::SIZE]
  __shared__ int s_last;
  int S = 1;
  if constexpr (SPLIT) S = sp.S;
  const long long nt = tiles_m * tiles_n, total = nt * batch * S;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm0 = SKINNY ? 0 : (w >> 1) * 64, wn0 = SKINNY ? w * 32 : (w & 1) * 64;
  const long long nk = K > 0 ? (K + HK - 1) / HK : 1;  // K = 0: one stage of zero fill
  // unit L: its tile origin, batch item, unit id u = (bz * nt + tile) * S + s and stage range [kt0, kt1)
  auto coords = [&](long long L, long long& m0, long long& n0, long long& bz, long long& u, long long& kt0, long long& kt1) {
    long long pid = mfma::xcd_band(L, total);
    u = pid;
    kt0 = 0;
    kt1 = nk;
    if constexpr (SPLIT) {  // the splits of a tile are neighbours in the walk: they run at the same time
      const long long s = pid % S, each = nk / S, rem = nk % S;
      pid /= S;
      kt0 = s * each + (s < rem ? s : rem);
      kt1 = kt0 + each + (s < rem ? 1 : 0);
    }
    bz = pid / nt;
    pid -= bz * nt;
    m0 = (pid / tiles_n) * TM;
    n0 = (pid % tiles_n) * HN;
  };
  long long L = blockIdx.x;
  if (L >= total) return;
  long long m0, n0, bz, u, kt0, kt1;
  coords(L, m0, n0, bz, u, kt0, kt1);
  SA sa;
  SB sb;
  sa.load(A + bz * sAb, lda, m0, kt0 * HK, M, K, vecA);
  sb.load(B + bz * sBb, ldb, n0, kt0 * HK, N, K, vecB);
  sa.store(As);
  sb.store(Bs);
  __syncthreads();
  int buf = 0;
  for (;;) {
    const long long Ln = L + gridDim.x;
    const bool has_next = Ln < total;
    long long m1 = 0, n1 = 0, b1 = 0, u1 = 0, kn0 = 0, kn1 = 0;
    if (has_next) coords(Ln, m1, n1, b1, u1, kn0, kn1);
    float16_t acc[2][NJ];
    mfma::zero_acc(acc);
    const hbits* Ab = A + bz * sAb;
    const hbits* Bb = B + bz * sBb;
    // (constants in the unsplit kernel, which then compiles to the registers and spills it had before there were units)
    const long long lo = SPLIT ? kt0 : 0, hi = SPLIT ? kt1 : nk, next_k = SPLIT ? kn0 * HK : 0;
    for (long long kt = lo; kt < hi; kt++) {
      const bool more = kt + 1 < hi;
      if (more || has_next) {  // the next stage of this unit, or the next unit's first one behind this unit's last MFMAs
        sa.load(more ? Ab : A + b1 * sAb, lda, more ? m0 : m1, more ? (kt + 1) * HK : next_k, M, K, vecA);
        sb.load(more ? Bb : B + b1 * sBb, ldb, more ? n0 : n1, more ? (kt + 1) * HK : next_k, N, K, vecB);
      }
      const hbits* as = As + buf * SA::SIZE;
      const hbits* bs = Bs + buf * SB::SIZE;
#pragma unroll
      for (int kk = 0; kk < HK / 16; kk++) {
        half8_t af[2], bf[NJ];
#pragma unroll
        for (int i = 0; i < 2; i++) af[i] = hfrag(as, wm0 + i * 32, kk, lane);
#pragma unroll
        for (int j = 0; j < NJ; j++) bf[j] = hfrag(bs, wn0 + j * 32, kk, lane);
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < NJ; j++)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      if (more || has_next) {
        sa.store(As + (buf ^ 1) * SA::SIZE);
        sb.store(Bs + (buf ^ 1) * SB::SIZE);
      }
      __syncthreads();
      buf ^= 1;
    }
    bool finish = true;  // workgroup-uniform
    if constexpr (SPLIT) {
      constexpr int SLAB = TM * HN;
      float* mine = sp.slabs + u * SLAB + threadIdx.x;
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) mine[((i * NJ + j) * 16 + r) * BLOCK] = acc[i][j][r];
      __threadfence();
      __syncthreads();
      if (threadIdx.x == 0) s_last = atomicAdd(sp.tickets + u / S, 1) == S - 1;
      __syncthreads();
      finish = s_last;  // (the next write of s_last is behind the barriers of the next unit's stages)
      if (finish) {     // the last arriver of this tile: every slab is in memory
        if (threadIdx.x == 0) __hip_atomic_store(sp.tickets + u / S, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const float* all = sp.slabs + (u / S) * S * SLAB + threadIdx.x;
        for (int s = 0; s < S; s++)
#pragma unroll
          for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < NJ; j++)
#pragma unroll
              for (int r = 0; r < 16; r++) {
                const float v = all[(long long)s * SLAB + ((i * NJ + j) * 16 + r) * BLOCK];
                acc[i][j][r] = s == 0 ? v : acc[i][j][r] + v;
              }
      }
    }
    // epilogue: one rounding per element, in registers.  A lane holds single columns (col = l&31), so a store
    // instruction writes two runs of 32 consecutive halves (64 bytes, rows 4 apart): as wide as the layout allows.
    hbits* ob = out + bz * M * N;
    const bool interior = m0 + TM <= M && n0 + HN <= N;  // workgroup-uniform: unconditional stores
    if (finish) {
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const long long row = mfma::acc32_row(m0 + wm0 + i * 32, r, lane);
            const long long col = mfma::acc32_col(n0 + wn0 + j * 32, lane);
            if (interior || (row < M && col < N)) ob[row * N + col] = to_half_bits(acc[i][j][r]);
          }
    }
    if (!has_next) break;
    L = Ln;
    m0 = m1;
    n0 = n1;
    bz = b1;
    u = u1;
    kt0 = kn0;
    kt1 = kn1;
  }
}

// Splits per tile.  1 (the unsplit kernel) when the tiles fill the resident grid on their own or K is shallow; otherwise
// as many as fill it, each at least H_MIN_STAGES stages deep, H_MAX_SPLITS at the most.  A split costs one slab written
// and read back (64 or 32 KB through L2), about what two stages of operands cost (32 / 24 KB each), and the finisher
// adds the S slabs of its tile alone: profiles/hgemm.md has the numbers behind both constants.  Units stay below
// resident + tiles < 1024 (slabs: 64 MB at the most) and tickets below resident (pthip_ticket_slots takes 8192).
constexpr long long H_MIN_STAGES = 8, H_MAX_SPLITS = 32;

long long hgemm_splits(long long batch, long long M, long long N, long long K) {
  if (batch <= 0 || M <= 0 || N <= 0) return 1;
  const long long TM = M <= 64 ? 64 : 128;
  const long long tiles = ((M + TM - 1) / TM) * ((N + HN - 1) / HN) * batch, nk = (K + HK - 1) / HK;
  const long long resident = (long long)pthip::kNumCU * 2;
  if (tiles >= resident || nk < 2 * H_MIN_STAGES) return 1;
  long long S = (resident + tiles - 1) / tiles;
  if (S > nk / H_MIN_STAGES) S = nk / H_MIN_STAGES;
  if (S > H_MAX_SPLITS) S = H_MAX_SPLITS;
  return S;
}

template <bool AKC, bool BKC, bool SKINNY>
int hgemm_launch(long long batch, long long M, long long N, long long K, const hbits* A, long long sAb, long long lda,
                 const hbits* B, long long sBb, long long ldb, hbits* out) {
  constexpr int TM = SKINNY ? 64 : 128;
  const long long S = hgemm_splits(batch, M, N, K);
  const void* k = S > 1 ? (const void*)hgemm_kernel<AKC, BKC, SKINNY, true> : (const void*)hgemm_kernel<AKC, BKC, SKINNY, false>;
  const size_t shmem = (size_t)(2 * HStage<AKC, TM>::SIZE + 2 * HStage<BKC, HN>::SIZE) * sizeof(hbits);
  if (int r = pthip::lds_opt_in(k, shmem)) return r;
  const long long tiles_m = (M + TM - 1) / TM, tiles_n = (N + HN - 1) / HN, tiles = tiles_m * tiles_n * batch;
  const long long total = tiles * S, resident = (long long)pthip::kNumCU * 2;
  const long long grid = total < resident ? total : resident;
  // 16-byte loads: pointer, leading dimension and batch stride all multiples of 8 halves
  const int vecA = (lda % 8 == 0) && (((uintptr_t)A) % 16 == 0) && (sAb % 8 == 0);
  const int vecB = (ldb % 8 == 0) && (((uintptr_t)B) % 16 == 0) && (sBb % 8 == 0);
  pthip::Scratch mem;  // (back to the pool at the return: reuse is stream-ordered behind this launch)
  void* slabs = nullptr;
  void* tickets = nullptr;
  if (S > 1) {
    if (int r = mem.alloc((size_t)total * TM * HN * sizeof(float), &slabs)) return r;
    if (int r = pthip_ticket_slots((int)tiles, &tickets)) return r;
    const HSplitArgs<true> sp{(int)S, (float*)slabs, (int*)tickets};
    PTHIP_KLAUNCH((hgemm_kernel<AKC, BKC, SKINNY, true>), dim3((unsigned)grid), dim3(BLOCK), shmem, pthip::ctx().stream, out, A, B, M, N,
                  K, lda, ldb, sAb, sBb, tiles_m, tiles_n, batch, vecA, vecB, sp);
    return pthip::post_launch("hgemm(split-K)");
  }
  PTHIP_KLAUNCH((hgemm_kernel<AKC, BKC, SKINNY, false>), dim3((unsigned)grid), dim3(BLOCK), shmem, pthip::ctx().stream, out, A, B, M, N,
                K, lda, ldb, sAb, sBb, tiles_m, tiles_n, batch, vecA, vecB, HSplitArgs<false>{});
  return pthip::post_launch("hgemm");
}

// ---------------------------------------------------------------------------------------------------------------
// matrix-vector: out[m] = half(sum_k A[m*sA0 + k*sA1] * x[k*sx]), fp32 accumulation in a fixed order
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float h2f(hbits b) {
  union { hbits b; _Float16 h; } u;
  u.b = b;
  return (float)u.h;
}

// Lane g of the G lanes of a row, over k in [k0, k1): 8 consecutive k per step (one 16-byte load when VEC; k0 is a
// multiple of 8 G, so the loads keep the row's alignment), products added in ascending k.
template <int G, bool VEC>
__device__ __forceinline__ float hgemv_lane_sum(const hbits* __restrict__ a, const hbits* __restrict__ x, int g,
                                                long long k0, long long k1, long long sA1, long long sx) {
  float acc = 0.f;
  for (long long k = k0 + g * 8; k < k1; k += G * 8) {
    if (VEC && k + 8 <= k1) {
      Vec8 av;
      av.q = *(const uint4*)(a + k);
#pragma unroll
      for (int e = 0; e < 8; e++) acc = fmaf(h2f(av.h[e]), h2f(x[(k + e) * sx]), acc);
    } else {
      for (int e = 0; e < 8 && k + e < k1; e++) acc = fmaf(h2f(a[(k + e) * sA1]), h2f(x[(k + e) * sx]), acc);
    }
  }
  return acc;
}

// Row layout: G lanes per row (64: a wave per row; 8: eight short rows per wave); the G partial sums of
// hgemv_lane_sum meet in group_sum's tree.
template <int G, bool VEC>
__global__ __launch_bounds__(BLOCK) void hgemv_row_kernel(hbits* __restrict__ out, const hbits* __restrict__ A,
                                                          const hbits* __restrict__ x, long long M, long long K,
                                                          long long sA0, long long sA1, long long sx) {
  constexpr int RPB = BLOCK / G;  // rows per block
  const int g = threadIdx.x % G;
  for (long long m = (long long)blockIdx.x * RPB + threadIdx.x / G; m - threadIdx.x / G < M; m += (long long)gridDim.x * RPB) {
    // (the loop bound is wave-uniform: every lane of a wave reaches the shuffles of group_sum)
    float acc = 0.f;
    if (m < M) acc = hgemv_lane_sum<G, VEC>(A + m * sA0, x, g, 0, K, sA1, sx);
    acc = wave::group_sum<G>(acc);
    if (g == 0 && m < M) out[m] = to_half_bits(acc);
  }
}

// The hand-over shared by the two split matrix-vector kernels: the block has stored its partial sums; the one that
// draws S - 1 from its row block's ticket puts the ticket back and goes on (true), every other block is done.
__device__ __forceinline__ bool hgemv_last_arriver(int* ticket, int S, int* s_last) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) *s_last = atomicAdd(ticket, 1) == S - 1;
  __syncthreads();
  if (!*s_last) return false;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  return true;
}

// Row layout, few rows and a deep K: block (row block rb, split s) takes k in [s * chunk, (s + 1) * chunk) of RPB rows
// (4: a wave per row; 1: the whole block on one row, so that an inner product fills every wave slot) and stores RPB
// fp32 partial sums at slabs[rb][s][row].  The last arriver of the row block adds them in a fixed order (wave `row`:
// lane l adds s = l, l + 64, ... ascending, then group_sum's tree) and rounds once.
template <int RPB, bool VEC>
__global__ __launch_bounds__(BLOCK) void hgemv_row_split_kernel(hbits* __restrict__ out, const hbits* __restrict__ A,
                                                                const hbits* __restrict__ x, long long M, long long K,
                                                                long long sA0, long long sA1, long long sx, int S,
                                                                long long chunk, float* slabs, int* tickets) {
  constexpr int G = BLOCK / RPB;
  __shared__ float s_w[BLOCK / 64];
  __shared__ int s_last;
  const long long rb = blockIdx.x / S;
  const int s = blockIdx.x % S, g = threadIdx.x % G, row = threadIdx.x / G;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long m = rb * RPB + row, k0 = s * chunk, k1 = k0 + chunk < K ? k0 + chunk : K;
  float acc = 0.f;
  if (m < M) acc = hgemv_lane_sum<G, VEC>(A + m * sA0, x, g, k0, k1, sA1, sx);
  acc = wave::group_sum<64>(acc);
  if constexpr (G > 64) {  // the four waves of the row, added in wave order
    if (lane == 0) s_w[w] = acc;
    __syncthreads();
    acc = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  }
  float* slab = slabs + rb * S * RPB;
  if (g == 0) slab[s * RPB + row] = acc;
  if (!hgemv_last_arriver(tickets + rb, S, &s_last)) return;
  if (w < RPB) {
    float t = 0.f;
    for (int p = lane; p < S; p += 64) t += slab[p * RPB + w];
    t = wave::group_sum<64>(t);
    if (lane == 0 && rb * RPB + w < M) out[rb * RPB + w] = to_half_bits(t);
  }
}

// Column layout (sA0 == 1): lane = output row, so a wave reads 64 consecutive halves of a column; the four waves of
// a block take k = w, w + 4, ... and their partial sums are added in wave order.
__global__ __launch_bounds__(BLOCK) void hgemv_col_kernel(hbits* __restrict__ out, const hbits* __restrict__ A,
                                                          const hbits* __restrict__ x, long long M, long long K,
                                                          long long sA1, long long sx) {
  __shared__ float s_part[BLOCK / 64][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long m0 = (long long)blockIdx.x * 64; m0 < M; m0 += (long long)gridDim.x * 64) {
    const long long m = m0 + lane;
    float acc = 0.f;
    if (m < M)
      for (long long k = w; k < K; k += BLOCK / 64) acc = fmaf(h2f(A[k * sA1 + m]), h2f(x[k * sx]), acc);
    s_part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && m < M) {
      float t = s_part[0][lane];
#pragma unroll
      for (int p = 1; p < BLOCK / 64; p++) t += s_part[p][lane];
      out[m] = to_half_bits(t);
    }
    __syncthreads();
  }
}

// Column layout, few 64-column blocks and a deep K: block (column block cb, split s) takes k in [s * chunk,
// (s + 1) * chunk), its four waves k = k0 + w, k0 + w + 4, ...; their sums, added in wave order, go to
// slabs[cb][s][lane].  The last arriver of the column block adds the S partial sums of a lane in ascending s.
__global__ __launch_bounds__(BLOCK) void hgemv_col_split_kernel(hbits* __restrict__ out, const hbits* __restrict__ A,
                                                                const hbits* __restrict__ x, long long M, long long K,
                                                                long long sA1, long long sx, int S, long long chunk,
                                                                float* slabs, int* tickets) {
  __shared__ float s_part[BLOCK / 64][64];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long cb = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const long long m = cb * 64 + lane, k0 = s * chunk, k1 = k0 + chunk < K ? k0 + chunk : K;
  float acc = 0.f;
  if (m < M)
    for (long long k = k0 + w; k < k1; k += BLOCK / 64) acc = fmaf(h2f(A[k * sA1 + m]), h2f(x[k * sx]), acc);
  s_part[w][lane] = acc;
  __syncthreads();
  float* slab = slabs + cb * S * 64;
  if (w == 0) {
    float t = s_part[0][lane];
#pragma unroll
    for (int p = 1; p < BLOCK / 64; p++) t += s_part[p][lane];
    slab[s * 64 + lane] = t;
  }
  if (!hgemv_last_arriver(tickets + cb, S, &s_last)) return;
  if (w == 0 && m < M) {
    float t = slab[lane];
    for (int p = 1; p < S; p++) t += slab[p * 64 + lane];
    out[m] = to_half_bits(t);
  }
}

// How pthip_hgemv runs a product: the layout, and the split of k when the row (column) blocks are few and K is deep.
// S = 1: the unsplit kernels.  Otherwise S blocks per row block, as many as fill H_GEMV_BLOCKS, each at least four
// steps of its lanes deep (row layout: chunks are multiples of 8 G, so the vector loads keep their alignment).
struct HgemvPlan {
  bool col;
  int rpb;          // row layout: rows per block of the split kernel (1 below four rows)
  long long units;  // row blocks / 64-column blocks
  long long S, chunk;
};
constexpr long long H_GEMV_BLOCKS = (long long)pthip::kNumCU * 4;

HgemvPlan hgemv_plan(long long M, long long K, long long sA0, long long sA1) {
  HgemvPlan p;
  if (K <= 1) sA1 = 1;
  p.col = sA0 == 1 && sA1 != 1 && M > 1;
  p.rpb = M < 4 ? 1 : 4;
  p.units = p.col ? (M + 63) / 64 : (M + p.rpb - 1) / p.rpb;
  const long long step = p.col ? BLOCK / 64 : (long long)(BLOCK / p.rpb) * 8;  // k per pass of the block's lanes
  const long long steps = (K + step - 1) / step, min_steps = p.col ? 64 : 4;
  p.S = 1;
  p.chunk = K;
  if (M <= 0 || p.units * 2 > H_GEMV_BLOCKS || steps < 2 * min_steps) return p;
  long long S = (H_GEMV_BLOCKS + p.units - 1) / p.units;
  if (S > steps / min_steps) S = steps / min_steps;
  p.chunk = (steps + S - 1) / S * step;
  p.S = (K + p.chunk - 1) / p.chunk;  // no empty chunk
  return p;
}

}  // namespace

extern "C" int64_t pthip_hgemm_splits(int64_t batch, int64_t M, int64_t N, int64_t K) { return hgemm_splits(batch, M, N, K); }

extern "C" int64_t pthip_hgemv_splits(int64_t M, int64_t K, int64_t sA0, int64_t sA1) { return hgemv_plan(M, K, sA0, sA1).S; }

extern "C" int pthip_hgemm(int64_t batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t sAb, int64_t sA0,
                           int64_t sA1, const void* B, int64_t sBb, int64_t sB0, int64_t sB1, void* out) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || M <= 0 || N <= 0) return 0;
  // strides of length-1 dimensions are free: normalise them, then classify as pthip_gemm does
  if (K <= 1) sA1 = 1;
  if (M == 1) { if (sA1 == 1) sA0 = K; else sA0 = 1; }
  if (N == 1) sB1 = 1;
  if (K <= 1) { if (sB1 == 1) sB0 = N; else sB0 = 1; }
  bool akc, bkc;
  long long lda, ldb;
  if (sA1 == 1) { akc = true; lda = sA0; }
  else if (sA0 == 1) { akc = false; lda = sA1; }
  else return pthip::set_error("pthip_hgemm: A has no unit stride (%lld, %lld)", (long long)sA0, (long long)sA1);
  if (sB1 == 1) { bkc = false; ldb = sB0; }
  else if (sB0 == 1) { bkc = true; ldb = sB1; }
  else return pthip::set_error("pthip_hgemm: B has no unit stride (%lld, %lld)", (long long)sB0, (long long)sB1);
  if (lda < 0 || ldb < 0 || sAb < 0 || sBb < 0) return pthip::set_error("pthip_hgemm: negative strides are not supported");
  const hbits* a = (const hbits*)A;
  const hbits* b = (const hbits*)B;
  hbits* o = (hbits*)out;
  const bool skinny = M <= 64;
#define GO(X, Y)                                                                            \
  do {                                                                                      \
    if (skinny) return hgemm_launch<X, Y, true>(batch, M, N, K, a, sAb, lda, b, sBb, ldb, o); \
    return hgemm_launch<X, Y, false>(batch, M, N, K, a, sAb, lda, b, sBb, ldb, o);          \
  } while (0)
  if (akc && bkc) GO(true, true);
  if (akc && !bkc) GO(true, false);
  if (!akc && bkc) GO(false, true);
  GO(false, false);
#undef GO
}

extern "C" int pthip_hgemv(int64_t M, int64_t K, const void* A, int64_t sA0, int64_t sA1, const void* x, int64_t sx,
                           void* out) {
  PTHIP_REQUIRE_INIT();
  if (M <= 0) return 0;
  if (K <= 1) sA1 = 1;
  const hbits* a = (const hbits*)A;
  const hbits* xv = (const hbits*)x;
  hbits* o = (hbits*)out;
  hipStream_t st = pthip::ctx().stream;
  const long long max_blocks = (long long)pthip::kNumCU * 8;
  const HgemvPlan p = hgemv_plan(M, K, sA0, sA1);
  if (p.S > 1) {  // few row blocks, deep K: S blocks per row block, finished by the last arriver in the same launch
    pthip::Scratch mem;
    void* slabs = nullptr;
    void* tickets = nullptr;
    if (int r = mem.alloc((size_t)(p.units * p.S * (p.col ? 64 : p.rpb)) * sizeof(float), &slabs)) return r;
    if (int r = pthip_ticket_slots((int)p.units, &tickets)) return r;
    const dim3 grid((unsigned)(p.units * p.S));
    if (p.col) {
      PTHIP_KLAUNCH(hgemv_col_split_kernel, grid, dim3(BLOCK), 0, st, o, a, xv, (long long)M, (long long)K, (long long)sA1,
                    (long long)sx, (int)p.S, p.chunk, (float*)slabs, (int*)tickets);
      return pthip::post_launch("hgemv(col, split-K)");
    }
    const bool vec = sA1 == 1 && ((uintptr_t)A) % 16 == 0 && (sA0 % 8 == 0 || M == 1);
#define GO(R, V)                                                                                                            \
  PTHIP_KLAUNCH((hgemv_row_split_kernel<R, V>), grid, dim3(BLOCK), 0, st, o, a, xv, (long long)M, (long long)K, (long long)sA0, \
                (long long)sA1, (long long)sx, (int)p.S, p.chunk, (float*)slabs, (int*)tickets)
    if (p.rpb == 1) { if (vec) GO(1, true); else GO(1, false); }
    else { if (vec) GO(4, true); else GO(4, false); }
#undef GO
    return pthip::post_launch("hgemv(row, split-K)");
  }
  if (sA0 == 1 && sA1 != 1 && M > 1) {
    long long blocks = (M + 63) / 64;
    if (blocks > max_blocks) blocks = max_blocks;
    PTHIP_KLAUNCH(hgemv_col_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, st, o, a, xv, (long long)M, (long long)K,
                  (long long)sA1, (long long)sx);
    return pthip::post_launch("hgemv(col)");
  }
  const bool vec = sA1 == 1 && ((uintptr_t)A) % 16 == 0 && (sA0 % 8 == 0 || M == 1);
  const bool shortrow = K <= 64;
  const int rpb = shortrow ? BLOCK / 8 : BLOCK / 64;
  long long blocks = (M + rpb - 1) / rpb;
  if (blocks > max_blocks) blocks = max_blocks;
#define GO(G, V)                                                                                                   \
  PTHIP_KLAUNCH((hgemv_row_kernel<G, V>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, o, a, xv, (long long)M, (long long)K, \
                (long long)sA0, (long long)sA1, (long long)sx)
  if (shortrow) { if (vec) GO(8, true); else GO(8, false); }
  else { if (vec) GO(64, true); else GO(64, false); }
#undef GO
  return pthip::post_launch("hgemv(row)");
}
