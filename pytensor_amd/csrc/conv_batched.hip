// conv_batched.hip — Blockwise(Convolve1d) / Blockwise(Convolve2d): a whole broadcast stack of direct convolutions in
// one launch (DESIGN §4 "Batched convolution").
//
// Reference: Convolve1d.perform (pytensor/tensor/signal/conv.py: np.convolve, "full" or "valid") and
// Convolve2d.perform (scipy.signal.convolve, direct sums) under Blockwise.perform (pytensor/tensor/blockwise.py).
//
// 1-d.  A workgroup of 256 lanes owns a tile of 256 * R consecutive outputs of one item, R = 8 consecutive outputs per
// lane in registers.  An item with fewer outputs than half a tile shares the workgroup with one or three others: whole
// waves go to each item (sub-groups of 128 or 64 lanes).  The signal window of the tile and the taps of a chunk are
// staged into LDS once, with coalesced loads through the operands' own strides (negative: the flipped operand of the
// gradient; batch stride 0: a shared operand).  The inner loop walks the taps: one broadcast LDS read of the tap and
// one new signal element per lane slide an R-wide register window, two LDS reads for R multiply-adds.  The window is
// kept in LDS with one pad element every R, so that the lanes' reads (R elements apart) fall on distinct banks.  Taps
// are taken in chunks of at most 256, the window staged again per chunk, the accumulators kept in registers.
//
// Every output is accumulated in increasing index of the longer operand with one accumulator, the order of
// convolve1d_kernel (misc.hip), whatever the tiling.  A tile whose outputs all have their full set of terms runs the
// loop without a branch (the window beyond the stored outputs is zero); a tile at an end of a "full" convolution
// predicates each term on its index, so that a zero of the padding never meets an Inf or NaN of the other operand.
//
// 2-d.  A workgroup owns a 16 x 64 output tile of one item, 4 outputs along the row per lane; smaller outputs share
// the workgroup (sub-tiles down to 16 columns, two or four items).  The kernel's rows are walked in chunks of at most
// 8 (columns in chunks of 64, one row at a time, when the kernel is wider than that), the image window of the chunk
// and the chunk in LDS, the window padded by one element every 4.  Terms are added in increasing (row, column) of the
// larger operand.
//
// No matrix instructions: see DESIGN §4.
#include "common.h"

// packed fp32 arithmetic is kept out of this file's device code: scalar v_fma_f32 only
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int kLanes = 256;
constexpr int kR1 = 8;                  // 1-d: outputs per lane
constexpr int kTile1 = kLanes * kR1;    // 1-d: outputs per workgroup
constexpr int kChunk1 = 256;            // 1-d: taps per staged chunk
constexpr int kMaxSub = 4;              // items per workgroup, at most (one wave each)
constexpr int kR2 = 4;                  // 2-d: outputs per lane, along the row
constexpr int kTileH = 16, kTileW = 64; // 2-d: output tile
constexpr int kRowChunk = 8;            // 2-d: kernel rows per staged chunk
constexpr int kColChunk = 64;           // 2-d: kernel columns per staged chunk
constexpr int kLds2 = 64 * 1024;        // 2-d: LDS of a workgroup, at most (two fit a CU with room to spare)

__host__ __device__ constexpr int pad8(int i) { return i + (i >> 3); }
__host__ __device__ constexpr int pad4(int i) { return i + (i >> 2); }

// a sub-group's LDS in the 1-d kernel: the padded window of its sub-tile, then the taps of the chunk
__host__ __device__ constexpr int region1(int lanes) { return pad8(lanes * kR1 + kChunk1 - 1) + 1 + kChunk1; }
constexpr int kLds1 = region1(kLanes) > kMaxSub * region1(kLanes / kMaxSub) ? region1(kLanes) : kMaxSub * region1(kLanes / kMaxSub);
static_assert(2 * region1(kLanes / 2) <= kLds1, "LDS of the two-item split");

// the broadcast batch: up to four dimensions, outermost first, with each operand's element stride along it (0 where
// the operand is shared); the output is contiguous
struct Batch {
  long long n[4], sa[4], sb[4];
};

__device__ __forceinline__ void item_offsets(const Batch& bt, long long item, long long& oa, long long& ob) {
  oa = 0;
  ob = 0;
#pragma unroll
  for (int d = 3; d >= 0; d--) {
    if (bt.n[d] == 1) continue;
    const long long i = item % bt.n[d];
    item /= bt.n[d];
    oa += i * bt.sa[d];
    ob += i * bt.sb[d];
  }
}

__device__ __forceinline__ int clamp_int(long long v, long long lo, long long hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// one chunk of taps of the 1-d kernel for one lane: acc[r] += win[base + r + s] * tp[s], s = 0 .. len - 1, where
// `base` is the lane's first window slot and slot base + r + s holds a[jl + r + s] (EDGE: terms outside [0, na) skipped)
template <class T, bool EDGE>
__device__ __forceinline__ void chunk1(const T* __restrict__ win, const T* __restrict__ tp, int lane, int len, long long jl,
                                       long long na, T (&acc)[kR1]) {
  const T* wl = win + lane * (kR1 + 1);  // = pad8(lane * kR1)
  const int qlo = clamp_int(-jl, 0, 1 << 30), qhi = clamp_int(na - 1 - jl, -1, 1 << 30);
  T w[kR1];
#pragma unroll
  for (int r = 0; r < kR1 - 1; r++) w[r] = wl[r];
  for (int s0 = 0; s0 < len; s0 += kR1) {
    const T* ws = wl + s0 + (s0 >> 3);  // s0 is a multiple of R: pad8(lane * R + s0 + e) = this + pad8(e)
#pragma unroll
    for (int u = 0; u < kR1; u++) {
      if (s0 + u >= len) break;
      w[kR1 - 1] = ws[pad8(kR1 - 1 + u)];
      const T t = tp[s0 + u];
#pragma unroll
      for (int r = 0; r < kR1; r++)
        if (!EDGE || (r + s0 + u >= qlo && r + s0 + u <= qhi)) acc[r] += w[r] * t;
#pragma unroll
      for (int r = 0; r < kR1 - 1; r++) w[r] = w[r + 1];
    }
  }
}

// out[item][i] = sum_j a[j] * b[i + lo - j], na >= nb; grid = tiles x item groups, `sub` items per workgroup (1, 2, 4)
template <class T>
__global__ __launch_bounds__(kLanes) void convolve1d_batched_kernel(const T* __restrict__ a, long long na, long long sa,
                                                                    const T* __restrict__ b, long long nb, long long sb, Batch bt,
                                                                    long long nitems, long long lo, long long nout, int sub,
                                                                    long long tiles, T* __restrict__ out) {
  __shared__ T lds[kLds1];
  const int L = kLanes / sub;  // lanes of a sub-group: whole waves
  const int g = threadIdx.x / L, lane = threadIdx.x % L;
  const int LR = L * kR1;
  const long long tile = blockIdx.x % tiles, item = (blockIdx.x / tiles) * sub + g;
  const bool live = item < nitems;
  T* win = lds + g * region1(L);
  T* tp = win + pad8(LR + kChunk1 - 1) + 1;
  long long oa = 0, ob = 0;
  if (live) item_offsets(bt, item, oa, ob);
  const T* ai = a + oa;
  const T* bi = b + ob;
  const long long f0 = lo + tile * LR;  // index in the full convolution of the sub-tile's first output
  const long long fend = lo + nout < f0 + LR ? lo + nout : f0 + LR;
  const bool edge = f0 - (nb - 1) < 0 || fend - 1 > na - 1;
  T acc[kR1];
#pragma unroll
  for (int r = 0; r < kR1; r++) acc[r] = T(0);
  // taps from the last to the first: increasing index of a
  for (long long k1 = nb - 1; k1 >= 0; k1 -= kChunk1) {
    const int len = (int)(k1 + 1 < kChunk1 ? k1 + 1 : kChunk1);
    const long long j0 = f0 - k1;  // index in a of window slot 0
    if (k1 != nb - 1) __syncthreads();
    if (live) {
      for (int i = lane; i < LR + len - 1; i += L) {
        const long long j = j0 + i;
        win[pad8(i)] = (j >= 0 && j < na) ? ai[j * sa] : T(0);
      }
      for (int s = lane; s < len; s += L) tp[s] = bi[(k1 - s) * sb];
    }
    __syncthreads();
    if (live) {
      if (edge) chunk1<T, true>(win, tp, lane, len, j0 + (long long)lane * kR1, na, acc);
      else chunk1<T, false>(win, tp, lane, len, 0, na, acc);
    }
  }
  if (!live) return;
  T* oi = out + item * nout;
#pragma unroll
  for (int r = 0; r < kR1; r++) {
    const long long f = f0 + (long long)lane * kR1 + r;
    if (f < fend) oi[f - lo] = acc[r];
  }
}

// the split of the 2-d kernel, made on the host from the shapes
struct Plan2 {
  int sub;         // items per workgroup
  int cgs;         // lanes along a row of the sub-tile (4 outputs each)
  int th, tw;      // sub-tile
  int rc, cc;      // kernel rows / columns per chunk
  int ws;          // window row stride in LDS (padded)
  int region;      // elements of LDS per sub-group
  int tiles_r, tiles_c;
};

// one kernel row of a chunk for one lane: acc[r] += wrow[c0 + r + s] * tp[s]; slot c0 + r + s holds column qlo-relative
template <class T, bool EDGE>
__device__ __forceinline__ void row2(const T* __restrict__ wrow, const T* __restrict__ tp, int cg, int len, bool rowok, int qlo,
                                     int qhi, T (&acc)[kR2]) {
  const T* wl = wrow + cg * (kR2 + 1);  // = pad4(cg * kR2)
  T w[kR2];
#pragma unroll
  for (int r = 0; r < kR2 - 1; r++) w[r] = wl[r];
  for (int s0 = 0; s0 < len; s0 += kR2) {
    const T* ws = wl + s0 + (s0 >> 2);
#pragma unroll
    for (int u = 0; u < kR2; u++) {
      if (s0 + u >= len) break;
      w[kR2 - 1] = ws[pad4(kR2 - 1 + u)];
      const T t = tp[s0 + u];
#pragma unroll
      for (int r = 0; r < kR2; r++)
        if (!EDGE || (rowok && r + s0 + u >= qlo && r + s0 + u <= qhi)) acc[r] += w[r] * t;
#pragma unroll
      for (int r = 0; r < kR2 - 1; r++) w[r] = w[r + 1];
    }
  }
}

// out[item][i][j] = sum_{p,q} a[p][q] * b[i + lo_r - p][j + lo_c - q]; grid = row tiles x column tiles x item groups
template <class T>
__global__ __launch_bounds__(kLanes) void convolve2d_batched_kernel(const T* __restrict__ a, int ha, int wa, long long sa0,
                                                                    long long sa1, const T* __restrict__ b, int hb, int wb,
                                                                    long long sb0, long long sb1, Batch bt, long long nitems, int lo_r,
                                                                    int lo_c, int ho, int wo, Plan2 pl, T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  T* lds = reinterpret_cast<T*>(lds_raw);
  const int L = kLanes / pl.sub;
  const int g = threadIdx.x / L, lane = threadIdx.x % L;
  const int cg = lane % pl.cgs, row = lane / pl.cgs;
  long long bid = blockIdx.x;
  const int tc = (int)(bid % pl.tiles_c);
  bid /= pl.tiles_c;
  const int tr = (int)(bid % pl.tiles_r);
  const long long item = (bid / pl.tiles_r) * pl.sub + g;
  const bool live = item < nitems;
  T* win = lds + (long long)g * pl.region;
  T* tp = win + (pl.th + pl.rc - 1) * pl.ws;
  long long oa = 0, ob = 0;
  if (live) item_offsets(bt, item, oa, ob);
  const T* ai = a + oa;
  const T* bi = b + ob;
  // full-convolution indices of the sub-tile's first output and one past its last stored one
  const int fr0 = lo_r + tr * pl.th, fc0 = lo_c + tc * pl.tw;
  const int frend = lo_r + ho < fr0 + pl.th ? lo_r + ho : fr0 + pl.th, fcend = lo_c + wo < fc0 + pl.tw ? lo_c + wo : fc0 + pl.tw;
  const bool edge = fr0 - (hb - 1) < 0 || frend - 1 > ha - 1 || fc0 - (wb - 1) < 0 || fcend - 1 > wa - 1;
  const int sx = lane & 63, sy = lane >> 6, sny = L >> 6;  // staging: 64 lanes along a row
  T acc[kR2];
#pragma unroll
  for (int r = 0; r < kR2; r++) acc[r] = T(0);
  bool first = true;
  for (int u1 = hb - 1; u1 >= 0; u1 -= pl.rc) {
    const int rl = u1 + 1 < pl.rc ? u1 + 1 : pl.rc;
    for (int v1 = wb - 1; v1 >= 0; v1 -= pl.cc) {
      const int cl = v1 + 1 < pl.cc ? v1 + 1 : pl.cc;
      const int p0 = fr0 - u1, q0 = fc0 - v1;  // image row / column of window slot (0, 0)
      if (!first) __syncthreads();
      first = false;
      if (live) {
        const int wr = pl.th + rl - 1, wc = pl.tw + cl - 1;
        for (int i = sy; i < wr; i += sny) {
          const int p = p0 + i;
          const bool pin = p >= 0 && p < ha;
          for (int j = sx; j < wc; j += 64) {
            const int q = q0 + j;
            win[i * pl.ws + pad4(j)] = (pin && q >= 0 && q < wa) ? ai[p * sa0 + q * sa1] : T(0);
          }
        }
        for (int i = sy; i < rl; i += sny)
          for (int j = sx; j < cl; j += 64) tp[i * cl + j] = bi[(u1 - i) * sb0 + (v1 - j) * sb1];
      }
      __syncthreads();
      if (live && row < pl.th) {
        // terms of this lane: image row p0 + row + du, column q0 + cg * R + r + s
        const int ql = q0 + cg * kR2;
        const int qlo = ql < 0 ? -ql : 0, qhi = wa - 1 - ql;
        for (int du = 0; du < rl; du++) {
          const T* wrow = win + (row + du) * pl.ws;
          const int p = p0 + row + du;
          if (edge) row2<T, true>(wrow, tp + du * cl, cg, cl, p >= 0 && p < ha, qlo, qhi, acc);
          else row2<T, false>(wrow, tp + du * cl, cg, cl, true, 0, 0, acc);
        }
      }
    }
  }
  if (!live || row >= pl.th) return;
  const int fr = fr0 + row;
  if (fr >= frend) return;
  T* oi = out + item * ((long long)ho * wo) + (long long)(fr - lo_r) * wo;
#pragma unroll
  for (int r = 0; r < kR2; r++) {
    const int fc = fc0 + cg * kR2 + r;
    if (fc < fcend) oi[fc - lo_c] = acc[r];
  }
}

int fill_batch(const char* who, int nbd, const int64_t* dims, const int64_t* sa, const int64_t* sb, bool swap, Batch* bt,
               long long* nitems) {
  if (nbd < 0 || nbd > 4) return pthip::set_error("%s: %d batch dimensions (at most 4)", who, nbd);
  long long n = 1;
  for (int d = 0; d < 4; d++) {
    const int s = d - (4 - nbd);
    bt->n[d] = s < 0 ? 1 : dims[s];
    bt->sa[d] = s < 0 ? 0 : (swap ? sb[s] : sa[s]);
    bt->sb[d] = s < 0 ? 0 : (swap ? sa[s] : sb[s]);
    if (bt->n[d] < 0) return pthip::set_error("%s: negative batch dimension", who);
    n *= bt->n[d];
  }
  *nitems = n;
  return 0;
}

template <class T>
int launch1(const void* a, long long na, long long sa, const void* b, long long nb, long long sb, const Batch& bt, long long nitems,
            int full, void* out) {
  const long long lo = full ? 0 : nb - 1, nout = full ? na + nb - 1 : na - nb + 1;
  // whole waves to each item: four items of up to 64 * R outputs, two of up to 128 * R, else one item per workgroup
  const int sub = nout <= kTile1 / 4 ? 4 : (nout <= kTile1 / 2 ? 2 : 1);
  const long long per = kTile1 / sub, tiles = (nout + per - 1) / per, groups = (nitems + sub - 1) / sub;
  if (tiles * groups > 0x7fffffffLL) return pthip::set_error("pthip_convolve1d_batched: %lld workgroups", tiles * groups);
  PTHIP_KLAUNCH(convolve1d_batched_kernel<T>, dim3((unsigned)(tiles * groups)), dim3(kLanes), 0, pthip::ctx().stream, (const T*)a, na,
                sa, (const T*)b, nb, sb, bt, nitems, lo, nout, sub, tiles, (T*)out);
  return pthip::post_launch("convolve1d_batched");
}

Plan2 plan2(int ho, int wo, int hb, int wb, int itemsize) {
  Plan2 pl;
  pl.sub = 1, pl.cgs = kTileW / kR2, pl.th = kTileH, pl.tw = kTileW;
  // the most items per workgroup whose sub-tile (whole waves; 64, 32 or 16 columns) holds the whole output
  for (int sub = kMaxSub; sub >= 2 && pl.sub == 1; sub /= 2)
    for (int tw = kTileW; tw >= 16; tw /= 2) {
      const int th = (kLanes / sub) / (tw / kR2);
      if (th >= ho && tw >= wo) {
        pl.sub = sub, pl.cgs = tw / kR2, pl.th = th, pl.tw = tw;
        break;
      }
    }
  pl.cc = wb < kColChunk ? wb : kColChunk;
  pl.rc = wb <= kColChunk ? (hb < kRowChunk ? hb : kRowChunk) : 1;
  for (;; pl.rc--) {
    pl.ws = (pad4(pl.tw + pl.cc - 1) + 1) | 1;
    pl.region = (pl.th + pl.rc - 1) * pl.ws + pl.rc * pl.cc;
    if (pl.rc == 1 || (long long)pl.sub * pl.region * itemsize <= kLds2) break;
  }
  pl.tiles_r = (ho + pl.th - 1) / pl.th;
  pl.tiles_c = (wo + pl.tw - 1) / pl.tw;
  return pl;
}

template <class T>
int launch2(const void* a, int ha, int wa, long long sa0, long long sa1, const void* b, int hb, int wb, long long sb0, long long sb1,
            const Batch& bt, long long nitems, int full, void* out) {
  const int lo_r = full ? 0 : hb - 1, lo_c = full ? 0 : wb - 1;
  const int ho = full ? ha + hb - 1 : ha - hb + 1, wo = full ? wa + wb - 1 : wa - wb + 1;
  const Plan2 pl = plan2(ho, wo, hb, wb, (int)sizeof(T));
  const size_t lds = (size_t)pl.sub * pl.region * sizeof(T);
  const long long groups = (nitems + pl.sub - 1) / pl.sub, grid = groups * pl.tiles_r * pl.tiles_c;
  if (lds > (size_t)kLds2) return pthip::set_error("pthip_convolve2d_batched: %zu bytes of LDS", lds);
  if (grid > 0x7fffffffLL) return pthip::set_error("pthip_convolve2d_batched: %lld workgroups", grid);
  PTHIP_KLAUNCH(convolve2d_batched_kernel<T>, dim3((unsigned)grid), dim3(kLanes), lds, pthip::ctx().stream, (const T*)a, ha, wa, sa0, sa1,
                (const T*)b, hb, wb, sb0, sb1, bt, nitems, lo_r, lo_c, ho, wo, pl, (T*)out);
  return pthip::post_launch("convolve2d_batched");
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" int pthip_convolve1d_batched(int dtype, int nbd, const int64_t* bdims, const int64_t* bsa, const int64_t* bsb, int64_t na,
                                        const void* a, int64_t sa, int64_t nb, const void* b, int64_t sb, int full, void* out) {
  PTHIP_REQUIRE_INIT();
  const bool swap = nb > na;  // np.convolve: the first operand is the longer one
  Batch bt;
  long long nitems;
  if (int r = fill_batch("pthip_convolve1d_batched", nbd, bdims, bsa, bsb, swap, &bt, &nitems)) return r;
  if (na <= 0 || nb <= 0 || nitems == 0) return 0;
  if (swap) {
    std::swap(na, nb);
    std::swap(a, b);
    std::swap(sa, sb);
  }
  if (dtype == PTHIP_F64) return launch1<double>(a, na, sa, b, nb, sb, bt, nitems, full, out);
  if (dtype == PTHIP_F32) return launch1<float>(a, na, sa, b, nb, sb, bt, nitems, full, out);
  if (dtype == PTHIP_I64) return launch1<long long>(a, na, sa, b, nb, sb, bt, nitems, full, out);
  return pthip::set_error("pthip_convolve1d_batched: dtype %d not supported (float32/float64/int64)", dtype);
}

extern "C" int pthip_convolve2d_batched(int dtype, int nbd, const int64_t* bdims, const int64_t* bsa, const int64_t* bsb, int64_t ha,
                                        int64_t wa, const void* a, int64_t sa0, int64_t sa1, int64_t hb, int64_t wb, const void* b,
                                        int64_t sb0, int64_t sb1, int full, void* out) {
  PTHIP_REQUIRE_INIT();
  if (!full && !((ha >= hb && wa >= wb) || (hb >= ha && wb >= wa)))
    return pthip::set_error("pthip_convolve2d_batched: for 'valid' mode, one must be at least as large as the other in every dimension");
  // the image is the operand that holds the other ("valid"), or the one with more entries ("full")
  const bool swap = full ? hb * wb > ha * wa : (hb > ha || wb > wa);
  Batch bt;
  long long nitems;
  if (int r = fill_batch("pthip_convolve2d_batched", nbd, bdims, bsa, bsb, swap, &bt, &nitems)) return r;
  if (ha <= 0 || wa <= 0 || hb <= 0 || wb <= 0 || nitems == 0) return 0;
  if (ha + hb > 0x3fffffffLL || wa + wb > 0x3fffffffLL) return pthip::set_error("pthip_convolve2d_batched: operand too large");
  if (swap) {
    std::swap(ha, hb);
    std::swap(wa, wb);
    std::swap(a, b);
    std::swap(sa0, sb0);
    std::swap(sa1, sb1);
  }
  if (dtype == PTHIP_F64) return launch2<double>(a, (int)ha, (int)wa, sa0, sa1, b, (int)hb, (int)wb, sb0, sb1, bt, nitems, full, out);
  if (dtype == PTHIP_F32) return launch2<float>(a, (int)ha, (int)wa, sa0, sa1, b, (int)hb, (int)wb, sb0, sb1, bt, nitems, full, out);
  if (dtype == PTHIP_I64) return launch2<long long>(a, (int)ha, (int)wa, sa0, sa1, b, (int)hb, (int)wb, sb0, sb1, bt, nitems, full, out);
  return pthip::set_error("pthip_convolve2d_batched: dtype %d not supported (float32/float64/int64)", dtype);
}
