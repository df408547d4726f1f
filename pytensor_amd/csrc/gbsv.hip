// gbsv.hip — batched banded solves (LAPACK gbsv: LU with partial pivoting inside the band, then the substitutions).
//
// Reference: Solve(assume_a="banded") (pytensor/tensor/linalg/solvers/general.py Solve.perform ->
// scipy.linalg.solve(assume_a="banded")): scipy finds (kl, ku) from the DATA (scipy.linalg.bandwidth: exact zeros,
// a NaN counts as non-zero, -0.0 as zero), calls gbsv and ignores `lower`.  The band is data, so it is found and
// consumed on the device — two launches, no host read:
//
//   * band_scan_kernel: one launch for the whole batch.  A is read through (batch, row, column) element strides with
//     the unit-stride axis across the lanes (16-byte loads where the alignment allows); a slab of rows of one item per
//     workgroup, several workgroups per item when n is large, combined with atomicMax on two ints per item that a
//     memset in the same stream zeroed.  This pass is the HBM-bound part: n^2 elements per item.
//   * gbsv_kernel: one workgroup per item.  It reads the item's (kl, ku), copies only the band into LAPACK's working
//     band layout ((2 kl + ku + 1) x n: kl + ku super-diagonals, U fills up to that) in LDS when that fits the
//     dynamic-LDS budget, otherwise into the item's dense n x n slab of a global workspace (the same elimination code
//     through a second accessor; only band entries are copied and touched).  The right-hand sides are copied into the
//     output and carried along: interchanged and updated at every step, then substituted backwards through U.
//     A narrow band (kl < 16, kl + ku < 32) is eliminated by ONE wave, wave-synchronously, with no barrier — the other
//     waves wait once; a wide band uses all four waves with workgroup barriers.  The choice is made per item in the
//     kernel, from (kl, ku).  While (kl + 1) * nrhs <= 64 the wave also keeps the kl + 1 rows of X a step touches in
//     registers, a lane per element (kl + ku + 1 rows on the way back): a finished row is stored, the next one comes
//     from blocks fetched ahead (RowFeed), so a step waits for LDS only, never for memory.
//   * pivot = the first maximum of pivot_abs (a NaN ranks as +inf, wave_device.h) among rows k .. k+kl of
//     column k, LAPACK's idamax order; multipliers scaled by the reciprocal pivot like dgbtf2.  An exactly zero or
//     NaN pivot NaN-fills the item's solution.  Workgroups never wait for each other: no flags, no spin loops; the
//     only atomics are the scan's atomicMax.
#include "common.h"
#include "wave_device.h"

namespace {

constexpr int WG = 256;
// dynamic LDS of the band layout: what decomp.hip leaves its QR panels beside the static arrays
constexpr size_t GB_LDS_MAX = 160 * 1024 - 12 * 1024;
constexpr int NARROW_KL = 16, NARROW_KV = 32;  // kl + 1 <= 16 rows and kl + ku + 1 <= 32 columns per step: one wave

// ---- band scan ------------------------------------------------------------------------------------------------
// element (s, f) of item m at A + m*sAb + s*sS + f*sF (f: the axis across the lanes).  lo = max(s - f), hi = max(f - s)
// over the entries that are not zero (a NaN is not zero); out[2m] = max(out[2m], col_fast ? lo : hi) is kl.
template <class T, int V>
__global__ __launch_bounds__(WG) void band_scan_kernel(const T* __restrict__ A, long long sAb, long long sS, long long sF, int col_fast,
                                                      int n, int rows_per, long long chunks, long long total, int* __restrict__ out) {
  const int cpr = (n + V - 1) / V;  // lane groups per row
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long m = w / chunks;
    const int s0 = (int)(w - m * chunks) * rows_per;
    const int rows = min(rows_per, n - s0);
    const T* Am = A + m * sAb;
    int lo = 0, hi = 0;
    const int work = rows * cpr;
#pragma unroll 4
    for (int e = threadIdx.x; e < work; e += WG) {
      const int rs = e / cpr;
      const int s = s0 + rs, f0 = (e - rs * cpr) * V;
      const T* p = Am + (long long)s * sS;
      if (V > 1 && f0 + V <= n) {
        T v[V];
        if constexpr (sizeof(T) * V == 16) {
          const uint4 q = *reinterpret_cast<const uint4*>(p + f0);
          memcpy(v, &q, 16);
        }
#pragma unroll
        for (int u = 0; u < V; u++)
          if (!(v[u] == T(0))) { lo = max(lo, s - (f0 + u)); hi = max(hi, f0 + u - s); }
      } else {
        for (int f = f0; f < min(f0 + V, n); f++)
          if (!(p[(long long)f * sF] == T(0))) { lo = max(lo, s - f); hi = max(hi, f - s); }
      }
    }
    lo = wave::wave_max(lo);
    hi = wave::wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
      const int kl = col_fast ? lo : hi, ku = col_fast ? hi : lo;
      if (kl > 0) atomicMax(out + 2 * m, kl);
      if (ku > 0) atomicMax(out + 2 * m + 1, ku);
    }
  }
}

template <class T>
int band_scan_typed(long long batch, long long n, const void* A, long long sAb, long long sA0, long long sA1, int* band) {
  constexpr int V = 16 / sizeof(T);
  PTHIP_CHECK(pthip::memset_async(band, 0, (size_t)batch * 2 * sizeof(int), pthip::ctx().stream));
  const bool col_fast = sA1 == 1 || (sA0 != 1 && llabs(sA1) <= llabs(sA0));  // the column index runs across the lanes
  const long long sS = col_fast ? sA0 : sA1, sF = col_fast ? sA1 : sA0;
  const bool vec = sF == 1 && ((uintptr_t)A % 16) == 0 && sAb % V == 0 && sS % V == 0;
  long long rows_per = (16384 + n - 1) / n;  // >= 16K elements per workgroup
  if (rows_per > n) rows_per = n;
  const long long chunks = (n + rows_per - 1) / rows_per, total = batch * chunks;
  const unsigned grid = (unsigned)(total < (1LL << 20) ? total : (1LL << 20));
  if (vec)
    PTHIP_KLAUNCH((band_scan_kernel<T, V>), dim3(grid), dim3(WG), 0, pthip::ctx().stream, (const T*)A, sAb, sS, sF, (int)col_fast, (int)n,
                  (int)rows_per, chunks, total, band);
  else
    PTHIP_KLAUNCH((band_scan_kernel<T, 1>), dim3(grid), dim3(WG), 0, pthip::ctx().stream, (const T*)A, sAb, sS, sF, (int)col_fast, (int)n,
                  (int)rows_per, chunks, total, band);
  return pthip::post_launch("band_scan");
}

// ---- factor and solve -----------------------------------------------------------------------------------------
// the two homes of the working band: entry (i, j), -(kl + ku) <= i - j <= kl
template <class T> struct LdsBand {  // LAPACK's AB, column-major: AB(kv + i - j, j), ld = 2 kl + ku + 1
  T* s;
  int ld, kv;
  __device__ __forceinline__ T& at(int i, int j) const { return s[j * ld + (kv + i - j)]; }
};
template <class T> struct SlabBand {  // a dense n x n slab in global memory, band entries only
  T* w;
  long long n;
  __device__ __forceinline__ T& at(int i, int j) const { return w[i * n + j]; }
};

// one wave works wave-synchronously (program order plus a compiler fence; LDS and the L1 of the CU keep a wave's
// accesses in order); four waves meet at a workgroup barrier, whose fences also cover the right-hand sides in global memory
template <bool NARROW> __device__ __forceinline__ void gb_sync() {
  if constexpr (NARROW) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// Rows of X (n x nc) handed out one at a time, ascending (dir = +1) or descending (-1) from a first row, to the one
// wave of a narrow item: the wave fetches them rb = 64 / nc rows at a time, a lane per element and two blocks ahead of
// their use, so no step of the elimination waits for memory.  Rows outside the matrix read as zero.
template <class T> struct RowFeed {
  const T* X;
  int n, nc, rb, dir, lane;
  int row0 = 0, t = 0;  // first row (in travel order) of the block in use, rows of it handed out
  T cur = T(0), nxt = T(0);
  __device__ __forceinline__ T load(int r0) const {
    const long long e = (long long)(dir > 0 ? r0 : r0 - rb + 1) * nc + lane;
    return (lane < rb * nc && e >= 0 && e < (long long)n * nc) ? X[e] : T(0);
  }
  __device__ __forceinline__ void start(int r0) {
    row0 = r0; t = 0;
    cur = load(r0);
    nxt = load(r0 + dir * rb);
  }
  __device__ __forceinline__ T next(int c) {  // column c of the next row, every lane of the wave calling
    if (t == rb) {
      cur = nxt;
      row0 += dir * rb; t = 0;
      nxt = load(row0 + dir * rb);
    }
    const int off = dir > 0 ? t : rb - 1 - t;
    t++;
    return __shfl(cur, off * nc + c, 64);
  }
};

// P A = L U inside the band with X (n x nrhs, row-major) carried along, then U x = y.  Returns true when a pivot was
// exactly zero or NaN (the same answer in every participating thread).
template <class T, class Acc, bool NARROW>
__device__ bool gb_eliminate(const Acc M, const int n, const int kl, const int ku, T* __restrict__ X, const long long nrhs, T* s_v, int* s_i) {
  constexpr int NT = NARROW ? 64 : WG;
  const int tid = NARROW ? (threadIdx.x & 63) : threadIdx.x;
  const int kv = kl + ku;
  int ju = 0;  // the last column a row interchange has reached so far (dgbtf2's JU)
  // a narrow item with few right-hand sides keeps the rows of X that a step touches in registers, lane wr * nc + wc
  // holding (row k + wr, column wc): rows k .. k+kl going down, rows k .. k-kv coming back.  Finished rows are stored,
  // new ones come from a RowFeed.  More right-hand sides than the wave has lanes for work in memory.
  const int nc = (int)(nrhs < 64 ? nrhs : 64), wr = tid / nc, wc = tid % nc;
  const bool freg = NARROW && nrhs * (kl + 1) <= 64, breg = NARROW && nrhs * (kv + 1) <= 64;
  T wv = T(0);
  RowFeed<T> feed{X, n, nc, 64 / nc, +1, tid};
  if (freg) {
    if (wr <= kl && wr < n) wv = X[wr * nc + wc];
    feed.start(kl + 1);
  }
  for (int k = 0; k < n; k++) {
    const int km = min(kl, n - 1 - k);
    // ---- pivot: first maximum of |.| among rows k .. k+km of column k ----
    T best = T(-1);
    int bi = 0x7fffffff;
    if constexpr (NARROW) {
      // at most 16 candidates, one per lane: a butterfly over just the lanes that hold one, lane 0 tells the rest
      if (tid <= km) { best = wave::pivot_abs(M.at(k + tid, k)); bi = tid; }
      for (int o = 1; o <= km; o <<= 1) {
        const T ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      bi = __builtin_amdgcn_readfirstlane(bi);
    } else {
      for (int r = tid; r <= km; r += NT) {
        const T v = wave::pivot_abs(M.at(k + r, k));
        if (v > best) { best = v; bi = r; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = bi; }
      __syncthreads();
      best = s_v[0]; bi = s_i[0];
#pragma unroll
      for (int w = 1; w < WG / 64; w++)
        if (s_v[w] > best || (s_v[w] == best && s_i[w] < bi)) { best = s_v[w]; bi = s_i[w]; }
    }
    const int p = k + bi;
    const T piv = M.at(p, k);
    if (piv == T(0) || piv != piv) return true;
    const T rp = T(1) / piv;
    ju = max(ju, min(p + ku, n - 1));
    gb_sync<NARROW>();  // every read of column k and of the slots is behind us
    // ---- interchange rows k and p of A (columns k .. ju) ----
    if (p != k) {
      for (int j = k + tid; j <= ju; j += NT) {
        const T t = M.at(k, j);
        M.at(k, j) = M.at(p, j);
        M.at(p, j) = t;
      }
      if constexpr (!NARROW)
        for (long long c = tid; c < nrhs; c += NT) {
          const T t = X[k * nrhs + c];
          X[k * nrhs + c] = X[p * nrhs + c];
          X[p * nrhs + c] = t;
        }
      gb_sync<NARROW>();
    }
    // ---- rows k+1 .. k+km -= l * row k, l = A(i, k) / pivot (column k itself is not written) ----
    const int w = ju - k;
    for (int e = tid; e < km * w; e += NT) {
      const int r = e / w;
      const int i = k + 1 + r, j = k + 1 + (e - r * w);
      M.at(i, j) -= (M.at(i, k) * rp) * M.at(k, j);
    }
    if (freg) {
      const int pr = p - k;
      const T v0 = __shfl(wv, wc, 64), vp = __shfl(wv, pr * nc + wc, 64);  // rows k and p change places
      if (wr == 0) wv = vp;
      else if (wr == pr) wv = v0;
      if (wr >= 1 && wr <= km) wv -= (M.at(k + wr, k) * rp) * vp;
      if (wr == 0) X[k * nrhs + wc] = wv;  // row k is final
      const T up = __shfl(wv, (wr + 1) * nc + wc, 64), in = feed.next(wc);
      wv = wr == kl ? in : up;  // the window moves down one row
    } else if constexpr (NARROW) {
      // the right-hand sides in one trip to memory: a lane per (row k .. k+km, column), every load of a pass in
      // front of every store of it; row k takes row p's values and the other way round
      const int rows = km + 1, cpp = 64 / rows, r = tid / cpp;
      for (long long c0 = 0; c0 < nrhs; c0 += cpp) {
        const long long c = c0 + tid % cpp;
        const bool on = r < rows && c < nrhs;
        T v = T(0), x0 = T(0), l = T(0);
        if (on) {
          const int src = r == 0 ? p : (k + r == p ? k : k + r);
          v = X[src * nrhs + c];
          x0 = X[p * nrhs + c];
          if (r > 0) l = M.at(k + r, k) * rp;
        }
        gb_sync<true>();
        if (on) X[(k + r) * nrhs + c] = r == 0 ? v : v - l * x0;
      }
    } else {
      for (long long e = tid; e < km * nrhs; e += NT) {
        const int r = (int)(e / nrhs);
        const long long c = e - r * nrhs;
        X[(k + 1 + r) * nrhs + c] -= (M.at(k + 1 + r, k) * rp) * X[k * nrhs + c];
      }
    }
    gb_sync<NARROW>();
  }
  // ---- U x = y, column by column from the last (dtbsv): row k is final once column k+1 has been applied ----
  if (breg) {
    gb_sync<NARROW>();
    wv = (wr <= kv && wr < n) ? X[(n - 1 - wr) * nc + wc] : T(0);
    if (wr == 0) wv /= M.at(n - 1, n - 1);
    feed.dir = -1;
    feed.start(n - 2 - kv);
    for (int k = n - 1;; k--) {
      const T xk = __shfl(wv, wc, 64);
      if (wr == 0) X[k * nrhs + wc] = wv;
      if (k == 0) break;
      if (wr >= 1 && wr <= min(kv, k)) wv -= M.at(k - wr, k) * xk;
      T up = __shfl(wv, (wr + 1) * nc + wc, 64);
      const T in = feed.next(wc);
      if (wr == kv) up = in;
      if (wr == 0) up /= M.at(k - 1, k - 1);  // row k - 1 has every column of U above it applied
      wv = up;
    }
    return false;
  }
  {
    const T d = M.at(n - 1, n - 1);
    for (long long c = tid; c < nrhs; c += NT) X[(n - 1) * nrhs + c] /= d;
    gb_sync<NARROW>();
  }
  for (int k = n - 1; k > 0; k--) {
    const int lo = min(kv, k);
    const T dn = M.at(k - 1, k - 1);
    for (long long e = tid; e < max(lo, 1) * nrhs; e += NT) {  // (row k - 1 is scaled even where U has no column above it)
      const int r = (int)(e / nrhs);  // row k - 1 - r
      const long long c = e - r * nrhs;
      T v = X[(k - 1 - r) * nrhs + c];
      if (r < lo) v -= M.at(k - 1 - r, k) * X[k * nrhs + c];
      if (r == 0) v /= dn;
      X[(k - 1 - r) * nrhs + c] = v;
    }
    gb_sync<NARROW>();
  }
  return false;
}

template <class T, class Acc>
__device__ void gb_item(const Acc M, const int n, const int kl, const int ku, const T* __restrict__ A, const long long sA0, const long long sA1,
                        T* __restrict__ X, const long long nrhs, T* s_v, int* s_i, int* s_bad) {
  // ---- the band of A into the working layout (the kl + ku super-diagonals beyond ku are zeros of A) ----
  const int kv = kl + ku, W = kl + kv + 1;
  const bool rowmaj = sA1 == 1 || sA0 != 1;
  for (long long e = threadIdx.x; e < (long long)n * W; e += WG) {
    const int a = (int)(e / W), d = (int)(e - (long long)a * W);
    const int i = rowmaj ? a : a - kv + d, j = rowmaj ? a - kl + d : a;
    if (i >= 0 && i < n && j >= 0 && j < n) M.at(i, j) = A[i * sA0 + j * sA1];
  }
  __syncthreads();
  if (kl < NARROW_KL && kv < NARROW_KV) {
    if (threadIdx.x < 64) {
      const bool bad = gb_eliminate<T, Acc, true>(M, n, kl, ku, X, nrhs, s_v, s_i);
      if (threadIdx.x == 0) *s_bad = bad;
    }
  } else {
    const bool bad = gb_eliminate<T, Acc, false>(M, n, kl, ku, X, nrhs, s_v, s_i);
    if (threadIdx.x == 0) *s_bad = bad;
  }
  __syncthreads();  // (the one wait of the idle waves of a narrow item)
  if (*s_bad)
    for (long long e = threadIdx.x; e < n * nrhs; e += WG) X[e] = T(NAN);
}

template <class T>
__global__ __launch_bounds__(WG) void gbsv_kernel(int n, long long nrhs, const T* __restrict__ A, long long sAb, long long sA0, long long sA1,
                                                  const T* __restrict__ B, long long sBb, T* __restrict__ X, const int* __restrict__ band,
                                                  T* __restrict__ ws, unsigned lds_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
  __shared__ T s_v[WG / 64];
  __shared__ int s_i[WG / 64];
  __shared__ int s_bad;
  const long long m = blockIdx.x;
  const int* bw = band + (sAb == 0 ? 0 : 2 * m);  // a shared matrix was scanned once
  const int kl = min(max(bw[0], 0), n - 1), ku = min(max(bw[1], 0), n - 1);
  const T* Am = A + m * sAb;
  const T* Bm = B + m * sBb;
  T* Xm = X + m * n * nrhs;
  for (long long e = threadIdx.x; e < n * nrhs; e += WG) Xm[e] = Bm[e];
  const long long ld = 2LL * kl + ku + 1;
  if ((unsigned long long)ld * n * sizeof(T) <= lds_bytes) {
    gb_item<T>(LdsBand<T>{(T*)gb_smem, (int)ld, kl + ku}, n, kl, ku, Am, sA0, sA1, Xm, nrhs, s_v, s_i, &s_bad);
  } else if (ws != nullptr) {
    gb_item<T>(SlabBand<T>{ws + m * n * n, n}, n, kl, ku, Am, sA0, sA1, Xm, nrhs, s_v, s_i, &s_bad);
  } else {  // (pthip_gbsv_batched refuses to launch without the workspace such a band needs)
    __syncthreads();
    for (long long e = threadIdx.x; e < n * nrhs; e += WG) Xm[e] = T(NAN);
  }
}

// the widest band of an n x n matrix: kl = ku = n - 1, 3n - 2 rows
template <class T> size_t gb_worst_bytes(long long n) { return (size_t)(3 * n - 2) * (size_t)n * sizeof(T); }

template <class T>
int gbsv_typed(long long batch, long long n, long long nrhs, const void* A, long long sAb, long long sA0, long long sA1, const void* B,
               long long sBb, void* X, const int* band, void* ws, size_t ws_bytes) {
  const size_t worst = gb_worst_bytes<T>(n);
  if (worst > GB_LDS_MAX && ws_bytes < (size_t)batch * n * n * sizeof(T))
    return pthip::set_error("pthip_gbsv_batched: workspace of %zu bytes, %zu needed (pthip_gbsv_workspace)", ws_bytes,
                            (size_t)batch * n * n * sizeof(T));
  const size_t lds = worst < GB_LDS_MAX ? (worst + 15) / 16 * 16 : GB_LDS_MAX;
  auto k = gbsv_kernel<T>;
  static bool attr = false;
  if (!attr) {
    PTHIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GB_LDS_MAX));
    attr = true;
  }
  PTHIP_KLAUNCH(k, dim3((unsigned)batch), dim3(WG), lds, pthip::ctx().stream, (int)n, nrhs, (const T*)A, sAb, sA0, sA1, (const T*)B, sBb, (T*)X,
                band, worst > GB_LDS_MAX ? (T*)ws : (T*)nullptr, (unsigned)lds);
  return pthip::post_launch("gbsv_batched");
}

constexpr long long GB_MAX_N = 1 << 20, GB_MAX_BATCH = (1LL << 31) - 1;

}  // namespace

extern "C" int pthip_band_scan(int dtype, int64_t batch, int64_t n, const void* A, int64_t sAb, int64_t sA0, int64_t sA1, void* band) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || n <= 0) return 0;
  if (n > GB_MAX_N || batch > GB_MAX_BATCH) return pthip::set_error("pthip_band_scan: n = %lld, batch = %lld out of range", (long long)n, (long long)batch);
  if (dtype == PTHIP_F64) return band_scan_typed<double>(batch, n, A, sAb, sA0, sA1, (int*)band);
  if (dtype == PTHIP_F32) return band_scan_typed<float>(batch, n, A, sAb, sA0, sA1, (int*)band);
  return pthip::set_error("pthip_band_scan: dtype %d not supported (float32/float64 only)", dtype);
}

extern "C" size_t pthip_gbsv_workspace(int dtype, int64_t batch, int64_t n) {
  if (batch <= 0 || n <= 0) return 0;
  const size_t isz = dtype == PTHIP_F32 ? sizeof(float) : sizeof(double);
  const size_t worst = (size_t)(3 * n - 2) * (size_t)n * isz;
  return worst > GB_LDS_MAX ? (size_t)batch * n * n * isz : 0;
}

extern "C" int pthip_gbsv_batched(int dtype, int64_t batch, int64_t n, int64_t nrhs, const void* A, int64_t sAb, int64_t sA0, int64_t sA1,
                                  const void* B, int64_t sBb, void* X, const void* band, void* ws, size_t ws_bytes) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || n <= 0 || nrhs <= 0) return 0;
  if (n > GB_MAX_N || batch > GB_MAX_BATCH) return pthip::set_error("pthip_gbsv_batched: n = %lld, batch = %lld out of range", (long long)n, (long long)batch);
  if (dtype == PTHIP_F64) return gbsv_typed<double>(batch, n, nrhs, A, sAb, sA0, sA1, B, sBb, X, (const int*)band, ws, ws_bytes);
  if (dtype == PTHIP_F32) return gbsv_typed<float>(batch, n, nrhs, A, sAb, sA0, sA1, B, sBb, X, (const int*)band, ws, ws_bytes);
  return pthip::set_error("pthip_gbsv_batched: dtype %d not supported (float32/float64 only)", dtype);
}
