// lu_batched.hip — one-launch batched general solves and inverses for small matrices (gesv, n <= 64).
//
// Reference: Blockwise(Solve) / Blockwise(MatrixInverse) (pytensor/tensor/blockwise.py:542 loops
// scipy.linalg.solve / np.linalg.inv per item: LAPACK gesv = getrf + getrs).  lu.hip gives one
// 256-thread workgroup to each matrix and leaves the row interchanges and the two substitutions to three more
// launches; here one lane group of a wavefront owns one system from the load to the store:
//
//   * lane i of a group of G = 8 / 16 / 32 / 64 lanes keeps row i of A in registers (a[NR], NR the template tier of
//     n: every index into it is a compile-time constant) — 64 / G systems per wave, 4 waves per workgroup, the batch
//     over grid.x with a guarded tail (a wave walks the batch with a wave-uniform stride; the groups past the end
//     compute on a clamped copy of the last item and store nothing).
//   * LU with partial pivoting, implicit like getrf_reg_kernel: the rows stay in their lanes, `pos` is the row's
//     place in LAPACK's current order.  Pivot = cross-lane arg-max of pivot_abs (NaN ranks as +inf), first maximum
//     in the current order like idamax; the multipliers are scaled by the reciprocal pivot like dgetf2.
//   * once the factors are complete the rows are gathered into pivot order (lane k <- the row pivoted at column k,
//     one cross-lane move per register), so both substitutions read their pivot value from a lane that is known at
//     compile time and the right-hand sides are loaded through the permutation.
//   * right-hand sides go through the resident factors in chunks of CH columns: any nrhs, one tier.  B == nullptr
//     is the identity (the inverse).  A batch stride of 0 shares one matrix: a wave factors it once, before its walk.
//   * an exactly zero or NaN pivot NaN-fills that item's result (what getrf + two trsm give); with `status` a zero
//     pivot also raises bit 1 of the device error word (np.linalg.inv's LinAlgError).  Groups never talk to each
//     other: no barriers, no waits (LDS only hands the pivot row from one lane of a group to the others of the same
//     wave); the only atomic is that OR into the error word.
//
// The composed tier above n = 64 (getrf, this file's batched row gather, two trsm) needs P*B — or P*I — for a whole
// batch in one launch: laswp_batched_kernel.
#include "common.h"
#include "wave_device.h"

#include <type_traits>

namespace {

constexpr int WG = 256;  // 4 independent waves
constexpr int CH = 8;    // right-hand-side columns per pass through the factors

// f(integral_constant<int, I>) for I = I0 .. N-1: the column index of every step is a compile-time constant, so
// the row array is only ever indexed by constants (a loop the optimiser leaves rolled would send it to scratch)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// value of lane `src` of this lane's group.  A 64-lane group's source is wave-uniform: v_readlane, no LDS crossbar.
template <int G, class T>
__device__ __forceinline__ T group_bcast(T x, int src, int gbase) {
  if constexpr (G == 64) return wave::lane_bcast(x, __builtin_amdgcn_readfirstlane(src));
  else return __shfl(x, gbase + src, 64);
}

template <class T, int G, int NR>
__global__ __launch_bounds__(WG) void gesv_wave_kernel(long long batch, int n, long long nrhs,
                                                      const T* __restrict__ A, long long sAb, long long sA0, long long sA1,
                                                      const T* __restrict__ B, long long sBb, T* __restrict__ X,
                                                      int* __restrict__ status) {
  static_assert(NR <= G && G <= 64, "one row per lane");
  constexpr int MPW = 64 / G;  // systems per wave
  const int lane = threadIdx.x & 63, lig = lane & (G - 1), gbase = lane & ~(G - 1);
  const long long wave = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (WG / 64) * MPW;
  const bool row = lig < n;
  __shared__ __align__(16) T s_rows[(WG / G) * NR];
  T* srow = s_rows + (threadIdx.x / G) * NR;
  T a[NR];
  T dinv = T(1);
  int invp = lig;
  bool bad = false, zero = false;
  for (long long m0 = wave * MPW; m0 < batch; m0 += stride) {  // wave-uniform trip count
    const long long m = m0 + lane / G;
    const bool valid = m < batch;
    const long long mc = valid ? m : batch - 1;
    if (sAb != 0 || m0 == wave * MPW) {
      // ---- load: lane i <- row i (zero padding to NR columns; padded lanes hold a zero row) ----
      const T* Am = A + mc * sAb + (long long)lig * sA0;
      if (sA1 == 1) {  // rows contiguous: one base address, constant offsets
#pragma unroll
        for (int j = 0; j < NR; j++) a[j] = (row && j < n) ? Am[j] : T(0);
      } else {
#pragma unroll
        for (int j = 0; j < NR; j++) a[j] = (row && j < n) ? Am[j * sA1] : T(0);
      }
      int pos = lig;
      bad = false; zero = false; dinv = T(1);
      // ---- P A = L U, rows in place ----
      static_for<0, NR>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if (k >= n) return;
        T v = (row && pos >= k) ? wave::pivot_abs(a[k]) : T(-1);
        int key = (pos << 6) | lig;
#pragma unroll
        for (int ob = 0; (1 << ob) < G; ob++) {
          const int o = 1 << ob;
          const T ov = __shfl_xor(v, o, 64);
          const int ok = __shfl_xor(key, o, 64);
          if (ov > v || (ov == v && ok < key)) { v = ov; key = ok; }
        }
        const int rho = key & 63, q = key >> 6;
        // the pivot row goes through this group's LDS slot: one lane writes, every lane reads the same addresses
        // (a broadcast read).  Same wave on both sides, so program order is the only synchronisation needed.
        if (lig == rho) {
#pragma unroll
          for (int j = k; j < NR; j++) srow[j] = a[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const T piv = srow[k];
        zero |= piv == T(0);
        bad |= piv == T(0) || piv != piv;
        const T rp = piv == T(0) ? T(1) : T(1) / piv;
        if (pos == k) pos = q;  // LAPACK's interchange k <-> q
        if (lig == rho) { pos = k; dinv = rp; }
        const T l = pos > k ? a[k] * rp : T(0);  // (a padded lane: a[k] = 0)
        if (pos > k) a[k] = l;
#pragma unroll
        for (int j = k + 1; j < NR; j++) a[j] -= l * srow[j];
        // (the next column's write of the slot stays behind these reads)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      });
      // ---- gather the rows into pivot order: lane k <- the lane whose row sits at position k ----
      invp = __builtin_amdgcn_ds_permute((gbase + pos) << 2, lig);  // pos is a permutation of the group's lanes
#pragma unroll
      for (int j = 0; j < NR; j++) a[j] = __shfl(a[j], gbase + invp, 64);
      dinv = __shfl(dinv, gbase + invp, 64);
    }
    if (zero && valid && lig == 0 && status != nullptr) atomicOr(status, 2);
    // ---- right-hand sides, CH columns at a time: lane k <- row invp of B, solves, lane k -> row k of X ----
    const T* Bm = B == nullptr ? nullptr : B + mc * sBb + (long long)invp * nrhs;
    T* Xm = X + (mc * n + lig) * nrhs;
    for (long long c0 = 0; c0 < nrhs; c0 += CH) {
      T b[CH];
      // the triangle masks below are rebuilt from this copy in every pass: as loop invariants the optimiser would keep
      // a masked copy of L, of U and of the diagonal scale alive next to the factors (three times the registers)
      int li = lig;
      asm volatile("" : "+v"(li));
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const long long col = c0 + c;
        const bool in = row && col < nrhs;
        b[c] = !in ? T(0) : (Bm != nullptr ? Bm[col] : (col == invp ? T(1) : T(0)));
      }
      static_for<0, NR>([&](auto kc) {  // L y = P b (unit diagonal)
        constexpr int k = decltype(kc)::value;
        if (k + 1 >= n) return;
        const T l = li > k ? a[k] : T(0);
#pragma unroll
        for (int c = 0; c < CH; c++) b[c] -= l * group_bcast<G>(b[c], k, gbase);
      });
      static_for<0, NR>([&](auto kc) {  // U x = y, last column first
        constexpr int k = NR - 1 - decltype(kc)::value;
        if (k >= n) return;
        const T s = li == k ? dinv : T(1);
        const T u = li < k ? a[k] : T(0);
#pragma unroll
        for (int c = 0; c < CH; c++) {
          b[c] *= s;
          b[c] -= u * group_bcast<G>(b[c], k, gbase);
        }
      });
      if (valid && row) {
#pragma unroll
        for (int c = 0; c < CH; c++)
          if (c0 + c < nrhs) Xm[c0 + c] = bad ? T(NAN) : b[c];
      }
    }
  }
}

template <class T, int G, int NR>
int launch_gesv(long long batch, long long n, long long nrhs, const void* A, long long sAb, long long sA0, long long sA1,
                const void* B, long long sBb, void* X, int flag_singular) {
  const long long per_wg = (WG / 64) * (64 / G);
  long long grid = (batch + per_wg - 1) / per_wg;
  if (grid > 8192) grid = 8192;  // (256 CUs x up to 8 workgroups of 4 waves; longer batches are walked)
  PTHIP_KLAUNCH((gesv_wave_kernel<T, G, NR>), dim3((unsigned)grid), dim3(WG), 0, pthip::ctx().stream, batch, (int)n, nrhs,
                (const T*)A, sAb, sA0, sA1, (const T*)B, sBb, (T*)X, flag_singular ? (int*)pthip_status_ptr() : (int*)nullptr);
  return pthip::post_launch("gesv_batched");
}

template <class T>
int gesv_typed(long long batch, long long n, long long nrhs, const void* A, long long sAb, long long sA0, long long sA1,
               const void* B, long long sBb, void* X, int flag_singular) {
#define PTHIP_GESV_TIER(G, NR) \
  if (n <= NR) return launch_gesv<T, G, NR>(batch, n, nrhs, A, sAb, sA0, sA1, B, sBb, X, flag_singular)
  PTHIP_GESV_TIER(8, 4);
  PTHIP_GESV_TIER(8, 8);
  PTHIP_GESV_TIER(16, 16);
  PTHIP_GESV_TIER(32, 24);
  PTHIP_GESV_TIER(32, 32);
  PTHIP_GESV_TIER(64, 48);
  PTHIP_GESV_TIER(64, 64);
#undef PTHIP_GESV_TIER
  return pthip::set_error("pthip_gesv_batched: n = %lld is beyond the wave tier (n <= 64)", n);
}

// out[m] (n x nrhs) = rows perm[m] of B[m] (P*B of pthip_getrf's gather vector, sPb = 0: one for all); B == nullptr:
// of the identity
template <class T>
__global__ __launch_bounds__(WG) void laswp_batched_kernel(T* __restrict__ out, const T* __restrict__ B, long long sBb,
                                                          const long long* __restrict__ perm, long long sPb, long long n,
                                                          long long nrhs, long long total) {
  const long long per = n * nrhs;
  for (long long e = (long long)blockIdx.x * WG + threadIdx.x; e < total; e += (long long)gridDim.x * WG) {
    const long long m = e / per, r = (e - m * per) / nrhs, c = e - m * per - r * nrhs;
    long long src = perm[m * sPb + r];
    if (src < 0 || src >= n) src = r;  // (a gather vector of pthip_getrf never is; keeps a foreign one in bounds)
    out[e] = B != nullptr ? B[m * sBb + src * nrhs + c] : (src == c ? T(1) : T(0));
  }
}

template <class T>
int laswp_typed(long long batch, long long n, long long nrhs, const void* B, long long sBb, const void* perm, long long sPb,
                void* out) {
  const long long total = batch * n * nrhs;
  long long grid = (total + WG - 1) / WG;
  if (grid > 16384) grid = 16384;
  PTHIP_KLAUNCH((laswp_batched_kernel<T>), dim3((unsigned)grid), dim3(WG), 0, pthip::ctx().stream, (T*)out, (const T*)B, sBb,
                (const long long*)perm, sPb, n, nrhs, total);
  return pthip::post_launch("laswp_batched");
}

}  // namespace

extern "C" int pthip_gesv_batched(int dtype, int64_t batch, int64_t n, int64_t nrhs, const void* A, int64_t sAb, int64_t sA0,
                                  int64_t sA1, const void* B, int64_t sBb, void* X, int flag_singular) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || n <= 0 || nrhs <= 0) return 0;
  if (dtype == PTHIP_F64) return gesv_typed<double>(batch, n, nrhs, A, sAb, sA0, sA1, B, sBb, X, flag_singular);
  if (dtype == PTHIP_F32) return gesv_typed<float>(batch, n, nrhs, A, sAb, sA0, sA1, B, sBb, X, flag_singular);
  return pthip::set_error("pthip_gesv_batched: dtype %d not supported (float32/float64 only)", dtype);
}

extern "C" int pthip_laswp_batched(int dtype, int64_t batch, int64_t n, int64_t nrhs, const void* B, int64_t sBb,
                                   const void* perm, int64_t sPb, void* out) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || n <= 0 || nrhs <= 0) return 0;
  if (dtype == PTHIP_F64) return laswp_typed<double>(batch, n, nrhs, B, sBb, perm, sPb, out);
  if (dtype == PTHIP_F32) return laswp_typed<float>(batch, n, nrhs, B, sBb, perm, sPb, out);
  return pthip::set_error("pthip_laswp_batched: dtype %d not supported (float32/float64 only)", dtype);
}
