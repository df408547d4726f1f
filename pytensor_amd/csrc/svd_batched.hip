// svd_batched.hip — one-launch batched Jacobi SVD / pseudo-inverse for small matrices (gesvj, max(m, n) <= 64).
//
// Reference: Blockwise(SVD) / Blockwise(MatrixPinv) (pytensor/tensor/blockwise.py:542 loops np.linalg.svd /
// np.linalg.pinv per item).  decomp.hip's svd_rows_kernel gives a 1024-thread workgroup to each matrix and leaves
// the completion of the factors to three more launches; here one lane group of a wavefront owns one matrix from the
// load to the store, in the idiom of lu_batched.hip:
//
//   * work happens in the wide orientation X (r x c, r <= c); a tall input is read transposed by swapping its two
//     strides.  Lane i of a group of G = 8 / 16 / 32 / 64 lanes keeps row i of X in registers (x[NR], NR the template
//     tier of c: every index is a compile-time constant) and, when vectors are wanted, row i of the rotation
//     accumulator (v[min(G, NR)]) — 64 / G matrices per wave, 4 waves per workgroup, the batch over grid.x with a
//     guarded tail (a wave walks the batch with a wave-uniform stride; the groups past the end compute on a clamped
//     copy of the last item and store nothing).
//   * one-sided Jacobi (Hestenes) on the rows: one round of the round-robin tournament pairs lanes p and q; each
//     fetches its partner's row through cross-lane moves and forms the dot product locally (both lanes add the same
//     products in the same order: the same bits), then applies its half of the rotation.  All r / 2 pairs of a round
//     rotate in the same instructions; no reduction.  The squared norms ride along (a' = a - t g, b' = b + t g; a
//     fresh sum when a row shrinks below 1 % of its old norm, and at the start of every sweep).
//   * rotate when |g| > tol sqrt(a b), tol = eps sqrt(c) as in LAPACK's gesvj: the computed dot product of two rows of
//     length c carries a rounding error of that order, and a threshold below it can rotate a pair back and forth for
//     ever (with the bare eps of svd_rows_kernel one 64 x 64 Gaussian item of 256 did, up to the 60-sweep cap, in the
//     instance with vectors and not in the one without).  A group is done when a whole sweep rotated nothing and then
//     rotates nothing more (the sweep loop is wave-uniform: it runs while any group of the wave is not done, so what a
//     group computes never depends on its neighbours).  60 sweeps without convergence raise bit 2 (value 4) of the
//     device error word.
//   * singular values = row norms, ranked descending, ties by position: each lane counts the rows that outrank its
//     own and stores through that rank.
//   * completion inside the group: a row with s == 0 — and under job 2 the c - r complementary rows, kept by the
//     lanes r .. c-1 (the group is then sized by c) — is a unit vector e_t orthogonalised twice against the rows
//     present (classical Gram-Schmidt with one re-orthogonalisation; the projection is a butterfly sum over the
//     group) and kept when its remainder has squared norm > 1 / (4 c): one pass over t = 0 .. c-1 fills every row,
//     because the remainders of the unit vectors cannot all be that short while a direction is missing.
//   * job 3: pinv = sum_i w_i (1 / s_i where s_i > rcond s_max) p_i^T, a butterfly sum over the group per entry.
//   * an item that holds a NaN or an Inf is all NaN in every output and is done before the first sweep.
// Groups never talk to each other: no barriers, no waits; the only atomic is the OR into the error word.  No LDS
// either, but for one instance (acc_in_lds below).  Every instance builds without scratch (profiles/svd_batched.md).
#include "common.h"
#include "wave_device.h"

namespace {

constexpr int WG = 256;  // 4 independent waves
constexpr int MAX_SWEEPS = 60;

// The float64 instance with 64 rows of 64 and vectors would need row + accumulator = 256 registers before anything is
// computed: its accumulator lives in LDS instead (acc[k][lane], 32 KiB: own and partner's element are both plain reads,
// conflict-free), one wave per workgroup.  Same wave on both sides of every exchange: program order is the only
// synchronisation needed.
template <class T, int G, int NR, bool VEC>
constexpr bool acc_in_lds() { return VEC && sizeof(T) == 8 && G == 64 && NR == 64; }
template <class T, int G, int NR, bool VEC>
constexpr int block_size() { return acc_in_lds<T, G, NR, VEC>() ? 64 : WG; }

template <class T, int G, int NR, bool VEC>
__global__ __launch_bounds__((block_size<T, G, NR, VEC>())) void gesvj_wave_kernel(long long batch, int m, int n, int job, const T* __restrict__ A,
                                                       long long sAb, long long sA0, long long sA1, T rcond,
                                                       T* __restrict__ U, T* __restrict__ S, T* __restrict__ Vt,
                                                       T* __restrict__ Pinv, int* __restrict__ status) {
  static_assert(G <= 64 && (G & (G - 1)) == 0, "a lane group is a power of two");
  constexpr int MPW = 64 / G;                           // matrices per wave
  constexpr bool VLDS = acc_in_lds<T, G, NR, VEC>();
  constexpr int BS = block_size<T, G, NR, VEC>();
  constexpr int NV = (VEC && !VLDS) ? (G < NR ? G : NR) : 1;  // r <= min(G, NR)
  __shared__ T acc[VLDS ? 64 * 64 : 1];
  // the partner's row stays in registers between the dot product and the rotation, except where row + accumulator +
  // partner would not fit the 512 registers of a lane (float64 rows of 64 with vectors): there it is fetched twice
  constexpr bool KEEP = !(VEC && sizeof(T) * NR >= 512);
  const int lane = threadIdx.x & 63, lig = lane & (G - 1), gbase = lane & ~(G - 1);
  const long long wave = (long long)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (BS / 64) * MPW;
  const bool tall = m >= n;
  const int r = tall ? n : m, c = tall ? m : n;
  const long long sR = tall ? sA1 : sA0, sC = tall ? sA0 : sA1;
  const int R = (r + 1) & ~1;  // players (one bye when r is odd)
  const unsigned long long gmask = G == 64 ? ~0ull : (((1ull << (G & 63)) - 1ull) << gbase);
  const T tol = (sizeof(T) == 8 ? T(2.220446049250313e-16) : T(1.1920929e-07)) * sqrt(T(c));
  const bool row = lig < r;
  for (long long m0 = wave * MPW; m0 < batch; m0 += stride) {  // wave-uniform trip count
    const long long item = m0 + lane / G;
    const bool valid = item < batch;
    const long long mc = valid ? item : batch - 1;
    // ---- load: lane i <- row i of X (zero padding to NR columns; lanes past r hold a zero row) ----
    T x[NR];
    T v[NV];
    const T* Am = A + mc * sAb + (long long)lig * sR;
    // (the column stride is made opaque per item: as a loop invariant of the batch walk the optimiser would keep the NR
    //  element offsets alive in registers through the whole kernel)
    long long sCi = sC;
    asm volatile("" : "+s"(sCi));
    bool fin = true;
#pragma unroll
    for (int j = 0; j < NR; j++) {
      x[j] = (row && j < c) ? Am[j * sCi] : T(0);
      fin = fin && (x[j] - x[j] == T(0));
    }
    const bool bad = (__ballot(!fin) & gmask) != 0;
    if constexpr (VLDS) {
      for (int k = 0; k < r; k++) acc[k * 64 + lane] = k == lane ? T(1) : T(0);
    } else if constexpr (VEC) {
      int li = lig;  // (opaque per item, for the same reason: the identity's rows are no loop invariant to keep)
      asm volatile("" : "+v"(li));
#pragma unroll
      for (int k = 0; k < NV; k++) v[k] = k == li ? T(1) : T(0);
    }
    // ---- sweeps ----
    bool done = bad || r < 2;
    for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
      if (__ballot(!done) == 0) break;
      T n2 = T(0);
#pragma unroll
      for (int j = 0; j < NR; j++) n2 += x[j] * x[j];
      bool rotated = false;
      for (int step = 0; step < R - 1; step++) {
        int partner;
        if (lig >= R) partner = lig;
        else if (lig == R - 1) partner = step;
        else if (lig == step) partner = R - 1;
        else {
          partner = 2 * step - lig;
          if (partner < 0) partner += R - 1;
          if (partner >= R - 1) partner -= R - 1;
        }
        const bool real = !done && row && partner < r && partner != lig;
        const int src = gbase + partner;
        T xp[KEEP ? NR : 1];
        T g = T(0);
#pragma unroll
        for (int j = 0; j < NR; j++) {
          const T p = __shfl(x[j], src, 64);
          if constexpr (KEEP) xp[j] = p;
          g += x[j] * p;
          if constexpr (!KEEP) if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // (bounds the cross-lane moves in flight)
        }
        const T pn2 = __shfl(n2, src, 64);
        const bool low = lig < partner;
        const T a = low ? n2 : pn2, b = low ? pn2 : n2;
        bool rotate = real && g != T(0) && wave::dev_abs(g) > tol * sqrt(a) * sqrt(b);
        const T gs = rotate ? g : T(1);
        const T zeta = (b - a) / (T(2) * gs);
        const T tt = (zeta >= T(0) ? T(1) : T(-1)) / (wave::dev_abs(zeta) + sqrt(T(1) + zeta * zeta));
        rotate = rotate && tt != T(0) && tt == tt;  // (t underflowed: nothing to do, and nothing that counts as a rotation)
        const T cs = T(1) / sqrt(T(1) + tt * tt);
        const T sn = low ? -(cs * tt) : cs * tt;  // p' = c p - s q, q' = s p + c q
#pragma unroll
        for (int j = 0; j < NR; j++) {
          T p;
          if constexpr (KEEP) p = xp[j];
          else p = __shfl(x[j], src, 64);  // (every lane reads the partner's old value before any lane writes its new one)
          x[j] = rotate ? cs * x[j] + sn * p : x[j];
          if constexpr (!KEEP) if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (VLDS) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          for (int k0 = 0; k0 < r; k0 += 8) {  // (8 elements of both rows are read before any is written)
            T mine[8], his[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
              mine[k] = acc[(k0 + k) * 64 + lane];
              his[k] = acc[(k0 + k) * 64 + src];
            }
#pragma unroll
            for (int k = 0; k < 8; k++)
              if (rotate) acc[(k0 + k) * 64 + lane] = cs * mine[k] + sn * his[k];
          }
        } else if constexpr (VEC) {
#pragma unroll
          for (int k = 0; k < NV; k++) {
            const T vp = __shfl(v[k], src, 64);
            v[k] = rotate ? cs * v[k] + sn * vp : v[k];
            if constexpr (!KEEP) if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
          }
        }
        if (rotate) {
          T nn = low ? a - tt * g : b + tt * g;
          if (!(nn > T(0.01) * n2)) {  // (cancellation: summed again from the rotated row)
            nn = T(0);
#pragma unroll
            for (int j = 0; j < NR; j++) nn += x[j] * x[j];
          }
          n2 = nn;
          rotated = true;
        }
      }
      if (!done) done = (__ballot(rotated) & gmask) == 0;
    }
    if (!done && valid && lig == 0 && status != nullptr) atomicOr(status, 4);
    // ---- singular values: row norms, ranked descending, ties by position ----
    T s2 = T(0);
#pragma unroll
    for (int j = 0; j < NR; j++) s2 += x[j] * x[j];
    const T s = sqrt(s2);
    int rank = 0;
    for (int j = 0; j < r; j++) {
      const T sj = __shfl(s, gbase + j, 64);
      rank += (sj > s || (sj == s && j < lig)) ? 1 : 0;
    }
    if (bad || !row) rank = lig;
    const T nan = T(NAN);
    if (valid && row && job != 3) S[mc * r + rank] = bad ? nan : s;  // (job 3 has no S: the pointer may be null)
    if constexpr (VEC) {
      const T inv = s > T(0) ? T(1) / s : T(0);
#pragma unroll
      for (int j = 0; j < NR; j++) x[j] = bad ? T(0) : x[j] * inv;
      if (job == 3) {
        // ---- pinv[j, k] = sum_i w_i[j] sinv_i p_i[k] ----
        T smax = s;
#pragma unroll
        for (int o = 1; o < G; o <<= 1) { const T t = __shfl_xor(smax, o, 64); smax = t > smax ? t : smax; }
        const T sinv = (row && !bad && s > rcond * smax) ? inv : T(0);
        T* P = Pinv + mc * (long long)m * n;
        for (int k = 0; k < r; k++) {
          T vk = T(0);
          if constexpr (VLDS) vk = acc[k * 64 + lane];
          else {
#pragma unroll
            for (int kk = 0; kk < NV; kk++) vk = kk == k ? v[kk] : vk;
          }
          const T cf = bad ? T(0) : vk * sinv;
#pragma unroll
          for (int j = 0; j < NR; j++) {
            if (j < c) {  // (wave-uniform)
              const T y = wave::group_sum<G>(cf * x[j]);
              if (valid && lig == (j & (G - 1))) P[tall ? (long long)k * c + j : (long long)j * r + k] = bad ? nan : y;
            }
          }
        }
      } else {
        // ---- completion: rows with s == 0, and under job 2 the rows r .. c-1 ----
        const int rows = job == 2 ? c : r;
        bool active = row && !bad && s > T(0);
        bool needy = !bad && lig < rows && !active;
        const T thr = T(0.25) / T(c);
        // the rotation accumulator goes out first, in its final layout (wide: U = P, m x m; tall: Vt = P^T, n x n): the
        // completion then has its registers for the candidate vector
        if (valid && row) {
          T* Pm = (tall ? Vt : U) + mc * (long long)r * r;
          if constexpr (VLDS) {
            for (int k = 0; k < r; k++) Pm[tall ? (long long)rank * r + k : (long long)k * r + rank] = bad ? nan : acc[k * 64 + lane];
          } else {
#pragma unroll
            for (int k = 0; k < NV; k++)
              if (k < r) Pm[tall ? (long long)rank * r + k : (long long)k * r + rank] = bad ? nan : v[k];
          }
        }
        for (int t = 0; t < c; t++) {
          const unsigned long long need = __ballot(needy);
          if (need == 0) break;
          T u[NR];
#pragma unroll
          for (int j = 0; j < NR; j++) u[j] = j == t ? T(1) : T(0);
          for (int pass = 0; pass < 2; pass++) {
            T d = T(0);
#pragma unroll
            for (int j = 0; j < NR; j++) d += x[j] * u[j];
            if (!active) d = T(0);
#pragma unroll
            for (int j = 0; j < NR; j++) {
              if (j < c) u[j] -= wave::group_sum<G>(active ? d * x[j] : T(0));
            }
          }
          T nu = T(0);
#pragma unroll
          for (int j = 0; j < NR; j++) nu += u[j] * u[j];
          const unsigned long long mine = need & gmask;
          const int first = mine == 0 ? -1 : __ffsll((long long)mine) - 1 - gbase;
          if (nu > thr && lig == first) {
            const T sc = T(1) / sqrt(nu);
#pragma unroll
            for (int j = 0; j < NR; j++) x[j] = u[j] * sc;
            active = true;
            needy = false;
          }
        }
        // ---- the completed rows, in their final layout ----
        if (valid && lig < rows) {
          if (!tall) {  // x = X: Vt = Wt (rows x n)
            T* Vm = Vt + (mc * rows + rank) * (long long)c;
#pragma unroll
            for (int j = 0; j < NR; j++)
              if (j < c) Vm[j] = bad ? nan : x[j];
          } else {  // x = X^T: U = Wt^T (m x rows)
            T* Um = U + mc * (long long)c * rows + rank;
#pragma unroll
            for (int j = 0; j < NR; j++)
              if (j < c) Um[(long long)j * rows] = bad ? nan : x[j];
          }
        }
      }
    }
  }
}

template <class T, int G, int NR>
int launch_gesvj(long long batch, int m, int n, int job, const void* A, long long sAb, long long sA0, long long sA1,
                 double rcond, void* U, void* S, void* Vt, void* Pinv) {
  constexpr int BS = block_size<T, G, NR, true>();  // (of the instance with vectors; the other keeps WG)
  const long long per_wg = ((job == 0 ? WG : BS) / 64) * (64 / G);
  long long grid = (batch + per_wg - 1) / per_wg;
  if (grid > 8192) grid = 8192;  // (longer batches are walked)
  int* status = (int*)pthip_status_ptr();
  if (job == 0)
    PTHIP_KLAUNCH((gesvj_wave_kernel<T, G, NR, false>), dim3((unsigned)grid), dim3(WG), 0, pthip::ctx().stream, batch, m, n, job,
                  (const T*)A, sAb, sA0, sA1, (T)rcond, (T*)U, (T*)S, (T*)Vt, (T*)Pinv, status);
  else
    PTHIP_KLAUNCH((gesvj_wave_kernel<T, G, NR, true>), dim3((unsigned)grid), dim3(BS), 0, pthip::ctx().stream, batch, m, n, job,
                  (const T*)A, sAb, sA0, sA1, (T)rcond, (T*)U, (T*)S, (T*)Vt, (T*)Pinv, status);
  return pthip::post_launch("gesvj_batched");
}

template <class T>
int gesvj_typed(long long batch, int m, int n, int job, const void* A, long long sAb, long long sA0, long long sA1, double rcond,
                void* U, void* S, void* Vt, void* Pinv) {
  const int r = m < n ? m : n, c = m < n ? n : m;
  const int players = (r + 1) & ~1;
  const int lanes = (job == 2 && c > players) ? c : players;  // the complementary rows of job 2 live in lanes r .. c-1
#define PTHIP_GESVJ_TIER(G, NR) \
  if (lanes <= G && c <= NR) return launch_gesvj<T, G, NR>(batch, m, n, job, A, sAb, sA0, sA1, rcond, U, S, Vt, Pinv)
  PTHIP_GESVJ_TIER(8, 4);
  PTHIP_GESVJ_TIER(8, 8);
  PTHIP_GESVJ_TIER(8, 16);
  PTHIP_GESVJ_TIER(16, 16);
  PTHIP_GESVJ_TIER(8, 32);
  PTHIP_GESVJ_TIER(16, 32);
  PTHIP_GESVJ_TIER(32, 32);
  PTHIP_GESVJ_TIER(8, 64);
  PTHIP_GESVJ_TIER(16, 64);
  PTHIP_GESVJ_TIER(32, 64);
  PTHIP_GESVJ_TIER(64, 64);
#undef PTHIP_GESVJ_TIER
  return pthip::set_error("pthip_gesvj_batched: max(m, n) = %d is beyond the wave tier (<= 64)", c);
}

}  // namespace

extern "C" int pthip_gesvj_batched(int dtype, int64_t batch, int64_t m, int64_t n, int job, const void* A, int64_t sAb,
                                   int64_t sA0, int64_t sA1, double rcond, void* U, void* S, void* Vt, void* pinv) {
  PTHIP_REQUIRE_INIT();
  if (batch <= 0 || m <= 0 || n <= 0) return 0;
  if (job < 0 || job > 3) return pthip::set_error("pthip_gesvj_batched: job %d (0 = S, 1 = economic, 2 = full, 3 = pinv)", job);
  if (m > 64 || n > 64) return pthip::set_error("pthip_gesvj_batched: max(m, n) = %lld is beyond the wave tier (<= 64)", (long long)(m > n ? m : n));
  if (dtype == PTHIP_F64) return gesvj_typed<double>(batch, (int)m, (int)n, job, A, sAb, sA0, sA1, rcond, U, S, Vt, pinv);
  if (dtype == PTHIP_F32) return gesvj_typed<float>(batch, (int)m, (int)n, job, A, sAb, sA0, sA1, rcond, U, S, Vt, pinv);
  return pthip::set_error("pthip_gesvj_batched: dtype %d not supported (float32/float64 only)", dtype);
}
