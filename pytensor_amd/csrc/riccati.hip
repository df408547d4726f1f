// riccati.hip — discrete algebraic Riccati equation A^T X A - X - A^T X B (R + B^T X B)^-1 B^T X A + Q = 0.
//
// Reference: SolveDiscreteARE (pytensor/tensor/linalg/solvers/linear_control.py: the QR-compressed
// extended pencil, QZ with sort="iuc", then U10 U00^-1, symmetrised; NaN when U00^T U10 is not
// symmetric).  The stabilising solution is unique, so it is computed here by the structure-preserving
// doubling algorithm (SDA; Chu, Fan, Lin & Wang 2004), which needs products and one LU per step and no
// eigen-decomposition:
//
//   A0 = A, G0 = B R^-1 B^T, H0 = Q, W = I + Gk Hk
//   A(k+1) = Ak W^-1 Ak,  G(k+1) = Gk + Ak W^-1 Gk Ak^T,  H(k+1) = Hk + Ak^T Hk W^-1 Ak
//   X = (H + H^T) / 2
//
// Ak is the closed loop raised to the power 2^k, so it tends to 0 exactly when the solution is
// stabilising; when it does not (an unstabilisable pair, an undetectable one where H would stall at a
// non-stabilising solution) it grows or stays O(1).  A step is converged when
//   max|dH| <= m eps max|H|  and  max|A(k+1)| <= sqrt(eps) max|A0|
// and the iteration stops there.  No convergence within DARE_MAX_STEPS, any non-finite value, or an
// exactly zero pivot in R or W gives an all-NaN X (DESIGN §4 "Riccati").
//
// Single-launch tier (pthip_dare): one workgroup of 256 threads per DARE (the batch is grid.x), the whole
// iteration in one kernel with no host round trip.  Everything is computed in fp64 whatever the I/O
// dtype (the reference's graph returns float64 for float32 operands).  Six m x m working matrices (A, G, H, W / its LU, W^-1 A, W^-1 G; the products reuse the dead
// slots) live in the LDS when they fit (leading dimension m|1: m <= 57), otherwise in an L2-resident
// per-item global workspace the caller passes (pthip_dare_workspace).  m <= 64, n <= m; n = 0 (G0 = 0) is the
// Stein equation X = A^T X A + Q, which the same iteration solves (Smith's doubling).
//
// The composed tier for larger m (dispatch/riccati.py) runs a fixed number of doubling steps out of the
// library's GEMM / LU kernels and ends with pthip_dare_finish, which applies the same convergence test
// to the last step on the device.
#include "common.h"
#include "wave_device.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int DARE_BLOCK = 256;
constexpr int DARE_WAVES = DARE_BLOCK / 64;
constexpr int DARE_MAX_M = 64;
constexpr int DARE_MAX_STEPS = 48;
constexpr double DARE_EPS = 2.220446049250313e-16;
constexpr double DARE_SQRT_EPS = 1.4901161193847656e-08;

// block-wide NaN-propagating max of four values at once (every thread gets the results)
__device__ void block_max4(double (&v)[4], double (*red)[DARE_WAVES]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    v[q] = wave::wave_nan_max(v[q]);
    if (lane == 0) red[q][wid] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; q++) {
    v[q] = red[q][0];
    for (int w = 1; w < DARE_WAVES; w++) v[q] = wave::nan_max(v[q], red[q][w]);
  }
  __syncthreads();
}

// C (M x N, ld ldc) <- [C +] X Y with X(i, k) = X[i xs0 + k xs1], Y(k, j) = Y[k ys0 + j ys1].  C is neither
// X nor Y.  Returns this thread's max|X Y| (the increment) and max|C| after the update.
__device__ void mm(double* C, int ldc, const double* X, int xs0, int xs1, const double* Y, int ys0, int ys1, int M, int N,
                   int K, bool acc, double& inc_max, double& c_max) {
  for (int e = threadIdx.x; e < M * N; e += DARE_BLOCK) {
    const int i = e / N, j = e - i * N;
    const double* x = X + i * xs0;
    const double* y = Y + j * ys1;
    double s = 0.0;
    for (int k = 0; k < K; k++) s = fma(x[k * xs1], y[k * ys0], s);
    const double c = acc ? C[i * ldc + j] + s : s;
    C[i * ldc + j] = c;
    inc_max = wave::nan_max(inc_max, fabs(s));
    c_max = wave::nan_max(c_max, fabs(c));
  }
}

// in-place LU with partial pivoting of the N x N matrix W (ld), N <= 64: row interchanges in piv.
// Returns false on an exactly zero (or non-finite) pivot.
__device__ bool lu_inplace(double* W, int ld, int N, int* piv, int* s_p) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int k = 0; k < N; k++) {
    if (wid == 0) {
      double v = (lane >= k && lane < N) ? fabs(W[lane * ld + k]) : -1.0;
      if (v != v) v = INFINITY;  // (a NaN pivot candidate fails the factorisation below)
      int idx = lane;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > v || (ov == v && oi < idx)) {
          v = ov;
          idx = oi;
        }
      }
      if (lane == 0) {
        piv[k] = idx;
        *s_p = (v > 0.0 && v <= DBL_MAX) ? idx : -1;
      }
    }
    __syncthreads();
    const int p = *s_p;
    if (p < 0) return false;  // (uniform: every thread read the same shared value)
    if (p != k)
      for (int j = tid; j < N; j += DARE_BLOCK) {
        const double t = W[k * ld + j];
        W[k * ld + j] = W[p * ld + j];
        W[p * ld + j] = t;
      }
    __syncthreads();
    const double rinv = 1.0 / W[k * ld + k];
    for (int i = k + 1 + tid; i < N; i += DARE_BLOCK) W[i * ld + k] *= rinv;
    __syncthreads();
    const int nt = N - k - 1;
    for (int e = tid; e < nt * nt; e += DARE_BLOCK) {
      const int i = k + 1 + e / nt, j = k + 1 + e % nt;
      W[i * ld + j] = fma(-W[i * ld + k], W[k * ld + j], W[i * ld + j]);
    }
    __syncthreads();
  }
  return true;
}

// Solve (LU of W, N x N) Y = RHS in place for RHS = [Y1 | Y2] (N x c1 and N x c2, both ld).
__device__ void lu_solve(const double* W, int ld, int N, const int* piv, double* Y1, int c1, double* Y2, int c2) {
  const int tid = threadIdx.x, nc = c1 + c2;
  auto col = [&](int c) -> double* { return c < c1 ? Y1 + c : Y2 + (c - c1); };
  for (int c = tid; c < nc; c += DARE_BLOCK) {
    double* y = col(c);
    for (int k = 0; k < N; k++) {
      const int p = piv[k];
      if (p != k) {
        const double t = y[k * ld];
        y[k * ld] = y[p * ld];
        y[p * ld] = t;
      }
    }
  }
  __syncthreads();
  for (int k = 0; k < N - 1; k++) {  // unit lower
    const int nr = N - k - 1;
    for (int e = tid; e < nr * nc; e += DARE_BLOCK) {
      const int i = k + 1 + e / nc, c = e % nc;
      double* y = col(c);
      y[i * ld] = fma(-W[i * ld + k], y[k * ld], y[i * ld]);
    }
    __syncthreads();
  }
  for (int k = N - 1; k >= 0; k--) {  // upper
    const double dinv = 1.0 / W[k * ld + k];
    for (int c = tid; c < nc; c += DARE_BLOCK) col(c)[k * ld] *= dinv;
    __syncthreads();
    for (int e = tid; e < k * nc; e += DARE_BLOCK) {
      const int i = e / nc, c = e % nc;
      double* y = col(c);
      y[i * ld] = fma(-W[i * ld + k], y[k * ld], y[i * ld]);
    }
    __syncthreads();
  }
}

template <class T, class TO>
__global__ __launch_bounds__(DARE_BLOCK) void dare_sda_kernel(const T* __restrict__ Ag, const T* __restrict__ Bg,
                                                              const T* __restrict__ Qg, const T* __restrict__ Rg,
                                                              TO* __restrict__ Xg, int* __restrict__ steps_out, int m, int n,
                                                              int in_lds, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dare_smem[];
  __shared__ int s_piv[DARE_MAX_M];
  __shared__ int s_p;
  __shared__ double s_red[4][DARE_WAVES];
  const long long item = blockIdx.x;
  const int tid = threadIdx.x;
  const int ld = m | 1;
  const long long mat = (long long)m * ld;
  double* base = in_lds ? (double*)dare_smem : ws + item * 6 * mat;
  double *sA = base, *sG = base + mat, *sH = base + 2 * mat, *sW = base + 3 * mat, *sY1 = base + 4 * mat, *sY2 = base + 5 * mat;
  const T* A = Ag + item * m * m;
  const T* B = Bg + item * m * n;
  const T* Q = Qg + item * m * m;
  const T* R = Rg + item * n * n;
  TO* X = Xg + item * m * m;

  double a0max = 0.0;
  for (int e = tid; e < m * m; e += DARE_BLOCK) {
    const int i = e / m, j = e - i * m;
    const double a = (double)A[e];
    sA[i * ld + j] = a;
    sH[i * ld + j] = (double)Q[e];
    a0max = wave::nan_max(a0max, fabs(a));
  }
  // G0 = B R^-1 B^T: R -> W, B^T (n x m) -> Y1, B (m x n) -> Y2
  for (int e = tid; e < n * n; e += DARE_BLOCK) sW[(e / n) * ld + e % n] = (double)R[e];
  for (int e = tid; e < m * n; e += DARE_BLOCK) {
    const int i = e / n, j = e - i * n;
    const double b = (double)B[e];
    sY1[j * ld + i] = b;
    sY2[i * ld + j] = b;
  }
  __syncthreads();
  bool ok = lu_inplace(sW, ld, n, s_piv, &s_p);
  int step = 0;
  bool converged = false;
  if (ok) {
    lu_solve(sW, ld, n, s_piv, sY1, m, nullptr, 0);  // Y1 = R^-1 B^T
    double d0 = 0.0, d1 = 0.0;
    mm(sG, ld, sY2, ld, 1, sY1, ld, 1, m, m, n, false, d0, d1);
    double r[4] = {a0max, d1, 0.0, 0.0};
    block_max4(r, s_red);
    a0max = r[0];
    ok = r[0] <= DBL_MAX && r[1] <= DBL_MAX;
  }
  const double a_tol = DARE_SQRT_EPS * a0max;
  const double h_tol = (double)m * DARE_EPS;
  while (ok && !converged && step < DARE_MAX_STEPS) {
    step++;
    double u = 0.0, v = 0.0;
    mm(sW, ld, sG, ld, 1, sH, ld, 1, m, m, m, false, u, v);  // W = G H (+ I below)
    __syncthreads();
    for (int i = tid; i < m; i += DARE_BLOCK) sW[i * ld + i] += 1.0;
    for (int e = tid; e < m * m; e += DARE_BLOCK) {
      const int i = e / m, j = e - i * m;
      sY1[i * ld + j] = sA[i * ld + j];
      sY2[i * ld + j] = sG[i * ld + j];
    }
    __syncthreads();
    if (!lu_inplace(sW, ld, m, s_piv, &s_p)) {
      ok = false;
      break;
    }
    lu_solve(sW, ld, m, s_piv, sY1, m, sY2, m);  // Y1 = W^-1 A, Y2 = W^-1 G
    mm(sW, ld, sA, ld, 1, sY2, ld, 1, m, m, m, false, u, v);  // T = A W^-1 G  (-> W)
    __syncthreads();
    double gmax = 0.0;
    u = 0.0;
    mm(sG, ld, sW, ld, 1, sA, 1, ld, m, m, m, true, u, gmax);  // G += T A^T
    mm(sY2, ld, sH, ld, 1, sY1, ld, 1, m, m, m, false, u, v);  // S = H W^-1 A  (-> Y2)
    __syncthreads();
    double dh = 0.0, hmax = 0.0;
    mm(sH, ld, sA, 1, ld, sY2, ld, 1, m, m, m, true, dh, hmax);  // H += A^T S
    double amax = 0.0;
    u = 0.0;
    mm(sW, ld, sA, ld, 1, sY1, ld, 1, m, m, m, false, u, amax);  // A' = A W^-1 A  (-> W)
    __syncthreads();
    double* t = sA;
    sA = sW;
    sW = t;
    double r[4] = {dh, hmax, amax, gmax};
    block_max4(r, s_red);
    if (!(r[0] <= DBL_MAX && r[1] <= DBL_MAX && r[2] <= DBL_MAX && r[3] <= DBL_MAX)) {
      ok = false;
      break;
    }
    converged = r[0] <= h_tol * r[1] && r[2] <= a_tol;
  }
  ok = ok && converged;
  const TO nanv = (TO)__builtin_nan("");
  for (int e = tid; e < m * m; e += DARE_BLOCK) {
    const int i = e / m, j = e - i * m;
    X[e] = ok ? (TO)(0.5 * (sH[i * ld + j] + sH[j * ld + i])) : nanv;
  }
  if (steps_out && tid == 0) steps_out[item] = ok ? step : -1;
}

// X <- (H + H^T) / 2 in the output dtype when the last doubling step passed the convergence test
// (max|dH| <= m eps max|H|, max|Ak| <= sqrt(eps) max|A0|, everything finite, the guard flag clear), else
// all NaN.  One workgroup: the composed tier's once-per-call finish.
template <class T>
__global__ __launch_bounds__(DARE_BLOCK) void dare_finish_kernel(const double* __restrict__ H, const double* __restrict__ dH,
                                                                 const double* __restrict__ A0, const double* __restrict__ Ak,
                                                                 const int* __restrict__ flag, T* __restrict__ X, long long m) {
  __shared__ double s_red[4][DARE_WAVES];
  const long long mm2 = m * m;
  double hm = 0.0, dm = 0.0, a0 = 0.0, ak = 0.0, z = 0.0;
  for (long long e = threadIdx.x; e < mm2; e += DARE_BLOCK) {
    hm = wave::nan_max(hm, fabs(H[e]));
    dm = wave::nan_max(dm, fabs(dH[e]));
    a0 = wave::nan_max(a0, fabs(A0[e]));
    ak = wave::nan_max(ak, fabs(Ak[e]));
  }
  double r[4] = {hm, dm, a0, ak};
  block_max4(r, s_red);
  const bool ok = *flag == 0 && r[0] <= DBL_MAX && r[1] <= DBL_MAX && r[2] <= DBL_MAX && r[3] <= DBL_MAX &&
                  r[1] <= (double)m * DARE_EPS * r[0] && r[3] <= DARE_SQRT_EPS * r[2];
  const T nanv = (T)__builtin_nan("");
  for (long long e = threadIdx.x; e < mm2; e += DARE_BLOCK) {
    const long long i = e / m, j = e - i * m;
    X[e] = ok ? (T)(0.5 * (H[e] + H[j * m + i])) : nanv;
  }
}

// The composed tier's guard in front of each LU (R once, W every step): a matrix with a non-finite entry
// sets *flag and is replaced by the identity, so the LU kernels only ever see finite values (a column of
// NaN leaves their pivot search without a candidate row).  A set flag keeps replacing: the result is NaN
// anyway.  first: the flag starts clear.  One workgroup.
__global__ __launch_bounds__(1024) void dare_guard_kernel(double* __restrict__ M, long long n, int* __restrict__ flag, int first) {
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = first ? 0 : *flag;
  __syncthreads();
  const long long nn = n * n;
  bool bad = false;
  for (long long e = threadIdx.x; e < nn; e += 1024) bad |= !(fabs(M[e]) <= DBL_MAX);
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  const int b = s_bad;
  if (b)
    for (long long e = threadIdx.x; e < nn; e += 1024) M[e] = (e / n == e % n) ? 1.0 : 0.0;
  if (threadIdx.x == 0) *flag = b;
}

size_t dare_lds_bytes(long long m) { return (size_t)6 * m * (m | 1) * sizeof(double); }
// static LDS of the kernel (pivots, reductions) + slack
constexpr size_t kDareLdsBudget = pthip::kLdsPerCU - 4 * 1024;

template <class T, class TO>
int dare_typed(long long batch, long long m, long long n, const void* A, const void* B, const void* Q, const void* R, void* X,
               void* steps, void* ws, size_t ws_bytes) {
  const size_t lds = dare_lds_bytes(m);
  const bool in_lds = lds <= kDareLdsBudget;
  if (!in_lds && ws_bytes < (size_t)batch * lds)
    return pthip::set_error("pthip_dare: workspace of %zu bytes, %zu needed", ws_bytes, (size_t)batch * lds);
  auto k = dare_sda_kernel<T, TO>;
  static bool attr = false;
  if (!attr) {
    PTHIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDareLdsBudget));
    attr = true;
  }
  hipStream_t st = pthip::ctx().stream;
  PTHIP_KLAUNCH(k, dim3((unsigned)batch), dim3(DARE_BLOCK), in_lds ? lds : 0, st, (const T*)A, (const T*)B, (const T*)Q,
                (const T*)R, (TO*)X, (int*)steps, (int)m, (int)n, in_lds ? 1 : 0, (double*)ws);
  return pthip::post_launch("dare_sda");
}

}  // namespace

extern "C" size_t pthip_dare_workspace(int64_t batch, int64_t m, int64_t n) {
  (void)n;
  const size_t lds = dare_lds_bytes(m);
  return lds <= kDareLdsBudget ? 0 : (size_t)batch * lds;
}

extern "C" int pthip_dare(int dtype, int out_dtype, int64_t batch, int64_t m, int64_t n, const void* A, const void* B, const void* Q, const void* R,
                          void* X, void* steps, void* ws, size_t ws_bytes) {
  PTHIP_REQUIRE_INIT();
  if (m < 1 || m > DARE_MAX_M || n < 0 || n > m)
    return pthip::set_error("pthip_dare: m = %lld, n = %lld outside the single-launch tier (0 <= n <= m <= %d)", (long long)m,
                            (long long)n, DARE_MAX_M);
  if (batch == 0) return 0;
  const bool o64 = out_dtype == PTHIP_F64;
  if (!o64 && out_dtype != PTHIP_F32)
    return pthip::set_error("pthip_dare: output dtype %d not supported (float32/float64 only)", out_dtype);
  if (dtype == PTHIP_F64)
    return o64 ? dare_typed<double, double>(batch, m, n, A, B, Q, R, X, steps, ws, ws_bytes)
               : dare_typed<double, float>(batch, m, n, A, B, Q, R, X, steps, ws, ws_bytes);
  if (dtype == PTHIP_F32)
    return o64 ? dare_typed<float, double>(batch, m, n, A, B, Q, R, X, steps, ws, ws_bytes)
               : dare_typed<float, float>(batch, m, n, A, B, Q, R, X, steps, ws, ws_bytes);
  return pthip::set_error("pthip_dare: dtype %d not supported (float32/float64 only)", dtype);
}

extern "C" int pthip_dare_guard(int64_t n, void* M, void* flag, int first) {
  PTHIP_REQUIRE_INIT();
  PTHIP_KLAUNCH(dare_guard_kernel, dim3(1), dim3(1024), 0, pthip::ctx().stream, (double*)M, (long long)n, (int*)flag, first);
  return pthip::post_launch("dare_guard");
}

extern "C" int pthip_dare_finish(int dtype, int64_t m, const void* H, const void* dH, const void* A0, const void* Ak, const void* flag,
                                 void* X) {
  PTHIP_REQUIRE_INIT();
  if (m == 0) return 0;
  hipStream_t st = pthip::ctx().stream;
  if (dtype == PTHIP_F64)
    PTHIP_KLAUNCH((dare_finish_kernel<double>), dim3(1), dim3(DARE_BLOCK), 0, st, (const double*)H, (const double*)dH,
                  (const double*)A0, (const double*)Ak, (const int*)flag, (double*)X, (long long)m);
  else if (dtype == PTHIP_F32)
    PTHIP_KLAUNCH((dare_finish_kernel<float>), dim3(1), dim3(DARE_BLOCK), 0, st, (const double*)H, (const double*)dH,
                  (const double*)A0, (const double*)Ak, (const int*)flag, (float*)X, (long long)m);
  else
    return pthip::set_error("pthip_dare_finish: dtype %d not supported (float32/float64 only)", dtype);
  return pthip::post_launch("dare_finish");
}
