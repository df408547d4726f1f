// sylvester.hip — the Sylvester equation A X + X B = C by Bartels-Stewart, for m n above the Kronecker tier.
//
// Reference: SolveSylvester (pytensor/tensor/linalg/solvers/linear_control.py: real Schur forms A = U R U^T and
// B = V S V^T, F = U^T C V, TRSYL for R Y + Y S = F, X = U Y V^T).  The two factorisations and the quasi-triangular
// solve are this file; the products F = U^T C V and X = U Y V^T run on the library's GEMM (dispatch/decomp.py).
// The numerical core is csrc/schur_device.h, which the host build of tests/test_sylvester_host.py checks against
// SciPy.  Everything is fp64 whatever the operand dtype.
//
// pthip_real_schur: one workgroup per Schur form, grid (batch, forms): form 0 factors A, form 1 factors B (forms = 1
// when B = A^T: the Lyapunov case needs one factorisation).  Hessenberg reduction, then Francis double-shift QR (LAPACK
// dlahqr), in the caller's global workspace.  A form whose operand holds a non-finite value, or whose QR iteration
// reaches its cap, records a non-zero info and is not used.
// pthip_trsyl: one workgroup per item: R Y + Y op(S) = F in place (dtrsyl; op(S) = S^T when forms = 1, where S = R).
// An item with a non-zero info in either form gets an all-NaN Y, and so an all-NaN X (DESIGN §4 "Sylvester /
// Lyapunov").  No host read anywhere: a graph holding the solve freezes into a replayable plan.
#include "common.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int SYL_BLOCK = 256;
constexpr int SYL_WAVES = SYL_BLOCK / 64;
constexpr int SYL_MAX_N = 1024;

// workgroup-wide max of non-negative values (NaN-propagating), every thread gets it
__device__ double syl_team_max(double v) {
  __shared__ double red[SYL_WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o);
    v = (v != v || w > v) ? (v != v ? v : w) : v;
  }
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < SYL_WAVES; w++) r = (r != r || red[w] > r) ? (r != r ? r : red[w]) : r;
  __syncthreads();
  return r;
}

}  // namespace

#define SCHUR_DEV __device__ inline
#define SCHUR_SYNC() __syncthreads()
#define SCHUR_TEAM_MAX(v) syl_team_max(v)
#include "schur_device.h"

namespace {

// workspace layout (doubles, then int32): for item b, form 0: T at b 2 m^2, Zt right after it; form 1 (forms = 2):
// T at 2 batch m^2 + b 2 n^2, Zt right after it; info[b forms + form] after all of them.
struct Layout {
  long long m, n, batch;
  int forms;
  __host__ __device__ double* t(double* ws, long long b, int form) const {
    return form == 0 ? ws + b * 2 * m * m : ws + 2 * batch * m * m + b * 2 * n * n;
  }
  __host__ __device__ long long dim(int form) const { return form == 0 ? m : n; }
  __host__ __device__ int* info(double* ws) const { return (int*)(ws + 2 * batch * (m * m + (forms == 2 ? n * n : 0))); }
  size_t bytes() const { return (size_t)2 * batch * (m * m + (forms == 2 ? n * n : 0)) * sizeof(double) + (size_t)batch * forms * sizeof(int); }
};

template <class T>
__global__ __launch_bounds__(SYL_BLOCK) void real_schur_kernel(const T* __restrict__ A, const T* __restrict__ B, Layout L,
                                                               double* __restrict__ ws) {
  const long long b = blockIdx.x;
  const int form = blockIdx.y;
  const int tid = threadIdx.x;
  const int n = (int)L.dim(form);
  const T* X = form == 0 ? A + b * L.m * L.m : B + b * L.n * L.n;
  double* H = L.t(ws, b, form);
  double* Zt = H + (long long)n * n;
  for (int e = tid; e < n * n; e += SYL_BLOCK) H[e] = (double)X[e];
  __syncthreads();
  int max_its, sweeps;
  const int info = pt_schur::real_schur(H, Zt, n, n, tid, SYL_BLOCK, &max_its, &sweeps);
  if (tid == 0) L.info(ws)[b * L.forms + form] = info;
}

__global__ __launch_bounds__(SYL_BLOCK) void trsyl_kernel(double* __restrict__ F, Layout L, double* __restrict__ ws) {
  const long long b = blockIdx.x;
  const int m = (int)L.m, n = (int)L.n;
  double* Fb = F + b * L.m * L.n;
  const int* info = L.info(ws) + b * L.forms;
  const bool ok = info[0] == 0 && (L.forms == 1 || info[1] == 0);
  if (!ok) {  // (uniform: every thread read the same flags)
    const double nanv = __builtin_nan("");
    for (int e = threadIdx.x; e < m * n; e += SYL_BLOCK) Fb[e] = nanv;
    return;
  }
  const double* R = L.t(ws, b, 0);
  const double* S = L.forms == 1 ? R : L.t(ws, b, 1);
  pt_schur::trsyl(R, m, S, L.forms == 1 ? m : n, Fb, n, m, n, L.forms == 1, threadIdx.x, SYL_BLOCK);
}

Layout make_layout(long long batch, long long m, long long n, int b_is_a_t) {
  Layout L;
  L.m = m;
  L.n = b_is_a_t ? m : n;
  L.batch = batch;
  L.forms = b_is_a_t ? 1 : 2;
  return L;
}

int check_dims(const char* what, long long m, long long n, int b_is_a_t) {
  if (m < 1 || n < 1 || m > SYL_MAX_N || n > SYL_MAX_N)
    return pthip::set_error("%s: m = %lld, n = %lld outside 1..%d", what, m, n, SYL_MAX_N);
  if (b_is_a_t && m != n) return pthip::set_error("%s: B = A^T needs m = n (m = %lld, n = %lld)", what, m, n);
  return 0;
}

}  // namespace

extern "C" size_t pthip_sylvester_workspace(int64_t batch, int64_t m, int64_t n, int b_is_a_t) {
  return make_layout(batch, m, n, b_is_a_t).bytes();
}

extern "C" int pthip_real_schur(int dtype, int64_t batch, int64_t m, int64_t n, int b_is_a_t, const void* A, const void* B, void* ws,
                                size_t ws_bytes) {
  PTHIP_REQUIRE_INIT();
  if (check_dims("pthip_real_schur", m, n, b_is_a_t)) return -1;
  if (batch == 0) return 0;
  const Layout L = make_layout(batch, m, n, b_is_a_t);
  if (ws_bytes < L.bytes()) return pthip::set_error("pthip_real_schur: workspace of %zu bytes, %zu needed", ws_bytes, L.bytes());
  hipStream_t st = pthip::ctx().stream;
  const dim3 grid((unsigned)batch, (unsigned)L.forms);
  if (dtype == PTHIP_F64)
    PTHIP_KLAUNCH(real_schur_kernel<double>, grid, dim3(SYL_BLOCK), 0, st, (const double*)A, (const double*)B, L, (double*)ws);
  else if (dtype == PTHIP_F32)
    PTHIP_KLAUNCH(real_schur_kernel<float>, grid, dim3(SYL_BLOCK), 0, st, (const float*)A, (const float*)B, L, (double*)ws);
  else
    return pthip::set_error("pthip_real_schur: dtype %d not supported (float32/float64 only)", dtype);
  return pthip::post_launch("real_schur");
}

extern "C" int pthip_trsyl(int64_t batch, int64_t m, int64_t n, int b_is_a_t, void* F, void* ws, size_t ws_bytes) {
  PTHIP_REQUIRE_INIT();
  if (check_dims("pthip_trsyl", m, n, b_is_a_t)) return -1;
  if (batch == 0) return 0;
  const Layout L = make_layout(batch, m, n, b_is_a_t);
  if (ws_bytes < L.bytes()) return pthip::set_error("pthip_trsyl: workspace of %zu bytes, %zu needed", ws_bytes, L.bytes());
  PTHIP_KLAUNCH(trsyl_kernel, dim3((unsigned)batch), dim3(SYL_BLOCK), 0, pthip::ctx().stream, (double*)F, L, (double*)ws);
  return pthip::post_launch("trsyl");
}
