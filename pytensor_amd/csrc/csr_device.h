// csr_device.h — what every CSR kernel file shares (sparse.hip, spgemm.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace csr {

// the entries [lo, hi) of row r, clamped to [0, nnz): a malformed indptr can skip entries, never leave the arrays
__device__ __forceinline__ void row_extent(const int* __restrict__ indptr, long long r, long long nnz, long long* lo,
                                           long long* hi) {
  long long a = indptr[r], b = indptr[r + 1];
  a = a < 0 ? 0 : (a > nnz ? nnz : a);
  b = b < a ? a : (b > nnz ? nnz : b);
  *lo = a;
  *hi = b;
}

}  // namespace csr
