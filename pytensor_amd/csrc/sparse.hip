// sparse.hip — compressed sparse row kernels for pytensor.sparse (csr / csc) on gfx950.
//
// Reference: pytensor/sparse/basic.py and math.py (CSM, Transpose, DenseFromSparse, SparseFromDense,
// StructuredDot and its gradients, SamplingDot, SpSum, the structure-preserving multiplies / adds).
// Every matrix is handed over as the three arrays of a CSR matrix: rows ("major"), their entries'
// column indices ("minor", int32) and values, row pointers (int32, rows + 1).  A csc matrix is the CSR
// of its transpose (pytensor_amd/dispatch/sparse.py), so one set of kernels serves both formats.
//
// Nothing here assumes sorted indices or the absence of duplicates (CSM passes the caller's arrays
// through).  Every kernel is bit-reproducible run to run: no floating-point atomics, each output
// element is summed by one owner in a fixed order.  A minor index out of range sets status bit 0
// (IndexError) and the entry is skipped; row extents are clamped to [0, nnz).  Grids are 1-D and
// grid-stride, never more than kMaxBlocks workgroups.
#include "common.h"
#include "wave_device.h"

namespace {

constexpr int BLOCK = 256;
constexpr long long kMaxBlocks = 1 << 20;
constexpr int kLongRow = 1024;  // rows longer than this are summed by a whole workgroup (spmm_long_kernel)

inline unsigned grid_for(long long work, int per_block) {
  long long b = (work + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (unsigned)b;
}

__device__ __forceinline__ void row_extent(const int* __restrict__ indptr, long long r, long long nnz, long long* lo,
                                           long long* hi) {
  long long a = indptr[r], b = indptr[r + 1];
  a = a < 0 ? 0 : (a > nnz ? nnz : a);
  b = b < a ? a : (b > nnz ? nnz : b);
  *lo = a;
  *hi = b;
}

// row owning entry e: the last r with indptr[r] <= e (rows of zero length are skipped); -1 if none
__device__ __forceinline__ long long row_of(const int* __restrict__ indptr, long long rows, long long e) {
  long long lo = 0, hi = rows;  // answer in [0, rows)
  if (rows <= 0 || e < indptr[0] || e >= indptr[rows]) return -1;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (indptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename T, int VEC>
struct Pack {
  T v[VEC];
};

// ---- SpMM: out[r, j] = sum_e data[e] * B[ind[e], j]  (B == nullptr: B = 1, the row sums) -------------
// k == 1: L lanes per row, lane-strided partial sums, fixed xor-tree within the group.
template <typename T, int L>
__global__ __launch_bounds__(BLOCK) void spmv_kernel(long long rows, long long n, long long nnz, const T* __restrict__ data,
                                                     const int* __restrict__ ind, const int* __restrict__ indptr,
                                                     const T* __restrict__ B, long long sb0, T* __restrict__ out,
                                                     long long so0, int* status) {
  const long long groups = (long long)gridDim.x * (BLOCK / L);
  const int sub = threadIdx.x % L;
  // (every lane of a group shares r: the loop bound and `skip` are uniform per group)
  for (long long r = (long long)blockIdx.x * (BLOCK / L) + threadIdx.x / L; r < rows; r += groups) {
    long long lo, hi;
    row_extent(indptr, r, nnz, &lo, &hi);
    const bool skip = hi - lo > kLongRow;  // spmm_long_kernel owns it
    T acc = 0;
    if (!skip) {
      for (long long e = lo + sub; e < hi; e += L) {
        const int c = ind[e];
        if (c < 0 || c >= n) {
          atomicOr(status, 1);
          continue;
        }
        acc += data[e] * (B ? B[(long long)c * sb0] : T(1));
      }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, L);
    if (sub == 0 && !skip) out[r * so0] = acc;
  }
}

// k > 1: one thread per (row, pack of VEC consecutive output columns), serial over the row's entries.
template <typename T, int VEC>
__global__ __launch_bounds__(BLOCK) void spmm_kernel(long long rows, long long n, long long k, long long nnz,
                                                     const T* __restrict__ data, const int* __restrict__ ind,
                                                     const int* __restrict__ indptr, const T* __restrict__ B, long long sb0,
                                                     long long sb1, T* __restrict__ out, long long so0, long long so1,
                                                     int* status) {
  const long long kv = k / VEC;
  const long long total = rows * kv;
  for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BLOCK) {
    const long long r = t / kv, j0 = (t % kv) * VEC;
    long long lo, hi;
    row_extent(indptr, r, nnz, &lo, &hi);
    if (hi - lo > kLongRow) continue;
    T acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; q++) acc[q] = 0;
    for (long long e = lo; e < hi; e++) {
      const int c = ind[e];
      if (c < 0 || c >= n) {
        atomicOr(status, 1);
        continue;
      }
      const T a = data[e];
      if (VEC > 1) {  // (sb1 == 1, 16-byte aligned rows: checked by the host)
        const Pack<T, VEC> p = *reinterpret_cast<const Pack<T, VEC>*>(B + (long long)c * sb0 + j0);
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[q] += a * p.v[q];
      } else {
        acc[0] += a * B[(long long)c * sb0 + j0 * sb1];
      }
    }
#pragma unroll
    for (int q = 0; q < VEC; q++) out[r * so0 + (j0 + q) * so1] = acc[q];
  }
}

// rows longer than kLongRow: one workgroup per row (grid-stride over rows in groups of BLOCK, the long
// ones found with a ballot), thread-strided partial sums, fixed LDS tree per output column.
template <typename T>
__global__ __launch_bounds__(BLOCK) void spmm_long_kernel(long long rows, long long n, long long k, long long nnz,
                                                          const T* __restrict__ data, const int* __restrict__ ind,
                                                          const int* __restrict__ indptr, const T* __restrict__ B,
                                                          long long sb0, long long sb1, T* __restrict__ out, long long so0,
                                                          long long so1, int* status) {
  __shared__ int s_rows[BLOCK];
  __shared__ int s_count;
  __shared__ T s_red[BLOCK];
  for (long long base = (long long)blockIdx.x * BLOCK; base < rows; base += (long long)gridDim.x * BLOCK) {
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const long long r = base + threadIdx.x;
    if (r < rows) {
      long long lo, hi;
      row_extent(indptr, r, nnz, &lo, &hi);
      if (hi - lo > kLongRow) s_rows[atomicAdd(&s_count, 1)] = threadIdx.x;  // (which slot: irrelevant to the sums)
    }
    __syncthreads();
    const int cnt = s_count;
    for (int q = 0; q < cnt; q++) {
      const long long rr = base + s_rows[q];
      long long lo, hi;
      row_extent(indptr, rr, nnz, &lo, &hi);
      for (long long j = 0; j < k; j++) {
        T acc = 0;
        for (long long e = lo + threadIdx.x; e < hi; e += BLOCK) {
          const int c = ind[e];
          if (c < 0 || c >= n) {
            atomicOr(status, 1);
            continue;
          }
          acc += data[e] * (B ? B[(long long)c * sb0 + j * sb1] : T(1));
        }
        s_red[threadIdx.x] = acc;
        __syncthreads();
        for (int s = BLOCK / 2; s > 0; s >>= 1) {
          if (threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
          __syncthreads();
        }
        if (threadIdx.x == 0) out[rr * so0 + j * so1] = s_red[0];
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

template <typename T>
int spmm_t(long long rows, long long n, long long k, long long nnz, const void* data_, const void* ind_, const void* indptr_,
           const void* B_, long long sb0, long long sb1, void* out_, long long so0, long long so1, int lanes, int has_long) {
  hipStream_t st = pthip::ctx().stream;
  int* status = pthip::ctx().status_dev;
  const T* data = (const T*)data_;
  const int* ind = (const int*)ind_;
  const int* indptr = (const int*)indptr_;
  const T* B = (const T*)B_;
  T* out = (T*)out_;
  if (rows <= 0 || k <= 0) return 0;
  if (k == 1) {
    switch (lanes) {
      case 1: PTHIP_KLAUNCH((spmv_kernel<T, 1>), dim3(grid_for(rows, BLOCK)), dim3(BLOCK), 0, st, rows, n, nnz, data, ind, indptr, B, sb0, out, so0, status); break;
      case 4: PTHIP_KLAUNCH((spmv_kernel<T, 4>), dim3(grid_for(rows, BLOCK / 4)), dim3(BLOCK), 0, st, rows, n, nnz, data, ind, indptr, B, sb0, out, so0, status); break;
      case 16: PTHIP_KLAUNCH((spmv_kernel<T, 16>), dim3(grid_for(rows, BLOCK / 16)), dim3(BLOCK), 0, st, rows, n, nnz, data, ind, indptr, B, sb0, out, so0, status); break;
      default: PTHIP_KLAUNCH((spmv_kernel<T, 64>), dim3(grid_for(rows, BLOCK / 64)), dim3(BLOCK), 0, st, rows, n, nnz, data, ind, indptr, B, sb0, out, so0, status); break;
    }
  } else {
    constexpr int V = 16 / sizeof(T);
    const bool packed = B && sb1 == 1 && k % V == 0 && sb0 % V == 0 && ((uintptr_t)B & 15) == 0;
    if (packed)
      PTHIP_KLAUNCH((spmm_kernel<T, V>), dim3(grid_for(rows * (k / V), BLOCK)), dim3(BLOCK), 0, st, rows, n, k, nnz, data, ind, indptr, B, sb0, sb1, out, so0, so1, status);
    else if (B)
      PTHIP_KLAUNCH((spmm_kernel<T, 1>), dim3(grid_for(rows * k, BLOCK)), dim3(BLOCK), 0, st, rows, n, k, nnz, data, ind, indptr, B, sb0, sb1, out, so0, so1, status);
    else
      return pthip::set_error("pthip_csr_spmm: B == NULL needs k == 1");
  }
  if (has_long)
    PTHIP_KLAUNCH((spmm_long_kernel<T>), dim3(grid_for(rows, BLOCK)), dim3(BLOCK), 0, st, rows, n, k, nnz, data, ind, indptr, B, sb0, sb1, out, so0, so1, status);
  return pthip::post_launch("csr_spmm");
}

// ---- exclusive scan of int32 counts: out[0..n] (out[n] = total) ------------------------------------
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = BLOCK * SCAN_ITEMS;

__global__ __launch_bounds__(BLOCK) void scan_tiles_kernel(const int* __restrict__ in, long long n, long long* __restrict__ sums) {
  const long long start = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  long long c = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; j++)
    if (start + j < n) c += in[start + j];
  long long total;
  wave::block_exclusive_scan<BLOCK>(c, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(BLOCK) void scan_sums_kernel(long long* __restrict__ sums, long long nb) {
  long long carry = 0;
  for (long long base = 0; base < nb; base += BLOCK) {
    const long long i = base + threadIdx.x;
    const long long v = i < nb ? sums[i] : 0;
    long long chunk;
    const long long ex = wave::block_exclusive_scan<BLOCK>(v, &chunk);
    if (i < nb) sums[i] = carry + ex;
    carry += chunk;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ __launch_bounds__(BLOCK) void scan_apply_kernel(const int* __restrict__ in, long long n, const long long* __restrict__ sums,
                                                           long long nb, int* __restrict__ out) {
  const long long start = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  long long c = 0;
  int v[SCAN_ITEMS];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; j++) {
    v[j] = start + j < n ? in[start + j] : 0;
    c += v[j];
  }
  long long total;
  long long pos = sums[blockIdx.x] + wave::block_exclusive_scan<BLOCK>(c, &total);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; j++) {
    if (start + j < n) out[start + j] = (int)pos;
    pos += v[j];
  }
  if (blockIdx.x == nb - 1 && threadIdx.x == 0) out[n] = (int)sums[nb];
}

// (in and out may not overlap; n >= 0; the grid of the tile kernels is nb <= 2^31 / SCAN_TILE blocks)
int exclusive_scan_i32(const int* in, long long n, int* out, hipStream_t st) {
  if (n <= 0) {
    PTHIP_CHECK(pthip::memset_async(out, 0, sizeof(int), st));
    return 0;
  }
  const long long nb = (n + SCAN_TILE - 1) / SCAN_TILE;
  void* sums = nullptr;
  int r = pthip_alloc((size_t)(nb + 1) * sizeof(long long), &sums);
  if (r) return r;
  PTHIP_KLAUNCH(scan_tiles_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, in, n, (long long*)sums);
  PTHIP_KLAUNCH(scan_sums_kernel, dim3(1), dim3(BLOCK), 0, st, (long long*)sums, nb);
  PTHIP_KLAUNCH(scan_apply_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, in, n, (const long long*)sums, nb, out);
  r = pthip::post_launch("exclusive_scan");
  pthip_free(sums);  // (stream-ordered pool)
  return r;
}

// ---- transpose: stable LSD radix sort of the entries by column ---------------------------------------
// key[e] = column of entry e (invalid / outside every row: the sentinel n, sorted last and dropped),
// val[e] = e.  Each 8-bit pass is a stable counting sort: per-tile digit histograms, one exclusive
// scan over (digit, tile), placement at the tile's offset plus the entry's rank among the same digit
// earlier in its tile (wave ballots, waves in order).  Stable passes keep row order within a column:
// the result is scipy's tocsc() ordering for sorted inputs, and deterministic for any input.
__global__ __launch_bounds__(BLOCK) void tr_keys_kernel(long long rows, long long n, long long nnz, const int* __restrict__ ind,
                                                        const int* __restrict__ indptr, int* __restrict__ key, int* __restrict__ val,
                                                        int* __restrict__ rowid, int* __restrict__ counts, int* status) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < nnz; e += (long long)gridDim.x * BLOCK) {
    const long long r = row_of(indptr, rows, e);
    int c = ind[e];
    if (r < 0) {
      c = (int)n;
    } else if (c < 0 || c >= n) {
      atomicOr(status, 1);
      c = (int)n;
    } else {
      atomicAdd(&counts[c], 1);  // (integer: the counts are exact whatever the order)
    }
    key[e] = c;
    val[e] = (int)e;
    rowid[e] = (int)r;
  }
}

__global__ __launch_bounds__(BLOCK) void radix_hist_kernel(const int* __restrict__ key, long long nnz, int shift,
                                                           long long nb, int* __restrict__ hist) {
  __shared__ int s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (e < nnz) atomicAdd(&s_h[(key[e] >> shift) & 255], 1);
  __syncthreads();
  hist[(long long)threadIdx.x * nb + blockIdx.x] = s_h[threadIdx.x];
}

__global__ __launch_bounds__(BLOCK) void radix_scatter_kernel(const int* __restrict__ key, const int* __restrict__ val, long long nnz,
                                                              int shift, long long nb, const int* __restrict__ offs,
                                                              int* __restrict__ key_out, int* __restrict__ val_out) {
  __shared__ int s_w[BLOCK / 64][256];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int w = 0; w < BLOCK / 64; w++) s_w[w][threadIdx.x] = 0;
  __syncthreads();
  const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool valid = e < nnz;
  const int k = valid ? key[e] : 0;
  const int d = (k >> shift) & 255;
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const unsigned long long m = __ballot((d >> b) & 1);
    peers &= ((d >> b) & 1) ? m : ~m;
  }
  const unsigned long long below = peers & ((1ull << lane) - 1);
  if (valid && below == 0) s_w[wid][d] = __popcll(peers);  // the lowest lane of its digit group
  __syncthreads();
  if (valid) {
    int rank = __popcll(below);
    for (int w = 0; w < wid; w++) rank += s_w[w][d];
    const long long pos = (long long)offs[(long long)d * nb + blockIdx.x] + rank;
    key_out[pos] = k;
    val_out[pos] = val[e];
  }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void tr_place_kernel(long long m_out, const int* __restrict__ perm, const int* __restrict__ rowid,
                                                         const T* __restrict__ data, T* __restrict__ data_out, int* __restrict__ ind_out) {
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < m_out; p += (long long)gridDim.x * BLOCK) {
    const int e = perm[p];
    data_out[p] = data[e];
    ind_out[p] = rowid[e];
  }
}

template <typename T>
int transpose_t(long long rows, long long n, long long nnz, const void* data, const void* ind, const void* indptr, void* data_out,
                void* ind_out, void* indptr_out) {
  hipStream_t st = pthip::ctx().stream;
  int* status = pthip::ctx().status_dev;
  if (nnz <= 0) {
    PTHIP_CHECK(pthip::memset_async(indptr_out, 0, (size_t)(n + 1) * sizeof(int), st));
    return 0;
  }
  const long long nb = (nnz + BLOCK - 1) / BLOCK;
  void *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr, *rowid = nullptr, *counts = nullptr, *hist = nullptr,
       *offs = nullptr;
  const size_t ib = (size_t)nnz * sizeof(int);
  int r = 0;
  if ((r = pthip_alloc(ib, &keys)) || (r = pthip_alloc(ib, &vals)) || (r = pthip_alloc(ib, &keys2)) || (r = pthip_alloc(ib, &vals2)) ||
      (r = pthip_alloc(ib, &rowid)) || (r = pthip_alloc((size_t)(n + 1) * sizeof(int), &counts)) ||
      (r = pthip_alloc((size_t)256 * nb * sizeof(int), &hist)) || (r = pthip_alloc(((size_t)256 * nb + 1) * sizeof(int), &offs)))
    return r;
  PTHIP_CHECK(pthip::memset_async(counts, 0, (size_t)(n + 1) * sizeof(int), st));
  PTHIP_KLAUNCH(tr_keys_kernel, dim3(grid_for(nnz, BLOCK)), dim3(BLOCK), 0, st, rows, n, nnz, (const int*)ind, (const int*)indptr,
                (int*)keys, (int*)vals, (int*)rowid, (int*)counts, status);
  int bits = 1;
  while ((1ll << bits) <= n) bits++;  // keys are in [0, n]
  for (int shift = 0; shift < bits; shift += 8) {
    PTHIP_KLAUNCH(radix_hist_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, (const int*)keys, nnz, shift, nb, (int*)hist);
    if ((r = exclusive_scan_i32((const int*)hist, 256 * nb, (int*)offs, st))) return r;
    PTHIP_KLAUNCH(radix_scatter_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, (const int*)keys, (const int*)vals, nnz, shift, nb,
                  (const int*)offs, (int*)keys2, (int*)vals2);
    void* t = keys; keys = keys2; keys2 = t;
    t = vals; vals = vals2; vals2 = t;
  }
  if ((r = exclusive_scan_i32((const int*)counts, n, (int*)indptr_out, st))) return r;
  // the valid entries come first (the sentinel sorts last); at most nnz of them
  PTHIP_KLAUNCH(tr_place_kernel<T>, dim3(grid_for(nnz, BLOCK)), dim3(BLOCK), 0, st, nnz, (const int*)vals, (const int*)rowid,
                (const T*)data, (T*)data_out, (int*)ind_out);
  r = pthip::post_launch("csr_transpose");
  for (void* p : {keys, vals, keys2, vals2, rowid, counts, hist, offs}) pthip_free(p);
  return r;
}

// ---- SDDMM: out[e] = (data ? data[e] : 1) * sum_j P[row(e), j] * Q[col(e), j] ---------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void sddmm_kernel(long long rows, long long n, long long k, long long nnz, const T* __restrict__ data,
                                                      const int* __restrict__ ind, const int* __restrict__ indptr,
                                                      const T* __restrict__ P, long long sp0, long long sp1,
                                                      const T* __restrict__ Q, long long sq0, long long sq1, T* __restrict__ out,
                                                      int* status) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < nnz; e += (long long)gridDim.x * BLOCK) {
    const long long r = row_of(indptr, rows, e);
    const int c = ind[e];
    T acc = 0;
    if (r >= 0) {
      if (c < 0 || c >= n) {
        atomicOr(status, 1);
      } else {
        const T* p = P + r * sp0;
        const T* q = Q + (long long)c * sq0;
        for (long long j = 0; j < k; j++) acc += p[j * sp1] * q[j * sq1];
        if (data) acc = data[e] * acc;
      }
    }
    out[e] = acc;
  }
}

// ---- structure-preserving gathers: out[e] = data[e] OP V[row(e) * s_major + col(e) * s_minor] ------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void gather_kernel(int op, long long rows, long long n, long long nnz, const T* __restrict__ data,
                                                       const int* __restrict__ ind, const int* __restrict__ indptr,
                                                       const T* __restrict__ V, long long s_major, long long s_minor,
                                                       T* __restrict__ out, int* status) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < nnz; e += (long long)gridDim.x * BLOCK) {
    const long long r = row_of(indptr, rows, e);
    const int c = ind[e];
    T v = 0;
    if (r >= 0) {
      if (c < 0 || c >= n) {
        atomicOr(status, 1);
      } else {
        v = V[r * s_major + (long long)c * s_minor];
      }
    }
    out[e] = op == 0 ? data[e] * v : data[e] + v;
  }
}

// ---- sparse -> dense: one owner per row adds its entries in stored order (duplicates summed) ---------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void todense_kernel(long long rows, long long n, long long nnz, const T* __restrict__ data,
                                                        const int* __restrict__ ind, const int* __restrict__ indptr,
                                                        T* __restrict__ out, long long so0, long long so1, int* status) {
  for (long long r = (long long)blockIdx.x * BLOCK + threadIdx.x; r < rows; r += (long long)gridDim.x * BLOCK) {
    long long lo, hi;
    row_extent(indptr, r, nnz, &lo, &hi);
    for (long long e = lo; e < hi; e++) {
      const int c = ind[e];
      if (c < 0 || c >= n) {
        atomicOr(status, 1);
        continue;
      }
      out[r * so0 + (long long)c * so1] += data[e];
    }
  }
}

// ---- dense -> sparse: a wave per row counts, then compacts in column order (sorted indices) -----------
template <typename T>
__global__ __launch_bounds__(BLOCK) void fromdense_count_kernel(long long rows, long long n, const T* __restrict__ x, long long sx0,
                                                                long long sx1, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  for (long long r = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * (BLOCK / 64)) {
    long long c = 0;
    for (long long j = lane; j < n; j += 64) c += x[r * sx0 + j * sx1] != T(0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) counts[r] = (int)c;
  }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void fromdense_fill_kernel(long long rows, long long n, const T* __restrict__ x, long long sx0,
                                                               long long sx1, const int* __restrict__ indptr, T* __restrict__ data,
                                                               int* __restrict__ ind) {
  const int lane = threadIdx.x & 63;
  const unsigned long long lt = (1ull << lane) - 1;
  for (long long r = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * (BLOCK / 64)) {
    long long pos = indptr[r];
    for (long long j0 = 0; j0 < n; j0 += 64) {
      const long long j = j0 + lane;
      const T v = j < n ? x[r * sx0 + j * sx1] : T(0);
      const bool nz = j < n && v != T(0);
      const unsigned long long m = __ballot(nz);
      if (nz) {
        const long long p = pos + __popcll(m & lt);
        data[p] = v;
        ind[p] = (int)j;
      }
      pos += __popcll(m);
    }
  }
}

// ---- CSMGrad: gout[e] = sum of the g entries of row(e) whose column is col(e) (stored order) --------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void csm_grad_kernel(long long rows, long long nnz_x, const int* __restrict__ xind,
                                                         const int* __restrict__ xptr, long long nnz_g, const T* __restrict__ gdata,
                                                         const int* __restrict__ gind, const int* __restrict__ gptr, T* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < nnz_x; e += (long long)gridDim.x * BLOCK) {
    const long long r = row_of(xptr, rows, e);
    T acc = 0;
    if (r >= 0) {
      const int c = xind[e];
      long long lo, hi;
      row_extent(gptr, r, nnz_g, &lo, &hi);
      for (long long q = lo; q < hi; q++)
        if (gind[q] == c) acc += gdata[q];
    }
    out[e] = acc;
  }
}

}  // namespace

#define PTHIP_SPARSE_DISPATCH(dtype, call)                                         \
  switch (dtype) {                                                                 \
    case PTHIP_F32: { using T = float; call; }                                     \
    case PTHIP_F64: { using T = double; call; }                                    \
    default: return pthip::set_error("pthip sparse: unsupported dtype %d", dtype); \
  }

extern "C" int pthip_exclusive_scan_i32(int64_t n, const void* in, void* out) {
  PTHIP_REQUIRE_INIT();
  return exclusive_scan_i32((const int*)in, n, (int*)out, pthip::ctx().stream);
}

extern "C" int pthip_csr_spmm(int dtype, int64_t rows, int64_t n, int64_t k, int64_t nnz, const void* data, const void* indices,
                              const void* indptr, const void* B, int64_t sb0, int64_t sb1, void* out, int64_t so0, int64_t so1,
                              int lanes, int has_long) {
  PTHIP_REQUIRE_INIT();
  PTHIP_SPARSE_DISPATCH(dtype, return spmm_t<T>(rows, n, k, nnz, data, indices, indptr, B, sb0, sb1, out, so0, so1, lanes, has_long))
}

extern "C" int pthip_csr_transpose(int dtype, int64_t rows, int64_t n, int64_t nnz, const void* data, const void* indices,
                                   const void* indptr, void* data_out, void* indices_out, void* indptr_out) {
  PTHIP_REQUIRE_INIT();
  if (nnz >= (1ll << 31) || n >= (1ll << 31) - 1) return pthip::set_error("pthip_csr_transpose: int32 index range exceeded");
  PTHIP_SPARSE_DISPATCH(dtype, return transpose_t<T>(rows, n, nnz, data, indices, indptr, data_out, indices_out, indptr_out))
}

extern "C" int pthip_csr_sddmm(int dtype, int64_t rows, int64_t n, int64_t k, int64_t nnz, const void* data, const void* indices,
                               const void* indptr, const void* P, int64_t sp0, int64_t sp1, const void* Q, int64_t sq0, int64_t sq1,
                               void* out) {
  PTHIP_REQUIRE_INIT();
  if (nnz <= 0) return 0;
  hipStream_t st = pthip::ctx().stream;
  int* status = pthip::ctx().status_dev;
  PTHIP_SPARSE_DISPATCH(dtype, {
    PTHIP_KLAUNCH(sddmm_kernel<T>, dim3(grid_for(nnz, BLOCK)), dim3(BLOCK), 0, st, rows, n, k, nnz, (const T*)data, (const int*)indices,
                  (const int*)indptr, (const T*)P, sp0, sp1, (const T*)Q, sq0, sq1, (T*)out, status);
    return pthip::post_launch("csr_sddmm");
  })
}

extern "C" int pthip_csr_gather(int dtype, int op, int64_t rows, int64_t n, int64_t nnz, const void* data, const void* indices,
                                const void* indptr, const void* V, int64_t s_major, int64_t s_minor, void* out) {
  PTHIP_REQUIRE_INIT();
  if (nnz <= 0) return 0;
  hipStream_t st = pthip::ctx().stream;
  int* status = pthip::ctx().status_dev;
  PTHIP_SPARSE_DISPATCH(dtype, {
    PTHIP_KLAUNCH(gather_kernel<T>, dim3(grid_for(nnz, BLOCK)), dim3(BLOCK), 0, st, op, rows, n, nnz, (const T*)data, (const int*)indices,
                  (const int*)indptr, (const T*)V, s_major, s_minor, (T*)out, status);
    return pthip::post_launch("csr_gather");
  })
}

extern "C" int pthip_csr_todense(int dtype, int64_t rows, int64_t n, int64_t nnz, const void* data, const void* indices,
                                 const void* indptr, void* out, int64_t so0, int64_t so1, int accumulate) {
  PTHIP_REQUIRE_INIT();
  hipStream_t st = pthip::ctx().stream;
  int* status = pthip::ctx().status_dev;
  PTHIP_SPARSE_DISPATCH(dtype, {
    if (!accumulate) {  // (out is contiguous when it is filled here: checked by the host)
      if (rows * n > 0) PTHIP_CHECK(pthip::memset_async(out, 0, (size_t)(rows * n) * sizeof(T), st));
    }
    if (rows <= 0 || nnz <= 0) return 0;
    PTHIP_KLAUNCH(todense_kernel<T>, dim3(grid_for(rows, BLOCK)), dim3(BLOCK), 0, st, rows, n, nnz, (const T*)data, (const int*)indices,
                  (const int*)indptr, (T*)out, so0, so1, status);
    return pthip::post_launch("csr_todense");
  })
}

extern "C" int pthip_csr_fromdense_count(int dtype, int64_t rows, int64_t n, const void* x, int64_t sx0, int64_t sx1, void* indptr) {
  PTHIP_REQUIRE_INIT();
  hipStream_t st = pthip::ctx().stream;
  if (rows <= 0) {
    PTHIP_CHECK(pthip::memset_async(indptr, 0, sizeof(int), st));
    return 0;
  }
  void* counts = nullptr;
  int r = pthip_alloc((size_t)rows * sizeof(int), &counts);
  if (r) return r;
  PTHIP_SPARSE_DISPATCH(dtype, {
    PTHIP_KLAUNCH(fromdense_count_kernel<T>, dim3(grid_for(rows, BLOCK / 64)), dim3(BLOCK), 0, st, rows, n, (const T*)x, sx0, sx1,
                  (int*)counts);
    r = exclusive_scan_i32((const int*)counts, rows, (int*)indptr, st);
    pthip_free(counts);
    return r ? r : pthip::post_launch("csr_fromdense_count");
  })
}

extern "C" int pthip_csr_fromdense_fill(int dtype, int64_t rows, int64_t n, const void* x, int64_t sx0, int64_t sx1, const void* indptr,
                                        void* data, void* indices) {
  PTHIP_REQUIRE_INIT();
  if (rows <= 0) return 0;
  hipStream_t st = pthip::ctx().stream;
  PTHIP_SPARSE_DISPATCH(dtype, {
    PTHIP_KLAUNCH(fromdense_fill_kernel<T>, dim3(grid_for(rows, BLOCK / 64)), dim3(BLOCK), 0, st, rows, n, (const T*)x, sx0, sx1,
                  (const int*)indptr, (T*)data, (int*)indices);
    return pthip::post_launch("csr_fromdense_fill");
  })
}

extern "C" int pthip_csr_csm_grad(int dtype, int64_t rows, int64_t nnz_x, const void* x_indices, const void* x_indptr, int64_t nnz_g,
                                  const void* g_data, const void* g_indices, const void* g_indptr, void* out) {
  PTHIP_REQUIRE_INIT();
  if (nnz_x <= 0) return 0;
  hipStream_t st = pthip::ctx().stream;
  PTHIP_SPARSE_DISPATCH(dtype, {
    PTHIP_KLAUNCH(csm_grad_kernel<T>, dim3(grid_for(nnz_x, BLOCK)), dim3(BLOCK), 0, st, rows, nnz_x, (const int*)x_indices,
                  (const int*)x_indptr, nnz_g, (const T*)g_data, (const int*)g_indices, (const int*)g_indptr, (T*)out);
    return pthip::post_launch("csr_csm_grad");
  })
}
