// spgemm.hip — C = A·B for two stored CSR matrices (TrueDot of two sparse operands) on gfx950.
//
// Reference: TrueDot.perform (pytensor/sparse/math.py: scipy's x * y, csr_matmat).  A is rows x k, B is k x n, int32
// indices / indptr, float32 / float64 data; a csc operand is the CSR of its transpose (dispatch/sparse.py picks the
// operand order).  Gustavson's row-wise form: row i of C is the sum over the entries (i, c) of A of a_ic · (row c of
// B).  As in sparse.hip nothing assumes sorted indices or the absence of duplicates, a column index out of range
// sets status bit 0 (IndexError) and the entry is skipped, and row extents are clamped to the arrays.
//
// Result: an entry is stored iff its computed value != 0 (NaN kept, exact cancellations dropped: csr_matmat), the
// indices of every row sorted and free of duplicates.
//
// Order.  The scalar products of row i are numbered p = 0 .. ub[i] - 1: A's entries of the row in stored order and,
// inside each, B's entries of that row in stored order (scipy's order).  The products that land on one (i, j) are
// added in increasing p, whatever the tier: a group of NT lanes takes NT consecutive p at a time (a "chunk"), lane l
// the l-th, and lanes of one chunk that hit the same column add one after the other in lane order — each pending
// lane does an integer atomicMin of its lane number on the column's owner word, the lowest adds and releases, the
// next round follows.  No floating-point atomics; integer atomics only claim hash slots, elect owners and fill the
// row lists, none of which reaches the result.  A lane finds its (A entry, offset into B's row) by binary search in
// an LDS prefix array of the B-row lengths of up to NT entries of A's row ("piece"), so a stencil row (5 entries of
// 5) fills a wave instead of running 5 steps of 5 lanes; a longer A row goes through the array piece by piece.
//
// Passes (the host reads two 4-byte totals, nothing per row):
//   1. bound and bin: ub[i] = sum of len(B row col(e)) over row i of A; one list of row numbers per tier (integer
//      atomic counter: the order inside a list is free, rows are independent).  Every tier's kernel is launched every
//      time, walks its list grid-stride and leaves at once when the list is empty.
//   2. structure: the distinct columns per row -> exclusive scan -> indptr_s.  Host read 1: the structural nnz.
//   3. values: accumulate, sort the row's columns, store (col, value) at indptr_s[i]; the entries != 0 per row ->
//      exclusive scan.  Host read 2: the final nnz.
//   4. compaction (only when the totals differ): a stable per-row copy of the entries != 0.
// Pass 2 is pass 3's code with the value work compiled out (template flag VALUES).
//
// Tiers by ub[i]:
//   wave      ub <= kWaveUb: a wave per row, four rows per workgroup; per wave an open-addressing table in LDS
//             (int32 keys, an owner word and a value per slot) of 2 * kWaveUb slots, of which a row clears and uses
//             the power of two >= 2 * ub (at least 64).
//   workgroup ub <= kWgUb: 256 lanes per row, one table of 2 * kWgUb slots; barriers between the owner rounds.
//   dense row anything larger: each resident workgroup owns n values and n flag bytes of the workspace, scatters with
//             one owner per column per chunk (elected in a chunk-local LDS table), then sweeps the row in column
//             order, which emits sorted output and clears the workspace row for the next use.
// After accumulation a hash tier compacts the row's d distinct keys into the (now idle) owner words, sorts them with a
// bitonic network in LDS and fetches each key's value by one probe.
//
// dense_out: the value pass adds every row into a strided dense array through the chunk-local election of the dense
// tier instead of a table (no passes 2 and 4): the numeric pass a sparse x sparse Dot with a dense result needs.
#include "common.h"
#include "csr_device.h"
#include "wave_device.h"

#include <climits>

// packed fp32 arithmetic is kept out of this file's device code: scalar v_fma_f32 only
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
// Tier bounds, from the 160 KB of LDS per CU at 16 bytes per slot (fp64): 4 x 2 * 256 slots = 32 KB per wave-tier
// workgroup, so four of them share a CU; 2 * 4096 slots = 128 KB, the one workgroup-tier table a CU holds.
constexpr int kWaveUb = 256;   // (dispatch/sparse.py SPGEMM_WAVE_UB)
constexpr int kWgUb = 4096;    // (dispatch/sparse.py SPGEMM_WG_UB)
constexpr int kEmpty = -1;       // hash key of a free slot
constexpr int kFree = INT_MAX;   // owner word nobody holds; also the padding of the sort
constexpr int kBinLanes = 8;     // lanes per row of the bound pass
constexpr size_t kDenseBudget = (size_t)256 << 20;  // bytes of dense-row workspace, at most (one row is always kept)

template <typename T>
struct Mat {
  const T* data;
  const int* ind;
  const int* indptr;
  long long nnz;
};

template <typename T>
struct Job {
  Mat<T> A, B;
  long long rows, k, n;
  const int* ub;        // rows: the products of each row, saturated
  const int* lists;     // tier t: lists + t * rows
  const int* counters;  // the length of each list
  int* counts;          // rows: distinct columns (structure) / entries != 0 (values)
  const int* indptr_s;  // values: where each row's entries go
  int* out_ind;
  T* out_data;
  T* dense;  // dense_out: out[i * ds0 + j * ds1]
  long long ds0, ds1;
  int* status;
};

// the LDS of one group of NT lanes with a table of S slots
template <typename T, int NT, int S>
struct Lds {
  T vals[S];
  T aval[NT];               // piece: A's values
  long long pref[NT + 1];   // piece: exclusive prefix of the B-row lengths
  int keys[S];
  int owner[S];             // owner words while accumulating, then the sort buffer
  int bstart[NT];           // piece: first entry of each B row
  int cnt[2];
};

template <int NT>
__device__ __forceinline__ void sync() {
  if constexpr (NT == WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

template <int NT>
__device__ __forceinline__ bool any(bool p) {
  if constexpr (NT == WAVE) return __ballot(p) != 0;
  else return __syncthreads_or(p) != 0;
}

template <int NT>
__device__ __forceinline__ long long inclusive_scan(long long v, long long* total) {
  if constexpr (NT == WAVE) {
    const int lane = threadIdx.x & 63;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(incl, o);
      if (lane >= o) incl += u;
    }
    *total = __shfl(incl, 63);
    return incl;
  } else {
    return wave::block_exclusive_scan<NT>(v, total) + v;
  }
}

template <int NT>
__device__ __forceinline__ int group_sum(int v) {
  long long total;
  inclusive_scan<NT>(v, &total);
  return (int)total;
}

__device__ __forceinline__ unsigned slot_of(int col, int lg) { return ((unsigned)col * 2654435761u) >> (32 - lg); }

// Row i of A·B through the group's table of 1 << lg slots.
//   !DENSE: the table belongs to the row (the caller cleared it): keys claim slots, VALUES adds into vals.  Returns
//           this lane's number of newly claimed slots (their sum over the group: the distinct columns).
//   DENSE:  the table belongs to the chunk and only elects owners; VALUES adds into drow[col * ds] (and sets
//           flags[col] when given), !VALUES only sets flags[col].
template <typename T, int NT, int S, bool VALUES, bool DENSE>
__device__ int accumulate_row(Lds<T, NT, S>& L, const int t, const int lg, const Job<T>& j, const long long i, T* drow,
                              const long long ds, unsigned char* flags) {
  const unsigned mask = (1u << lg) - 1;
  int fresh = 0;
  long long lo, hi;
  csr::row_extent(j.A.indptr, i, j.A.nnz, &lo, &hi);
  for (long long e0 = lo; e0 < hi; e0 += NT) {  // a piece: NT entries of A's row
    const long long e = e0 + t;
    long long bl = 0, bh = 0;
    if (e < hi) {
      const int c = j.A.ind[e];
      if (c < 0 || c >= j.k) atomicOr(j.status, 1);
      else csr::row_extent(j.B.indptr, c, j.B.nnz, &bl, &bh);
      if constexpr (VALUES) L.aval[t] = j.A.data[e];
    }
    L.bstart[t] = (int)bl;
    long long total;
    L.pref[t + 1] = inclusive_scan<NT>(bh - bl, &total);
    if (t == 0) L.pref[0] = 0;
    sync<NT>();
    for (long long p0 = 0; p0 < total; p0 += NT) {  // a chunk: NT products
      const long long p = p0 + t;
      bool act = p < total;
      int col = 0;
      T prod = 0;
      if (act) {
        int a = 0, b = NT;  // pref[a] <= p < pref[b]
        while (b - a > 1) {
          const int mid = (a + b) >> 1;
          if (L.pref[mid] <= p) a = mid; else b = mid;
        }
        const long long be = L.bstart[a] + (p - L.pref[a]);
        col = j.B.ind[be];
        if (col < 0 || col >= j.n) {
          atomicOr(j.status, 1);
          act = false;
        } else if constexpr (VALUES) {
          prod = L.aval[a] * j.B.data[be];
        }
      }
      if constexpr (DENSE && !VALUES) {
        if (act) flags[col] = 1;
      } else {
        if constexpr (DENSE) {
          static_assert(S == 2 * NT, "the chunk-local table");
          L.keys[t] = L.keys[t + NT] = kEmpty;
          L.owner[t] = L.owner[t + NT] = kFree;
          sync<NT>();
        }
        unsigned slot = 0;
        if (act) {
          slot = slot_of(col, lg);
          for (;;) {  // (never full: at most half the slots are ever claimed)
            const int old = atomicCAS(&L.keys[slot], kEmpty, col);
            if (old == kEmpty) fresh++;
            if (old == kEmpty || old == col) break;
            slot = (slot + 1) & mask;
          }
        }
        if constexpr (VALUES) {
          bool pending = act;
          while (any<NT>(pending)) {  // one round per lane that shares a column within the chunk
            if (pending) atomicMin(&L.owner[slot], t);
            sync<NT>();
            if (pending && L.owner[slot] == t) {
              if constexpr (DENSE) {
                drow[(long long)col * ds] += prod;
                if (flags) flags[col] = 1;
              } else {
                L.vals[slot] += prod;
              }
              L.owner[slot] = kFree;
              pending = false;
            }
            sync<NT>();
          }
        }
      }
    }
    sync<NT>();  // the piece arrays are rewritten next
  }
  return fresh;
}

template <int NT>
__device__ void bitonic_sort(int* a, const int P, const int t) {  // P a power of two; ends on a sync
  for (int k = 2; k <= P; k <<= 1)
    for (int d = k >> 1; d > 0; d >>= 1) {
      for (int x = t; x < P; x += NT) {
        const int y = x ^ d;
        if (y > x) {
          const int ax = a[x], ay = a[y];
          if ((ax > ay) == ((x & k) == 0)) {
            a[x] = ay;
            a[y] = ax;
          }
        }
      }
      sync<NT>();
    }
}

// ---- pass 1: products per row, and the tier lists ------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void bound_bin_kernel(long long rows, long long k, long long nnz_a, const int* __restrict__ a_ind,
                                                          const int* __restrict__ a_ptr, long long nnz_b, const int* __restrict__ b_ptr,
                                                          int* __restrict__ ub, int* __restrict__ lists, int* __restrict__ counters,
                                                          int* __restrict__ counts, int* status) {
  const int sub = threadIdx.x % kBinLanes;
  const long long groups = (long long)gridDim.x * (BLOCK / kBinLanes);
  for (long long r = (long long)blockIdx.x * (BLOCK / kBinLanes) + threadIdx.x / kBinLanes; r < rows; r += groups) {
    long long lo, hi, s = 0;
    csr::row_extent(a_ptr, r, nnz_a, &lo, &hi);
    for (long long e = lo + sub; e < hi; e += kBinLanes) {
      const int c = a_ind[e];
      if (c < 0 || c >= k) {
        atomicOr(status, 1);
        continue;
      }
      long long bl, bh;
      csr::row_extent(b_ptr, c, nnz_b, &bl, &bh);
      s += bh - bl;
    }
    for (int o = kBinLanes / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kBinLanes);
    if (sub == 0) {
      ub[r] = s > INT_MAX ? INT_MAX : (int)s;
      counts[r] = 0;  // (a row without products is in no list)
      if (s > 0) {
        const int tier = s <= kWaveUb ? 0 : s <= kWgUb ? 1 : 2;
        lists[tier * rows + atomicAdd(&counters[tier], 1)] = (int)r;
      }
    }
  }
}

// ---- the hash tiers: NT = 64, a wave per row; NT = 256, the workgroup per row ------------------------------------
template <typename T, int NT, int S, bool VALUES>
__global__ __launch_bounds__(BLOCK) void hash_kernel(const Job<T> j, const int tier) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  constexpr int G = BLOCK / NT;
  Lds<T, NT, S>& L = reinterpret_cast<Lds<T, NT, S>*>(lds_raw)[threadIdx.x / NT];
  const int t = threadIdx.x % NT;
  const int cnt = j.counters[tier];
  const int* list = j.lists + tier * j.rows;
  for (long long q = (long long)blockIdx.x * G + threadIdx.x / NT; q < cnt; q += (long long)gridDim.x * G) {
    const long long i = list[q];
    int lg = 6;
    while ((1 << lg) < 2 * j.ub[i] && (1 << lg) < S) lg++;  // (ub <= S / 2 in this tier)
    const int slots = 1 << lg;
    const unsigned mask = slots - 1;
    for (int s = t; s < slots; s += NT) {
      L.keys[s] = kEmpty;
      L.owner[s] = kFree;
      if constexpr (VALUES) L.vals[s] = 0;
    }
    if (t == 0) L.cnt[0] = 0;
    sync<NT>();
    const int fresh = accumulate_row<T, NT, S, VALUES, false>(L, t, lg, j, i, nullptr, 0, nullptr);
    if constexpr (!VALUES) {
      const int d = group_sum<NT>(fresh);
      if (t == 0) j.counts[i] = d;
    } else {
      // the distinct keys, in any order, into the owner words (all free again): then sorted
      for (int s = t; s < slots; s += NT) {
        const int key = L.keys[s];
        if (key != kEmpty) L.owner[atomicAdd(&L.cnt[0], 1)] = key;
      }
      sync<NT>();
      const int d = L.cnt[0];  // (<= ub <= slots / 2; the words from d on still hold kFree, the largest int)
      int P = 1;
      while (P < d) P <<= 1;
      bitonic_sort<NT>(L.owner, P, t);
      const long long base = j.indptr_s[i];
      int nz = 0;
      for (int r = t; r < d; r += NT) {
        const int col = L.owner[r];
        unsigned slot = slot_of(col, lg);
        while (L.keys[slot] != col) slot = (slot + 1) & mask;
        const T v = L.vals[slot];
        j.out_ind[base + r] = col;
        j.out_data[base + r] = v;
        nz += v != T(0);
      }
      nz = group_sum<NT>(nz);
      if (t == 0) j.counts[i] = nz;
    }
    sync<NT>();  // the next row clears the table
  }
}

// ---- the dense-row tier: workgroup b owns row b of the workspace (n8 values, n8 flag bytes; n8 = n up to 8) --------
template <typename T, bool VALUES>
__global__ __launch_bounds__(BLOCK) void dense_row_kernel(const Job<T> j, T* __restrict__ ws_vals, unsigned char* __restrict__ ws_flags,
                                                          const long long n8) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  Lds<T, BLOCK, 2 * BLOCK>& L = *reinterpret_cast<Lds<T, BLOCK, 2 * BLOCK>*>(lds_raw);
  const int t = threadIdx.x;
  const int cnt = j.counters[2];
  if ((int)blockIdx.x >= cnt) return;
  const int* list = j.lists + 2 * j.rows;
  T* wv = ws_vals + (long long)blockIdx.x * n8;
  unsigned char* wf = ws_flags + (long long)blockIdx.x * n8;
  if constexpr (!VALUES) {  // first use of the workspace row in this product: the sweeps keep it clear from here on
    for (long long c = (long long)t * 8; c < n8; c += BLOCK * 8) {
      *reinterpret_cast<unsigned long long*>(wf + c) = 0;
#pragma unroll
      for (int b = 0; b < 8; b++) wv[c + b] = 0;
    }
    __syncthreads();
  }
  for (long long q = blockIdx.x; q < cnt; q += gridDim.x) {
    const long long i = list[q];
    accumulate_row<T, BLOCK, 2 * BLOCK, VALUES, true>(L, t, 9, j, i, wv, 1, wf);
    __syncthreads();
    // the sweep, 8 columns per lane: count (structure) or emit in column order (values), and clear
    long long pos = VALUES ? j.indptr_s[i] : 0;
    const long long first = pos;
    int nz = 0;
    for (long long c0 = 0; c0 < n8; c0 += BLOCK * 8) {
      const long long c = c0 + (long long)t * 8;
      const unsigned long long f = c < n8 ? *reinterpret_cast<const unsigned long long*>(wf + c) : 0ull;
      long long total;
      long long p = pos + wave::block_exclusive_scan<BLOCK>((long long)__popcll(f), &total);
      if (f) {
        if constexpr (VALUES) {
#pragma unroll
          for (int b = 0; b < 8; b++)
            if ((f >> (8 * b)) & 1) {
              const T v = wv[c + b];
              j.out_ind[p] = (int)(c + b);
              j.out_data[p] = v;
              nz += v != T(0);
              wv[c + b] = 0;
              p++;
            }
        }
        *reinterpret_cast<unsigned long long*>(wf + c) = 0;
      }
      pos += total;
    }
    const int kept = VALUES ? group_sum<BLOCK>(nz) : (int)(pos - first);
    if (t == 0) j.counts[i] = kept;
    __syncthreads();
  }
}

// ---- dense_out: every row of a tier's list added into its row of a dense array -----------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(BLOCK) void dense_out_kernel(const Job<T> j, const int tier) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  constexpr int G = BLOCK / NT;
  Lds<T, NT, 2 * NT>& L = reinterpret_cast<Lds<T, NT, 2 * NT>*>(lds_raw)[threadIdx.x / NT];
  const int cnt = j.counters[tier];
  const int* list = j.lists + tier * j.rows;
  for (long long q = (long long)blockIdx.x * G + threadIdx.x / NT; q < cnt; q += (long long)gridDim.x * G) {
    const long long i = list[q];
    accumulate_row<T, NT, 2 * NT, true, true>(L, threadIdx.x % NT, NT == WAVE ? 7 : 9, j, i, j.dense + i * j.ds0, j.ds1, nullptr);
  }
}

// ---- pass 4: the entries != 0 of each row, in order, to their final place (a wave per row) -------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void compact_kernel(long long rows, const int* __restrict__ indptr_s, const int* __restrict__ ind,
                                                        const T* __restrict__ data, const int* __restrict__ indptr,
                                                        int* __restrict__ ind_out, T* __restrict__ data_out) {
  const int lane = threadIdx.x & 63;
  const unsigned long long lt = (1ull << lane) - 1;
  for (long long r = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * (BLOCK / 64)) {
    const long long hi = indptr_s[r + 1];
    long long pos = indptr[r];
    for (long long e0 = indptr_s[r]; e0 < hi; e0 += 64) {
      const long long e = e0 + lane;
      const T v = e < hi ? data[e] : T(0);
      const bool keep = e < hi && v != T(0);
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const long long p = pos + __popcll(m & lt);
        data_out[p] = v;
        ind_out[p] = ind[e];
      }
      pos += __popcll(m);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the workspace: counters[4] | ub[rows] | lists[3 rows] | counts[rows] | dense rows: values, then flags
struct Layout {
  size_t ub, lists, counts, vals, flags, total;
  long long n8;
  int wgs;  // resident dense-row workgroups (0: no dense-row tier)
};

Layout layout(int esize, long long rows, long long n, bool dense) {
  Layout l;
  l.ub = 4 * sizeof(int);
  l.lists = l.ub + (size_t)rows * sizeof(int);
  l.counts = l.lists + (size_t)rows * 3 * sizeof(int);
  l.vals = (l.counts + (size_t)rows * sizeof(int) + 15) & ~(size_t)15;
  l.n8 = (n + 7) & ~7ll;
  const size_t per = (size_t)l.n8 * (esize + 1);
  long long w = per ? (long long)(kDenseBudget / per) : 0;
  w = w < 1 ? 1 : (w > pthip::kNumCU ? pthip::kNumCU : w);
  l.wgs = dense ? (int)(w < rows ? w : rows) : 0;
  l.flags = l.vals + (size_t)l.wgs * l.n8 * esize;
  l.total = l.flags + (size_t)l.wgs * l.n8;
  return l;
}

inline unsigned grid_for(long long work, int per_block, long long cap) {
  long long b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <typename T>
Job<T> make_job(long long rows, long long k, long long n, long long nnz_a, const void* a_data, const void* a_ind, const void* a_ptr,
                long long nnz_b, const void* b_data, const void* b_ind, const void* b_ptr, void* ws, const Layout& l) {
  Job<T> j{};
  j.A = {(const T*)a_data, (const int*)a_ind, (const int*)a_ptr, nnz_a};
  j.B = {(const T*)b_data, (const int*)b_ind, (const int*)b_ptr, nnz_b};
  j.rows = rows, j.k = k, j.n = n;
  char* w = (char*)ws;
  j.counters = (const int*)w;
  j.ub = (const int*)(w + l.ub);
  j.lists = (const int*)(w + l.lists);
  j.counts = (int*)(w + l.counts);
  j.status = pthip::ctx().status_dev;
  return j;
}

template <typename T>
int bound_and_bin(const Job<T>& j, hipStream_t st) {
  PTHIP_CHECK(pthip::memset_async((void*)j.counters, 0, 4 * sizeof(int), st));
  PTHIP_KLAUNCH(bound_bin_kernel, dim3(grid_for(j.rows, BLOCK / kBinLanes, 1 << 16)), dim3(BLOCK), 0, st, j.rows, j.k, j.A.nnz, j.A.ind,
                j.A.indptr, j.B.nnz, j.B.indptr, (int*)j.ub, (int*)j.lists, (int*)j.counters, j.counts, j.status);
  return 0;
}

// the three tier kernels over their lists (pass 2: VALUES = false, pass 3: true)
template <typename T, bool VALUES>
int run_tiers(const Job<T>& j, const Layout& l, void* ws, hipStream_t st) {
  using LW = Lds<T, WAVE, 2 * kWaveUb>;
  using LG = Lds<T, BLOCK, 2 * kWgUb>;
  using LD = Lds<T, BLOCK, 2 * BLOCK>;
  constexpr size_t lds_w = sizeof(LW) * (BLOCK / WAVE), lds_g = sizeof(LG), lds_d = sizeof(LD);
  static_assert(lds_g <= (size_t)pthip::kLdsPerCU && 4 * lds_w <= (size_t)pthip::kLdsPerCU, "tier bounds against the LDS of a CU");
  auto kw = hash_kernel<T, WAVE, 2 * kWaveUb, VALUES>;
  auto kg = hash_kernel<T, BLOCK, 2 * kWgUb, VALUES>;
  if (int r = pthip::lds_opt_in((const void*)kg, lds_g)) return r;
  PTHIP_KLAUNCH(kw, dim3(grid_for(j.rows, BLOCK / WAVE, 8 * pthip::kNumCU)), dim3(BLOCK), lds_w, st, j, 0);
  PTHIP_KLAUNCH(kg, dim3(grid_for(j.rows, 1, pthip::kNumCU)), dim3(BLOCK), lds_g, st, j, 1);
  if (l.wgs > 0) {
    char* w = (char*)ws;
    PTHIP_KLAUNCH((dense_row_kernel<T, VALUES>), dim3((unsigned)l.wgs), dim3(BLOCK), lds_d, st, j, (T*)(w + l.vals),
                  (unsigned char*)(w + l.flags), l.n8);
  }
  return 0;
}

template <typename T>
int structure_t(long long rows, long long k, long long n, long long nnz_a, const void* a_ind, const void* a_ptr, long long nnz_b,
                const void* b_ind, const void* b_ptr, void* ws, const Layout& l, void* indptr_out) {
  hipStream_t st = pthip::ctx().stream;
  Job<T> j = make_job<T>(rows, k, n, nnz_a, nullptr, a_ind, a_ptr, nnz_b, nullptr, b_ind, b_ptr, ws, l);
  int r;
  if ((r = bound_and_bin(j, st)) || (r = run_tiers<T, false>(j, l, ws, st))) return r;
  if ((r = pthip_exclusive_scan_i32(rows, j.counts, indptr_out))) return r;
  return pthip::post_launch("spgemm_structure");
}

template <typename T>
int values_t(long long rows, long long k, long long n, long long nnz_a, const void* a_data, const void* a_ind, const void* a_ptr,
             long long nnz_b, const void* b_data, const void* b_ind, const void* b_ptr, void* ws, const Layout& l, const void* indptr_s,
             void* indices, void* data, void* indptr_out) {
  hipStream_t st = pthip::ctx().stream;
  Job<T> j = make_job<T>(rows, k, n, nnz_a, a_data, a_ind, a_ptr, nnz_b, b_data, b_ind, b_ptr, ws, l);
  j.indptr_s = (const int*)indptr_s;
  j.out_ind = (int*)indices;
  j.out_data = (T*)data;
  int r;
  if ((r = run_tiers<T, true>(j, l, ws, st))) return r;
  if ((r = pthip_exclusive_scan_i32(rows, j.counts, indptr_out))) return r;
  return pthip::post_launch("spgemm_values");
}

template <typename T>
int dense_out_t(long long rows, long long k, long long n, long long nnz_a, const void* a_data, const void* a_ind, const void* a_ptr,
                long long nnz_b, const void* b_data, const void* b_ind, const void* b_ptr, void* ws, const Layout& l, void* out,
                long long so0, long long so1) {
  hipStream_t st = pthip::ctx().stream;
  Job<T> j = make_job<T>(rows, k, n, nnz_a, a_data, a_ind, a_ptr, nnz_b, b_data, b_ind, b_ptr, ws, l);
  j.dense = (T*)out, j.ds0 = so0, j.ds1 = so1;
  int r;
  if ((r = bound_and_bin(j, st))) return r;
  constexpr size_t lds_w = sizeof(Lds<T, WAVE, 2 * WAVE>) * (BLOCK / WAVE), lds_g = sizeof(Lds<T, BLOCK, 2 * BLOCK>);
  PTHIP_KLAUNCH((dense_out_kernel<T, WAVE>), dim3(grid_for(rows, BLOCK / WAVE, 8 * pthip::kNumCU)), dim3(BLOCK), lds_w, st, j, 0);
  for (int tier = 1; tier <= 2; tier++)
    PTHIP_KLAUNCH((dense_out_kernel<T, BLOCK>), dim3(grid_for(rows, 1, 8 * pthip::kNumCU)), dim3(BLOCK), lds_g, st, j, tier);
  return pthip::post_launch("spgemm_dense");
}

}  // namespace

#define PTHIP_SPGEMM_DISPATCH(dtype, call)                                         \
  switch (dtype) {                                                                 \
    case PTHIP_F32: { using T = float; call; }                                     \
    case PTHIP_F64: { using T = double; call; }                                    \
    default: return pthip::set_error("pthip spgemm: unsupported dtype %d", dtype); \
  }

#define PTHIP_SPGEMM_LAYOUT(name)                                                                                         \
  if (rows < 0 || k < 0 || n < 0 || rows >= INT_MAX || n >= INT_MAX - 8)                                                  \
    return pthip::set_error(name ": int32 index range exceeded");                                                        \
  const int esize = pthip::dtype_size(dtype);                                                                             \
  const bool dense_tier = ws_bytes > layout(esize, rows, n, false).total;                                                 \
  const Layout l = layout(esize, rows, n, dense_tier);                                                                    \
  if (!ws || ws_bytes < l.total) return pthip::set_error(name ": workspace of %zu bytes, %zu needed", ws_bytes, l.total)

extern "C" size_t pthip_spgemm_workspace(int dtype, int64_t rows, int64_t n, int dense_tier) {
  return layout(pthip::dtype_size(dtype), rows < 0 ? 0 : rows, n < 0 ? 0 : n, dense_tier != 0).total;
}

extern "C" int pthip_spgemm_structure(int dtype, int64_t rows, int64_t k, int64_t n, int64_t nnz_a, const void* a_indices,
                                      const void* a_indptr, int64_t nnz_b, const void* b_indices, const void* b_indptr, void* ws,
                                      size_t ws_bytes, void* indptr_out) {
  PTHIP_REQUIRE_INIT();
  PTHIP_SPGEMM_LAYOUT("pthip_spgemm_structure");
  PTHIP_SPGEMM_DISPATCH(dtype, return structure_t<T>(rows, k, n, nnz_a, a_indices, a_indptr, nnz_b, b_indices, b_indptr, ws, l, indptr_out))
}

extern "C" int pthip_spgemm_values(int dtype, int64_t rows, int64_t k, int64_t n, int64_t nnz_a, const void* a_data, const void* a_indices,
                                   const void* a_indptr, int64_t nnz_b, const void* b_data, const void* b_indices, const void* b_indptr,
                                   void* ws, size_t ws_bytes, const void* indptr_s, void* indices, void* data, void* indptr_out) {
  PTHIP_REQUIRE_INIT();
  PTHIP_SPGEMM_LAYOUT("pthip_spgemm_values");
  PTHIP_SPGEMM_DISPATCH(dtype, return values_t<T>(rows, k, n, nnz_a, a_data, a_indices, a_indptr, nnz_b, b_data, b_indices, b_indptr, ws, l,
                                                  indptr_s, indices, data, indptr_out))
}

extern "C" int pthip_spgemm_compact(int dtype, int64_t rows, const void* indptr_s, const void* indices, const void* data,
                                    const void* indptr, void* indices_out, void* data_out) {
  PTHIP_REQUIRE_INIT();
  if (rows <= 0) return 0;
  hipStream_t st = pthip::ctx().stream;
  PTHIP_SPGEMM_DISPATCH(dtype, {
    PTHIP_KLAUNCH(compact_kernel<T>, dim3(grid_for(rows, BLOCK / 64, 1 << 20)), dim3(BLOCK), 0, st, rows, (const int*)indptr_s,
                  (const int*)indices, (const T*)data, (const int*)indptr, (int*)indices_out, (T*)data_out);
    return pthip::post_launch("spgemm_compact");
  })
}

extern "C" int pthip_spgemm_dense(int dtype, int64_t rows, int64_t k, int64_t n, int64_t nnz_a, const void* a_data, const void* a_indices,
                                  const void* a_indptr, int64_t nnz_b, const void* b_data, const void* b_indices, const void* b_indptr,
                                  void* ws, size_t ws_bytes, void* out, int64_t so0, int64_t so1) {
  PTHIP_REQUIRE_INIT();
  PTHIP_SPGEMM_LAYOUT("pthip_spgemm_dense");
  PTHIP_SPGEMM_DISPATCH(dtype, return dense_out_t<T>(rows, k, n, nnz_a, a_data, a_indices, a_indptr, nnz_b, b_data, b_indices, b_indptr, ws, l,
                                                     out, so0, so1))
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
