// wave_device.h — wave64 and workgroup primitives of the hand-written linear-algebra kernels: lane exchange, sums,
// maxima, arg-max, the block scan, |x|.  Device-only and header-only; a .hip file includes it after common.h.
// (reduce_device.h is the generated kernels' counterpart: it is pasted in front of their source and includes nothing.)
//
// Every function here is a fixed tree: the same inputs give the same bits in every lane and on every run.  Two
// functions that differ in the order of their floating-point additions have two names.  A kernel that keeps a
// butterfly written out in its own loop does so because moving it here changed its machine code.
#pragma once

namespace wave {

// ---- scalars ------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ T dev_abs(T x) { return x < T(0) ? -x : x; }
// |x| for the pivot searches, with NaN ranked as +inf: every row still in the search is a candidate (a column of NaN
// would otherwise leave none, and the "no candidate" key would index past the matrix), and a NaN pivot carries the
// NaN into the factors as LAPACK's idamax-based getrf does
template <class T> __device__ __forceinline__ T pivot_abs(T x) { return x != x ? T(INFINITY) : dev_abs(x); }

// ---- lane exchange ------------------------------------------------------------------------------------------------
// One 32-bit move per register of an int, a float or a double.
// v of the lane that the DPP control word CTRL names, all rows and banks; a lane without a source reads 0
template <int CTRL, class T> __device__ __forceinline__ T dpp_mov(T v) {
  if constexpr (sizeof(T) == 8)
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false));
  else if constexpr (T(0.5) != T(0)) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
  else return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// v of lane `lane` (wave-uniform) in every lane: v_readlane, no LDS crossbar
template <class T> __device__ __forceinline__ T lane_bcast(T v, int lane) {
  if constexpr (sizeof(T) == 8)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
  else if constexpr (T(0.5) != T(0)) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
  else return __builtin_amdgcn_readlane(v, lane);
}
// the same move of an int in the rows of ROW_MASK only; every other lane, and a lane without a source, keeps its own
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_mov_or_own(int own) {
  return __builtin_amdgcn_update_dpp(own, own, CTRL, ROW_MASK, 0xf, false);
}

// ---- sums ---------------------------------------------------------------------------------------------------------
// xor butterfly over the wave, in every lane: offsets 32 .. 1
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// ... and over each group of G lanes, offsets 1 .. G/2: the other order of additions
template <int G, class T> __device__ __forceinline__ T group_sum(T y) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) y += __shfl_xor(y, o, 64);
  return y;
}
// sum over the block; every thread gets the result (two barriers).  s_red: BLOCK / 64
template <int BLOCK, class T> __device__ T block_sum(T v, T* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = T(0);
#pragma unroll
  for (int w = 0; w < BLOCK / 64; w++) r += s_red[w];
  return r;
}

// Sums out of DPP row operations and v_readlane (no LDS permutes: __shfl_xor is a ds_bpermute round trip per step,
// six dependent ones per sum) — used where a wave sum sits on the critical path of every Jacobi rotation.
// The sum over each 16-lane row of the wave, in every lane of that row: four DPP steps, nothing else
template <class T> __device__ __forceinline__ T row_sum_dpp(T v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror: every lane of a 16-lane row holds the row's sum
  return v;
}
// The sum over the 64 lanes, in every lane, the four row sums r0, r16, r32, r48 added as (r0 + r16) + (r32 + r48) ...
template <class T> __device__ __forceinline__ T wave_sum_dpp_pairwise(T v) {
  v = row_sum_dpp(v);
  return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
// ... or as (((0 + r0) + r16) + r32) + r48: another rounding, and +0 where the pairwise sum of four -0 is -0
template <class T> __device__ __forceinline__ T wave_sum_dpp_sequential(T v) {
  v = row_sum_dpp(v);
  T t = T(0);
#pragma unroll
  for (int r = 0; r < 4; r++) t += lane_bcast(v, 16 * r);
  return t;
}

// ---- maxima -------------------------------------------------------------------------------------------------------
// max that propagates NaN (fmax drops it)
template <class T> __device__ __forceinline__ T nan_max(T a, T b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
template <class T> __device__ __forceinline__ T wave_nan_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
// for floating values that are never NaN (a partner's NaN would be dropped, an own one kept)
template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const T ov = __shfl_xor(v, o); v = ov > v ? ov : v; }
  return v;
}

// ---- arg-max ------------------------------------------------------------------------------------------------------
// (value, key) maximum: the larger value wins, the lower key among equal values; a total order, so the result does
// not depend on the order in which pairs meet
template <class T> __device__ __forceinline__ void argmax_take(T& v, int& key, T ov, int okey) {
  if (ov > v || (ov == v && okey < key)) { v = ov; key = okey; }
}
// over the wave, in every lane: the DPP steps of wave_sum_dpp_pairwise, for a search on the critical path
template <int CTRL, class T> __device__ __forceinline__ void argmax_dpp_step(T& v, int& key) {
  const T ov = dpp_mov<CTRL>(v);
  const int okey = dpp_mov<CTRL>(key);
  argmax_take(v, key, ov, okey);
}
template <class T> __device__ __forceinline__ void wave_argmax_dpp(T& v, int& key) {
  argmax_dpp_step<0xB1>(v, key);
  argmax_dpp_step<0x4E>(v, key);
  argmax_dpp_step<0x141>(v, key);
  argmax_dpp_step<0x140>(v, key);  // every lane of a 16-lane row holds the row's pair
  const T v0 = lane_bcast(v, 0);
  const int k0 = lane_bcast(key, 0);
  T bv = v0;
  int bk = k0;
  argmax_take(bv, bk, lane_bcast(v, 16), lane_bcast(key, 16));
  argmax_take(bv, bk, lane_bcast(v, 32), lane_bcast(key, 32));
  argmax_take(bv, bk, lane_bcast(v, 48), lane_bcast(key, 48));
  v = bv; key = bk;
}
// over the wave by shifts and row broadcasts towards the last lane (no v_readlane): result valid in lane 63
template <int CTRL, int ROW_MASK, class T> __device__ __forceinline__ void argmax_dpp_or_own_step(T& v, int& key) {
  T ov;
  if constexpr (sizeof(T) == 8) {
    const int lo = dpp_mov_or_own<CTRL, ROW_MASK>(__double2loint(v));
    const int hi = dpp_mov_or_own<CTRL, ROW_MASK>(__double2hiint(v));
    ov = __hiloint2double(hi, lo);
  } else {
    ov = __int_as_float(dpp_mov_or_own<CTRL, ROW_MASK>(__float_as_int(v)));
  }
  const int okey = dpp_mov_or_own<CTRL, ROW_MASK>(key);
  argmax_take(v, key, ov, okey);
}
template <class T> __device__ __forceinline__ void wave_argmax_dpp_lane63(T& v, int& key) {
  argmax_dpp_or_own_step<0x111, 0xf>(v, key);  // row_shr:1
  argmax_dpp_or_own_step<0x112, 0xf>(v, key);  // row_shr:2
  argmax_dpp_or_own_step<0x114, 0xf>(v, key);  // row_shr:4
  argmax_dpp_or_own_step<0x118, 0xf>(v, key);  // row_shr:8
  argmax_dpp_or_own_step<0x142, 0xa>(v, key);  // row_bcast:15 into rows 1, 3
  argmax_dpp_or_own_step<0x143, 0xc>(v, key);  // row_bcast:31 into rows 2, 3
}

// ---- scan ---------------------------------------------------------------------------------------------------------
// exclusive prefix sum over the block's threads, and the block's total in every thread (two barriers)
template <int BLOCK> __device__ __forceinline__ long long block_exclusive_scan(long long v, long long* total) {
  __shared__ long long s_wave[BLOCK / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_wave[wid] = incl;
  __syncthreads();
  long long base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; w++) {
    if (w < wid) base += s_wave[w];
    all += s_wave[w];
  }
  __syncthreads();
  *total = all;
  return base + incl - v;
}

}  // namespace wave
