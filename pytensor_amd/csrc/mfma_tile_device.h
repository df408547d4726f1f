// mfma_tile_device.h — what every matrix-core tile kernel (gemm.hip, hgemm.hip, hattention.hip) has in common: the
// XCD band remap of workgroup ids, the accumulator-register -> (row, column) maps of the MFMA forms in use, accumulator
// zeroing and the fp32 k-step.  Device-only and header-only; a .hip file includes it after common.h.  Everything is
// force-inlined and restates the loops the kernels had; whether a kernel still compiles to the registers, scratch and
// instructions it had is checked per kernel (profiles/gemm_tile_header.md), and a site where it does not keeps its own
// loop.  A new kernel starts from these instead of copying a neighbour's.
#pragma once

namespace mfma {

typedef double double4_t __attribute__((ext_vector_type(4)));    // accumulator of v_mfma_f64_16x16x4_f64
typedef float float16_t __attribute__((ext_vector_type(16)));    // accumulator of the 32x32 forms
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));    // A / B fragment of v_mfma_f32_32x32x16_f16

// ---- XCD band remap ------------------------------------------------------------------------------------------------
// Workgroups are dispatched x-fastest and workgroup L runs on XCD L % 8, so XCD x is given the contiguous range
// [x*total/8, (x+1)*total/8) of the walk when total % 8 == 0: the tiles of one matrix, and the tiles of one band of a
// big matrix, share an L2.  (Remapping the tiles of one matrix only put the four 128x128 tiles of a 256x256 batch item
// on four XCDs and every operand was fetched from HBM twice.)  I: 64-bit, or unsigned where a kernel computes this per
// tile in front of its first MFMA and the walk is far below 2^31 (a 64-bit division is a few hundred instructions).
template <class I> __device__ __forceinline__ I xcd_band(I pid, I total) {
  if (total % 8 == 0) {
    const I per = total / 8;
    pid = (pid % 8) * per + pid / 8;
  }
  return pid;
}

// ---- accumulator layouts -------------------------------------------------------------------------------------------
// Each map adds an element's offset to a base of the caller's integer type (the origin of the MFMA block; 0 for the
// bare offset), term by term, so an epilogue's address arithmetic stays in the type and the order it was written in.
// 32x32 forms (32x32x2 f32 and 32x32x16 f16 alike): D reg r of lane l -> row (r&3) + 8(r>>2) + 4(l>>5), col l&31.
// acc32_reg_row adds the register's share of the row only, for addressing that keeps the lane's share in a pointer.
template <class I> __device__ __forceinline__ I acc32_reg_row(I base, int r) { return base + (r & 3) + 8 * (r >> 2); }
template <class I> __device__ __forceinline__ I acc32_row(I base, int r, int lane) { return acc32_reg_row(base, r) + 4 * (lane >> 5); }
template <class I> __device__ __forceinline__ I acc32_col(I base, int lane) { return base + (lane & 31); }
// 16x16x4 f64: D reg r of lane l -> row (l>>4) + 4r, col l&15
template <class I> __device__ __forceinline__ I acc16_row(I base, int r, int lane) { return base + (lane >> 4) + 4 * r; }
template <class I> __device__ __forceinline__ I acc16_col(I base, int lane) { return base + (lane & 15); }

// ---- zeroing -------------------------------------------------------------------------------------------------------
template <class V, int N> __device__ __forceinline__ void zero_acc(V (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int r = 0; r < (int)(sizeof(V) / sizeof(acc[i][0])); r++) acc[i][r] = 0;
}
template <class V, int NI, int NJ> __device__ __forceinline__ void zero_acc(V (&acc)[NI][NJ]) {
#pragma unroll
  for (int i = 0; i < NI; i++) zero_acc(acc[i]);
}

// ---- fp32 k-step ---------------------------------------------------------------------------------------------------
// acc[i][j] += af[i].x * bf[j].x for all i, j, then the .y pass (two k values of v_mfma_f32_32x32x2_f32 per fragment).
// Two passes so that consecutive MFMAs never share an accumulator: a dependent back-to-back pair stalls the matrix
// pipe (98 -> 102 TFLOP/s at 4096^3).
template <int NI, int NJ>
__device__ __forceinline__ void kstep_f32(float16_t (&acc)[NI][NJ], const float2 (&af)[NI], const float2 (&bf)[NJ]) {
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
}

}  // namespace mfma
