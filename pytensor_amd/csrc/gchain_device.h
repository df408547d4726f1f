// gchain_device.h — the row-group machinery of the one-pass ``gchain`` kernel (codegen_gchain.py) in its pipelined form.
// Prepended verbatim to the hiprtc-generated kernel, so it must not include anything.
//
// A wave owns groups of RG consecutive rows and works on them in two halves of RH = RG/2 rows.  A half lives in a
// `Rows` buffer exactly as it was loaded (16-byte packs per lane and 128-column chunk); the kernel keeps two buffers
// and asks for the next half's rows before it reduces the current one, so that the dot products, the butterfly, the
// scalar graph and the ``A.T@w`` accumulation of one half run while the loads of the next are in flight.
//
// Everything here is wave-uniform control flow with all 64 lanes active (the lane-swap instructions below ignore
// nothing but EXEC): call it only from code every lane of the wave reaches.
#pragma once

namespace gchain {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned int u2 __attribute__((ext_vector_type(2)));

// The matrix is streamed once: non-temporal loads (codegen._stream_load; GCHAIN_PLAIN_LOADS: the PTHIP_NT_LOADS=0 form).
template <class V> static __device__ __forceinline__ V stream(const V* p) {
#ifdef GCHAIN_PLAIN_LOADS
  return *p;
#else
  return __builtin_nontemporal_load(p);
#endif
}

// ---- what one lane holds of one row piece, as loaded (converted to double only when it is used) ----
// PACK 2: columns {2l, 2l+1} of a 128-column chunk, one 16-byte (fp32: 8-byte) load.  PACK 1: columns {l, l+64}, two
// element loads (any K, any lda).  PACK 4 (fp32): columns {4l .. 4l+3} of a chunk PAIR — SPAN 2 chunks of the
// double-precision image.  A piece is NL loads; load i of piece q is `inside` the row when its first column is below K
// (a pack is inside or outside as a whole: K is a multiple of the pack where packs are used), and a piece that is not
// loaded stays zero.  The address is the row's wave-uniform base plus a 32-bit lane offset (the saddr form of a load).
template <int PACK, class AT> struct Piece;

template <class V, class AT> static __device__ __forceinline__ V stream_at(const AT* __restrict__ Ar, unsigned col) {
  return stream((const V*)((const char*)Ar + col * (unsigned)sizeof(AT)));
}

template <> struct Piece<2, double> {
  static constexpr int SPAN = 1, NL = 1;
  d2 v;
  static __device__ __forceinline__ bool inside(int, int q, int lane, long long K) { return q * 128 + 2 * lane < K; }
  __device__ __forceinline__ void zero() { v = (d2){0.0, 0.0}; }
  __device__ __forceinline__ void ld(int, const double* __restrict__ Ar, int q, int lane) { v = stream_at<d2>(Ar, q * 128 + 2 * lane); }
  __device__ __forceinline__ d2 get(int) const { return v; }
};
template <> struct Piece<2, float> {
  static constexpr int SPAN = 1, NL = 1;
  f2 v;
  static __device__ __forceinline__ bool inside(int, int q, int lane, long long K) { return q * 128 + 2 * lane < K; }
  __device__ __forceinline__ void zero() { v = (f2){0.f, 0.f}; }
  __device__ __forceinline__ void ld(int, const float* __restrict__ Ar, int q, int lane) { v = stream_at<f2>(Ar, q * 128 + 2 * lane); }
  __device__ __forceinline__ d2 get(int) const { return (d2){(double)v.x, (double)v.y}; }
};
template <class AT> struct Piece<1, AT> {
  static constexpr int SPAN = 1, NL = 2;
  AT a[2];
  static __device__ __forceinline__ bool inside(int i, int q, int lane, long long K) { return q * 128 + 64 * i + lane < K; }
  __device__ __forceinline__ void zero() { a[0] = a[1] = AT(0); }
  __device__ __forceinline__ void ld(int i, const AT* __restrict__ Ar, int q, int lane) { a[i] = Ar[q * 128 + 64 * i + lane]; }
  __device__ __forceinline__ d2 get(int) const { return (d2){(double)a[0], (double)a[1]}; }
};
template <> struct Piece<4, float> {
  static constexpr int SPAN = 2, NL = 1;
  f4 v;
  static __device__ __forceinline__ bool inside(int, int q, int lane, long long K) { return q * 256 + 4 * lane < K; }
  __device__ __forceinline__ void zero() { v = (f4){0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void ld(int, const float* __restrict__ Ar, int q, int lane) { v = stream_at<f4>(Ar, q * 256 + 4 * lane); }
  __device__ __forceinline__ d2 get(int sub) const { return sub ? (d2){(double)v.z, (double)v.w} : (d2){(double)v.x, (double)v.y}; }
};

// ---- RH rows x C chunks of one half group in registers ----
// FULL: K fills every chunk (K = 128 C), so no lane is ever outside a row: no predicate, no zero fill.
template <int RH, int C, int PACK, class AT, bool FULL> struct Rows {
  typedef Piece<PACK, AT> piece_t;
  static constexpr int NP = C / piece_t::SPAN;
  piece_t p[RH][NP];

  // Rows first .. first+RH-1, clamped to N-1 (never a byte past the matrix).  `first`, N and lda are wave-uniform, so
  // the row numbers, the clamp and the row base addresses are scalar work: one multiply for the half, then steps of lda.
  __device__ __forceinline__ void load(const AT* __restrict__ A, long long lda, long long first, long long N, long long K, int lane) {
    const AT* Ar[RH];
    Ar[0] = A + ((first < N) ? first : N - 1) * lda;
#pragma unroll
    for (int r = 1; r < RH; r++) Ar[r] = (first + r < N) ? Ar[r - 1] + lda : Ar[r - 1];
#pragma unroll
    for (int q = 0; q < NP; q++) {
#pragma unroll
      for (int i = 0; i < piece_t::NL; i++) {
        if constexpr (FULL) {
#pragma unroll
          for (int r = 0; r < RH; r++) p[r][q].ld(i, Ar[r], q, lane);
        } else {
          if (i == 0) {
#pragma unroll
            for (int r = 0; r < RH; r++) p[r][q].zero();
          }
          if (piece_t::inside(i, q, lane, K)) {
#pragma unroll
            for (int r = 0; r < RH; r++) p[r][q].ld(i, Ar[r], q, lane);
          }
        }
      }
    }
  }
  __device__ __forceinline__ d2 get(int r, int c) const { return p[r][c / piece_t::SPAN].get(c % piece_t::SPAN); }

  // the lane's share of every row's dot product with the multiplier vector.  The expression is the plain loop's, letter
  // for letter, and so is the one in axpy(): both loops are compiled with the default fp contraction, and that the
  // compiler contracts the two sources alike is not pinned by anything here — the bitwise comparison of the two loops in
  // tests/test_zz_gpu_gchain_pipeline.py is the guard.
  __device__ __forceinline__ void dots(const d2 (&b)[C], double (&out)[RH]) const {
#pragma unroll
    for (int r = 0; r < RH; r++) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < C; c++) { const d2 x = get(r, c); const d2 bc = b[c]; s += x.x * bc.x + x.y * bc.y; }
      out[r] = s;
    }
  }
  // acc[c] += row r * wr — rows in order, the caller supplies wr
  __device__ __forceinline__ void axpy(int r, double wr, d2 (&acc)[C]) const {
#pragma unroll
    for (int c = 0; c < C; c++) { const d2 x = get(r, c); acc[c].x += x.x * wr; acc[c].y += x.y * wr; }
  }
};

// ---- lane exchanges ----
union dw { double d; unsigned int u[2]; int i[2]; };

static __device__ __forceinline__ double readlane(double v, int l) {
  dw u; u.d = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], l); u.i[1] = __builtin_amdgcn_readlane(u.i[1], l);
  return u.d;
}

// v of lane ^ D for D = 8, 2, 1: one DPP move per 32-bit word (row_ror:8 | quad_perm [2,3,0,1] | quad_perm [1,0,3,2]).
// D = 4 stays a ds_bpermute; its two-move DPP form (row_shl:4 on banks 0 and 2, row_shr:4 on banks 1 and 3) was not tried.
template <int D> static __device__ __forceinline__ double xor_lane(double v) {
  dw u; u.d = v;
  if constexpr (D == 8 || D == 2 || D == 1) {
    constexpr int ctrl = D == 8 ? 0x128 : (D == 2 ? 0x4E : 0xB1);
    u.i[0] = __builtin_amdgcn_update_dpp(0, u.i[0], ctrl, 0xf, 0xf, true);
    u.i[1] = __builtin_amdgcn_update_dpp(0, u.i[1], ctrl, 0xf, 0xf, true);
  } else {
    u.i[0] = __shfl_xor(u.i[0], D, 64); u.i[1] = __shfl_xor(u.i[1], D, 64);
  }
  return u.d;
}

// One exchange of a transposing butterfly step at distance D: lanes with bit D clear end up with x(lane) + x(lane ^ D),
// lanes with bit D set with y(lane) + y(lane ^ D) — ``keep + recv`` of the select-and-shuffle form, the same two
// addends on every lane.  D = 32 / 16: the gfx950 half-swaps exchange the upper half (odd rows of 16) of x with the
// lower half (even rows) of y in place: two swaps and one add, no select, no LDS crossbar.
template <int D> static __device__ __forceinline__ double xchg_add(double x, double y, int lane) {
  if constexpr (D == 32 || D == 16) {
    dw a, b; a.d = x; b.d = y;
#pragma unroll
    for (int w = 0; w < 2; w++) {
      u2 r;
      if constexpr (D == 32) r = __builtin_amdgcn_permlane32_swap(a.u[w], b.u[w], false, false);
      else r = __builtin_amdgcn_permlane16_swap(a.u[w], b.u[w], false, false);
      a.u[w] = r.x; b.u[w] = r.y;
    }
    return a.d + b.d;
  } else {
    const bool up = (lane & D) != 0;
    const double send = up ? x : y, keep = up ? y : x;
    return keep + xor_lane<D>(send);
  }
}

// One half group through the butterfly: p[r] is the lane's share of row r; returns the finished dot product of row
// (lane >> (6 - log2 RH)) & (RH - 1).  log2(RH) transposing steps (every lane gives away half of its rows), then plain
// ones; the pairwise add tree of a row is lanes at distance 32, 16, 8, 4, 2, 1 in that order, whatever RH is.
template <int RH, int D = 32> static __device__ __forceinline__ double butterfly(double (&p)[RH], int lane) {
  if constexpr (RH > 1) {
    double q[RH / 2];
#pragma unroll
    for (int i = 0; i < RH / 2; i++) q[i] = xchg_add<D>(p[i], p[i + RH / 2], lane);
    return butterfly<RH / 2, D / 2>(q, lane);
  } else {
    double v = p[0];
    if constexpr (D >= 32) v = xchg_add<32>(v, v, lane);
    if constexpr (D >= 16) v = xchg_add<16>(v, v, lane);
    if constexpr (D >= 8) v += xor_lane<8>(v);
    if constexpr (D >= 4) v += xor_lane<4>(v);
    if constexpr (D >= 2) v += xor_lane<2>(v);
    v += xor_lane<1>(v);
    return v;
  }
}

// The halves finish their rows on other lanes than the whole-group butterfly did (row j of half h on lane
// j << (7 - log2 RG) instead of row r on lane r << (6 - log2 RG)), so a per-lane reduction accumulator is kept per
// half and moved once, after the row loop, to the lane that owned those rows: the block combine that follows sees the
// values it always saw, in the same lanes.
template <int RG, class T> static __device__ __forceinline__ T to_group_lanes(T a0, T a1, T identity, int lane) {
  constexpr int RH = RG / 2;
  int lg = 0;
  for (int v = RG; v > 1; v >>= 1) lg++;
  const int rest = 6 - lg, resth = rest + 1;
  const int r = (lane >> rest) & (RG - 1);
  const int src = (r & (RH - 1)) << resth;
  constexpr int NW = (sizeof(T) + 3) / 4;
  union { T t; int i[NW]; } u0, u1;
#pragma unroll
  for (int w = 0; w < NW; w++) u0.i[w] = u1.i[w] = 0;
  u0.t = a0; u1.t = a1;
#pragma unroll
  for (int w = 0; w < NW; w++) { u0.i[w] = __shfl(u0.i[w], src, 64); u1.i[w] = __shfl(u1.i[w], src, 64); }
  const bool owner = (lane & ((1 << rest) - 1)) == 0;
  return owner ? (r >= RH ? u1.t : u0.t) : identity;
}

}  // namespace gchain
