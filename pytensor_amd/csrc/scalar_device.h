
// ---- scalar helpers (formulas follow the reference c_code; citations in codegen.py) ----
#define PT_DEV static __device__ __forceinline__
template <class T> PT_DEV T pt_sqr(T x) { return x * x; }
template <class T> PT_DEV T pt_max(T x, T y) { return (y > x) ? y : ((x >= y) ? x : (T)__builtin_nan("")); }
template <class T> PT_DEV T pt_min(T x, T y) { return (y < x) ? y : ((x <= y) ? x : (T)__builtin_nan("")); }
PT_DEV bool pt_max(bool x, bool y) { return x || y; }
PT_DEV bool pt_min(bool x, bool y) { return x && y; }
PT_DEV double pt_sign(double x) { return (x > 0) ? 1. : ((x < 0) ? -1. : (isnan(x) ? __builtin_nan("") : 0.)); }
PT_DEV float pt_sign(float x) { return (x > 0) ? 1.f : ((x < 0) ? -1.f : (isnan(x) ? __builtin_nanf("") : 0.f)); }
template <class T> PT_DEV T pt_sign(T x) { return (x >= 0) ? ((x == 0) ? 0 : 1) : -1; }
// fp64 exp in 24 VALU instructions (the device library's is ~34; in BASELINE config #2 that one call was 41 % of
// the kernel's VALU work next to a 25 us HBM floor): n = rint(x log2 e); r = x - n ln2 in two FMAs (ln2_hi has 21
// trailing zero bits: n ln2_hi is exact); exp(r) = 1 + r + r^2 Q(r), Q a degree-9 Chebyshev fit on
// |r| <= ln2/2 computed with mpmath at 60 digits; 2^n by v_ldexp_f64.  <= 1 ulp from the correctly rounded
// value on 6e5 points in [-700, 700] (mean 0.10 ulp); Exp.c_code of the reference is libm's exp
// (pytensor/scalar/basic.py:3085-3118), itself < 1 ulp.  Overflow -> inf, underflow -> 0, NaN -> NaN.
PT_DEV double pt_exp(double x) {
  const double n = __builtin_rint(x * 0x1.71547652b82fep+0);
  double r = __builtin_fma(n, -0x1.62e42fee00000p-1, x);
  r = __builtin_fma(n, -0x1.a39ef35793c76p-33, r);
  double q = 0x1.af38a9b0ec855p-26;
  q = __builtin_fma(q, r, 0x1.289185613a3d6p-22);
  q = __builtin_fma(q, r, 0x1.71de0dae63bb3p-19);
  q = __builtin_fma(q, r, 0x1.a019b90d2ae7ap-16);
  q = __builtin_fma(q, r, 0x1.a01a01a7c41d5p-13);
  q = __builtin_fma(q, r, 0x1.6c16c1788bd90p-10);
  q = __builtin_fma(q, r, 0x1.11111111109b3p-7);
  q = __builtin_fma(q, r, 0x1.5555555553d63p-5);
  q = __builtin_fma(q, r, 0x1.5555555555556p-3);
  q = __builtin_fma(q, r, 0x1.0000000000001p-1);
  const double p = __builtin_fma(q * r, r, r) + 1.0;
  double y = __builtin_ldexp(p, (int)n);
  y = x > 0x1.62e42fefa39efp+9 ? __builtin_huge_val() : y;
  y = x < -0x1.74910d52d3051p+9 ? 0.0 : y;
  return y;
}
// The same exp with its constants held in registers by the caller (pt_expk_load once per kernel): in straight-line code with
// dozens of exp instances (the log-sum-exp reduction: n + 1 per tile visit, fully unrolled) the compiler materialises every
// polynomial coefficient again for every instance — v_fmac overwrites its addend, so each Horner step is two v_mov_b32 of a
// literal plus the fmac: 44 instructions per exp instead of 24 (profiles/r5w_lse_pmc.md: 94 VALU instructions per element).
// With the coefficients live in VGPRs across instances each step is one v_fma_f64.
struct pt_expk { double l2e, nh, nl, c[10], hi, lo; };
PT_DEV pt_expk pt_expk_load() {
  pt_expk k = {0x1.71547652b82fep+0, -0x1.62e42fee00000p-1, -0x1.a39ef35793c76p-33,
               {0x1.af38a9b0ec855p-26, 0x1.289185613a3d6p-22, 0x1.71de0dae63bb3p-19, 0x1.a019b90d2ae7ap-16, 0x1.a01a01a7c41d5p-13,
                0x1.6c16c1788bd90p-10, 0x1.11111111109b3p-7, 0x1.5555555553d63p-5, 0x1.5555555555556p-3, 0x1.0000000000001p-1},
               0x1.62e42fefa39efp+9, -0x1.74910d52d3051p+9};
  asm volatile("" : "+v"(k.l2e), "+v"(k.nh), "+v"(k.nl), "+v"(k.hi), "+v"(k.lo));
#pragma unroll
  for (int i = 0; i < 10; i++) asm volatile("" : "+v"(k.c[i]));
  return k;
}
PT_DEV double pt_exp_k(double x, const pt_expk& k) {
  const double n = __builtin_rint(x * k.l2e);
  double r = __builtin_fma(n, k.nh, x);
  r = __builtin_fma(n, k.nl, r);
  double q = k.c[0];
#pragma unroll
  for (int i = 1; i < 10; i++) q = __builtin_fma(q, r, k.c[i]);
  const double p = __builtin_fma(q * r, r, r) + 1.0;
  double y = __builtin_ldexp(p, (int)n);
  y = x > k.hi ? __builtin_huge_val() : y;
  y = x < k.lo ? 0.0 : y;
  return y;
}
// fp64 tanh in ~45 VALU instructions (the device library's is ~85: BASELINE config #2's transcendental variant is 10 tanh + 10
// exp per element and VALU-issue bound).  |x| < 0.35: the odd Taylor series to x^27 (coefficients 2^2n (2^2n - 1) B_2n / (2n)!
// from mpmath at 60 digits; the first neglected term is < 2e-18 relative): 0.55 ulp on 2e4 points.  Otherwise
// (1 - u) / (1 + u), u = exp(-2|x|) <= 0.497 (no cancellation in 1 - u): 1.95 ulp max, 0.52 mean on 2e4 points; saturates to
// +-1 from |x| = 19.07 on because u drops below 2^-55.  Tanh.c_code of the reference is libm's tanh (scalar/basic.py:3702;
// glibc: 1.2 ulp).  NaN -> NaN.
PT_DEV double pt_tanh(double x) {
  const double ax = __builtin_fabs(x);
  if (ax < 0.35) {
    const double z = x * x;
    double p = -0x1.b0f72d3ee24e9p-18;
    p = __builtin_fma(p, z, 0x1.0b132d39a6050p-16);
    p = __builtin_fma(p, z, -0x1.497d8eea25259p-15);
    p = __builtin_fma(p, z, 0x1.967e18afcafadp-14);
    p = __builtin_fma(p, z, -0x1.f57d7734d1664p-13);
    p = __builtin_fma(p, z, 0x1.3558248036744p-11);
    p = __builtin_fma(p, z, -0x1.7da36452b75e3p-10);
    p = __builtin_fma(p, z, 0x1.d6d3d0e157de0p-9);
    p = __builtin_fma(p, z, -0x1.226e355e6c23dp-7);
    p = __builtin_fma(p, z, 0x1.664f4882c10fap-6);
    p = __builtin_fma(p, z, -0x1.ba1ba1ba1ba1cp-5);
    p = __builtin_fma(p, z, 0x1.1111111111111p-3);
    p = __builtin_fma(p, z, -0x1.5555555555555p-2);
    return __builtin_fma(x, z * p, x);
  }
  const double u = pt_exp(-2.0 * ax);
  return __builtin_copysign((1.0 - u) / (1.0 + u), x);
}
// Python-style floor division / modulo for integers (IntDiv / Mod c_code, scalar/basic.py)
template <class T> PT_DEV T pt_intdiv_i(T x, T y) {
  if (y == 0) return 0;
  T q = x / y;
  if ((x % y != 0) && ((x < 0) != (y < 0))) q -= 1;
  return q;
}
template <class T> PT_DEV T pt_mod_i(T x, T y) {
  if (y == 0) return 0;
  T r = x % y;
  if (r != 0 && ((r < 0) != (y < 0))) r += y;
  return r;
}
PT_DEV double pt_intdiv_f(double x, double y) { return floor(x / y); }
PT_DEV float pt_intdiv_f(float x, float y) { return floorf(x / y); }
PT_DEV double pt_mod_f(double x, double y) {
  if (y == 0) return __builtin_nan("");
  double r = fmod(x, y);
  if (r != 0 && ((r < 0) != (y < 0))) r += y;
  return r;
}
PT_DEV float pt_mod_f(float x, float y) {
  if (y == 0) return __builtin_nanf("");
  float r = fmodf(x, y);
  if (r != 0 && ((r < 0) != (y < 0))) r += y;
  return r;
}
// fp64 log1p in ~50 VALU instructions (the device library's is ~125; a logistic or Student-t log-density term is one log1p
// per element and VALU-issue bound: profiles/r7_wide200_pmc.md).  The classical reduction: 1 + x = 2^k (1 + f) with 1 + f in
// (sqrt(1/2), sqrt(2)], s = f / (2 + f), log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)) with the degree-7 minimax R of the
// fdlibm family, k ln2 added as a hi/lo pair, and c = the rounding error of 1 + x (relative to 1 + x) added back; f = x itself
// while k = 0.  The two divisions have tame denominators (2 + f in [1.7, 2.42]; 1 + x only scales a term below one ulp), so
// they are v_rcp_f64 + Newton steps without the scale/fixup of a general fp64 division.  2.1 ulp max against long-double
// log1pl on 4e7 host-emulated points (all magnitudes, both signs, the k = 0 / 1 boundaries), 0.5 ulp typical;
// Log1p.c_code of the reference is libm's log1p (scalar/basic.py:3042; glibc < 1 ulp).  x < -1 -> NaN, -1 -> -inf,
// +inf -> +inf, NaN -> NaN, |x| < 2^-54 -> x (keeps -0.0).
PT_DEV double pt_log1p(double x) {
  const double u = 1.0 + x;
  double m = 2.0 * __builtin_amdgcn_frexp_mant(u);  // [1, 2)
  int k = __builtin_amdgcn_frexp_exp(u) - 1;
  const bool up = m > 0x1.6a09e667f3bcdp+0;
  m = up ? 0.5 * m : m;
  k = up ? k + 1 : k;
  double c = k > 0 ? 1.0 - (u - x) : x - (u - 1.0);
  c = k == 0 ? 0.0 : c * __builtin_amdgcn_rcp(u);
  const double f = k == 0 ? x : m - 1.0;
  const double d = 2.0 + f;
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  double sq = f * r;
  sq = __builtin_fma(__builtin_fma(-d, sq, f), r, sq);
  const double z = sq * sq, w = z * z;
  const double t1 = w * __builtin_fma(w, __builtin_fma(w, 0x1.39a09d078c69fp-3, 0x1.c71c51d8e78afp-3), 0x1.999999997fa04p-2);
  const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, 0x1.2f112df3e5244p-3, 0x1.7466496cb03dep-3), 0x1.2492494229359p-2), 0x1.5555555555593p-1);
  const double hf = 0.5 * f * f, dk = (double)k;
  double y = __builtin_fma(dk, 0x1.62e42fee00000p-1, f - (hf - __builtin_fma(sq, hf + (t1 + t2), __builtin_fma(dk, 0x1.a39ef35793c76p-33, c))));
  y = __builtin_fabs(x) < 0x1p-54 ? x : y;
  y = x > -1.0 ? y : (x == -1.0 ? -__builtin_huge_val() : __builtin_nan(""));
  y = x == __builtin_huge_val() ? x : y;
  return y;
}
// pow with the exact cases exact.  The device library's pow is within ~1.3 ulp but NOT exact where the result is
// representable: pow(3, 1) = 2.9999999999999996, pow(19, 3) = 6858.999999999999 — and an integer power, which Pow.c_code
// (scalar/basic.py:2250) computes as (T)pow((double)x, (double)y), then truncates to 6858.  libm's pow (the reference's) is
// correctly rounded in these cases.  So: an integer exponent |y| <= 64 of an integer-valued base is repeated squaring, taken
// when every product in it was exact (zero fma residual: always so while the result is below 2^53, and beyond for bases
// with factors of two) — and 1 / that for y < 0 (one correctly rounded division); y = +-1, +-2, +-3 of any base are products (<= 1.5 ulp); everything else is the library's value.
PT_DEV double pt_pow(double x, double y) {
  double r = pow(x, y);
  const double ay = __builtin_fabs(y);
  if (y == __builtin_rint(y) && ay >= 1.0 && ay <= 64.0) {
    const int n = (int)ay;
    if (x == __builtin_rint(x) && x != 0.0 && __builtin_fabs(x) < 0x1p53) {
      double b = __builtin_fabs(x), p = 1.0;
      bool exact = true;  // every product that went into p had a zero rounding error (fma residual)
#pragma unroll
      for (int k = 0; k < 7; k++) {
        if ((n >> k) & 1) {
          const double q = p * b;
          exact = exact && __builtin_fma(p, b, -q) == 0.0;
          p = q;
        }
        if ((n >> (k + 1)) != 0) {
          const double q = b * b;
          exact = exact && __builtin_fma(b, b, -q) == 0.0;
          b = q;
        }
      }
      if (exact && p < __builtin_huge_val()) {
        p = (x < 0.0 && (n & 1)) ? -p : p;
        r = y < 0.0 ? 1.0 / p : p;
      }
    } else if (n <= 3) {
      const double p = n == 1 ? x : n == 2 ? x * x : x * x * x;
      r = y < 0.0 ? 1.0 / p : p;
    }
  }
  return r;
}
// fp64 log by the same reduction (x = 2^k (1 + f), no rounding term): ~45 VALU instructions against the device library's ~90;
// 0.86 ulp max against long-double logl on 4e7 host-emulated points (normal and subnormal arguments, the neighbourhoods of 1,
// sqrt(2) and sqrt(1/2)).  Log.c_code of the reference is libm's log (scalar/basic.py:2896).  x < 0 -> NaN, +-0 -> -inf,
// +inf -> +inf, NaN -> NaN; subnormal arguments are normalised by v_frexp_mant_f64 / v_frexp_exp_i32_f64.
PT_DEV double pt_log(double x) {
  double m = 2.0 * __builtin_amdgcn_frexp_mant(x);
  int k = __builtin_amdgcn_frexp_exp(x) - 1;
  const bool up = m > 0x1.6a09e667f3bcdp+0;
  m = up ? 0.5 * m : m;
  k = up ? k + 1 : k;
  const double f = m - 1.0, d = 2.0 + f;
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  double sq = f * r;
  sq = __builtin_fma(__builtin_fma(-d, sq, f), r, sq);
  const double z = sq * sq, w = z * z;
  const double t1 = w * __builtin_fma(w, __builtin_fma(w, 0x1.39a09d078c69fp-3, 0x1.c71c51d8e78afp-3), 0x1.999999997fa04p-2);
  const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, 0x1.2f112df3e5244p-3, 0x1.7466496cb03dep-3), 0x1.2492494229359p-2), 0x1.5555555555593p-1);
  const double hf = 0.5 * f * f, dk = (double)k;
  double y = __builtin_fma(dk, 0x1.62e42fee00000p-1, f - (hf - __builtin_fma(sq, hf + (t1 + t2), dk * 0x1.a39ef35793c76p-33)));
  y = x > 0.0 ? y : (x == 0.0 ? -__builtin_huge_val() : __builtin_nan(""));
  y = x == __builtin_huge_val() ? x : y;
  return y;
}
PT_DEV double pt_sigmoid(double x) { return 1.0 / (1.0 + pt_exp(-x)); }
PT_DEV float pt_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
PT_DEV double pt_softplus(double x) {
  return x < -37.0 ? pt_exp(x) : x < 18.0 ? pt_log1p(pt_exp(x)) : x < 33.3 ? x + pt_exp(-x) : x;
}
// sigmoid(x) and softplus(x) of ONE argument (the logistic log-density and its gradient; a Bernoulli-logit likelihood):
// both from e = exp(-|x|) in (0, 1] — one exp instead of two or three, no overflow on either side.
//   sigmoid = 1 / (1 + e)        (x >= 0)      e / (1 + e)   (x < 0)
//   softplus = max(x, 0) + log1p(e)
// Within 2 ulp of pt_sigmoid / pt_softplus (Sigmoid.c_code: 1 / (1 + exp(-x)); Softplus.c_code: the four-branch form of
// scalar/math.py); NaN -> NaN, +inf -> (1, +inf), -inf -> (0, 0).  emit_body uses it when a body holds both of one operand.
PT_DEV void pt_sig_sp(double x, double& sg, double& sp) {
  const double e = pt_exp(-__builtin_fabs(x));
  const double inv = 1.0 / (1.0 + e);
  sg = x >= 0.0 ? inv : e * inv;
  sp = (x > 0.0 ? x : 0.0) + pt_log1p(e);
  if (x != x) { sg = x; sp = x; }
}
PT_DEV float pt_softplus(float x) {
  return x < -37.0f ? expf(x) : x < 18.0f ? log1pf(expf(x)) : x < 33.3f ? x + expf(-x) : x;
}
PT_DEV double pt_log1mexp(double x) { return x < -0.6931471805599453 ? pt_log1p(-exp(x)) : log(-expm1(x)); }
PT_DEV float pt_log1mexp(float x) { return x < -0.6931471805599453f ? log1pf(-expf(x)) : logf(-expm1f(x)); }
// RoundHalfToEven (scalar/basic.py:2737-2766 restates npy_rint with floor arithmetic): the
// hardware's v_rndne is that function exactly, and — unlike `x - floor(x)` — cannot have the
// producer of x contracted into it (x = a*b fused into an fma changes which side of a tie
// the value lands on: found by the golden vectors, 2.5 rounded to 3).
PT_DEV double pt_rint_even(double x) { return __builtin_rint(x); }
PT_DEV float pt_rint_even(float x) { return __builtin_rintf(x); }
// digamma (Psi): asymptotic series with recurrence shift, as in the reference's
// support code (scalar/math.py:403-470 `_psi`)
PT_DEV double pt_psi(double x) {
  const double S = 1.0e-5, C = 8.5, S3 = 8.333333333e-2, S4 = 8.333333333e-3, S5 = 3.968253968e-3,
               D1 = -0.5772156649;
  double y = x, psi = 0.0, R;
  if (y <= 0.0) {
    // poles at 0, -1, -2, ...: +inf (the reference's choice); elsewhere the reflection formula
    if (y == floor(y)) return __builtin_inf();
    const double pix = 3.14159265358979323846 * y;
    psi = -3.14159265358979323846 * (cos(pix) / sin(pix));
    y = 1.0 - y;
  }
  if (y <= S) return psi + D1 - 1.0 / y;
  while (y < C) { psi = psi - 1.0 / y; y = y + 1; }
  R = 1.0 / y;
  psi = psi + log(y) - .5 * R;
  R = R * R;
  psi = psi - R * (S3 - R * (S4 - R * S5));
  return psi;
}
PT_DEV float pt_psi(float x) { return (float)pt_psi((double)x); }
// trigamma: AS 121 with the 10-digit constants of TriGamma.c_support_code (scalar/math.py:518-567)
PT_DEV double pt_trigamma(double x) {
  const double b2 = 0.1666666667, b4 = -0.03333333333, b6 = 0.02380952381, b8 = -0.03333333333;
  if (x <= 0) return 0.0;  // (NaN compares false and runs through the series: NaN out)
  if (x <= 0.0001) return 1.0 / x / x;
  double value = 0.0, z = x;
  while (z < 5.0) { value += 1.0 / z / z; z += 1.0; }
  const double y = 1.0 / z / z;
  value += 0.5 * y + (1.0 + y * (b2 + y * (b4 + y * (b6 + y * b8)))) / z;
  return value;
}
PT_DEV float pt_trigamma(float x) { return (float)pt_trigamma((double)x); }
