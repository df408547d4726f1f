// Owen's T function, fp64, for the generated elementwise kernels.
//
// Emitted by codegen.prelude_for into a kernel only when its body uses Owens_t (scalar/math.py of the
// reference: scipy.special.owens_t); tests/test_special_bessel_host.py compiles this same text on the host.
//
// T(h, a) = e^{-h^2/2} / (2 pi) * int_0^a e^{-h^2 x^2 / 2} / (1 + x^2) dx  (Owen 1956)
//   * |a| <= 1: 40-point Gauss-Legendre on [0, min(a, PT_OT_TCUT / h)].  The pole of 1/(1 + x^2) at i lies
//     outside the Bernstein ellipse of ratio 4.6 around [0, 1], and past h x = PT_OT_TCUT the Gaussian is
//     below e^{-45} of its value at 0, so 40 nodes resolve the integrand at every h (a fixed trip count:
//     no lane of a wave waits on another).  e^{-h^2/2} is taken out of the integral with h^2 split exactly.
//   * |a| > 1: T(h, a) = (Q(h) + Q(ah)) / 2 - Q(h) Q(ah) - T(ah, 1/a), Q(h) = P(Z > h); since
//     T(h, a) >= T(h, 1) ~ Q(h) / 2 the subtraction loses at most two bits.
#ifndef PT_SF_FN
#define PT_SF_FN static __device__ __noinline__
#endif
#define PT_OT_PI 3.141592653589793
#define PT_OT_TCUT 9.5
// 40-point Gauss-Legendre on [-1, 1]: the 20 positive nodes and their weights (50-digit roots of P_40)
static __constant__ const double pt_ot_gx[20] = {
    0x1.3d9fa7259c6f9p-5, 0x1.db7af8723039bp-4, 0x1.8aa507790bb18p-3, 0x1.12967c83d4110p-2, 0x1.5e33b2ee16696p-2,
    0x1.a7b5bc5a29ed2p-2, 0x1.eeab6c46ecaa8p-2, 0x1.1953c149057cap-1, 0x1.39a0a9d652b8fp-1, 0x1.580ab4e17e33ap-1,
    0x1.74630eefa6276p-1, 0x1.8e7e140e56770p-1, 0x1.a63393069f110p-1, 0x1.bb5f0b43ea03fp-1, 0x1.cddfe5136244fp-1,
    0x1.dd99a3f1b1943p-1, 0x1.ea7412c59f876p-1, 0x1.f45b6a89bde77p-1, 0x1.fb40783501aafp-1, 0x1.ff190359ae7c8p-1};
static __constant__ const double pt_ot_gw[20] = {
    0x1.3d76e07d01470p-4, 0x1.3b8e1ab8156dfp-4, 0x1.37bf7fb3ffa5fp-4, 0x1.3210ebf5b8207p-4, 0x1.2a8b1efb50a42p-4,
    0x1.2139adc432380p-4, 0x1.162af0fc7e7f7p-4, 0x1.096feee7215d1p-4, 0x1.f638825187601p-5, 0x1.d68bed38b1964p-5,
    0x1.b40ae2c10a3f5p-5, 0x1.8eea82a7d6915p-5, 0x1.6763f67ce7b6cp-5, 0x1.3db419e3c9685p-5, 0x1.121b1d8e9a250p-5,
    0x1.c9b84cd4f2e15p-6, 0x1.6c79dab0af3a4p-6, 0x1.0d0ae92dd2f62p-6, 0x1.5801fe5cda0a0p-7, 0x1.284e71463c0d6p-8};

// Q(h) = P(Z > h) for h >= 0: erfc at h/sqrt(2) corrected for the rounding of that argument
PT_DEV double pt_ot_q(double h) {
  const double shi = 0x1.6a09e667f3bcdp-1, slo = -0x1.bdd3413b26456p-55;  // 1/sqrt(2) = shi + slo
  const double y = h * shi, dy = fma(h, shi, -y) + h * slo;
  return 0.5 * (erfc(y) - 1.1283791670955126 * dy * exp(-y * y));
}

// T(h, a) for h >= 0 finite, 0 <= a <= 1: Gauss-Legendre on [0, min(a, PT_OT_TCUT / h)]
PT_DEV double pt_ot_quad(double h, double a) {
  const double b = h * a > PT_OT_TCUT ? PT_OT_TCUT / h : a;
  const double hb = 0.5 * b, h2 = 0.5 * h * h;
  double s = 0.0;
  for (int i = 0; i < 20; i++) {
    const double u = hb * pt_ot_gx[i], x1 = hb + u, x2 = hb - u;
    s += pt_ot_gw[i] * (exp(-h2 * x1 * x1) / (1.0 + x1 * x1) + exp(-h2 * x2 * x2) / (1.0 + x2 * x2));
  }
  // e^{-h^2/2} with h^2 split exactly (h^2 = p + e) so that the rounding of h^2 costs nothing at h ~ 37
  const double p = h * h, e = fma(h, h, -p);
  return s * hb * (exp(-0.5 * p) * (1.0 - 0.5 * e)) / (2.0 * PT_OT_PI);
}

// Owen's T function
PT_SF_FN double pt_owens_t(double h, double a) {
  if (isnan(h) || isnan(a)) return __builtin_nan("");
  h = fabs(h);
  if (isinf(h)) return 0.0;
  const double sa = a < 0.0 ? -1.0 : 1.0;
  a = fabs(a);
  if (h == 0.0) return sa * atan(a) / (2.0 * PT_OT_PI);
  double t;
  if (a <= 1.0) {
    t = pt_ot_quad(h, a);
  } else {
    const double q1 = pt_ot_q(h);
    if (isinf(a)) {
      t = 0.25 * erfc(h / 1.4142135623730951);  // the limit Q(h) / 2, rounded as scipy rounds it
    } else {
      const double ah = a * h, q2 = pt_ot_q(ah);
      t = 0.5 * (q1 + q2) - q1 * q2 - pt_ot_quad(ah, 1.0 / a);
    }
  }
  return sa * t;
}

PT_DEV float pt_owens_t(float h, float a) { return (float)pt_owens_t((double)h, (double)a); }
