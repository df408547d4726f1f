
// inverses of the regularised incomplete gamma functions (GammaIncInv / GammaIncCInv.impl,
// scalar/math.py: scipy.special.gammaincinv / gammainccinv): the root of P(a, x) = p or Q(a, x) = q,
// always posed on the smaller tail, by safeguarded Halley steps from a Wilson-Hilferty / power-law
// starting point, iterated to the last bit of the forward function above
PT_DEV double pt_gamma_tail_root(double a, double tail, bool is_upper) {
  const double EPS = 2.220446049250313e-16;
  const double lg = lgamma(a);
  double z = -1.4142135623730951 * erfcinv(2.0 * tail);
  if (is_upper) z = -z;
  const double t = 1.0 - 1.0 / (9.0 * a) + z / (3.0 * sqrt(a));
  double x = t > 0.0 ? a * t * t * t : 0.0;
  if (!is_upper && (a < 1.0 || x <= 0.0 || tail < 1e-3)) {
    const double x2 = exp((log(tail) + lg + log(a)) / a);
    if (x <= 0.0 || x2 < x) x = x2;
  }
  if (is_upper && x <= 0.0) x = fmax(-log(tail) - lg, 1e-3);
  if (!(x > 0.0) || isinf(x)) x = 1.0;
  double lo = 0.0, hi = __builtin_inf();
  for (int it = 0; it < 300; it++) {
    const double f = (is_upper ? pt_gammaincc(a, x) : pt_gammainc(a, x)) - tail;
    if (f == 0.0) return x;
    const bool right = is_upper ? f > 0.0 : f < 0.0;
    if (right) lo = fmax(lo, x); else hi = fmin(hi, x);
    const double dens = exp((a - 1.0) * log(x) - x - lg);
    double xn = -1.0;
    if (dens > 0.0 && !isinf(dens)) {
      const double r = f / (is_upper ? -dens : dens);
      const double h = 1.0 - 0.5 * r * ((a - 1.0) / x - 1.0);
      xn = x - (h > 0.5 ? r / h : r);
    }
    if (!(xn > lo && xn < hi)) xn = isinf(hi) ? 2.0 * x : (lo > 0.0 ? 0.5 * (lo + hi) : 0.5 * hi);
    if (fabs(xn - x) <= 2.0 * EPS * xn) return xn;
    x = xn;
  }
  return x;
}
PT_DEV double pt_gammaincinv(double a, double p) {
  if (!(a > 0.0) || !(p >= 0.0 && p <= 1.0)) return __builtin_nan("");
  if (p == 0.0) return 0.0;
  if (p == 1.0) return __builtin_inf();
  return p <= 0.5 ? pt_gamma_tail_root(a, p, false) : pt_gamma_tail_root(a, 1.0 - p, true);
}
PT_DEV double pt_gammainccinv(double a, double q) {
  if (!(a > 0.0) || !(q >= 0.0 && q <= 1.0)) return __builtin_nan("");
  if (q == 0.0) return __builtin_inf();
  if (q == 1.0) return 0.0;
  return q <= 0.5 ? pt_gamma_tail_root(a, q, true) : pt_gamma_tail_root(a, 1.0 - q, false);
}
PT_DEV float pt_gammaincinv(float a, float p) { return (float)pt_gammaincinv((double)a, (double)p); }
PT_DEV float pt_gammainccinv(float a, float q) { return (float)pt_gammainccinv((double)a, (double)q); }
