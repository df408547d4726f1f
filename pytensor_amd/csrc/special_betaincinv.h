
// inverse of the regularised incomplete beta function (BetaIncInv.impl, scalar/math.py:
// scipy.special.betaincinv): the root is sought on the half of (0, 1) it lies in (t = x or 1 - x,
// decided by I_1/2), the residual is P - p or q - Q, whichever is known more precisely, and
// safeguarded Halley steps run to the last bit of the forward function above
PT_DEV double pt_betaincinv(double a, double b, double p) {
  const double EPS = 2.220446049250313e-16;
  if (!(a > 0.0 && b > 0.0) || !(p >= 0.0 && p <= 1.0)) return __builtin_nan("");
  if (p == 0.0) return 0.0;
  if (p == 1.0) return 1.0;
  double q = 1.0 - p;
  const bool flip = p > pt_betainc(a, b, 0.5);
  if (flip) { double s = a; a = b; b = s; s = p; p = q; q = s; }
  const double lbeta = lgamma(a) + lgamma(b) - lgamma(a + b);
  double t = fmin(0.5, a / (a + b));
  if (p <= 0.5) {
    const double lt = (log(p) + log(a) + lbeta) / a;
    if (lt < log(t)) t = fmax(exp(lt), 1e-300);
  }
  double lo = 0.0, hi = 1.0, res = t;
  for (int it = 0; it < 300; it++) {
    const double ld = (a - 1.0) * log(t) + (b - 1.0) * log1p(-t) - lbeta;
    const double dens = exp(ld);
    const double f = (p <= q + dens) ? pt_betainc(a, b, t) - p : q - pt_betainc(b, a, 1.0 - t);
    if (f == 0.0) { res = t; break; }
    if (f < 0.0) lo = fmax(lo, t); else hi = fmin(hi, t);
    double tn = -1.0;
    if (dens > 0.0 && !isinf(dens)) {
      const double r = f / dens;
      const double h = 1.0 - 0.5 * r * ((a - 1.0) / t - (b - 1.0) / (1.0 - t));
      tn = t - (h > 0.5 ? r / h : r);
    }
    if (!(tn > lo && tn < hi)) {
      tn = lo > 0.0 ? (hi > 4.0 * lo ? sqrt(lo * hi) : 0.5 * (lo + hi)) : 1e-3 * hi;
      if (tn <= 0.0) { res = 0.0; break; }
    }
    res = tn;
    if (fabs(tn - t) <= 2.0 * EPS * tn) break;
    t = tn;
  }
  return flip ? 1.0 - res : res;
}
PT_DEV float pt_betaincinv(float a, float b, float p) { return (float)pt_betaincinv((double)a, (double)b, (double)p); }
