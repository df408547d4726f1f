
// ndtri(exp(y)) without forming exp(y) where it underflows (NdtriExp.impl, scalar/math.py:281:
// scipy.special.ndtri_exp): the upper tail through erfcinv(2 (1 - e^y)) near y = 0, erfcinv(2 e^y) down
// to y = -2, below that Newton steps on log Phi(x) = log(erfcx(-x / sqrt 2) / 2) - x^2 / 2 = y from the
// asymptotic root — quadratic, 3-5 steps
PT_DEV double pt_ndtri_exp(double y) {
  if (y != y || y > 0.0) return __builtin_nan("");
  if (y == 0.0) return __builtin_inf();
  if (y == -__builtin_inf()) return y;
  const double SQ2 = 1.4142135623730951;
  if (y >= -0.6931471805599453) return SQ2 * erfcinv(2.0 * (-expm1(y)));
  if (y >= -2.0) return -SQ2 * erfcinv(2.0 * exp(y));
  const double t = -2.0 * y;
  double x = -sqrt(t - log(6.283185307179586 * t));
  for (int it = 0; it < 8; it++) {
    const double r = erfcx(-x / SQ2);  // Phi(x) / phi(x) = r sqrt(pi / 2)
    const double dx = (log(0.5 * r) - 0.5 * x * x - y) * r * 1.2533141373155003;
    x -= dx;
    if (fabs(dx) <= 1e-16 * fabs(x)) break;
  }
  return x;
}
PT_DEV float pt_ndtri_exp(float y) { return (float)pt_ndtri_exp((double)y); }
