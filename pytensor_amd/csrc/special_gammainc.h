
// regularised incomplete gamma P / Q as the reference's C backend computes them
// (scalar/c_code/gamma.c: logGamma 83-106, _series 143-155, _cfrac 172-189, GammaP 207-218,
//  GammaQ 222-233; called from GammaInc/GammaIncC.c_code, scalar/math.py:648-655, 695-702)
#define PT_G_EPS 2.2204460492503131e-16
#define PT_G_TINY (PT_G_EPS * PT_G_EPS * PT_G_EPS)
PT_DEV double pt_g_loggamma(double n) {
  if (n <= 0) return __builtin_nan("");
  if (n < 171 + 4 * PT_G_EPS) {
    if (fabs(n - floor(n)) < 4 * PT_G_EPS) { const int i = (int)floor(n) - 1; return pt_g_logfs[i < 0 ? 0 : i]; }
    if (fabs(2 * n - floor(2 * n)) < 4 * PT_G_EPS) return pt_g_loghs[(int)floor(n)];
  }
  double s = 0.99999999999980993227684700473478;
  s += 676.520368121885098567009190444019 / (n + 1);
  s += -1259.13921672240287047156078755283 / (n + 2);
  s += 771.3234287776530788486528258894 / (n + 3);
  s += -176.61502916214059906584551354 / (n + 4);
  s += 12.507343278686904814458936853 / (n + 5);
  s += -0.13857109526572011689554707 / (n + 6);
  s += 9.984369578019570859563e-6 / (n + 7);
  s += 1.50563273514931155834e-7 / (n + 8);
  return (n + 0.5) * log((n + 7.5) / 2.71828182845904523536028747135) + (0.918938533204672741780329736406 + log(s / n) - 7.0);
}
PT_DEV double pt_g_series(double n, double x) {
  double t = 1.0 / n, sum = t;
  for (int i = 0; i < 1024; i++) {
    n += 1.0;
    t *= x / n;
    sum += t;
    if (fabs(t) < fabs(sum) * PT_G_EPS) break;
  }
  return sum;
}
PT_DEV double pt_g_cfrac(double n, double x) {
  double b = x + 1 - n, c = 1 / PT_G_TINY, d = 1 / b, f = d;
  for (int i = 1; i < 1024; i++) {
    const double a = i * (n - i);
    b += 2;
    d = a * d + b;
    if (fabs(d) < PT_G_TINY) d = PT_G_TINY;
    c = b + a / c;
    if (fabs(c) < PT_G_TINY) c = PT_G_TINY;
    d = 1 / d;
    const double e = d * c;
    f *= e;
    if (fabs(e - 1) < PT_G_EPS) break;
  }
  return f;
}
PT_DEV double pt_gammainc(double n, double x) {
  if (isnan(n) || isnan(x)) return __builtin_nan("");
  if ((n <= 0) || (x < 0)) return __builtin_nan("");
  if (x <= 0) return 0;
  if (isinf(n)) return isinf(x) ? __builtin_nan("") : 0.0;
  if (isinf(x)) return 1;
  const double sc = exp(n * log(x) - x - pt_g_loggamma(n));
  if (x < n + 1) return pt_g_series(n, x) * sc;
  return 1 - pt_g_cfrac(n, x) * sc;
}
PT_DEV double pt_gammaincc(double n, double x) {
  if (isnan(n) || isnan(x)) return __builtin_nan("");
  if ((n <= 0) || (x < 0)) return __builtin_nan("");
  if (x <= 0) return 1;
  if (isinf(n)) return isinf(x) ? __builtin_nan("") : 1.0;
  if (isinf(x)) return 0;
  const double sc = exp(n * log(x) - x - pt_g_loggamma(n));
  if (x < n + 1) return 1 - pt_g_series(n, x) * sc;
  return pt_g_cfrac(n, x) * sc;
}
PT_DEV float pt_gammainc(float n, float x) { return (float)pt_gammainc((double)n, (double)x); }
PT_DEV float pt_gammaincc(float n, float x) { return (float)pt_gammaincc((double)n, (double)x); }
