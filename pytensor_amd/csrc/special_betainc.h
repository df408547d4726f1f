
// regularised incomplete beta (Cephes incbet) as the reference's C backend computes it
// (scalar/c_code/incbet.c: BetaInc 33-90, incbcf 96-178, incbd 184-268, pseries 274-311;
//  called from BetaInc.c_code, scalar/math.py:1371-1381).  The reference flips (a, b, x) by
//  calling itself once; here the flipped evaluation is a second call of the same body.
#define PT_B_MINLOG -7.451332191019412076235E2
#define PT_B_MAXLOG 7.09782712893383996732E2
#define PT_B_MAXGAM 171.624376956302725
#define PT_B_EPS 1.11022302462515654042e-16
#define PT_B_BIG 4.503599627370496e15
#define PT_B_BIGINV 2.22044604925031308085e-16
// both continued fractions share one three-term recurrence: k1..k8 and their increments differ
PT_DEV double pt_b_cf(double xz, double k1, double k2, double k3, double k4, double k5, double k6,
                      double k7, double k8, double d2, double d6) {
  double pkm2 = 0.0, qkm2 = 1.0, pkm1 = 1.0, qkm1 = 1.0, ans = 1.0, r = 1.0, t;
  const double thresh = 3.0 * PT_B_EPS;
  int n = 0;
  do {
    double xk = -(xz * k1 * k2) / (k3 * k4);
    double pk = pkm1 + pkm2 * xk, qk = qkm1 + qkm2 * xk;
    pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
    xk = (xz * k5 * k6) / (k7 * k8);
    pk = pkm1 + pkm2 * xk; qk = qkm1 + qkm2 * xk;
    pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
    if (qk != 0.0) r = pk / qk;
    if (r != 0.0) { t = fabs((ans - r) / r); ans = r; } else t = 1.0;
    if (t < thresh) break;
    k1 += 1.0; k2 += d2; k3 += 2.0; k4 += 2.0; k5 += 1.0; k6 += d6; k7 += 2.0; k8 += 2.0;
    if ((fabs(qk) + fabs(pk)) > PT_B_BIG) { pkm2 *= PT_B_BIGINV; pkm1 *= PT_B_BIGINV; qkm2 *= PT_B_BIGINV; qkm1 *= PT_B_BIGINV; }
    if ((fabs(qk) < PT_B_BIGINV) || (fabs(pk) < PT_B_BIGINV)) { pkm2 *= PT_B_BIG; pkm1 *= PT_B_BIG; qkm2 *= PT_B_BIG; qkm1 *= PT_B_BIG; }
  } while (++n < 300);
  return ans;
}
PT_DEV double pt_b_pseries(double a, double b, double x) {
  const double ai = 1.0 / a;
  double u = (1.0 - b) * x, v = u / (a + 1.0), t = u, n = 2.0, s = 0.0;
  const double t1 = v, z = PT_B_EPS * ai;
  while (fabs(v) > z) {
    u = (n - b) * x / n;
    t *= u;
    v = t / (a + n);
    s += v;
    n += 1.0;
  }
  s += t1;
  s += ai;
  u = a * log(x);
  if ((a + b) < PT_B_MAXGAM && fabs(u) < PT_B_MAXLOG) {
    t = tgamma(a + b) / (tgamma(a) * tgamma(b));
    s = s * t * pow(x, a);
  } else {
    t = lgamma(a + b) - lgamma(a) - lgamma(b) + u + log(s);
    s = t < PT_B_MINLOG ? 0.0 : exp(t);
  }
  return s;
}
// everything of BetaInc() except the symmetry flip; *flip is set when the caller has to flip
PT_DEV double pt_b_body(double a, double b, double x, bool may_flip, bool* flip) {
  *flip = false;
  if (x == 0.0) return 0.0;
  if (x == 1.0) return 1.0;
  if ((b * x) <= 1.0 && x <= 0.95) return pt_b_pseries(a, b, x);
  const double xc = 1.0 - x;
  if (may_flip && x > (a / (a + b))) { *flip = true; return 0.0; }
  double y = x * (a + b - 2.0) - (a - 1.0), w, t;
  if (y < 0.0) w = pt_b_cf(x, a, a + b, a, a + 1.0, 1.0, b - 1.0, a + 1.0, a + 2.0, 1.0, -1.0);
  else w = pt_b_cf(x / (1.0 - x), a, b - 1.0, a, a + 1.0, 1.0, a + b, a + 1.0, a + 2.0, -1.0, 1.0) / xc;
  y = a * log(x);
  t = b * log(xc);
  if ((a + b) < PT_B_MAXGAM && fabs(y) < PT_B_MAXLOG && fabs(t) < PT_B_MAXLOG) {
    t = pow(xc, b);
    t *= pow(x, a);
    t /= a;
    t *= w;
    t *= tgamma(a + b) / (tgamma(a) * tgamma(b));
    return t;
  }
  y += t + lgamma(a + b) - lgamma(a) - lgamma(b);
  y += log(w / a);
  return y < PT_B_MINLOG ? 0.0 : exp(y);
}
PT_DEV double pt_betainc(double a, double b, double x) {
  if (isnan(a) || isnan(b) || isnan(x)) return __builtin_nan("");
  if (a <= 0.0 || b <= 0.0 || x < 0.0 || 1.0 < x) return __builtin_nan("");
  bool flip;
  double t = pt_b_body(a, b, x, true, &flip);
  if (!flip) return t;
  t = pt_b_body(b, a, 1.0 - x, false, &flip);
  return t <= PT_B_EPS ? 1.0 - PT_B_EPS : 1.0 - t;
}
PT_DEV float pt_betainc(float a, float b, float x) { return (float)pt_betainc((double)a, (double)b, (double)x); }
