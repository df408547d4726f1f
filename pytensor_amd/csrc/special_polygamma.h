
// polygamma(n, x) as scipy.special.polygamma computes it (PolyGamma.impl, scalar/math.py:607-608):
// n = 0: digamma (reflection, recurrence to x >= 10, asymptotic series); n >= 1:
// (-1)^(n+1) n! zeta(n + 1, x), the Hurwitz zeta function by Euler-Maclaurin summation
// (Cephes zeta.c: direct terms until the argument exceeds 9, then 12 Bernoulli corrections)
PT_DEV double pt_zeta(double x, double q) {
  const double A[12] = {12.0, -720.0, 30240.0, -1209600.0, 47900160.0, -1.8924375803183791606e9, 7.47242496e10,
                        -2.950130727918164224e12, 1.1646782814350067249e14, -4.5979787224074726105e15,
                        1.8152105401943546773e17, -7.1661652561756670113e18};
  const double MACHEP = 1.11022302462515654042e-16;
  if (x == 1.0) return __builtin_inf();
  if (!(x >= 1.0)) return __builtin_nan("");
  if (q <= 0.0) {
    if (q == floor(q)) return __builtin_inf();
    if (x != floor(x)) return __builtin_nan("");
  }
  if (q > 1e8) return (1.0 / (x - 1.0) + 1.0 / (2.0 * q)) * pow(q, 1.0 - x);
  double s = pow(q, -x), a = q, b = 0.0;
  int i = 0;
  while (i < 9 || a <= 9.0) {
    i++;
    a += 1.0;
    b = pow(a, -x);
    s += b;
    if (fabs(b / s) < MACHEP) return s;
  }
  const double w = a;
  s += b * w / (x - 1.0);
  s -= 0.5 * b;
  a = 1.0;
  double k = 0.0;
  for (i = 0; i < 12; i++) {
    a *= x + k;
    b /= w;
    const double t = a * b / A[i];
    s += t;
    if (fabs(t / s) < MACHEP) return s;
    k += 1.0;
    a *= x + k;
    b /= w;
    k += 1.0;
  }
  return s;
}
PT_DEV double pt_digamma_acc(double x) {
  if (x != x || x == __builtin_inf()) return x;
  double nz = 0.0;
  bool neg = false;
  if (x <= 0.0) {
    if (x == floor(x)) return __builtin_nan("");
    neg = true;
    const double q = x;
    double p = floor(q);
    nz = q - p;
    if (nz != 0.5) {
      if (nz > 0.5) { p += 1.0; nz = q - p; }
      nz = 3.14159265358979323846 / tan(3.14159265358979323846 * nz);
    } else {
      nz = 0.0;
    }
    x = 1.0 - x;
  }
  double y;
  if (x <= 10.0 && x == floor(x)) {
    y = 0.0;
    for (int i = 1; i < (int)x; i++) y += 1.0 / i;
    y -= 0.57721566490153286061;
  } else {
    double s = x, w = 0.0;
    while (s < 10.0) { w += 1.0 / s; s += 1.0; }
    const double z = 1.0 / (s * s);
    double yy = 8.33333333333333333333E-2;
    yy = yy * z + -2.10927960927960927961E-2;
    yy = yy * z + 7.57575757575757575758E-3;
    yy = yy * z + -4.16666666666666666667E-3;
    yy = yy * z + 3.96825396825396825397E-3;
    yy = yy * z + -8.33333333333333333333E-3;
    yy = yy * z + 8.33333333333333333333E-2;
    yy *= z;
    y = log(s) - 0.5 / s - yy - w;
  }
  return neg ? y - nz : y;
}
PT_DEV double pt_polygamma(double n, double x) {
  if (n == 0.0) return pt_digamma_acc(x);
  if (!(n > 0.0) || n != floor(n)) return __builtin_nan("");
  const double sgn = (((long long)n) & 1) ? 1.0 : -1.0;
  return sgn * tgamma(n + 1.0) * pt_zeta(n + 1.0, x);
}
PT_DEV float pt_polygamma(float n, float x) { return (float)pt_polygamma((double)n, (double)x); }
