// Bessel functions of real order, fp64, for the generated elementwise kernels.
//
// Emitted by codegen.prelude_for into a kernel only when its body uses Jv / Ive / Kve
// (scalar/math.py of the reference: scipy.special.jv / ive / kve); the host test
// tests/test_special_bessel_host.py compiles this same text with PT_DEV and __constant__ defined away.
//
// Algorithms (all from the literature; DESIGN.md §4 has the regions, caps and measured accuracy):
//   * small x (x^2 <= 4(nu+1)): the ascending series of J_nu / I_nu, every term ratio <= 1/k;
//   * large x (x >= max(PT_SF_XA, PT_SF_XB nu^2)): Hankel's asymptotic expansions (DLMF 10.17, 10.40);
//   * in between: Steed's method.  CF1 (modified Lentz) gives J'_nu/J_nu or I'_nu/I_nu, a downward
//     recurrence carries the ratio to mu = nu - round(nu), |mu| <= 1/2; Temme's series (x < 2) or CF2
//     (x >= 2: Steed's complex fraction for J/Y, Thompson & Barnett's for K) gives Y_mu or K_mu, and the
//     Wronskian fixes the normalisation (Temme 1975, 1976; Barnett et al. 1974; Thompson & Barnett 1987).
//     Y and K are carried upward by their (stable) forward recurrences.
// Every loop has a fixed cap; a loop that reaches it without converging makes the result NaN.
// Lanes of a wave take different regions: the regions are ordinary branches, each with a short
// straight-line body, so a wave pays for the union of the regions its lanes fall in.

#ifndef PT_SF_COUNT
#define PT_SF_COUNT(slot, n)
#endif
// the long region bodies are real calls: inlined into a kernel that unrolls 4 elements per thread they need ~380
// VGPRs and spill; as calls each is compiled once and the unrolled loop keeps its own registers
#ifndef PT_SF_FN
#define PT_SF_FN static __device__ __noinline__
#endif

#define PT_SF_EPS 1.1102230246251565e-16
#define PT_SF_TINY 1e-300
#define PT_SF_PI 3.141592653589793
#define PT_SF_XA 25.0  // Hankel region: x >= max(PT_SF_XA, PT_SF_XB nu^2) for J, Y and K; max(PT_SF_XA, PT_SF_XBI nu^2) for I
#define PT_SF_XB 0.0625
#define PT_SF_XBI 0.5
#define PT_SF_CAP_SERIES 200
#define PT_SF_CAP_CF1 20000
#define PT_SF_CAP_CF2 1000
#define PT_SF_CAP_REC 20000
#define PT_SF_CAP_ASY 200

// 1/Gamma(1+z) = sum c_k z^k (Taylor coefficients at 40 digits), split into even / odd k
static __constant__ const double pt_sf_rge[15] = {
    0x1.0000000000000p+0, -0x1.4fcf4026afa2ep-1, 0x1.5512320b43fbep-3, -0x1.3b4af28483e21p-7, -0x1.317112ce3a2a8p-10,
    0x1.0c8a78cd9f9d2p-13, -0x1.4fad41fc34fbbp-20, -0x1.b9986666c225dp-23, 0x1.57bc3fc384334p-28, 0x1.cae7675c18607p-34,
    -0x1.0423bac8ca3fbp-38, -0x1.72cb88ea5ae6ep-46, 0x1.6198491a83bcdp-50, 0x1.5e3fee81de0eap-60, -0x1.0f635344a29eap-62};
static __constant__ const double pt_sf_rgo[15] = {
    0x1.2788cfc6fb619p-1, -0x1.5815e8fa27048p-5, -0x1.59af103c34092p-5, 0x1.d919c527f60b2p-8, -0x1.c364fe6f1563dp-13,
    -0x1.51ce8af47eabep-16, 0x1.302509dbc0de3p-20, 0x1.a44b7ba22d629p-28, -0x1.44b4cedca388fp-30, 0x1.11d065bfaf067p-37,
    0x1.1f20151323cd0p-41, -0x1.815f72a05f16fp-48, -0x1.10613dde57a89p-53, 0x1.a0dc770fb8a4ap-60, 0x1.43d79a4b90ce8p-66};
// sin(pi t), cos(pi t) with exact zeros at the integers / half-integers
PT_DEV void pt_sf_sincospi(double t, double* s, double* c) {
  double r = t - 2.0 * rint(0.5 * t);  // exact, in [-1, 1]
  double sg = 1.0;
  if (r > 0.5) { r = 1.0 - r; sg = -1.0; }
  else if (r < -0.5) { r = -1.0 - r; sg = -1.0; }
  *s = sin(PT_SF_PI * r);
  *c = fabs(r) == 0.5 ? 0.0 : sg * cos(PT_SF_PI * r);
}

// Temme's Gamma_1(mu), Gamma_2(mu) and 1/Gamma(1 +- mu), |mu| <= 1/2, without cancellation
PT_DEV void pt_sf_temme_gam(double mu, double* g1, double* g2, double* rgp, double* rgm) {
  const double m2 = mu * mu;
  double e = pt_sf_rge[14], o = pt_sf_rgo[14];
  for (int k = 13; k >= 0; k--) { e = e * m2 + pt_sf_rge[k]; o = o * m2 + pt_sf_rgo[k]; }
  *g1 = -o;
  *g2 = e;
  *rgp = e + mu * o;
  *rgm = e - mu * o;
}

// (x/2)^nu / Gamma(nu + 1) * e^{-s}
PT_DEV double pt_sf_lead(double nu, double x, double s) {
  if (nu <= 170.0) {
    const double p = pow(0.5 * x, nu), g = tgamma(nu + 1.0);
    if (p > 1e-290 && p < 1e290) return p / g * exp(-s);
  }
  return exp(nu * log(0.5 * x) - lgamma(nu + 1.0) - s);
}

// ascending series: sum_k (sg x^2/4)^k / (k! (nu+1)_k), sg = -1 for J, +1 for I; x^2 <= 4(nu+1)
PT_DEV double pt_sf_series(double nu, double x, double sg) {
  const double q = sg * 0.25 * x * x;
  double t = 1.0, s = 1.0;
  int k = 1;
  for (; k <= PT_SF_CAP_SERIES; k++) {
    t *= q / (k * (nu + k));
    s += t;
    if (fabs(t) <= PT_SF_EPS * 0.5 * fabs(s)) break;
  }
  PT_SF_COUNT(0, k);
  return k > PT_SF_CAP_SERIES ? __builtin_nan("") : s;
}

// the largest term of the expansion is about e^{nu^2/(2x)} times the first, and for I the sum is about e^{-nu^2/(2x)}:
// the cancellation costs at most e^{8} ulp at the J/K boundary (measured: 3e-16 of the envelope) and e^{2} at the I boundary
PT_DEV bool pt_sf_hankel_region(double nu, double x) { return x >= PT_SF_XA && x >= PT_SF_XB * nu * nu; }
PT_DEV bool pt_sf_hankel_region_i(double nu, double x) { return x >= PT_SF_XA && x >= PT_SF_XBI * nu * nu; }

// Hankel's expansion terms t_k = a_k(nu) / x^k; mode 0: P and Q of J/Y, 1: sum (-1)^k t_k (I), 2: sum t_k (K)
PT_DEV double pt_sf_hankel(double nu, double x, int mode, double* Q) {
  const double m = 4.0 * nu * nu;
  double t = 1.0, p = 1.0, q = 0.0, s = 1.0, prev = 2.0;
  int k = 1;
  bool ok = false;
  for (; k <= PT_SF_CAP_ASY; k++) {
    const double j = 2.0 * k - 1.0;
    t *= (m - j * j) / (8.0 * k * x);
    const double at = fabs(t);
    if (mode == 0) {
      const int r = k & 3;
      if (r == 1) q += t; else if (r == 2) p -= t; else if (r == 3) q -= t; else p += t;
      s = fabs(p) + fabs(q);
    } else {
      s += (mode == 1 && (k & 1)) ? -t : t;
    }
    if (at <= PT_SF_EPS * 0.125 * fabs(s)) { ok = true; break; }
    if (at > prev && j * j > m) break;  // past the smallest term: the expansion diverges from here
    prev = at;
  }
  PT_SF_COUNT(1, k);
  if (!ok) return __builtin_nan("");
  if (mode == 0) { *Q = q; return p; }
  return s;
}

// J_{nu}(x) and Y_{nu}(x) in the Hankel region (any real nu)
PT_DEV void pt_sf_jy_hankel(double nu, double x, double* J, double* Y) {
  double Q = 0.0;
  const double P = pt_sf_hankel(nu, x, 0, &Q);
  // chi = x - (nu/2 + 1/4) pi; cos(chi), sin(chi) from the library's sin/cos of x and an exact sincospi
  double sp, cp;
  pt_sf_sincospi(0.5 * nu + 0.25, &sp, &cp);
  const double sx = sin(x), cx = cos(x);
  const double cc = cx * cp + sx * sp, sc = sx * cp - cx * sp;
  const double f = sqrt(2.0 / (PT_SF_PI * x));
  *J = f * (P * cc - Q * sc);
  *Y = f * (P * sc + Q * cc);
}

// Steed / Temme: J_nu and (optionally) Y_nu, nu >= 0, 0 < x outside the Hankel region.
// want_j = false skips CF1's recurrence at nu (only Y is wanted): CF1 then runs at mu.
PT_DEV void pt_sf_jy_steed(double nu, double x, bool want_j, double* J, double* Y) {
  const double nan = __builtin_nan("");
  const int nl = (int)(nu + 0.5);
  const double mu = nu - nl, xi = 1.0 / x, xi2 = 2.0 * xi, w = xi2 / PT_SF_PI;
  if (nl > PT_SF_CAP_REC) { *J = nan; *Y = nan; return; }
  // CF1: h = J'_o / J_o at o = nu (or mu), modified Lentz; the sign of J_o relative to the start is tracked
  const double o = want_j ? nu : mu;
  double h = fabs(o * xi) < PT_SF_TINY ? PT_SF_TINY : o * xi, b = xi2 * o, d = 0.0, c = h, sgn = 1.0;
  int i = 1;
  for (; i <= PT_SF_CAP_CF1; i++) {
    b += xi2;
    d = b - d;
    if (fabs(d) < PT_SF_TINY) d = PT_SF_TINY;
    c = b - 1.0 / c;
    if (fabs(c) < PT_SF_TINY) c = PT_SF_TINY;
    d = 1.0 / d;
    const double del = c * d;
    h *= del;
    if (d < 0.0) sgn = -sgn;
    if (fabs(del - 1.0) < PT_SF_EPS) break;
  }
  PT_SF_COUNT(2, i);
  if (i > PT_SF_CAP_CF1) { *J = nan; *Y = nan; return; }
  // downward recurrence of (J, J') from o to mu, unnormalised, rescaled away from overflow
  double jl = sgn, jpl = h * sgn, fct = o * xi;
  const double jtop0 = jl;
  double jtop = jtop0;
  if (want_j) {
    for (int l = nl; l >= 1; l--) {
      const double jt = fct * jl + jpl;
      fct -= xi;
      jpl = fct * jt - jl;
      jl = jt;
      if (fabs(jl) > 1e200) { jl *= 1e-200; jpl *= 1e-200; jtop *= 1e-200; }
    }
    PT_SF_COUNT(3, nl);
  }
  if (jl == 0.0) jl = PT_SF_EPS;
  const double f = jpl / jl;  // J'_mu / J_mu
  double ymu, ymu1, jmu;
  if (x < 2.0) {
    // Temme's series for Y_mu, Y_{mu+1}
    double g1, g2, rgp, rgm;
    pt_sf_temme_gam(mu, &g1, &g2, &rgp, &rgm);
    const double x2 = 0.5 * x, pimu = PT_SF_PI * mu;
    const double fa = fabs(pimu) < PT_SF_EPS ? 1.0 : pimu / sin(pimu);
    const double dl = -log(x2), e = mu * dl;
    const double fb = fabs(e) < PT_SF_EPS ? 1.0 : sinh(e) / e;
    const double fc = fabs(0.5 * pimu) < PT_SF_EPS ? 1.0 : sin(0.5 * pimu) / (0.5 * pimu);
    const double r = PT_SF_PI * 0.5 * pimu * fc * fc;
    double ff = 2.0 / PT_SF_PI * fa * (g1 * cosh(e) + g2 * fb * dl);
    const double ee = exp(e);
    // p = (x/2)^-mu Gamma(1+mu) / pi, q = (x/2)^mu Gamma(1-mu) / pi
    double p = ee / (rgp * PT_SF_PI), q = 1.0 / (ee * PT_SF_PI * rgm);
    const double dd = -x2 * x2;
    double cc = 1.0, sum = ff + r * q, sum1 = p;
    int k = 1;
    for (; k <= PT_SF_CAP_SERIES; k++) {
      ff = (k * ff + p + q) / (k * (double)k - mu * mu);
      cc *= dd / k;
      p /= k - mu;
      q /= k + mu;
      const double del = cc * (ff + r * q);
      sum += del;
      sum1 += cc * p - k * del;
      if (fabs(del) < (1.0 + fabs(sum)) * PT_SF_EPS) break;
    }
    PT_SF_COUNT(4, k);
    if (k > PT_SF_CAP_SERIES) { *J = nan; *Y = nan; return; }
    ymu = -sum;
    ymu1 = -sum1 * xi2;
    const double ymup = mu * xi * ymu - ymu1;
    jmu = w / (ymup - f * ymu);
  } else {
    // CF2: p + i q = (J'_mu + i Y'_mu) / (J_mu + i Y_mu), Steed's algorithm in complex arithmetic
    double a = 0.25 - mu * mu, p = -0.5 * xi, q = 1.0;
    const double br = 2.0 * x;
    double bi = 2.0;
    double fct2 = a * xi / (p * p + q * q);
    double cr = br + q * fct2, ci = bi + p * fct2;
    double den = br * br + bi * bi, dr = br / den, di = -bi / den;
    double dlr = cr * dr - ci * di, dli = cr * di + ci * dr;
    double t = p * dlr - q * dli;
    q = p * dli + q * dlr;
    p = t;
    int k = 2;
    for (; k <= PT_SF_CAP_CF2; k++) {
      a += 2.0 * (k - 1);
      bi += 2.0;
      dr = a * dr + br;
      di = a * di + bi;
      if (fabs(dr) + fabs(di) < PT_SF_TINY) dr = PT_SF_TINY;
      fct2 = a / (cr * cr + ci * ci);
      cr = br + cr * fct2;
      ci = bi - ci * fct2;
      if (fabs(cr) + fabs(ci) < PT_SF_TINY) cr = PT_SF_TINY;
      den = dr * dr + di * di;
      dr /= den;
      di /= -den;
      dlr = cr * dr - ci * di;
      dli = cr * di + ci * dr;
      t = p * dlr - q * dli;
      q = p * dli + q * dlr;
      p = t;
      if (fabs(dlr - 1.0) + fabs(dli) < PT_SF_EPS) break;
    }
    PT_SF_COUNT(5, k);
    if (k > PT_SF_CAP_CF2) { *J = nan; *Y = nan; return; }
    const double gam = (p - f) / q;
    jmu = copysign(sqrt(w / ((p - f) * gam + q)), jl);
    ymu = jmu * gam;
    const double ymup = ymu * (p + q / gam);
    ymu1 = mu * xi * ymu - ymup;
  }
  *J = want_j ? jtop * (jmu / jl) : jmu;
  // forward recurrence of Y from mu to nu; an overflow ends it (Y keeps its sign towards x -> 0)
  int l = 1;
  for (; l <= nl && !isinf(ymu1); l++) {
    const double yt = (mu + l) * xi2 * ymu1 - ymu;
    ymu = ymu1;
    ymu1 = yt;
  }
  PT_SF_COUNT(6, l - 1);
  *Y = l <= nl ? ymu1 : ymu;
}

// K_mu e^x, K_{mu+1} e^x for |mu| <= 1/2, x > 0 (Temme's series for x < 2, Thompson & Barnett's CF2 above)
PT_DEV bool pt_sf_kmu(double mu, double x, double* k0, double* k1) {
  const double xi = 1.0 / x;
  if (x < 2.0) {
    double g1, g2, rgp, rgm;
    pt_sf_temme_gam(mu, &g1, &g2, &rgp, &rgm);
    const double x2 = 0.5 * x, pimu = PT_SF_PI * mu;
    const double fa = fabs(pimu) < PT_SF_EPS ? 1.0 : pimu / sin(pimu);
    const double dl = -log(x2), e = mu * dl;
    const double fb = fabs(e) < PT_SF_EPS ? 1.0 : sinh(e) / e;
    double ff = fa * (g1 * cosh(e) + g2 * fb * dl);
    const double ee = exp(e);
    double p = 0.5 * ee / rgp, q = 0.5 / (ee * rgm), cc = 1.0, sum = ff, sum1 = p;
    const double dd = x2 * x2;
    int k = 1;
    for (; k <= PT_SF_CAP_SERIES; k++) {
      ff = (k * ff + p + q) / (k * (double)k - mu * mu);
      cc *= dd / k;
      p /= k - mu;
      q /= k + mu;
      const double del = cc * ff;
      sum += del;
      sum1 += cc * (p - k * ff);
      if (fabs(del) < fabs(sum) * PT_SF_EPS) break;
    }
    PT_SF_COUNT(7, k);
    if (k > PT_SF_CAP_SERIES) return false;
    const double ex = exp(x);
    *k0 = sum * ex;
    *k1 = sum1 * 2.0 * xi * ex;
    return true;
  }
  double b = 2.0 * (1.0 + x), d = 1.0 / b, h = d, delh = d, q1 = 0.0, q2 = 1.0;
  const double a1 = 0.25 - mu * mu;
  double q = a1, c = a1, a = -a1, s = 1.0 + q * delh;
  int i = 1;
  for (; i <= PT_SF_CAP_CF2; i++) {
    a -= 2.0 * i;
    c = -a * c / (i + 1.0);
    const double qn = (q1 - b * q2) / a;
    q1 = q2;
    q2 = qn;
    q += c * qn;
    b += 2.0;
    d = 1.0 / (b + a * d);
    delh = (b * d - 1.0) * delh;
    h += delh;
    const double dels = q * delh;
    s += dels;
    if (fabs(dels / s) < PT_SF_EPS) break;
  }
  PT_SF_COUNT(8, i);
  if (i > PT_SF_CAP_CF2) return false;
  h *= a1;
  *k0 = sqrt(PT_SF_PI / (2.0 * x)) / s;
  *k1 = *k0 * (mu + x + 0.5 - h) * xi;
  return true;
}

// K_nu(x) e^x, nu >= 0, x > 0 finite
PT_SF_FN double pt_sf_kve_pos(double nu, double x) {
  if (pt_sf_hankel_region(nu, x)) return sqrt(PT_SF_PI / (2.0 * x)) * pt_sf_hankel(nu, x, 2, nullptr);
  const double nl = floor(nu + 0.5), mu = nu - nl;
  double k0, k1;
  if (!pt_sf_kmu(mu, x, &k0, &k1)) return __builtin_nan("");
  const double xi2 = 2.0 / x;
  int l = 1;
  for (; l <= nl && l <= PT_SF_CAP_REC && !isinf(k1); l++) {
    const double kt = (mu + l) * xi2 * k1 + k0;
    k0 = k1;
    k1 = kt;
  }
  PT_SF_COUNT(9, l - 1);
  if (isinf(k1)) return l <= nl ? k1 : k0;
  return l <= nl ? __builtin_nan("") : k0;
}

// I_nu(x) e^{-x}, nu >= 0, x > 0 finite
PT_SF_FN double pt_sf_ive_pos(double nu, double x) {
  if (x * x <= 4.0 * (nu + 1.0)) return pt_sf_lead(nu, x, x) * pt_sf_series(nu, x, 1.0);
  if (pt_sf_hankel_region_i(nu, x)) return pt_sf_hankel(nu, x, 1, nullptr) / sqrt(2.0 * PT_SF_PI * x);
  const int nl = (int)(nu + 0.5);
  const double mu = nu - nl, xi = 1.0 / x, xi2 = 2.0 * xi;
  if (nl > PT_SF_CAP_REC) return __builtin_nan("");
  // CF1 for I'_nu / I_nu (modified Lentz)
  double h = fmax(nu * xi, PT_SF_TINY), b = xi2 * nu, d = 0.0, c = h;
  int i = 1;
  for (; i <= PT_SF_CAP_CF1; i++) {
    b += xi2;
    d = 1.0 / (b + d);
    c = b + 1.0 / c;
    const double del = c * d;
    h *= del;
    if (fabs(del - 1.0) < PT_SF_EPS) break;
  }
  PT_SF_COUNT(10, i);
  if (i > PT_SF_CAP_CF1) return __builtin_nan("");
  double il = 1.0, ipl = h, fct = nu * xi, itop = 1.0;
  for (int l = nl; l >= 1; l--) {
    const double it = fct * il + ipl;
    fct -= xi;
    ipl = fct * it + il;
    il = it;
    if (il > 1e200) { il *= 1e-200; ipl *= 1e-200; itop *= 1e-200; }
  }
  PT_SF_COUNT(11, nl);
  const double f = ipl / il;
  double k0, k1;
  if (!pt_sf_kmu(mu, x, &k0, &k1)) return __builtin_nan("");
  const double kp = mu * xi * k0 - k1;
  const double imu = xi / (f * k0 - kp);
  return imu * (itop / il);
}

// ---- public entries (the edge cases are scipy.special's, observed with SciPy 1.15) ----

// J_v(x)
PT_SF_FN double pt_jv(double v, double x) {
  if (isnan(v) || isnan(x) || isinf(x)) return __builtin_nan("");
  if (isinf(v)) return x < 0.0 ? __builtin_nan("") : 0.0;  // scipy: J_{+-inf}(x >= 0) = 0
  const bool vint = v == floor(v);
  double sg = 1.0;
  if (x < 0.0) {
    if (!vint) return __builtin_nan("");
    x = -x;
    if (fmod(v, 2.0) != 0.0) sg = -sg;
  }
  if (vint && v < 0.0) {  // J_{-n} = (-1)^n J_n
    v = -v;
    if (fmod(v, 2.0) != 0.0) sg = -sg;
  }
  if (x == 0.0) return v == 0.0 ? sg : (v > 0.0 ? sg * 0.0 : __builtin_inf());
  if (pt_sf_hankel_region(v, x)) {
    double J, Y;
    pt_sf_jy_hankel(v, x, &J, &Y);
    return sg * J;
  }
  const double nu = fabs(v);
  const bool series = x * x <= 4.0 * (nu + 1.0);
  double J = 0.0, Y = 0.0;
  if (series) J = pt_sf_lead(nu, x, 0.0) * pt_sf_series(nu, x, -1.0);
  if (v >= 0.0) {
    if (!series) pt_sf_jy_steed(nu, x, true, &J, &Y);
    return sg * J;
  }
  // J_{-nu} = cos(nu pi) J_nu - sin(nu pi) Y_nu, nu not an integer
  double Jt;
  pt_sf_jy_steed(nu, x, !series, &Jt, &Y);
  if (!series) J = Jt;
  double s, c;
  pt_sf_sincospi(nu, &s, &c);
  return sg * (c * J - s * Y);
}

// I_v(x) e^{-|x|}
PT_SF_FN double pt_ive(double v, double x) {
  if (isnan(v) || isnan(x) || isinf(x) || isinf(v)) return __builtin_nan("");
  const bool vint = v == floor(v);
  double sg = 1.0;
  if (x < 0.0) {
    if (!vint) return __builtin_nan("");
    x = -x;
    if (fmod(v, 2.0) != 0.0) sg = -sg;
  }
  if (vint) v = fabs(v);  // I_{-n} = I_n
  if (x == 0.0) return v == 0.0 ? sg : (v > 0.0 ? sg * 0.0 : __builtin_nan(""));
  const double nu = fabs(v);
  const double r = pt_sf_ive_pos(nu, x);
  if (v >= 0.0) return sg * r;
  // I_{-nu} = I_nu + (2/pi) sin(nu pi) K_nu
  double s, c;
  pt_sf_sincospi(nu, &s, &c);
  if (s == 0.0 || 2.0 * x > 745.2) return sg * r;
  return sg * (r + (2.0 / PT_SF_PI) * s * pt_sf_kve_pos(nu, x) * exp(-2.0 * x));
}

// K_v(x) e^x
PT_SF_FN double pt_kve(double v, double x) {
  if (isnan(x) || x < 0.0 || isinf(x)) return __builtin_nan("");
  if (x == 0.0) return __builtin_inf();
  if (isnan(v) || isinf(v)) return __builtin_nan("");
  return pt_sf_kve_pos(fabs(v), x);
}

PT_DEV float pt_jv(float v, float x) { return (float)pt_jv((double)v, (double)x); }
PT_DEV float pt_ive(float v, float x) { return (float)pt_ive((double)v, (double)x); }
PT_DEV float pt_kve(float v, float x) { return (float)pt_kve((double)v, (double)x); }
