// schur_device.h — real Schur form and the quasi-triangular Sylvester solve, written once for a team of threads.
//
// The numerical core of csrc/sylvester.hip (Bartels-Stewart; DESIGN §4 "Sylvester / Lyapunov"):
//   pt_schur::hessenberg   Householder reduction to upper Hessenberg form with the orthogonal factor (dgehd2 + dorghr)
//   pt_schur::francis      real Schur form by Francis double-shift QR, as LAPACK dlahqr with wantt = wantz = true
//   pt_schur::trsyl        R Y + Y op(S) = F for quasi-triangular R, S in standard form (dtrsyl, isgn = +1, scale = 1)
// Everything is fp64.  Matrices are row-major with a leading dimension, except the orthogonal factor, which is kept
// transposed (Zt = Z^T) so that the per-row updates of Z read contiguous memory across threads.
//
// Every function runs on a team of `nt` threads, `tid` being this thread: its loops are `for (j = tid; j < n; j +=
// nt)` and its phases end in SCHUR_SYNC().  The scalars that steer the iteration (reflectors, shifts, deflation tests,
// 2x2 standardisation) are computed redundantly and identically by every thread, so control flow is uniform.  The
// includer defines SCHUR_DEV (function qualifier), SCHUR_SYNC() (team barrier) and SCHUR_TEAM_MAX(v) (team-wide max of
// non-negative values, every thread receiving it); a host build defines them as "static inline", nothing and the
// identity, with tid = 0 and nt = 1, which is how tests/test_sylvester_host.py checks this text against SciPy.
#pragma once

#include <cmath>

namespace pt_schur {

constexpr double kUlp = 2.220446049250313e-16;      // dlamch('P')
constexpr double kSafmin = 2.2250738585072014e-308;  // dlamch('S')
constexpr double kSafmn2 = 1.0010415475915505e-146;  // dlanv2: 2^-485
constexpr double kSafmx2 = 9.989595361011175e+145;   // 2^485

SCHUR_DEV double dmax(double a, double b) { return a > b ? a : b; }
SCHUR_DEV double dmin(double a, double b) { return a < b ? a : b; }
SCHUR_DEV double sgn(double a, double b) { return b >= 0.0 ? fabs(a) : -fabs(a); }  // Fortran SIGN(a, b)

// sqrt(x^2 + y^2) without needless overflow (dlapy2)
SCHUR_DEV double lapy2(double x, double y) {
  const double xa = fabs(x), ya = fabs(y);
  const double w = dmax(xa, ya), z = dmin(xa, ya);
  if (z == 0.0 || w > 1.79e308) return w;
  const double q = z / w;
  return w * sqrt(1.0 + q * q);
}

// Householder reflector of order nr (2 or 3): (I - tau v v^T) [alpha; x1; x2] = [beta; 0; 0], v = [1; x1; x2] on return,
// alpha <- beta (dlarfg; LAPACK's rescaling loop for |beta| < safmin / eps is not needed at these magnitudes)
SCHUR_DEV void larfg(int nr, double& alpha, double& x1, double& x2, double& tau) {
  const double xnorm = nr == 3 ? lapy2(x1, x2) : fabs(x1);
  if (xnorm == 0.0) {
    tau = 0.0;
    return;
  }
  const double beta = -sgn(lapy2(alpha, xnorm), alpha);
  tau = (beta - alpha) / beta;
  const double scal = 1.0 / (alpha - beta);
  x1 *= scal;
  x2 *= scal;
  alpha = beta;
}

// Schur factorisation of a real 2x2 block in standard form (dlanv2): [a b; c d] = [cs -sn; sn cs] [aa bb; cc dd]
// [cs sn; -sn cs] with cc = 0 (real eigenvalues) or aa = dd and bb cc < 0 (a complex pair)
SCHUR_DEV void lanv2(double& a, double& b, double& c, double& d, double& cs, double& sn) {
  const double eps = kUlp;
  if (c == 0.0) {
    cs = 1.0;
    sn = 0.0;
  } else if (b == 0.0) {
    cs = 0.0;
    sn = 1.0;
    const double t = d;
    d = a;
    a = t;
    b = -c;
    c = 0.0;
  } else if ((a - d) == 0.0 && sgn(1.0, b) != sgn(1.0, c)) {
    cs = 1.0;
    sn = 0.0;
  } else {
    double temp = a - d;
    double p = 0.5 * temp;
    const double bcmax = dmax(fabs(b), fabs(c));
    const double bcmis = dmin(fabs(b), fabs(c)) * sgn(1.0, b) * sgn(1.0, c);
    double scale = dmax(fabs(p), bcmax);
    double z = (p / scale) * p + (bcmax / scale) * bcmis;
    if (z >= 4.0 * eps) {  // real eigenvalues
      z = p + sgn(sqrt(scale) * sqrt(z), p);
      a = d + z;
      d = d - (bcmax / z) * bcmis;
      const double tau = lapy2(c, z);
      cs = z / tau;
      sn = c / tau;
      b = b - c;
      c = 0.0;
    } else {  // complex or almost equal real eigenvalues: make the diagonal equal
      double sigma = b + c;
      for (int count = 1; count <= 20; count++) {
        scale = dmax(fabs(temp), fabs(sigma));
        if (scale >= kSafmx2) {
          sigma *= kSafmn2;
          temp *= kSafmn2;
          continue;
        }
        if (scale <= kSafmn2) {
          sigma *= kSafmx2;
          temp *= kSafmx2;
          continue;
        }
        break;
      }
      p = 0.5 * temp;
      double tau = lapy2(sigma, temp);
      cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau));
      sn = -(p / (tau * cs)) * sgn(1.0, sigma);
      const double aa = a * cs + b * sn, bb = -a * sn + b * cs, cc = c * cs + d * sn, dd = -c * sn + d * cs;
      a = aa * cs + cc * sn;
      b = bb * cs + dd * sn;
      c = -aa * sn + cc * cs;
      d = -bb * sn + dd * cs;
      temp = 0.5 * (a + d);
      a = temp;
      d = temp;
      if (c != 0.0) {
        if (b != 0.0) {
          if (sgn(1.0, b) == sgn(1.0, c)) {  // real eigenvalues after all: upper triangular
            const double sab = sqrt(fabs(b)), sac = sqrt(fabs(c));
            p = sgn(sab * sac, c);
            tau = 1.0 / sqrt(fabs(b + c));
            a = temp + p;
            d = temp - p;
            b = b - c;
            c = 0.0;
            const double cs1 = sab * tau, sn1 = sac * tau;
            temp = cs * cs1 - sn * sn1;
            sn = cs * sn1 + sn * cs1;
            cs = temp;
          }
        } else {
          b = -c;
          c = 0.0;
          temp = cs;
          cs = -sn;
          sn = temp;
        }
      }
    }
  }
}

// H (n x n, ld) <- Q^T H Q upper Hessenberg, Zt (ld) <- Q^T, Q = H_0 H_1 ... H_{n-3} (dgehd2 + dorghr)
SCHUR_DEV void hessenberg(double* H, double* Zt, int n, int ld, int tid, int nt) {
#define PT_H(i, j) H[(long)(i) * ld + (j)]
#define PT_Z(i, j) Zt[(long)(j) * ld + (i)]  // Z(i, j)
  for (long e = tid; e < (long)n * n; e += nt) Zt[(e / n) * ld + e % n] = (e / n == e % n) ? 1.0 : 0.0;
  SCHUR_SYNC();
  for (int k = 0; k + 2 < n; k++) {
    // reflector of x = H(k+1:n, k), every thread (the scaled sum of squares of dnrm2)
    const double alpha = PT_H(k + 1, k);
    double scale = 0.0, ssq = 1.0;
    for (int r = k + 2; r < n; r++) {
      const double x = fabs(PT_H(r, k));
      if (x != 0.0) {
        if (scale < x) {
          const double q = scale / x;
          ssq = 1.0 + ssq * q * q;
          scale = x;
        } else {
          const double q = x / scale;
          ssq += q * q;
        }
      }
    }
    const double xnorm = scale * sqrt(ssq);
    if (xnorm == 0.0) continue;  // (tau = 0: the column is already reduced)
    const double beta = -sgn(lapy2(alpha, xnorm), alpha);
    const double tau = (beta - alpha) / beta;
    const double scal = 1.0 / (alpha - beta);  // v = [1; H(k+2:n, k) scal]
    // H <- H (I - tau v v^T) on columns k+1..n-1, every row
    for (int i = tid; i < n; i += nt) {
      double w = PT_H(i, k + 1);
      for (int j = k + 2; j < n; j++) w += PT_H(i, j) * (PT_H(j, k) * scal);
      w *= tau;
      PT_H(i, k + 1) -= w;
      for (int j = k + 2; j < n; j++) PT_H(i, j) -= w * (PT_H(j, k) * scal);
    }
    SCHUR_SYNC();
    // H <- (I - tau v v^T) H on rows k+1..n-1, columns k+1..n-1;  Z <- Z (I - tau v v^T)
    for (int j = k + 1 + tid; j < n; j += nt) {
      double w = PT_H(k + 1, j);
      for (int r = k + 2; r < n; r++) w += (PT_H(r, k) * scal) * PT_H(r, j);
      w *= tau;
      PT_H(k + 1, j) -= w;
      for (int r = k + 2; r < n; r++) PT_H(r, j) -= w * (PT_H(r, k) * scal);
    }
    for (int i = tid; i < n; i += nt) {
      double w = PT_Z(i, k + 1);
      for (int j = k + 2; j < n; j++) w += PT_Z(i, j) * (PT_H(j, k) * scal);
      w *= tau;
      PT_Z(i, k + 1) -= w;
      for (int j = k + 2; j < n; j++) PT_Z(i, j) -= w * (PT_H(j, k) * scal);
    }
    SCHUR_SYNC();
    // column k after every thread has read v from it (no later step reads or writes column k)
    for (int r = k + 2 + tid; r < n; r += nt) PT_H(r, k) = 0.0;
    if (tid == 0) PT_H(k + 1, k) = beta;
  }
  SCHUR_SYNC();
}

// One 3- (or 2-) element reflector of a bulge step applied to H(k.., k..) and Z(:, k..k+nr-1), deferred column fix-up
struct Fixup {
  int kind;  // 0 none, 1 H(k, k-1) = v1 and zeros below, 2 H(k, k-1) = value
  int k, nr;
  double val;
};

SCHUR_DEV void apply_fixup(double* H, int ld, const Fixup& f) {
  if (f.kind == 1) {
    PT_H(f.k, f.k - 1) = f.val;
    PT_H(f.k + 1, f.k - 1) = 0.0;
    if (f.nr == 3) PT_H(f.k + 2, f.k - 1) = 0.0;
  } else if (f.kind == 2) {
    PT_H(f.k, f.k - 1) = f.val;
  }
}

// Real Schur form of the upper Hessenberg H (n x n, ld): H <- T = Q^T H Q quasi-upper-triangular with 2x2 blocks in
// standard form, Z <- Z Q (Zt transposed).  LAPACK dlahqr with wantt = wantz = true, ilo = 1, ihi = n: Ahues-Kressner
// deflation, exceptional shifts at the 10th and 20th iteration since a deflation, at most 30 max(10, n) iterations per
// deflation.  Returns 0, or (like dlahqr's info) the 1-based row at which that cap was reached.  *max_its: the most
// iterations any deflation took; *sweeps: the total number of QR sweeps.
//
// Each bulge step is one phase ending in one barrier: the reflector is computed by every thread, the rows k..k+2 x
// columns k..k+2 corner is updated by one thread (left then right), the columns right of it (left reflector), the rows
// above and below it (right reflector) and the rows of Z by the others.  These sets are disjoint.  The step's write
// into column k-1 (the chased bulge) is deferred to the next phase, because every thread reads that column first.
SCHUR_DEV int francis(double* H, double* Zt, int n, int ld, int tid, int nt, int* max_its, int* sweeps) {
  const double ulp = kUlp;
  const double smlnum = kSafmin * ((double)n / ulp);
  const int itmax = 30 * (n > 10 ? n : 10);
  const int kexsh = 10;
  *max_its = 0;
  *sweeps = 0;
  int kdefl = 0;
  int i = n - 1;
  while (i >= 0) {
    int l = 0;
    bool split = false;
    for (int its = 0; its <= itmax; its++) {
      // a single negligible subdiagonal element
      int k;
      for (k = i; k > 0; k--) {
        const double hkk1 = fabs(PT_H(k, k - 1));
        if (hkk1 <= smlnum) break;
        double tst = fabs(PT_H(k - 1, k - 1)) + fabs(PT_H(k, k));
        if (tst == 0.0) {
          if (k - 2 >= 0) tst += fabs(PT_H(k - 1, k - 2));
          if (k + 1 <= n - 1) tst += fabs(PT_H(k + 1, k));
        }
        if (hkk1 <= ulp * tst) {
          const double hk1k = fabs(PT_H(k - 1, k));
          const double ab = dmax(hkk1, hk1k), ba = dmin(hkk1, hk1k);
          const double dd = fabs(PT_H(k - 1, k - 1) - PT_H(k, k)), hkk = fabs(PT_H(k, k));
          const double aa = dmax(hkk, dd), bb = dmin(hkk, dd);
          const double s = aa + ab;
          if (ba * (ab / s) <= dmax(smlnum, ulp * (bb * (aa / s)))) break;
        }
      }
      l = k;
      if (l >= i - 1) {  // a 1x1 or 2x2 block has split off
        if (its > *max_its) *max_its = its;
        double a = 0.0, b = 0.0, c = 0.0, d = 0.0, cs = 1.0, sn = 0.0;
        if (l == i - 1) {
          a = PT_H(i - 1, i - 1);
          b = PT_H(i - 1, i);
          c = PT_H(i, i - 1);
          d = PT_H(i, i);
          lanv2(a, b, c, d, cs, sn);
        }
        SCHUR_SYNC();  // (every thread has read the block and the subdiagonal)
        if (tid == 0) {
          if (l > 0) PT_H(l, l - 1) = 0.0;
          if (l == i - 1) {
            PT_H(i - 1, i - 1) = a;
            PT_H(i - 1, i) = b;
            PT_H(i, i - 1) = c;
            PT_H(i, i) = d;
          }
        }
        if (l == i - 1) {  // the rotation on the rest of H and on Z (drot)
          for (int j = i + 1 + tid; j < n; j += nt) {
            const double x = PT_H(i - 1, j), y = PT_H(i, j);
            PT_H(i - 1, j) = cs * x + sn * y;
            PT_H(i, j) = cs * y - sn * x;
          }
          for (int j = tid; j < i - 1; j += nt) {
            const double x = PT_H(j, i - 1), y = PT_H(j, i);
            PT_H(j, i - 1) = cs * x + sn * y;
            PT_H(j, i) = cs * y - sn * x;
          }
          for (int j = tid; j < n; j += nt) {
            const double x = PT_Z(j, i - 1), y = PT_Z(j, i);
            PT_Z(j, i - 1) = cs * x + sn * y;
            PT_Z(j, i) = cs * y - sn * x;
          }
        }
        SCHUR_SYNC();
        split = true;
        break;
      }
      kdefl++;
      (*sweeps)++;
      // shifts
      double h11, h12, h21, h22;
      if (kdefl % (2 * kexsh) == 0) {
        const double s = fabs(PT_H(i, i - 1)) + fabs(PT_H(i - 1, i - 2));
        h11 = 0.75 * s + PT_H(i, i);
        h12 = -0.4375 * s;
        h21 = s;
        h22 = h11;
      } else if (kdefl % kexsh == 0) {
        const double s = fabs(PT_H(l + 1, l)) + fabs(PT_H(l + 2, l + 1));
        h11 = 0.75 * s + PT_H(l, l);
        h12 = -0.4375 * s;
        h21 = s;
        h22 = h11;
      } else {
        h11 = PT_H(i - 1, i - 1);
        h21 = PT_H(i, i - 1);
        h12 = PT_H(i - 1, i);
        h22 = PT_H(i, i);
      }
      double rt1r, rt1i, rt2r, rt2i;
      {
        const double s = fabs(h11) + fabs(h12) + fabs(h21) + fabs(h22);
        if (s == 0.0) {
          rt1r = rt1i = rt2r = rt2i = 0.0;
        } else {
          h11 /= s;
          h21 /= s;
          h12 /= s;
          h22 /= s;
          const double tr = (h11 + h22) / 2.0;
          const double det = (h11 - tr) * (h22 - tr) - h12 * h21;
          const double rtdisc = sqrt(fabs(det));
          if (det >= 0.0) {
            rt1r = tr * s;
            rt2r = rt1r;
            rt1i = rtdisc * s;
            rt2i = -rt1i;
          } else {
            rt1r = tr + rtdisc;
            rt2r = tr - rtdisc;
            if (fabs(rt1r - h22) <= fabs(rt2r - h22)) {
              rt1r *= s;
              rt2r = rt1r;
            } else {
              rt2r *= s;
              rt1r = rt2r;
            }
            rt1i = rt2i = 0.0;
          }
        }
      }
      // two consecutive small subdiagonal elements: where the sweep starts
      int m;
      double v[3] = {0.0, 0.0, 0.0};
      for (m = i - 2; m >= l; m--) {
        double h21s = PT_H(m + 1, m);
        double s = fabs(PT_H(m, m) - rt2r) + fabs(rt2i) + fabs(h21s);
        h21s = PT_H(m + 1, m) / s;
        v[0] = h21s * PT_H(m, m + 1) + (PT_H(m, m) - rt1r) * ((PT_H(m, m) - rt2r) / s) - rt1i * (rt2i / s);
        v[1] = h21s * (PT_H(m, m) + PT_H(m + 1, m + 1) - rt1r - rt2r);
        v[2] = h21s * PT_H(m + 2, m + 1);
        s = fabs(v[0]) + fabs(v[1]) + fabs(v[2]);
        v[0] /= s;
        v[1] /= s;
        v[2] /= s;
        if (m == l) break;
        const double h00 = fabs(PT_H(m, m - 1)) * (fabs(v[1]) + fabs(v[2]));
        const double h01 = ulp * fabs(v[0]) * (fabs(PT_H(m - 1, m - 1)) + fabs(PT_H(m, m)) + fabs(PT_H(m + 1, m + 1)));
        if (h00 <= h01) break;
      }
      const double hmm1 = m > l ? PT_H(m, m - 1) : 0.0;
      SCHUR_SYNC();  // (every thread has read what the sweep overwrites)
      if (tid == 0 && l > 0) PT_H(l, l - 1) = 0.0;  // (column l - 1: the sweep touches columns >= m >= l)
      Fixup pend = {0, 0, 0, 0.0};
      for (int k = m; k <= i - 1; k++) {
        const int nr = (i - k + 1) < 3 ? (i - k + 1) : 3;
        double v1 = 0.0, v2 = 0.0, v3 = 0.0, t1 = 0.0;
        if (k > m) {
          v1 = PT_H(k, k - 1);
          v2 = PT_H(k + 1, k - 1);
          if (nr == 3) v3 = PT_H(k + 2, k - 1);
        } else {
          v1 = v[0];
          v2 = v[1];
          v3 = nr == 3 ? v[2] : 0.0;
        }
        larfg(nr, v1, v2, v3, t1);
        if (tid == 0) apply_fixup(H, ld, pend);
        if (k > m)
          pend = {1, k, nr, v1};
        else if (m > l)
          pend = {2, k, nr, hmm1 * (1.0 - t1)};  // (rather than -H(k, k-1): v2, v3 may have underflowed)
        else
          pend = {0, k, nr, 0.0};
        const double t2 = t1 * v2, t3 = t1 * v3;
        const int kb = k + nr;  // first row / column outside the corner
        if (tid == nt - 1) {  // the corner: left reflector, then right
          double c[3][3];
          for (int r = 0; r < nr; r++)
            for (int q = 0; q < nr; q++) c[r][q] = PT_H(k + r, k + q);
          for (int q = 0; q < nr; q++) {
            const double sum = c[0][q] + v2 * c[1][q] + (nr == 3 ? v3 * c[2][q] : 0.0);
            c[0][q] -= sum * t1;
            c[1][q] -= sum * t2;
            if (nr == 3) c[2][q] -= sum * t3;
          }
          for (int r = 0; r < nr; r++) {
            const double sum = c[r][0] + v2 * c[r][1] + (nr == 3 ? v3 * c[r][2] : 0.0);
            c[r][0] -= sum * t1;
            c[r][1] -= sum * t2;
            if (nr == 3) c[r][2] -= sum * t3;
          }
          for (int r = 0; r < nr; r++)
            for (int q = 0; q < nr; q++) PT_H(k + r, k + q) = c[r][q];
        }
        // left reflector on rows k..k+nr-1, columns kb..n-1
        for (int j = kb + tid; j < n; j += nt) {
          if (nr == 3) {
            const double sum = PT_H(k, j) + v2 * PT_H(k + 1, j) + v3 * PT_H(k + 2, j);
            PT_H(k, j) -= sum * t1;
            PT_H(k + 1, j) -= sum * t2;
            PT_H(k + 2, j) -= sum * t3;
          } else {
            const double sum = PT_H(k, j) + v2 * PT_H(k + 1, j);
            PT_H(k, j) -= sum * t1;
            PT_H(k + 1, j) -= sum * t2;
          }
        }
        // right reflector on columns k..k+nr-1, rows 0..k-1 and (nr = 3) row k+3 when k+3 <= i
        const int extra = (nr == 3 && k + 3 <= i) ? 1 : 0;
        for (int e = tid; e < k + extra; e += nt) {
          const int j = e < k ? e : k + 3;
          if (nr == 3) {
            const double sum = PT_H(j, k) + v2 * PT_H(j, k + 1) + v3 * PT_H(j, k + 2);
            PT_H(j, k) -= sum * t1;
            PT_H(j, k + 1) -= sum * t2;
            PT_H(j, k + 2) -= sum * t3;
          } else {
            const double sum = PT_H(j, k) + v2 * PT_H(j, k + 1);
            PT_H(j, k) -= sum * t1;
            PT_H(j, k + 1) -= sum * t2;
          }
        }
        // Z <- Z G
        for (int j = tid; j < n; j += nt) {
          if (nr == 3) {
            const double sum = PT_Z(j, k) + v2 * PT_Z(j, k + 1) + v3 * PT_Z(j, k + 2);
            PT_Z(j, k) -= sum * t1;
            PT_Z(j, k + 1) -= sum * t2;
            PT_Z(j, k + 2) -= sum * t3;
          } else {
            const double sum = PT_Z(j, k) + v2 * PT_Z(j, k + 1);
            PT_Z(j, k) -= sum * t1;
            PT_Z(j, k + 1) -= sum * t2;
          }
        }
        SCHUR_SYNC();
      }
      if (tid == 0) apply_fixup(H, ld, pend);
      SCHUR_SYNC();
    }
    if (!split) return i + 1;  // (dlahqr: info = i, 1-based)
    kdefl = 0;
    i = l - 1;
  }
  return 0;
}

// Real Schur form of the general H (n x n, ld) in place, Zt <- its orthogonal factor transposed.  Returns -1 when H
// holds a non-finite value (the reference NaN-fills then; H and Zt are left as they are), else francis's info.
SCHUR_DEV int real_schur(double* H, double* Zt, int n, int ld, int tid, int nt, int* max_its, int* sweeps) {
  double bad = 0.0;
  for (long e = tid; e < (long)n * n; e += nt)
    if (!(fabs(H[(e / n) * ld + e % n]) <= 1.7976931348623157e308)) bad = 1.0;
  *max_its = *sweeps = 0;
  if (SCHUR_TEAM_MAX(bad) != 0.0) return -1;
  hessenberg(H, Zt, n, ld, tid, nt);
  return francis(H, Zt, n, ld, tid, nt, max_its, sweeps);
}

// Solve the block pair T_L X + X op(T_R) = B (n1, n2 in {1, 2}) by Gaussian elimination with complete pivoting on its
// Kronecker form, pivots below smin raised to smin (dlasy2; no scaling).  b[r][q] in, x[r][q] out.  Every loop runs
// over the fixed bound 4 (unused slots hold the identity), so the arrays stay in registers.
// a[r][q] of a 2x2 array for run-time r, q in {0, 1} without indexing it dynamically (which would put it in memory)
SCHUR_DEV double at2(const double (&a)[2][2], int r, int q) { return r ? (q ? a[1][1] : a[1][0]) : (q ? a[0][1] : a[0][0]); }

SCHUR_DEV void sy2(const double (&tl)[2][2], const double (&tr)[2][2], int n1, int n2, bool trans_r, double smin,
                   const double (&b)[2][2], double (&x)[2][2]) {
  const int p = n1 * n2;
  double K[4][4], rhs[4];
  int perm[4];
  // unknown u = r n2 + q  <->  x[r][q];  equation (r, q): sum_s tl[r][s] x[s][q] + sum_t x[r][t] op(tr)[t][q]
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int r = e / n2, q = e % n2;
    rhs[e] = e < p ? at2(b, r, q) : 0.0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int s = u / n2, t = u % n2;
      double v = 0.0;
      if (e < p && u < p) {
        if (t == q) v += at2(tl, r, s);
        if (s == r) v += trans_r ? at2(tr, q, t) : at2(tr, t, q);
      } else if (e == u) {
        v = 1.0;
      }
      K[e][u] = v;
    }
    perm[e] = e;
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (c >= p) break;
    int pr = c, pc = c;
    double big = -1.0;
#pragma unroll
    for (int r = c; r < 4; r++)
#pragma unroll
      for (int q = c; q < 4; q++)
        if (r < p && q < p && fabs(K[r][q]) > big) {
          big = fabs(K[r][q]);
          pr = r;
          pc = q;
        }
#pragma unroll
    for (int r = c + 1; r < 4; r++)
      if (r == pr) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const double t = K[c][q];
          K[c][q] = K[r][q];
          K[r][q] = t;
        }
        const double t = rhs[c];
        rhs[c] = rhs[r];
        rhs[r] = t;
      }
#pragma unroll
    for (int q = c + 1; q < 4; q++)
      if (q == pc) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const double t = K[r][c];
          K[r][c] = K[r][q];
          K[r][q] = t;
        }
        const int t = perm[c];
        perm[c] = perm[q];
        perm[q] = t;
      }
    if (fabs(K[c][c]) < smin) K[c][c] = smin;
#pragma unroll
    for (int r = c + 1; r < 4; r++) {
      const double f = K[r][c] / K[c][c];
#pragma unroll
      for (int q = c + 1; q < 4; q++) K[r][q] -= f * K[c][q];
      rhs[r] -= f * rhs[c];
    }
  }
  double u[4];
#pragma unroll
  for (int c = 3; c >= 0; c--) {
    double s = rhs[c];
#pragma unroll
    for (int q = c + 1; q < 4; q++) s -= K[c][q] * u[q];
    u[c] = s / K[c][c];
  }
  x[0][0] = x[0][1] = x[1][0] = x[1][1] = 0.0;
#pragma unroll
  for (int e = 0; e < 4; e++)
#pragma unroll
    for (int w = 0; w < 4; w++)
      if (w < p && perm[e] == w) {
        const int r = w / n2, q = w % n2;
        if (r == 0 && q == 0) x[0][0] = u[e];
        if (r == 0 && q == 1) x[0][1] = u[e];
        if (r == 1 && q == 0) x[1][0] = u[e];
        if (r == 1 && q == 1) x[1][1] = u[e];
      }
}

// Solve R Y + Y op(S) = F in place (Y overwrites F: m x n, ld ldf).  R (m x m, ld ldr) and S (n x n, ld lds)
// quasi-upper-triangular in standard form; op(S) = S^T when trans_s (dtrsyl with trana = 'N', isgn = +1).  A pivot of a
// block pair below smin = max(eps max(max|R|, max|S|), safmin m n / eps) is raised to smin, as dtrsyl does (a nearly
// resonant pair stays finite).  The column blocks of Y run left to right (op = N) or right to left (op = T); in each,
// the contribution of the finished columns is subtracted row-parallel, then the row blocks run bottom up, each one
// phase: the block pair is solved by every thread and the rows above it are updated.  The block's own write is
// deferred to the next phase, because every thread reads its right-hand side first.
SCHUR_DEV void trsyl(const double* R, int ldr, const double* S, int lds, double* F, int ldf, int m, int n, bool trans_s, int tid,
                     int nt) {
#define PT_R(i, j) R[(long)(i) * ldr + (j)]
#define PT_S(i, j) S[(long)(i) * lds + (j)]
#define PT_F(i, j) F[(long)(i) * ldf + (j)]
  double rmax = 0.0;
  for (long e = tid; e < (long)m * m; e += nt) rmax = dmax(rmax, fabs(R[(e / m) * ldr + e % m]));
  for (long e = tid; e < (long)n * n; e += nt) rmax = dmax(rmax, fabs(S[(e / n) * lds + e % n]));
  rmax = SCHUR_TEAM_MAX(rmax);
  const double smin = dmax(kUlp * rmax, kSafmin * ((double)m * (double)n / kUlp));
  int l = trans_s ? n - 1 : 0;
  while (trans_s ? l >= 0 : l < n) {
    int l1, l2, next;
    if (!trans_s) {
      l1 = l;
      l2 = (l + 1 < n && PT_S(l + 1, l) != 0.0) ? l + 1 : l;
      next = l2 + 1;
    } else {
      l2 = l;
      l1 = (l > 0 && PT_S(l, l - 1) != 0.0) ? l - 1 : l;
      next = l1 - 1;
    }
    const int n2 = l2 - l1 + 1;
    double tr[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (r < n2 && q < n2) tr[r][q] = PT_S(l1 + r, l1 + q);
    // F(:, l1..l2) -= Y(:, finished) op(S)(finished, l1..l2)
    const int j0 = trans_s ? l2 + 1 : 0, j1 = trans_s ? n : l1;
    if (j1 > j0)
      for (int i = tid; i < m; i += nt)
        for (int c = l1; c <= l2; c++) {
          double s = 0.0;
          for (int j = j0; j < j1; j++) s += PT_F(i, j) * (trans_s ? PT_S(c, j) : PT_S(j, c));
          PT_F(i, c) -= s;
        }
    SCHUR_SYNC();
    int pk1 = -1, pn1 = 0;
    double px[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    int k = m - 1;
    while (k >= 0) {
      const int k2 = k;
      const int k1 = (k > 0 && PT_R(k, k - 1) != 0.0) ? k - 1 : k;
      const int n1 = k2 - k1 + 1;
      double tl[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, b[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, x[2][2];
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int q = 0; q < 2; q++) {
          if (r < n1 && q < n1) tl[r][q] = PT_R(k1 + r, k1 + q);
          if (r < n1 && q < n2) b[r][q] = PT_F(k1 + r, l1 + q);
        }
      sy2(tl, tr, n1, n2, trans_s, smin, b, x);
      if (tid == 0 && pk1 >= 0)
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
          for (int q = 0; q < 2; q++)
            if (r < pn1 && q < n2) PT_F(pk1 + r, l1 + q) = px[r][q];
      for (int i = tid; i < k1; i += nt) {
        const double r0 = PT_R(i, k1), r1 = n1 == 2 ? PT_R(i, k2) : 0.0;
        PT_F(i, l1) -= r0 * x[0][0] + r1 * x[1][0];
        if (n2 == 2) PT_F(i, l1 + 1) -= r0 * x[0][1] + r1 * x[1][1];
      }
      SCHUR_SYNC();
      pk1 = k1;
      pn1 = n1;
      for (int r = 0; r < 2; r++)
        for (int q = 0; q < 2; q++) px[r][q] = x[r][q];
      k = k1 - 1;
    }
    if (tid == 0 && pk1 >= 0)
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int q = 0; q < 2; q++)
          if (r < pn1 && q < n2) PT_F(pk1 + r, l1 + q) = px[r][q];
    SCHUR_SYNC();
    l = next;
  }
#undef PT_R
#undef PT_S
#undef PT_F
}

#undef PT_H
#undef PT_Z

}  // namespace pt_schur
