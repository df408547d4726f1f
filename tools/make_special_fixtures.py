"""Reference values of jv / ive / kve / owens_t at 40 digits (mpmath) → tests/golden/special_functions/special_bessel.{npz,json}.

The points cover x from 1e-300 to 1e4 and orders in [-100, 100] (integers, half-integers, values within 1e-9 of an
integer and random reals), the boundaries between the regions of csrc/special_bessel.h (x^2 = 4(nu+1), x = 25,
x = nu^2/8, x = nu^2/2, x = 2), points next to the zeros of J_nu, float32-representable points, and x up to 1e300.
Each row stores the value and the error envelope its bar is measured against:

    jv       sqrt(J_v^2 + Y_v^2)
    ive      ive(|v|, x) + (2/pi) |sin v pi| kve(|v|, x) e^{-2x}
    kve      |kve(v, x)|
    owens_t  |T(h, a)|

Run:  python tools/make_special_fixtures.py  (a few minutes on one core).
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

mp.mp.dps = 40
# a subdirectory: every *.json directly under tests/golden is a graph case of tests/util.golden_cases
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "special_functions")


def _points(rng):
    v, x = [], []

    def add(vs, xs):
        v.extend(float(a) for a in vs)
        x.extend(float(b) for b in xs)

    n = 160
    add(rng.uniform(-100, 100, n), 10 ** rng.uniform(-300, 4, n))
    add(rng.uniform(-100, 100, n), 10 ** rng.uniform(-3, 4, n))
    add(rng.integers(-100, 101, n), 10 ** rng.uniform(-3, 4, n))
    add(rng.integers(-100, 100, n) + 0.5, 10 ** rng.uniform(-3, 4, n))
    near = rng.integers(-100, 101, n) + rng.choice([-1, 1], n) * 10 ** rng.uniform(-12, -6, n)
    add(near, 10 ** rng.uniform(-3, 3.5, n))
    add(rng.uniform(-10, 10, n), rng.uniform(0, 50, n))
    nu = rng.uniform(0, 100, n)
    sg = rng.choice([-1.0, 1.0], n)
    for edge in (2 * np.sqrt(nu + 1), np.maximum(25, nu * nu / 8), np.maximum(25, nu * nu / 2)):
        add(sg * nu, edge * (1 + rng.uniform(-1e-3, 1e-3, n)))
    add(sg[:40] * nu[:40], 2.0 * (1 + rng.uniform(-1e-3, 1e-3, 40)))
    # float32-representable operands
    add(np.float32(rng.uniform(-20, 20, n)), np.float32(10 ** rng.uniform(-3, 2, n)))
    # far range: only the asymptotic expansions apply
    add(rng.uniform(-100, 100, 60), 10 ** rng.uniform(4, 300, 60))
    return np.array(v), np.array(x)


def _jzeros(rng):
    v, x = [], []
    for nu in rng.uniform(0, 60, 40):
        k = int(rng.integers(1, 8))
        z = float(mp.besseljzero(mp.mpf(nu), k))
        for d in (0.0, 1e-10, -1e-7):
            v.append(float(nu))
            x.append(z * (1 + d))
    return np.array(v), np.array(x)


def _safe(f):
    try:
        r = f()
        return r if mp.isfinite(r) else mp.nan
    except Exception:  # mpmath gives up (deep underflow / overflow): the row is dropped
        return mp.nan


def _kve(nu, x):
    """K_nu(x) e^x; near an integer order mpmath's besselk cancels (and raises its precision without end), so there it
    is int_0^inf exp(-x (cosh t - 1)) cosh(nu t) dt (DLMF 10.32.9), cut where it has fallen below e^-100"""
    if abs(nu - mp.nint(nu)) > mp.mpf("1e-5") or x > 1e3:
        return mp.besselk(nu, x) * mp.exp(x)
    f = lambda t: mp.exp(-x * (mp.cosh(t) - 1)) * mp.cosh(nu * t)  # noqa: E731
    t1 = mp.acosh(1 + 1 / x)
    t2 = mp.acosh(1 + (100 + abs(nu) * 10) / x)
    return mp.quad(f, [0, t1 / 4, t1, t2, 2 * t2])  # past 2 t2 the integrand is below e^-(100 e^t2)


def _y_env(nu, x, **kw):
    # the envelope is a scale, not a value: at an order within 1e-5 of an integer the integer order serves
    n = mp.nint(nu)
    return mp.bessely(n if abs(nu - n) < mp.mpf("1e-5") else nu, x, **kw)


def _bessel(v, x):
    rows = {"jv": [], "ive": [], "kve": []}
    for i, (a, b) in enumerate(zip(v, x)):
        if i % 500 == 0:
            print(f"bessel {i}/{len(v)}", file=sys.stderr, flush=True)
        va, xa = mp.mpf(a), mp.mpf(b)
        kw = dict(maxterms=10**6)
        jv = _safe(lambda: mp.besselj(va, xa, **kw))
        env = _safe(lambda: mp.sqrt(mp.besselj(va, xa, **kw) ** 2 + _y_env(va, xa, **kw) ** 2))
        rows["jv"].append((a, b, jv, env))
        iv = _safe(lambda: mp.besseli(va, xa, **kw) * mp.exp(-xa))
        ia = _safe(lambda: mp.besseli(abs(va), xa, **kw) * mp.exp(-xa))
        ka = _safe(lambda: _kve(abs(va), xa))
        ienv = ia + (0 if a == int(a) else 2 / mp.pi * abs(mp.sinpi(va)) * ka * mp.exp(-2 * xa))
        rows["ive"].append((a, b, iv, ienv))
        rows["kve"].append((a, b, ka, abs(ka)))
    return rows


def _owens(rng):
    n = 300
    h = np.concatenate([rng.uniform(-38, 38, n), 10 ** rng.uniform(-6, 1.58, n), [0.0, 1.0, 5.0, 37.0]])
    a = np.concatenate([rng.uniform(-5, 5, n), rng.choice([-1, 1], n) * 10 ** rng.uniform(-6, 6, n), [0.5, 1.0, 1e3, 0.999]])
    rows = []
    for hv, av in zip(h, a):
        hh, aa = mp.mpf(abs(hv)), mp.mpf(abs(av))
        # T = e^{-h^2/2}/(2 pi) int_0^a e^{-h^2 t^2/2}/(1+t^2) dt: the Gaussian is split at multiples of 1/h
        pts = sorted({mp.mpf(0), aa, *[mp.mpf(k) / hh for k in range(1, 16) if hh > 0 and k / hh < aa]})
        if aa > 1:
            pts = sorted(set(pts) | {mp.mpf(1)})
        r = mp.exp(-hh**2 / 2) / (2 * mp.pi) * mp.quad(lambda t: mp.exp(-hh**2 * t**2 / 2) / (1 + t**2), pts)
        r = -r if av < 0 else r
        rows.append((float(hv), float(av), r, abs(r)))
    return rows


def main():
    rng = np.random.default_rng(20261015)
    v, x = _points(rng)
    vz, xz = _jzeros(rng)
    v, x = np.concatenate([v, vz]), np.concatenate([x, xz])
    rows = _bessel(v, x)
    rows["owens_t"] = _owens(rng)
    arrays = {}
    for k, rs in rows.items():
        a = np.array([[r[0], r[1], float(r[2]), float(r[3])] for r in rs])
        keep = np.isfinite(a).all(axis=1) & (np.abs(a[:, 2]) >= 1e-300) & (np.abs(a[:, 3]) < 1e300)
        arrays[k] = a[keep]
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "special_bessel.npz"), **arrays)
    recipe = {
        "generator": "tools/make_special_fixtures.py",
        "reference": f"mpmath {mp.__version__} at {mp.mp.dps} digits",
        "columns": ["first argument (v or h)", "second argument (x or a)", "value", "envelope"],
        "rows": {k: int(len(a)) for k, a in arrays.items()},
    }
    with open(os.path.join(OUT, "special_bessel.json"), "w") as fh:
        json.dump(recipe, fh, indent=1)
    print(json.dumps(recipe), file=sys.stderr)


if __name__ == "__main__":
    main()
