"""Write the discrete-Riccati fixtures: tests/golden/riccati/<case>.npz + tests/golden/riccati/cases.json.

Each expected X (and the gradients of ``grad_m{2,10,40}.npz``, the seasonal Kalman logp + gradient of
``kalman.npz``) is the reference's own ``solve_discrete_are`` graph (QR-compressed pencil + QZ) run by its C
linker (``Mode(linker="cvm")``) on the importable reference copy that ``build()`` makes (oracle/_ref);
``scipy.linalg.solve_discrete_are`` is a cross-check whose distance is recorded in the JSON.  Inputs are
not stored: tests/riccati_cases.py regenerates them (random systems from their seed, checked against the
SHA-256 recorded here).  float32 expectations are the same graph on float32 inputs.

Usage:  python tools/make_riccati_fixtures.py
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "riccati")

import make_ref  # noqa: E402
import riccati_cases as rc  # noqa: E402

F32_CASES = ("reference", "random_5x3", "random_14x1")


def main():
    make_ref.build()
    make_ref.activate()
    import pytensor
    import pytensor.tensor as pt
    import scipy.linalg as sl
    from pytensor.compile.mode import Mode
    from pytensor.tensor.linalg import solve_discrete_are

    fns = {}

    def ref(A, B, Q, R):
        dt = str(A.dtype)
        if dt not in fns:
            ins = [pt.matrix(nm, dtype=dt) for nm in "ABQR"]
            fns[dt] = pytensor.function(ins, solve_discrete_are(*ins), mode=Mode(linker="cvm", optimizer="fast_run"))
        return np.asarray(fns[dt](A, B, Q, R))

    cases = []
    for k, (m, n) in enumerate(rc.RANDOM_SIZES):
        cases.append({"name": f"random_{m}x{n}", "kind": "random", "m": m, "n": n, "seed": 1000 + k})
    for kind in ("reference", "seasonal", "unstabilizable", "singular_r", "undetectable_scalar", "undetectable_2x2", "lyapunov_n0"):
        cases.append({"name": kind, "kind": kind})
    os.makedirs(OUT, exist_ok=True)
    for meta in cases:
        if meta["kind"] == "random":
            arrs = rc.random_case(meta["m"], meta["n"], meta["seed"])
        else:
            meta["sha256"] = None
            arrs = {**rc.SPECIAL, "seasonal": lambda: (lambda T, Z, Qs, H: (T.T.copy(), Z.T.copy(), Qs, H))(*rc.seasonal_model())}[meta["kind"]]()
        A, B, Q, R = arrs
        meta["m"], meta["n"] = B.shape
        meta["sha256"] = rc.sha(arrs)
        X = ref(A, B, Q, R)
        out = {"X": X}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                Xs = sl.solve_discrete_are(A, B, Q, R)
                meta["scipy_rel_diff"] = float(np.max(np.abs(X - Xs)) / np.max(np.abs(Xs))) if np.all(np.isfinite(X)) else None
            except Exception as e:  # noqa: BLE001
                meta["scipy_rel_diff"] = None
                meta["scipy_error"] = f"{type(e).__name__}: {e}"
        meta["reference_all_nan"] = bool(np.all(np.isnan(X)))
        if meta["name"] in F32_CASES:
            out["X32"] = ref(*(a.astype(np.float32) for a in arrs))
        if np.all(np.isfinite(X)) and meta["n"] > 0:
            # the closed loop's spectral radius and the conditioning of the solution, for the tolerance
            K = np.linalg.solve(R + B.T @ X @ B, B.T @ X @ A)
            meta["closed_loop_rho"] = float(np.max(np.abs(np.linalg.eigvals(A - B @ K))))
            meta["cond_X"] = float(np.linalg.cond(X)) if meta["m"] else None
        np.savez_compressed(os.path.join(OUT, meta["name"] + ".npz"), **out)
        print(meta["name"], {k: v for k, v in meta.items() if k not in ("sha256", "name")})
    # gradients (the reference's pullback under its C linker) and the seasonal Kalman logp + gradient: inputs stored
    # with the expected values (they are small)
    mode = Mode(linker="cvm", optimizer="fast_run")
    ins = [pt.dmatrix(nm) for nm in "ABQR"]
    Wv = pt.dmatrix("W")
    cost = rc.gradient_cost(pt, solve_discrete_are(*ins), Wv)
    fgrad = pytensor.function([*ins, Wv], [cost, *pytensor.grad(cost, ins)], mode=mode)
    for m in (2, 10, 40):
        vals = list(rc.reference_problem()) if m == 2 else list(rc.random_case(m, 2, 5000 + m))
        W = np.random.default_rng(m).normal(size=(m, m))
        c, *g = fgrad(*vals, W)
        np.savez_compressed(os.path.join(OUT, f"grad_m{m}.npz"), A=vals[0], B=vals[1], Q=vals[2], R=vals[3], W=W, cost=c,
                            gA=g[0], gB=g[1], gQ=g[2], gR=g[3])
        print(f"grad_m{m}", float(c))
    kins, logp = rc.kalman_graph(pt, solve_discrete_are, pytensor.scan)
    fk = pytensor.function(kins, [logp, pytensor.grad(logp, kins[0])], mode=mode)
    rng = np.random.default_rng(3)
    y = np.cumsum(rng.normal(size=96)) * 0.3 + np.tile(np.sin(np.arange(12)), 8)
    log_sd = np.log(np.array([0.5, 0.2, 0.4, 0.3, 1.0]))
    lp, g = fk(log_sd, y)
    np.savez_compressed(os.path.join(OUT, "kalman.npz"), log_sd=log_sd, y=y, logp=lp, grad=g)
    print("kalman", float(lp), g)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump({"generator": "tools/make_riccati_fixtures.py", "numpy": np.__version__, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
