"""Per-call time of the Sylvester / Lyapunov solves under ``mode="hip"`` above the Kronecker tier (Bartels-Stewart,
csrc/sylvester.hip), one JSON line per configuration (default output: profiles/sylvester_bench.jsonl).

Configurations: ``solve_sylvester`` at m = n in {65, 128, 256, 512, 1024} against ``scipy.linalg.solve_sylvester`` on
this machine's host; ``solve_continuous_lyapunov`` at 128 and 512 (one Schur form) against SciPy; the DARE value and
gradient at m = 100 against the reference's C linker; and the Bartels-Stewart path called directly against the
Kronecker tier at m = n = 64.  Calls through ``pytensor.function`` include the host upload of the operands and the
download of X (which synchronises the device); the direct calls end in a device synchronise.  Each side runs one
warm-up call, then is called until it has run for about a second (at least 3 calls; one call when it takes over 10 s).

Usage:  python tools/bench_sylvester.py [--out PATH] [--max-n N]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def _time(f, args, budget=1.0):
    f(*args)  # warm-up (compilation, plan capture)
    ts = []
    t_end = time.perf_counter() + budget
    while len(ts) < 3 or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        f(*args)
        ts.append(time.perf_counter() - t0)
        if ts[-1] > 10.0 or len(ts) >= 200:
            break
    return float(np.median(ts)), len(ts)


def _problem(m, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(m, m)) / np.sqrt(m) + 3.0 * np.eye(m), rng.normal(size=(n, n)) / np.sqrt(n) + 3.0 * np.eye(n),
            rng.normal(size=(m, n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sylvester_bench.jsonl"))
    ap.add_argument("--max-n", type=int, default=1024)
    a = ap.parse_args()
    import make_ref

    make_ref.activate()
    import pytensor
    import pytensor.tensor as pt
    import scipy.linalg as sl
    from pytensor.compile.mode import Mode
    from pytensor.tensor.linalg import solve_continuous_lyapunov, solve_discrete_are, solve_sylvester

    import pytensor_amd
    from pytensor_amd import ffi
    from pytensor_amd.device import DeviceArray

    pytensor_amd.register()
    lib = ffi.lib()
    buf = ctypes.create_string_buffer(256)
    ffi.check(lib.pthip_device_name(buf, 256))
    device = buf.value.decode()
    rows = []

    def emit(row):
        row["device"] = device
        print(json.dumps(row), flush=True)
        rows.append(row)

    A, B, C = (pt.dmatrix(nm) for nm in "ABC")
    f_syl = pytensor.function([A, B, C], solve_sylvester(A, B, C), mode="hip")
    for n in (65, 128, 256, 512, 1024):
        if n > a.max_n:
            continue
        vals = _problem(n, n, n)
        X = f_syl(*vals)
        t_hip, k_hip = _time(f_syl, vals)
        t_sp, k_sp = _time(sl.solve_sylvester, vals)
        res = np.linalg.norm(vals[0] @ X + X @ vals[1] - vals[2]) / np.linalg.norm(vals[2])
        emit({"case": f"solve_sylvester_{n}", "m": n, "n": n, "hip_ms": round(t_hip * 1e3, 3), "scipy_host_ms": round(t_sp * 1e3, 3),
              "speedup_vs_scipy": round(t_sp / t_hip, 3), "rel_residual": float(res), "calls": [k_hip, k_sp]})
    f_lyap = pytensor.function([A, C], solve_continuous_lyapunov(A, C), mode="hip")
    for n in (128, 512):
        if n > a.max_n:
            continue
        rng = np.random.default_rng(n)
        vals = (rng.normal(size=(n, n)) / np.sqrt(n) - 2.0 * np.eye(n), rng.normal(size=(n, n)))
        X = f_lyap(*vals)
        t_hip, k_hip = _time(f_lyap, vals)
        t_sp, k_sp = _time(sl.solve_continuous_lyapunov, vals)
        err = float(np.max(np.abs(X - sl.solve_continuous_lyapunov(*vals))) / np.max(np.abs(X)))
        emit({"case": f"continuous_lyapunov_{n}", "m": n, "hip_ms": round(t_hip * 1e3, 3), "scipy_host_ms": round(t_sp * 1e3, 3),
              "speedup_vs_scipy": round(t_sp / t_hip, 3), "max_rel_diff_vs_scipy": err, "calls": [k_hip, k_sp]})
    # the DARE value and gradient at m = 100: its pullback's bilinear Lyapunov solve is on this tier
    m = 100
    rng = np.random.default_rng(m)
    vals = [0.9 * rng.normal(size=(m, m)) / np.sqrt(m), rng.normal(size=(m, 2)), np.eye(m), np.eye(2), rng.normal(size=(m, m))]
    ins = [pt.dmatrix(nm) for nm in "ABQR"]
    w = pt.dmatrix("W")
    cost = (solve_discrete_are(*ins) * w).sum()
    outs = [cost, *pytensor.grad(cost, ins)]
    f_hip = pytensor.function([*ins, w], outs, mode="hip")
    f_ref = pytensor.function([*ins, w], outs, mode=Mode(linker="cvm", optimizer="fast_run"))
    got, want = f_hip(*vals), f_ref(*vals)
    err = max(float(np.max(np.abs(g - r)) / max(float(np.max(np.abs(r))), 1e-300)) for g, r in zip(got, want))
    t_hip, k_hip = _time(f_hip, vals)
    t_ref, k_ref = _time(f_ref, vals)
    emit({"case": "dare_value_grad_100", "m": m, "n": 2, "hip_ms": round(t_hip * 1e3, 3), "ref_c_linker_ms": round(t_ref * 1e3, 3),
          "speedup": round(t_ref / t_hip, 3), "max_rel_diff": err, "calls": [k_hip, k_ref]})
    # Bartels-Stewart against the Kronecker tier at m = n = 64 (both on device-resident operands)
    from pytensor_amd.dispatch.decomp import solve_sylvester_schur
    from pytensor_amd.executor import HipExecutable  # noqa: F401  (the library is initialised by f_syl above)

    class _Env:
        lib = ffi.lib()
        keepalive = []

        @staticmethod
        def to_device(v):
            return v

        @staticmethod
        def timed(name, fn):
            fn()

    n = 64
    vals = _problem(n, n, n)
    dev = [DeviceArray.from_host(np.ascontiguousarray(v)) for v in vals]

    def run_bs():
        X = solve_sylvester_schur(_Env, *dev)
        ffi.check(lib.pthip_synchronize())
        _Env.keepalive.clear()
        return X

    X_bs = run_bs().to_host()
    X_kr = f_syl(*vals)
    t_bs, k_bs = _time(run_bs, [])
    t_kr, k_kr = _time(f_syl, vals)
    emit({"case": "schur_vs_kronecker_64", "m": n, "n": n, "schur_direct_ms": round(t_bs * 1e3, 3),
          "kronecker_call_ms": round(t_kr * 1e3, 3), "max_rel_diff": float(np.max(np.abs(X_bs - X_kr)) / np.max(np.abs(X_kr))),
          "calls": [k_bs, k_kr], "note": "kronecker_call_ms includes the upload of A, B, C and the download of X"})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
