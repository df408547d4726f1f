"""Bessel functions of real order and Owen's T under ``mode="hip"`` against the reference's C linker.

Graphs, on fp64 vectors of 1e6 and 1e7 elements (v in [-10, 10], x in [0, 50], h in [-5, 5]):
    jv         sum(jv(v, x))
    log_iv     sum(log(iv(v, x))) and its gradient in x       (v in [0, 10], so that iv > 0)
    kv         sum(kv(v, x))
    owens_t    sum(owens_t(h, x / 10))
The device time is the wall time of a whole call of the compiled function: the host operands are uploaded on
every call (so they arrive cold, from host memory through HBM), the kernels run, and a scalar (the jv, kv and
owens_t graphs) or the gradient vector (log_iv) comes back.  Median of 5 calls after 2 warm calls.  The C linker
(which evaluates these ops through SciPy on one core) is timed once at 1e6 elements.  The graph's scalar ops in
the lowered IR are listed to show that the four ops sit inside the fused device kernels.
One JSON line per case.   usage: python tools/bench_special.py [--quick]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import e2e_util as E  # noqa: E402


def graphs(pytensor, ptt):
    v, x, h = ptt.dvector("v"), ptt.dvector("x"), ptt.dvector("h")
    liv = ptt.log(ptt.iv(v, x)).sum()
    return {
        "jv": ([v, x], [ptt.jv(v, x).sum()]),
        "log_iv": ([v, x], [liv, pytensor.grad(liv, x)]),
        "kv": ([v, x], [ptt.kv(v, x).sum()]),
        "owens_t": ([h, x], [ptt.owens_t(h, x / 10).sum()]),
    }


def inputs(name, n, rng):
    x = rng.uniform(0, 50, n)
    if name == "owens_t":
        return [rng.uniform(-5, 5, n), x]
    if name == "log_iv":
        return [rng.uniform(0, 10, n), x]
    return [rng.uniform(-10, 10, n), x]


def wall(f, args, reps=5, warm=2):
    for _ in range(warm):
        f(*args)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f(*args)
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    quick = "--quick" in sys.argv
    pytensor = E.activate()
    import pytensor.tensor as ptt

    from pytensor_amd import codegen_scalar

    rng = np.random.default_rng(0)
    for name, (ins, outs) in graphs(pytensor, ptt).items():
        f = pytensor.function(ins, outs, mode="hip")
        ops = sorted({op for nd in f.maker.linker.last_ir.nodes if nd.op == "Elemwise" for op in codegen_scalar.body_ops(nd.params["scalar"])})
        kinds = sorted({nd.op for nd in f.maker.linker.last_ir.nodes})
        c_s = None
        if not quick:
            g = pytensor.function(ins, outs, mode=E.reference_mode())
            args = inputs(name, 10**6, rng)
            t = time.perf_counter()
            g(*args)
            c_s = time.perf_counter() - t
        for n in (10**6, 10**7) if not quick else (10**5,):
            args = inputs(name, n, rng)
            dev = wall(f, args)
            line = {"graph": name, "n": n, "device_s": round(dev, 6), "device_elems_per_s": round(n / dev, 1), "scalar_ops": ops, "ir_nodes": kinds}
            if c_s is not None and n == 10**6:
                line.update({"c_linker_s": round(c_s, 4), "speedup_vs_c_linker": round(c_s / dev, 1)})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
