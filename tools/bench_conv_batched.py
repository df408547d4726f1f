"""Call time of ``Blockwise(Convolve1d)`` and ``Blockwise(Convolve2d)`` on stacks, on the one-launch path
(csrc/conv_batched.hip) and on the per-item loop, in the same run.

Both go through ``HipExecutable`` on one ``Blockwise`` node with a constant ``full_mode``.  The baseline is the same
executable with ``dispatch.misc.conv_tier`` answering "loop", which sends the node to ``_blockwise_loop`` as before the
batched kernels: same commit, same box, same run, the two paths alternating call by call.

Sweep: adstock-like stacks, batch 8 / 256 / 4096 x signal 128 / 1024 / 16384 x taps 12 / 64 / 1024 (taps <= signal), one
kernel per item; image stacks 64 x (128 x 128) with 5 x 5 and 31 x 31 kernels; "full" and "valid"; float64 and float32.
Per point: the median host-clock time of a whole executable call (upload of both operands, the device work, download of
the result, ending in the synchronise of the download) over ``--reps`` calls after ``--warmup`` (two calls where one
takes over a second).  The transfers are the same on both paths, so the difference of the two columns is the device
work and the host loop; ``max_abs_diff`` is the largest difference between the two results.

usage: python tools/bench_conv_batched.py [--jsonl FILE] [--md FILE] [--quick]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES, SIGNALS, TAPS = [8, 256, 4096], [128, 1024, 16384], [12, 64, 1024]
IMAGES = [(64, (128, 128), (5, 5)), (64, (128, 128), (31, 31))]


def executable(core_ndim, dtype, full):
    from pytensor_amd.executor import HipExecutable
    from pytensor_amd.ir import Graph

    g = Graph(name=f"conv{core_ndim}d")
    ins = [g.new_var(dtype, (None,) * (core_ndim + 1)) for _ in range(2)]
    mode = g.new_var("bool", (), const=np.asarray(bool(full)))
    out = g.new_var(dtype, (None,) * (core_ndim + 1))
    sig = "(n),(k),()->(o)" if core_ndim == 1 else "(m,n),(p,q),()->(o,r)"
    g.add_node("Blockwise", {"core_op": f"Convolve{core_ndim}d", "core_params": {}, "signature": sig}, [*ins, mode], [out])
    g.inputs, g.outputs = ins, [out]
    return HipExecutable(g)


def timed_pair(fns, warmup, reps):
    """medians of the callables of ``fns``, alternating them call by call"""
    first = []
    for fn in fns:
        t0 = time.perf_counter()
        fn()
        first.append(time.perf_counter() - t0)
    if max(first) > 1.0:
        warmup, reps = 0, 2
    ts = [[] for _ in fns]
    for k in range(warmup + reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            if k >= warmup:
                t.append(time.perf_counter() - t0)
    return [statistics.median(t) for t in ts]


def measure(args):
    from pytensor_amd import ffi
    from pytensor_amd.dispatch import misc

    ffi.init(0)
    stack_tier = misc.conv_tier
    rng = np.random.default_rng(0)
    points = [(1, b, (n,), (k,)) for b in BATCHES for n in SIGNALS for k in TAPS if k <= n] + [(2, b, i, k) for b, i, k in IMAGES]
    if args.quick:
        points = [p for p in points if p[1] <= 256 and p[2][0] <= 1024]
    rows = []
    out = open(args.jsonl, "w") if args.jsonl else None
    for dtype in ("float64", "float32"):
        for core_ndim, batch, sa, sb in points:
            a, b = rng.standard_normal((batch, *sa)).astype(dtype), rng.standard_normal((batch, *sb)).astype(dtype)
            for full in (True, False):
                exe = executable(core_ndim, dtype, full)
                got = {}

                def run(tier):
                    misc.conv_tier = stack_tier if tier == "stack" else (lambda *_: "loop")
                    try:
                        (got[tier],) = exe(a, b)
                    finally:
                        misc.conv_tier = stack_tier

                t_stack, t_loop = timed_pair([lambda: run("stack"), lambda: run("loop")], args.warmup, args.reps)
                row = {"dtype": dtype, "core": f"{core_ndim}d", "batch": batch, "a": list(sa), "b": list(sb), "mode": "full" if full else "valid",
                       "stack_us": round(t_stack * 1e6, 1), "loop_us": round(t_loop * 1e6, 1), "max_abs_diff": float(np.abs(got["stack"] - got["loop"]).max())}
                rows.append(row)
                print(json.dumps(row), flush=True)
                if out:
                    out.write(json.dumps(row) + "\n")
                    out.flush()
    if args.md:
        lines = ["| dtype | op | batch | operand | kernel | mode | loop_us | stack_us | loop / stack | max abs diff |", "|" + "---|" * 10]
        for r in rows:
            shape = lambda s: " x ".join(map(str, s))
            lines.append(f"| {r['dtype']} | {r['core']} | {r['batch']} | {shape(r['a'])} | {shape(r['b'])} | {r['mode']} | {r['loop_us']:.1f} | {r['stack_us']:.1f} | "
                         f"{r['loop_us'] / r['stack_us']:.1f} | {r['max_abs_diff']:.1e} |")
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jsonl")
    ap.add_argument("--md")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="batches up to 256, signals up to 1024")
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
