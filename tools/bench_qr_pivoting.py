"""Device time of the column-pivoted factorisation ``pthip_geqp3`` next to the unpivoted ``pthip_geqrf`` at the same
shape (csrc/decomp.hip: one workgroup per matrix in both).

Shapes, float64: 128 x 128, one matrix (the LDS form); 512 x 512, one matrix (the global form); 32 x 32 with batch 256.
Both factor in place, so every call gets a fresh copy of the operand, made before the timed window.  A window is
``inner`` calls between two HIP events (``inner`` chosen so that a window lasts about ``--window-ms``); the two
kernels alternate window by window, ``--rounds`` windows each after ``--warmup`` untimed ones, and the figure is the
median time per call with the spread (max - min) / median over the windows beside it.  ``extra_passes`` is what
pivoting adds per column by count: one search over n norms, one swap of m values, one downdating pass over n
values, against the 2 m n values the reflector application reads and writes — the ratio those passes would explain if
every value cost the same.

usage: python tools/bench_qr_pivoting.py [--out FILE.jsonl]
Prints one JSON line per shape and, with --out, writes the same lines to the file."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytensor_amd import ffi  # noqa: E402
from pytensor_amd.device import DeviceArray, copy_into  # noqa: E402
from pytensor_amd.dispatch.decomp import geqp3_lds_fits  # noqa: E402
from pytensor_amd.executor import Env, HipExecutable, HostValue  # noqa: E402
from pytensor_amd.ir import Graph  # noqa: E402

SHAPES = [(1, 128, 128), (1, 512, 512), (256, 32, 32)]


def make_env():
    g = Graph(name="bench")
    a = g.new_var("float64", (None,), name="a")
    g.inputs, g.outputs = [a], [a]
    return Env(HipExecutable(g))


class Timer:
    def __init__(self, lib):
        self.lib = lib
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        lib.pthip_event_create(C.byref(self.e0))
        lib.pthip_event_create(C.byref(self.e1))

    def __call__(self, fn):
        lib = self.lib
        lib.pthip_event_record(self.e0)
        fn()
        lib.pthip_event_record(self.e1)
        lib.pthip_event_synchronize(self.e1)
        ms = C.c_float()
        lib.pthip_event_elapsed_ms(self.e0, self.e1, C.byref(ms))
        return ms.value * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--max-inner", type=int, default=64)
    args = ap.parse_args()
    ffi.init(0)
    lib = ffi.lib()
    env = make_env()
    timer = Timer(lib)
    rng = np.random.default_rng(0)
    dt = ffi.np_dtype_code(np.dtype("float64"))
    lines = []
    for batch, m, n in SHAPES:
        master = env.to_device(HostValue(rng.standard_normal((batch, m, n))))
        tau = DeviceArray.empty((batch, min(m, n)), "float64")
        jpvt = DeviceArray.empty((batch, n), "int32")
        calls = {
            "geqrf": lambda a: ffi.check(lib.pthip_geqrf(dt, batch, m, n, a.ptr, tau.ptr)),
            "geqp3": lambda a: ffi.check(lib.pthip_geqp3(dt, batch, m, n, a.ptr, tau.ptr, jpvt.ptr)),
        }
        # one untimed call each (code object load), then one timed call sizes the window
        once = {}
        for name, fn in calls.items():
            fn(master.contiguous_copy())
            a = master.contiguous_copy()
            once[name] = timer(lambda: fn(a))
        inner = int(max(1, min(args.max_inner, args.window_ms * 1e-3 / max(once.values()))))
        work = [DeviceArray.empty(master.shape, "float64") for _ in range(inner)]
        times = {name: [] for name in calls}
        for r in range(args.warmup + args.rounds):
            for name, fn in calls.items():
                for w in work:
                    copy_into(w, master)
                t = timer(lambda: [fn(w) for w in work]) / inner
                if r >= args.warmup:
                    times[name].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        line = {"dtype": "float64", "batch": batch, "m": m, "n": n, "form": "lds" if geqp3_lds_fits(m, n, 8) else "global",
                "geqrf_us": round(med["geqrf"] * 1e6, 1), "geqp3_us": round(med["geqp3"] * 1e6, 1),
                "ratio": round(med["geqp3"] / med["geqrf"], 3),
                "geqrf_spread": round((max(times["geqrf"]) - min(times["geqrf"])) / med["geqrf"], 3),
                "geqp3_spread": round((max(times["geqp3"]) - min(times["geqp3"])) / med["geqp3"], 3),
                "extra_passes": round(1 + (2 * n + m) / (2 * m * n), 3), "inner": inner, "rounds": args.rounds}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
