"""Device time of batched small ``Solve`` / ``MatrixInverse`` (dispatch/lu.py tiers) against the per-item host loop
they replace, and the share of the HBM copy ceiling the one-launch kernel reaches.

Sweep: batch in {1e3, 1e5} x n in {4, 8, 16, 32, 64} x nrhs in {1, n}, float64 and float32.  Per point: the median
of ``--reps`` timings between HIP events (after ``--warmup`` calls), operands rotated through enough copies to exceed
the Infinity Cache where that takes at most ``--max-copies`` (``cold`` says whether it did).  ``loop`` is the path of
the parent commit, restated here call for call — per item getrf, row gather, two trsm and a copy into the result
(for the inverse: getrf, permuted identity, two trsm, copy); above ``--loop-items`` items it is timed on that many
and scaled by the item count (it is linear in it: every item is the same launches), which ``loop_scaled`` records.
``ceiling`` = a device-to-device copy of 1 GiB (bytes read + written over its time), measured in the same run.

usage: python tools/bench_solve_batched.py [--out FILE.md] [--quick]
Prints one JSON line per point and, with --out, writes the table as markdown."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytensor_amd import ffi  # noqa: E402
from pytensor_amd.device import DeviceArray, contiguous_strides, copy_into  # noqa: E402
from pytensor_amd.dispatch import linalg, lu  # noqa: E402
from pytensor_amd.executor import Env, HipExecutable, HostValue  # noqa: E402
from pytensor_amd.ir import Graph  # noqa: E402

INFINITY_CACHE = 256 << 20


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
        out = fn()
        lib.pthip_event_record(self.e1)
        lib.pthip_event_synchronize(self.e1)
        ms = C.c_float()
        lib.pthip_event_elapsed_ms(self.e0, self.e1, C.byref(ms))
        del out
        return ms.value * 1e-3


def loop_solve(env, A, b, b_ndim, items):
    """the parent's solve_general over a batch: the host loop, one item at a time"""
    n = A.shape[-1]
    core = b.shape[1:]
    step = int(np.prod(core))
    out = DeviceArray.empty(b.shape, b.dtype)
    for k in range(items):
        Ak = A.view((n, n), (n, 1), k * n * n)
        bk = b.view(core, contiguous_strides(core), k * step)
        LU, perm, _, _, _ = lu.getrf_device(env, Ak)
        f = LU.view((n, n), (n, 1))
        pb = lu._permute_rows(env, bk, perm.view((n,), (1,)))
        y = linalg.trsm_device(env, f, pb, True, True, b_ndim)
        copy_into(out.view(core, contiguous_strides(core), k * step), linalg.trsm_device(env, f, y, False, False, b_ndim))
    return out


def loop_inverse(env, A, items):
    """the parent's Blockwise(MatrixInverse): _blockwise_loop over the unbatched handler"""
    n = A.shape[-1]
    out = DeviceArray.empty(A.shape, A.dtype)
    for k in range(items):
        Ak = A.view((n, n), (n, 1), k * n * n)
        LU, perm, _, _, _ = lu.getrf_device(env, Ak, flag_singular=True)
        f = LU.view((n, n), (n, 1))
        pb = DeviceArray.empty((n, n), A.dtype)
        ffi.check(env.lib.pthip_permuted_identity(ffi.np_dtype_code(A.dtype), n, perm.ptr, pb.ptr))
        y = linalg.trsm_device(env, f, pb, True, True, 2)
        copy_into(out.view((n, n), (n, 1), k * n * n), linalg.trsm_device(env, f, y, False, False, 2))
    return out


def copy_ceiling(lib, timer):
    nbytes = 1 << 30
    src, dst = DeviceArray.empty((nbytes,), "uint8"), DeviceArray.empty((nbytes,), "uint8")
    ts = [timer(lambda: lib.pthip_d2d(dst.ptr, src.ptr, nbytes)) for _ in range(6)][1:]
    return 2 * nbytes / statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-copies", type=int, default=24)
    ap.add_argument("--loop-items", type=int, default=1000)
    ap.add_argument("--quick", action="store_true", help="batch 1e3 only, n in {4, 64}")
    args = ap.parse_args()
    ffi.init(0)
    lib = ffi.lib()
    env = make_env()
    timer = Timer(lib)
    ceiling = copy_ceiling(lib, timer)
    print(json.dumps({"copy_ceiling_GBps": round(ceiling / 1e9, 1)}), flush=True)
    rows = []
    rng = np.random.default_rng(0)
    for dtype in ("float64", "float32"):
        for batch in ((1000,) if args.quick else (1000, 100000)):
            for n in ((4, 64) if args.quick else (4, 8, 16, 32, 64)):
                for op, nrhs in (("Solve", 1), ("Solve", n), ("MatrixInverse", n)):
                    isz = np.dtype(dtype).itemsize
                    nbytes = batch * isz * (n * n + (n * nrhs if op == "Solve" else 0) + n * nrhs)
                    copies = max(1, min(args.max_copies, -(-2 * INFINITY_CACHE // nbytes)))
                    cold = copies * nbytes >= 2 * INFINITY_CACHE
                    sets = []
                    for _ in range(copies):
                        A = env.to_device(HostValue((rng.standard_normal((batch, n, n)) + n * np.eye(n)).astype(dtype)))
                        b = env.to_device(HostValue(rng.standard_normal((batch, n, nrhs)).astype(dtype))) if op == "Solve" else None
                        sets.append((A, b))
                    if op == "Solve":
                        new = lambda A, b: lu.solve_general(env, A, b, 2)  # noqa: E731
                        old = lambda A, b, k: loop_solve(env, A, b, 2, k)  # noqa: E731
                    else:
                        new = lambda A, b: lu.matrix_inverse(None, [A], env)  # noqa: E731
                        old = lambda A, b, k: loop_inverse(env, A, k)  # noqa: E731
                    ts = [timer(lambda s=sets[i % copies]: new(*s)) for i in range(args.warmup + args.reps)][args.warmup:]
                    t_new = statistics.median(ts)
                    items = min(batch, args.loop_items)
                    tl = [timer(lambda s=sets[i % copies]: old(*s, items)) for i in range(3)][1:]
                    t_old = statistics.median(tl) * batch / items
                    row = {"dtype": dtype, "op": op, "batch": batch, "n": n, "nrhs": nrhs, "new_us": round(t_new * 1e6, 1),
                           "loop_us": round(t_old * 1e6, 1), "loop_scaled": items < batch, "speedup": round(t_old / t_new, 1),
                           "GBps": round(nbytes / t_new / 1e9, 1), "of_copy_ceiling": round(nbytes / t_new / ceiling, 3), "cold": cold,
                           "spread": round((max(ts) - min(ts)) / t_new, 2)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del sets
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"copy ceiling (1 GiB device-to-device, read + written): {ceiling / 1e9:.0f} GB/s\n\n")
            f.write("`loop_us` is the parent commit's per-item path restated inside tools/bench_solve_batched.py on this commit "
                    f"(a stand-in, not a run of the parent), timed on at most {args.loop_items} items and scaled by the item "
                    "count where `loop_scaled` is true.  Times are medians of device time between events.\n\n")
            cols = list(rows[0])
            f.write("| " + " | ".join(cols) + " |\n|" + "---|" * len(cols) + "\n")
            for r in rows:
                f.write("| " + " | ".join(str(r[c]) for c in cols) + " |\n")


if __name__ == "__main__":
    main()
