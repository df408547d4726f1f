"""Device-side runners of the softmax / log-sum-exp sweep (tests/test_gpu_tiers_softmax.py), and its child process.

As a module: ``run`` uploads the NaN-padded parent of an operand (tests/softmax_cases.py), calls the C ABI with the
pointer at the aligned or the off-by-one element, counts the launches the call made and verifies the sentinels around
the output and the workspace.  ``job`` runs one named (case, dtype, generator, alignment, output) the same way in the
parent and in the child and holds it to the checker.

As a program: ``_softmax_tiers_worker.py OUT.json ROUTE_KW_JSON JOB...`` (or ``OUT.npz graph``, see ``graph_job``) — the ``PTHIP_*`` switches of csrc/softmax.hip
are read once into ``static const``s, so the parent sets them in the environment of a fresh child.  The child checks its
own outputs with the same checker (they are tens of megabytes: only the worst ratio, the launch count and a SHA-256 of
the raw bytes travel back, the last for the bit-equality the parent asserts).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import softmax_cases as sc  # noqa: E402

GUARD = 256  # bytes of sentinel on each side of an output


class Out:
    """``n`` elements inside a longer device buffer, ``off`` elements behind a 256-byte boundary: sentinel bytes on both
    sides, NaN bits in between (an element the kernel does not write fails the checker)."""

    def __init__(self, n, dt, off=0):
        from pytensor_amd.device import DeviceArray

        self.dt, self.n = np.dtype(dt), int(n)
        nbytes = self.n * self.dt.itemsize
        self.lead = GUARD + off * self.dt.itemsize
        host = np.full(self.lead + nbytes + GUARD, 0xFF, dtype=np.uint8)
        host[:self.lead] = (np.arange(self.lead) * 37 + 11).astype(np.uint8)
        host[self.lead + nbytes:] = (np.arange(GUARD) * 41 + 5).astype(np.uint8)
        self.host = host
        self.dev = DeviceArray.from_host(host)
        assert self.dev.ptr % 256 == 0
        self.ptr = self.dev.ptr + self.lead

    def fetch(self, shape=None):
        """the output; raises if a sentinel byte changed"""
        back = self.dev.to_host()
        nbytes = self.n * self.dt.itemsize
        assert np.array_equal(back[:self.lead], self.host[:self.lead]), "bytes IN FRONT of the output were overwritten"
        assert np.array_equal(back[self.lead + nbytes:], self.host[self.lead + nbytes:]), "bytes BEHIND the output were overwritten"
        out = back[self.lead:self.lead + nbytes].copy().view(self.dt)
        return out.reshape(shape) if shape is not None else out


def upload(parent, off):
    from pytensor_amd.device import DeviceArray

    d = DeviceArray.from_host(parent)
    assert d.ptr % 256 == 0
    return d, d.ptr + off * parent.itemsize


def run(ffi, case, what, x, mis="aligned", ws_short=0):
    """One call of the entry point of ``case`` computing ``what`` on the operand ``x``.  ``mis``: "aligned", or which of
    x / out sits one element behind a 16-byte boundary.  Returns (rc, output or None, launches)."""
    lib = ffi.lib()
    dt = x.dtype
    code = ffi.np_dtype_code(dt)
    parent, lead = sc.embed(x, 1 if mis in ("x", "both") else 0)
    dx, px = upload(parent, lead)
    ooff = 1 if mis in ("out", "both") else 0
    before = lib.pthip_launch_count()
    ws = None
    if case.entry == "softmax":
        rows, cols = case.shape
        out, shape = Out(rows * cols, dt, ooff), (rows, cols)
        rc = lib.pthip_softmax(code, int(what == "log_softmax"), rows, cols, px, out.ptr)
    elif case.entry == "lse_rows":
        rows, cols = case.shape
        out, shape = Out(rows, dt, ooff), (rows,)
        rc = lib.pthip_logsumexp_rows(code, rows, cols, px, out.ptr)
    else:
        b, R, Cc = case.shape
        wsb = int(lib.pthip_colstat_workspace(code, b, R, Cc)) - ws_short
        ws = Out(wsb, np.uint8)
        if what == "lse":
            out, shape = Out(b * Cc, dt, ooff), (b, Cc)
            rc = lib.pthip_logsumexp_cols(code, b, R, Cc, px, out.ptr, ws.ptr, wsb)
        else:
            out, shape = Out(b * R * Cc, dt, ooff), (b, R, Cc)
            rc = lib.pthip_softmax_cols(code, int(what == "log_softmax"), b, R, Cc, px, out.ptr, ws.ptr, wsb)
    launches = int(lib.pthip_launch_count() - before)
    got = out.fetch(shape)
    if ws is not None:
        ws.fetch()
    del dx
    return rc, (got if rc == 0 else None), launches


def expected_launches(case, what):
    return 1 if case.entry != "cols" else 2 if what == "lse" else 3


_CHILD = {(c.entry, c.name): c for c in sc.CHILD_CASES}


def spec_of(case, dt, gen, mis, what):
    return f"{case.entry}:{case.name}:{dt}:{gen}:{mis}:{what}"


_STATS = {}


def job(ffi, spec, route_kw=None, keep_stats=False):
    """``ENTRY:CASE:DT:GEN:MIS:WHAT`` (a case of softmax_cases.CHILD_CASES) -> {"ratio", "launches", "digest", "tier"}; the
    output is held to the checker here, with the geometry the switch of this process gives (``route_kw``)"""
    entry, name, dt, gen, mis, what = spec.split(":")
    case = _CHILD[entry, name]
    key = (entry, name, dt, gen)
    if key in _STATS:
        x, st = _STATS[key]
    else:
        x = sc.values(case, dt, gen)
        st = sc.Stats(x)
        if keep_stats:  # (the last one only: the jobs of a case are adjacent, and a Stats is hundreds of megabytes)
            _STATS.clear()
            _STATS[key] = (x, st)
    r = sc.route_of(case, dt, what, mis, **(route_kw or {}))
    rc, got, launches = run(ffi, case, what, x, mis)
    ffi.check(rc)
    ex = sc.expect(st, what, dt, sc.c_exp_of(case, dt, r), sc.levels_of(case, dt, r))
    ratio = sc.check(got, ex, dt, spec)
    return {"ratio": ratio, "launches": launches, "digest": sc.digest(got), "tier": sc.tier_name(case, dt, r, what)}


def graph_job(path):
    """``softmax(x, axis=0)`` through a one-node graph, clean and with the non-finite columns of
    tests/test_gpu_softmax_cols.py: with ``PTHIP_SOFTMAX_COLS=0`` in the environment it runs on the generated N-d tile"""
    from pytensor_amd.dispatch import extra
    from pytensor_amd.executor import HipExecutable
    from pytensor_amd.ir import Graph

    # the route: every Softmax node must go through _softmax_any_axes and get its result from it (a None there falls
    # through to a transposed copy and the row kernels, which would hide the form under test)
    taken = {"calls": 0, "declined": 0}
    inner = extra._softmax_any_axes

    def counted(*a, **k):
        out = inner(*a, **k)
        taken["calls"] += 1
        taken["declined"] += out is None
        return out

    extra._softmax_any_axes = counted
    res = {}
    for dt in sc.DTYPES:
        var = {"dtype": dt, "shape": [None, None], "kind": "tensor"}
        d = {"name": "graph", "inputs": [0], "outputs": [1], "vars": [dict(var, id=0, name="x"), dict(var, id=1)], "input_names": ["x"],
             "nodes": [{"op": "Softmax", "params": {"axis": [0], "log": False}, "inputs": [0], "outputs": [1]}]}
        exe = HipExecutable(Graph.from_dict(d), device=0)
        x = np.random.default_rng(6).normal(size=(600, 6)).astype(dt)
        res[f"clean:{dt}"] = np.asarray(exe(x)[0])
        x[:, 1] = -np.inf
        x[17, 2] = np.inf
        x[500, 3] = np.nan
        x[3, 4] = -np.inf
        res[f"planted:{dt}"] = np.asarray(exe(x)[0])
        res[f"route:{dt}"] = np.array([taken["calls"], taken["declined"]])
    np.savez(path, **res)


def main(argv):
    from pytensor_amd import ffi

    if argv[2] == "graph":
        return graph_job(argv[1])
    ffi.init(0)
    route_kw = json.loads(argv[2])
    res = {}
    for spec in argv[3:]:
        res[spec] = job(ffi, spec, route_kw, keep_stats=True)
    with open(argv[1], "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv)
