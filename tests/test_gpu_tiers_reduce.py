"""GPU: every route of ``pthip_reduce`` (csrc/reduce.hip) through the C ABI, against the references and the derived bound
of tests/reduce_cases.py (no tuned factor; the worst ``|err| / bound`` per route and dtype is printed,
profiles/reduce_tiers.md).

Each row of the table is the smallest view that reaches one route of ``make_plan`` at one of its edges
(tests/test_reduce_cases.py proves the coverage on the CPU).  Seven dtype families run every row with every op that applies
to them, every other (in, acc, out) line of the three dispatch tables runs on a contig and a strided two-stage row.  Each
call runs with x, out and the workspace on 16-byte boundaries and with x and out one element behind one, inside poisoned
parents and between sentinels (the guarded buffers of tests/_softmax_tiers_worker.py), and the number of launches is held
to the restated plan.  Integer and bool results, Max / Min, and float sums or products of exactly representable data are
bit-exact; rounded float data is held to the bound.
"""
import numpy as np
import pytest

import reduce_cases as rc
import _softmax_tiers_worker as dev

pytestmark = pytest.mark.gpu
WORST = {}  # (route, triple, op) -> worst |err| / bound


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def call(ffi, row, op, tri, X0, off=0, ws_short=0, extents=None):
    """One ``pthip_reduce`` of the view of ``row`` holding ``X0``.  ``off``: x and out one element behind a 16-byte
    boundary.  Returns (rc, (A, B) output, launches); the sentinels around out and the workspace are verified."""
    lib = ffi.lib()
    parent, first, _ = rc.build(row, X0, off)
    dx, px = dev.upload(parent, first)
    sA, sR, sB, _ = row.strides()
    A, R, B = extents or (row.A, row.R, row.B)
    codes = [ffi.np_dtype_code(t) for t in tri]
    wsb = max(int(lib.pthip_reduce_workspace(codes[1], max(A, 0), max(R, 0), max(B, 0))) - ws_short, 0)
    ws = dev.Out(wsb, np.uint8)
    out = dev.Out(row.n_out, tri[2], off)
    before = lib.pthip_launch_count()
    r = lib.pthip_reduce(rc.OPS[op], *codes, px, out.ptr, A, R, B, sA, sR, sB, ws.ptr, wsb)
    launches = int(lib.pthip_launch_count() - before)
    got = out.fetch((row.A, row.B))
    ws.fetch()
    del dx
    return r, got, launches


def run_op(hip, row, op, tri, what, gens=None):
    """every generator (or ``gens``) of (row, op, triple), aligned and misaligned"""
    p = row.plan()
    lines = []
    for gen in gens or rc.gens_for(op, tri[0], row):
        X0 = rc.generate(row, op, gen, tri[0], tri[2])
        _, _, X = rc.build(row, X0)
        exact = rc.is_exact(op, gen, tri)
        fl = op in ("Add", "Mul") and np.dtype(tri[0]).kind == "f"
        if fl:
            want, bound = rc.float_expect(op, X, tri, p)
        for off in (0, 1):
            tag = f"{what} {row.name} {op} {'/'.join(tri)} {gen} {'misaligned' if off else 'aligned'} [{rc.route_name(p)}]"
            r, got, launches = call(hip, row, op, tri, X0, off)
            hip.check(r)
            assert launches == p.launches, f"{tag}: {launches} launches, the plan makes {p.launches}"
            ratio = 0.0
            if fl:
                ratio = rc.check_float(got, want, bound, tag)
                assert ratio <= 1.0
                if exact:
                    with np.errstate(over="ignore"):
                        rc.check_exact(got, want.astype(tri[2]), tag)
            else:
                rc.check_exact(got, rc.np_reduce(op, X, tri), tag)
            key = (rc.route_name(p), "/".join(tri), op)
            WORST[key] = max(WORST.get(key, 0.0), ratio)
            lines.append(f"{tag}: worst |err|/bound = {ratio:.3g}")
    print("\n".join(lines))


# (Max / Min of an empty row are refused: test_refusals)
@pytest.mark.parametrize("fam,row,op,gen", [pytest.param(fam, row, op, gen, id=f"{fam}-{row.name}-{op}-{gen}") for fam in rc.FAMILIES for row in rc.ROWS
                                            for op, tri in rc.FAMILIES[fam].items() if row.R or op not in ("Max", "Min")
                                            for gen in rc.gens_for(op, tri[0], row)])
def test_family(hip, fam, row, op, gen):
    run_op(hip, row, op, rc.FAMILIES[fam][op], fam, (gen,))


@pytest.mark.parametrize("op,tri", rc.other_runs(), ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_other_triples(hip, op, tri):
    for name in rc.OTHER_ROWS:
        run_op(hip, rc.BY_NAME[name], op, tri, "other")


MINMAX_FLOAT = [t for t in rc.MINMAX_TRIPLES if np.dtype(t[0]).kind == "f"]


@pytest.mark.parametrize("name", rc.PLANT_ROWS)
def test_minmax_nan_at_every_split_boundary(hip, name):
    """one NaN in the row of output (0, 0): that output is NaN, every other output bit-identical to the clean run"""
    row = rc.BY_NAME[name]
    tris = MINMAX_FLOAT if row.R < 10 ** 6 else [("float32",) * 3]
    for tri in tris:
        X0 = rc.generate(row, "Max", "flat", tri[0], tri[2])
        for op in ("Max", "Min"):
            r, clean, _ = call(hip, row, op, tri, X0)
            hip.check(r)
            rc.check_exact(clean, rc.np_reduce(op, X0, tri), f"{name} {op} clean")
            for pos in rc.plant_positions(row):
                P0 = X0.copy()
                P0[0, pos, 0] = np.nan
                r, got, _ = call(hip, row, op, tri, P0)
                hip.check(r)
                assert np.isnan(got[0, 0]), f"{name} {op} {tri}: NaN at r = {pos} lost: {got[0, 0]!r}"
                got[0, 0] = clean[0, 0]
                rc.check_exact(got, clean, f"{name} {op} {tri} NaN at r = {pos}: another output changed")


@pytest.mark.parametrize("name", ("rows3_R257", "contig256_two", "strided_two_257", "strided_one_255"))
def test_minmax_extremes(hip, name):
    row = rc.BY_NAME[name]
    shape = (row.A, row.R, row.B)
    for tri in rc.MINMAX_TRIPLES:
        dt = np.dtype(tri[0])
        if dt.kind == "f":
            fills = (-np.inf, np.inf)
        else:
            fills = (np.iinfo(dt).min, np.iinfo(dt).max)
        for fill in fills:
            X0 = np.full(shape, fill, dtype=dt)
            for op in ("Max", "Min"):
                for off in (0, 1):
                    r, got, _ = call(hip, row, op, tri, X0, off)
                    hip.check(r)
                    rc.check_exact(got, rc.np_reduce(op, X0, tri), f"{name} {op} {tri} all {fill}")
        if dt.kind != "f":
            # the identity everywhere but one element: Max over lowest with one lowest + 1, Min over highest with one highest - 1
            for op, fill, one in (("Max", np.iinfo(dt).min, np.iinfo(dt).min + 1), ("Min", np.iinfo(dt).max, np.iinfo(dt).max - 1)):
                X0 = np.full(shape, fill, dtype=dt)
                X0[:, row.R - 1, :] = one
                r, got, _ = call(hip, row, op, tri, X0)
                hip.check(r)
                rc.check_exact(got, rc.np_reduce(op, X0, tri), f"{name} {op} {tri} one element off the identity")


def test_refusals(hip):
    lib = hip.lib()
    row = rc.BY_NAME["contig64_two"]
    f64 = ("float64",) * 3
    X0 = rc.generate(row, "Add", "flat", "float64", "float64")

    def refused(msg, *a, **k):
        r, got, launches = call(hip, *a, **k)
        assert r != 0 and launches == 0, (msg, r, launches)
        assert msg.encode() in lib.pthip_last_error(), lib.pthip_last_error()

    for op, tri in (("Add", ("float64", "float32", "float64")), ("Add", ("float16", "float16", "float16")), ("Max", ("int32", "int64", "int64")),
                    ("And", ("float32",) * 3), ("Xor", ("bool", "int64", "int64")), ("Mul", ("bool",) * 3)):
        t = tuple(tri)
        refused(f"pthip_reduce: unsupported dtype combination in={hip.np_dtype_code(t[0])} acc={hip.np_dtype_code(t[1])} out={hip.np_dtype_code(t[2])}",
                row, op, t, X0.astype(t[0]))
    for ext in ((-1, row.R, 1), (row.A, -1, 1), (row.A, row.R, -1)):
        refused("pthip_reduce: negative extent", row, "Add", f64, X0, extents=ext)
    for name in ("contig64_two", "strided_two_257", "finisher256"):
        r2 = rc.BY_NAME[name]
        refused("pthip_reduce: workspace too small", r2, "Add", f64, rc.generate(r2, "Add", "ints", "float64", "float64"), ws_short=1)
    for name in ("rows3_R0", "strided_R0"):
        r0 = rc.BY_NAME[name]
        E = np.zeros((r0.A, 0, r0.B))
        refused("zero-size array to reduction operation maximum which has no identity", r0, "Max", f64, E)
        refused("zero-size array to reduction operation minimum which has no identity", r0, "Min", f64, E)
        refused("zero-size array to reduction operation maximum which has no identity", r0, "Max", ("bool",) * 3, E.astype(bool))
    before = lib.pthip_launch_count()
    assert lib.pthip_reduce(7, 7, 7, 7, None, None, 1, 1, 1, 1, 1, 1, None, 0) != 0 and lib.pthip_launch_count() == before
    assert b"pthip_reduce: unknown op 7" in lib.pthip_last_error()


def test_degenerate_shapes(hip):
    for name in ("rows3_R0", "full_R0", "strided_R0"):
        row = rc.BY_NAME[name]
        for tri in (("float64",) * 3, ("float32", "float64", "float32"), ("int32", "int64", "int64"), ("float16", "float32", "float16")):
            E = np.zeros((row.A, 0, row.B), tri[0])
            for op, val in (("Add", 0), ("Mul", 1)):
                r, got, launches = call(hip, row, op, tri, E)
                hip.check(r)
                assert launches == 1 and np.array_equal(got, np.full((row.A, row.B), val, tri[2])), (name, op, tri, got)
    for A, R, B in ((0, 5, 3), (3, 5, 0), (0, 0, 0)):
        row = rc.Row("empty", A, R, B)
        r, got, launches = call(hip, row, "Add", ("float64",) * 3, np.zeros((A, R, B)))
        hip.check(r)
        assert launches == 0 and got.size == 0


def test_two_runs_are_bit_equal(hip):
    for name in ("contig64_two", "contig256_two_3", "strided_two_257", "finisher256_2"):
        row = rc.BY_NAME[name]
        for tri in (("float64",) * 3, ("float32",) * 3):
            X0 = rc.generate(row, "Add", "flat", tri[0], tri[2])
            a = call(hip, row, "Add", tri, X0)[1]
            b = call(hip, row, "Add", tri, X0)[1]
            assert np.array_equal(a, b), (name, tri)


def test_zz_report():
    """the worst ratio per route and dtype of this run (the table of profiles/reduce_tiers.md)"""
    table = {}
    for (route, tri, op), v in WORST.items():
        if op in ("Add", "Mul") and tri.startswith("float"):
            k = (route, tri)
            table[k] = max(table.get(k, 0.0), v)
    for route, tri in sorted(table):
        print(f"ROUTE {route} | {tri}: {table[route, tri]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
