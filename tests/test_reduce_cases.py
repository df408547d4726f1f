"""CPU self-test of tests/reduce_cases.py: the table reaches every route and edge of csrc/reduce.hip ``make_plan``, names
every dtype line of its three dispatch tables, the restated workspace agrees with the library's (host-only) function, the
bound is attainable by a plain NumPy evaluation in the kernel's order of magnitude, and the ``cancel`` generator tells a
float32 accumulator from a float64 one on every row it runs on."""
import ctypes
import os

import numpy as np
import pytest

import order_cases as oc
import reduce_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plans():
    return [(r, r.plan(), r.strides()) for r in rc.ROWS]


def test_every_route_and_edge_is_reached():
    P = _plans()
    cond = {}
    for route in rc.ROUTES:
        cond[route] = any(rc.route_name(p) == route for r, p, s in P)
    cond["routes are the seven"] = {rc.route_name(p) for r, p, s in P} == set(rc.ROUTES)
    for R in (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048):
        cond[f"contig R = {R}"] = any(r.R == R and p.route != "strided" for r, p, s in P)
    cond["group switch: 2047 on 64 lanes, 2048 on 256"] = any(r.R == 2047 and p.group == 64 for r, p, s in P) and any(r.R == 2048 and p.group == 256 for r, p, s in P)
    cond["inactive 64-lane groups, one stage"] = any(p.group == 64 and p.nsplit == 1 and r.n_out % 4 for r, p, s in P)
    cond["inactive 64-lane groups, two stages"] = any(p.group == 64 and p.nsplit > 1 and (r.n_out * p.nsplit) % 4 for r, p, s in P)
    cond["inactive 64-lane groups in stage 2"] = any(p.g2 == 64 and r.n_out % 4 for r, p, s in P)
    for n in (255, 256, 257):
        for st in (1, 2):
            cond[f"strided n_out = {n}, {st} stage(s)"] = any(p.route == "strided" and r.n_out == n and p.launches == st for r, p, s in P)
    cond["R = 32, 255 outputs: contig"] = any(r.R == 32 and r.n_out == 255 and p.route == "contig-64" for r, p, s in P)
    cond["R = 32, 256 outputs: strided"] = any(r.R == 32 and r.n_out == 256 and p.route == "strided" for r, p, s in P)
    cond["R = 33, 256 outputs: contig"] = any(r.R == 33 and r.n_out == 256 and p.route == "contig-64" for r, p, s in P)
    cond["sB = 1, sR = -1, B = 63: contig"] = any(s[1] == -1 and s[2] == 1 and r.B == 63 and p.route == "contig-64" for r, p, s in P)
    cond["sB = 1, sR = -1, B = 64: strided"] = any(s[1] == -1 and s[2] == 1 and r.B == 64 and p.route == "strided" for r, p, s in P)
    cond["sR = -1, base at the last element, one and two groups"] = {p.group for r, p, s in P if r.layout == "rev" and s[3] == r.R - 1} == {64, 256}
    cond["sR > 1 with B = 1, one and two stages"] = {p.launches for r, p, s in P if s[1] > 1 and r.B == 1 and p.route == "contig-64"} == {1, 2}
    cond["padded rows, contig and strided"] = {p.route for r, p, s in P if r.layout == "pad"} >= {"contig-64", "strided"}
    cond["an empty last split"] = any(p.nsplit > 1 and (p.nsplit - 1) * p.chunk >= r.R for r, p, s in P)
    cond["stage-2 finisher of 256 lanes, one and two outputs"] = {r.n_out for r, p, s in P if p.g2 == 256} >= {1, 2}
    cond["n_out * nsplit beyond one block row of the strided grid"] = any(p.route == "strided" and r.n_out > 256 and p.nsplit > 1 for r, p, s in P)
    cond["R = 0 on both kernels"] = {p.route for r, p, s in P if r.R == 0} == {"contig-64", "strided"}
    missed = [k for k, v in cond.items() if not v]
    assert not missed, "the table misses:\n  " + "\n  ".join(missed)
    for name in rc.OTHER_ROWS + rc.PLANT_ROWS:
        assert name in rc.BY_NAME
    assert {rc.route_name(rc.BY_NAME[n].plan()) for n in rc.OTHER_ROWS} == {"contig-64 two-stage", "strided two-stage"}


def test_the_empty_split_search():
    """the comment of reduce_cases: the strided kernel admits an empty last split, the contig kernel none"""
    found = rc.find_empty_split()
    assert "contig" not in found and "strided" in found
    A, R, B = found["strided"]
    p = rc.make_plan(A, R, B, B, 1)
    assert (p.nsplit - 1) * p.chunk >= R
    r = rc.BY_NAME["strided_empty_split"]
    assert r.n_out * r.R <= A * R * B * 1.2  # the table's row is no larger than what the search finds


def test_every_dispatch_line_is_named():
    src = open(os.path.join(ROOT, "pytensor_amd", "csrc", "reduce.hip")).read()
    lines = rc.parse_dispatch(src)
    assert lines["dispatch_types"] == list(rc.TYPES_TRIPLES)
    assert lines["dispatch_minmax"] == list(rc.MINMAX_TRIPLES)
    assert lines["dispatch_bool"] == list(rc.BOOL_TRIPLES)
    ran = {(op, tri) for fam in rc.FAMILIES.values() for op, tri in fam.items()} | set(rc.other_runs())
    for op in rc.OPS:
        for tri in rc.TABLE_OF[op]:
            assert (op, tri) in ran, (op, tri)
    for fam in rc.FAMILIES.values():
        for op, tri in fam.items():
            table = rc.BOOL_TRIPLES if tri[0] == "bool" and op in ("Max", "Min") else rc.TABLE_OF[op]  # (bool Max / Min: Or / And)
            assert tri in table, (op, tri)


def test_restated_workspace_matches_the_library():
    import __graft_entry__ as ge
    from pytensor_amd import ffi

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "pytensor_amd", "libpthip.so"))
    lib.pthip_reduce_workspace.restype = ctypes.c_size_t
    lib.pthip_reduce_workspace.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    for r, p, s in _plans():
        for acc in ("float64", "float32", "int64", "uint8", "bool", "float16"):
            have = int(lib.pthip_reduce_workspace(ffi.np_dtype_code(acc), r.A, r.R, r.B))
            assert have == rc.reduce_workspace(acc, r.A, r.R, r.B), (r.name, acc)
            need = p.nsplit * r.n_out * np.dtype(acc).itemsize if p.nsplit > 1 else 0
            assert need <= have, (r.name, acc, need, have)
            assert (rc.reduce_workspace(acc, r.A, r.R, r.B) == 0) == (have == 0)


def _np_in_kernel_order(X, op, tri, plan):
    """Add / Mul of the view as a correct kernel could form it: splits in the accumulator type, then the partials, then
    the cast to out"""
    acc = np.dtype(tri[1])
    uf = np.add if op == "Add" else np.multiply
    parts = [uf.reduce(X[:, s * plan.chunk:(s + 1) * plan.chunk].astype(acc), axis=1, dtype=acc) for s in range(plan.nsplit)]
    return uf.reduce(np.stack(parts, axis=1), axis=1, dtype=acc).astype(tri[2])


@pytest.mark.parametrize("row", [r for r in rc.ROWS if r.A * r.R * r.B <= 3e6], ids=lambda r: r.name)
def test_numpy_meets_the_bound_and_mutations_miss_it(row):
    p = row.plan()
    for fam in ("f64", "f32_f64", "f32", "f16"):
        for op in ("Add", "Mul"):
            tri = rc.FAMILIES[fam][op]
            for gen in rc.gens_for(op, tri[0], row):
                _, _, X = rc.build(row, rc.generate(row, op, gen, tri[0], tri[2]))
                want, bound = rc.float_expect(op, X, tri, p)
                assert np.all(np.isfinite(want.astype(np.float64)))
                got = _np_in_kernel_order(X, op, tri, p)
                assert rc.check_float(got, want, bound, f"{row.name} {fam} {op} {gen}") <= 1.0
                if rc.is_exact(op, gen, tri):
                    rc.check_exact(got, want.astype(tri[2]))
                if gen == "ints" and row.R >= 1 and row.n_out:
                    # an element dropped or taken twice: the answer is off by an integer, far above the bound
                    # (except under a float32 accumulator over a million elements, whose own bound is above one unit)
                    first = X[:, :1].astype(np.longdouble).sum(axis=1)
                    first = np.where(first == 0, 1, first)
                    assert np.all(np.abs(first) > 2 * bound) or (tri[1] == "float32" and row.R > 10 ** 6)
                    for bad in (want - first, want + first):
                        if np.any(np.abs(first) > 2 * bound):
                            with pytest.raises(AssertionError):
                                rc.check_float(bad.astype(tri[2]), want, bound)
                if op == "Mul" and gen == "prod" and row.n_out:
                    tiny = float(np.finfo(tri[2]).tiny)
                    assert np.all(np.abs(want) >= tiny) and np.all(np.abs(want) <= float(np.finfo(tri[2]).max))


def test_cancel_tells_a_float32_accumulator_from_a_float64_one():
    tri = rc.FAMILIES["f32_f64"]["Add"]
    n = 0
    for row in rc.ROWS:
        if "cancel" not in rc.gens_for("Add", "float32", row) or row.A * row.R * row.B > 3e6 or not row.n_out:
            continue
        _, _, X = rc.build(row, rc.generate(row, "Add", "cancel", "float32", "float32"))
        want, bound = rc.float_expect("Add", X, tri, row.plan())
        mag = np.abs(X.astype(np.float64)).sum(axis=1)
        assert np.all(mag > 1e4 * np.abs(want.astype(np.float64))), row.name  # sum|x| / |sum x| is large
        seq = np.cumsum(X, axis=1, dtype=np.float32)[:, -1]  # strictly sequential in float32
        err = np.abs(seq.astype(np.longdouble) - want)
        assert np.all(err > bound), f"{row.name}: a float32 sequential sum passes the float64 bound on {int((err <= bound).sum())} outputs"
        n += 1
    assert n >= 25


def test_integer_references_wrap():
    row = rc.BY_NAME["contig64_two"]
    X = rc.generate(row, "Add", "wide", "int32", "int32")
    got = rc.np_reduce("Add", X, ("int32", "int64", "int32"))
    assert got.dtype == np.int32
    exact = [sum(int(v) for v in X[a, :, 0]) for a in range(row.A)]
    assert [int(v) for v in got[:, 0]] == [((e + 2 ** 31) % 2 ** 32) - 2 ** 31 for e in exact]
    assert any(abs(e) >= 2 ** 31 for e in exact)
    X = rc.generate(row, "Mul", "odd", "uint8", "uint8")
    got = rc.np_reduce("Mul", X, ("uint8", "uint64", "uint8"))
    want = [np.uint8(int(np.prod([int(v) for v in X[a, :, 0]], dtype=object)) % 256) for a in range(row.A)]
    assert list(got[:, 0]) == want and all(v % 2 for v in want)


def test_plants_cover_the_split_boundaries():
    for name in rc.PLANT_ROWS:
        row = rc.BY_NAME[name]
        p = row.plan()
        pos = rc.plant_positions(row)
        assert 0 in pos and row.R - 1 in pos
        if p.nsplit > 1:
            assert p.chunk - 1 in pos and p.chunk in pos and (p.nsplit - 1) * p.chunk in pos
        assert len(pos) <= 16
    assert {rc.route_name(rc.BY_NAME[n].plan()) for n in rc.PLANT_ROWS} >= set(rc.ROUTES) - {"contig-256 one-stage", "strided one-stage"}


def test_search_pairs_follow_numpy_promotion():
    """the comparison type restated from ``pthip_searchsorted`` is the one ``np.result_type`` gives the pair: float64 for a
    float with anything and for uint64 with a signed integer, uint64 for uint64 with an unsigned integer or bool, and a
    signed integer (which int64 holds) for every other pair"""
    seen = set()
    for xdt, vdt in oc.SEARCH_PAIRS:
        rt = np.result_type(np.dtype(xdt), np.dtype(vdt))
        path = oc.search_path(xdt, vdt)
        assert path == {"f": "float", "u": "unsigned" if rt == np.uint64 else "signed", "i": "signed", "b": "signed"}[rt.kind], (xdt, vdt, rt, path)
        seen.add((path, np.uint64 in (np.dtype(xdt), np.dtype(vdt))))
    assert seen == {("float", False), ("float", True), ("signed", False), ("unsigned", True)}
    for pair in (("float16", "float16"), ("uint64", "uint64"), ("uint64", "int64"), ("uint64", "int8"), ("uint32", "int64"), ("bool", "uint64")):
        assert pair in oc.SEARCH_PAIRS


def test_sort_tiers_restated():
    assert [oc.sort_far_phases(n) for n in oc.SORT_N_LONG] == [1, 2, 3]
    assert [oc.sort_launches(1, n) for n in (1, 4096, 4097, 8193, 16385)] == [1, 1, 5, 8, 12]
    assert oc.sort_launches(0, 5) == 0 and oc.sort_launches(3, 0) == 0
    for dt in oc.SORT_DTYPES:
        for kind in oc.sort_kinds(dt):
            x = oc.sort_data(kind, dt, 2, 257)
            assert x.dtype == np.dtype(dt) and x.shape == (2, 257)
            if kind == "four":
                assert len(np.unique(x)) == (2 if dt == "bool" else 4)
            if kind == "nan":
                b = rc.bits(x[np.isnan(x)])
                assert len(np.unique(b)) > 10 and (b >> (8 * x.itemsize - 1)).min() == 0 and (b >> (8 * x.itemsize - 1)).max() == 1
            if kind == "high":
                assert x.min() >= 2 ** 63
