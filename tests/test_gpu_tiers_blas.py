"""GPU: every kernel variant behind ``pthip_gemm`` / ``pthip_gemm_partials`` / ``pthip_gemv`` / ``pthip_gemv_finish`` /
``pthip_ger`` / ``pthip_imatmul`` through the C ABI, against the high-precision reference and the derived bound of
tests/blas_cases.py (no tuned factor: ``|err| <= (K + 4) u (|alpha| |A||B| + |beta| |C|)``).

Each row of the table is the smallest shape that reaches one branch of the dispatch in csrc/gemm.hip (fp64 128-tile,
64-tile, skinny, split-K + finish; fp32 32-deep K tile, persistent, 256 x 256), and the test asserts the route from what the
library itself reports: ``pthip_gemm_nslabs`` and the difference of ``pthip_launch_count`` around the call.  Every row runs
in the four operand orientations, aligned and misaligned (pointer off by one element, odd pitch: the scalar staging path),
with shared and odd batch strides, a full / broadcast-row / broadcast-column C, ``beta == 0`` with a NaN C that must not
be read, and twice for run-to-run bit equality.  Operands are views into NaN-padded parents and outputs sit between
sentinels, so a read or a write out of range fails the case.

The ``PTHIP_*`` A/B switches are read once into ``static const``s: ``test_switch`` runs the rows they affect in a fresh
child process (tests/_blas_tiers_worker.py) per setting and holds the child's raw outputs to the same checker; where the
switch only re-tiles the work without changing an element's summation order, and that sum is carried by MFMA instructions
(decided from the code, stated per switch in ``SWITCHES``), the outputs must also be bit-identical to the default's.  Not
included: ``PTHIP_SGEMM_DIAG`` (its results are invalid by design) and ``PTHIP_SIDE_GEMM_*`` (they act only on a product
enqueued on a side stream of a Scan plan).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import blas_cases as bc
import _blas_tiers_worker as dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

PTR_OFF = dict(ptr=1, pitch="aligned", bstride="aligned")
ODD_PITCH = dict(ptr=0, pitch="odd", bstride="aligned")
ODD_BATCH = dict(ptr=0, pitch="aligned", bstride="odd")
LAYOUTS = {"aligned": (bc.ALIGNED, bc.ALIGNED), "a_ptr_b_pitch": (PTR_OFF, ODD_PITCH), "a_pitch_b_ptr": (ODD_PITCH, PTR_OFF)}
ORIENT = ((False, False), (False, True), (True, False), (True, True))


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


_DATA = {}


def gemm_data(name, dt):
    """operand values and high-precision products of a (row, dtype): computed once, shared, never modified"""
    if (name, dt) not in _DATA:
        _DATA[name, dt] = bc.GemmData(bc.GEMM_BY_NAME[name], dt)
    return _DATA[name, dt]


def _expected_launches(row, dt):
    return 2 if row.branch(dt) in bc.SPLIT_BRANCHES else 1


# ---------------------------------------------------------------------------------------------------------------
# pthip_gemm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", bc.DTYPES)
@pytest.mark.parametrize("row", bc.GEMM_ROWS, ids=lambda r: r.name)
def test_gemm_row(hip, row, dt):
    d = gemm_data(row.name, dt)
    shape = row.shape
    nb, M, N, K = shape
    want_launches = _expected_launches(row, dt)
    # the route the library reports
    nslabs = int(hip.lib().pthip_gemm_nslabs(*shape))
    assert nslabs == bc.split_plan(*shape)[0]
    assert (nslabs > 1) == (row.branch(dt) in bc.SPLIT_BRANCHES or row.name == "t64_for_split")
    worst = 0.0

    def run(tag, alpha, beta, opA, opB, opC=None, Cv=None, share_a=False, share_b=False):
        nonlocal worst
        got, launches = dev.run_gemm(hip, dt, shape, alpha, opA, opB, beta, opC)
        assert launches == want_launches, f"{row.name} {dt} {tag}: {launches} launches, the table says {want_launches} ({row.branch(dt)})"
        want, bound = d.expect(alpha, beta, Cv, share_a, share_b)
        worst = max(worst, bc.check(got, want, bound, dt, f"{row.name} {dt} {tag}"))
        return got

    # four orientations x (aligned, misaligned pointer / odd pitch)
    for tA, tB in ORIENT:
        for lname, (la, lb) in LAYOUTS.items():
            run(f"A{'T' if tA else 'N'}B{'T' if tB else 'N'} {lname}", 1.0, 0.0, bc.embed(d.A, trans=tA, **la), bc.embed(d.B, trans=tB, **lb))
    al = lambda v, **kw: bc.embed(v, **{**bc.ALIGNED, **kw})  # noqa: E731
    # alpha, beta and a full C (row-major, then a transposed view with an odd pitch)
    run("full C", bc.ALPHA, bc.BETA, al(d.A), al(d.B), al(d.C), d.C)
    run("full C^T", bc.ALPHA, bc.BETA, al(d.A, trans=True), al(d.B), bc.embed(d.C, trans=True, **ODD_PITCH), d.C)
    # broadcast row / column as C
    run("row C", bc.ALPHA, bc.BETA, al(d.A), al(d.B, trans=True), al(d.C[:, :1, :], bcast="row"), d.C[:, :1, :])
    run("col C", bc.ALPHA, bc.BETA, al(d.A, trans=True), al(d.B, trans=True), al(d.C[:, :, :1], bcast="col"), d.C[:, :, :1])
    # beta == 0: C is not read (pthip.h), so a C full of NaN must not show
    run("beta=0, NaN C", bc.ALPHA, 0.0, al(d.A), al(d.B), al(np.full_like(d.C, np.nan)), None)
    # run to run
    a = run("repeat 1", bc.ALPHA, bc.BETA, al(d.A, trans=True), al(d.B), al(d.C), d.C)
    b = run("repeat 2", bc.ALPHA, bc.BETA, al(d.A, trans=True), al(d.B), al(d.C), d.C)
    assert np.array_equal(a, b), f"{row.name} {dt}: two runs differ"
    if nb > 1:
        # batch stride 0 (a shared operand) on A, on B and on C; an odd batch stride
        zero = dict(ptr=0, pitch="aligned", bstride="zero")
        if nb <= 16:
            run("shared A", 1.0, 0.0, bc.embed(d.A[:1], **zero), al(d.B), share_a=True)
            run("shared B", 1.0, 0.0, al(d.A), bc.embed(d.B[:1], trans=True, **zero), share_b=True)
        else:  # (one call: the reference of a shared operand costs a full product, these rows have hundreds of items)
            run("shared A and B", 1.0, 0.0, bc.embed(d.A[:1], **zero), bc.embed(d.B[:1], trans=True, **zero), share_a=True, share_b=True)
        run("shared C", bc.ALPHA, bc.BETA, al(d.A), al(d.B), bc.embed(d.C[:1], **zero), d.C[:1])
        run("odd batch stride", bc.ALPHA, bc.BETA, bc.embed(d.A, **ODD_BATCH), bc.embed(d.B, trans=True, **ODD_BATCH), bc.embed(d.C, **ODD_BATCH), d.C)
    print(f"gemm {row.name} {dt} [{row.branch(dt)}]: worst |err|/bound = {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------
# pthip_gemm_partials
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", bc.DTYPES)
@pytest.mark.parametrize("name", bc.PARTIALS_ROWS)
def test_gemm_partials(hip, name, dt):
    row = bc.GEMM_BY_NAME[name]
    d = gemm_data(name, dt)
    shape = row.shape
    ns = int(hip.lib().pthip_gemm_nslabs(*shape))
    assert (ns > 1) == (name != "plain")
    want, bound = d.expect(1.0, 0.0)
    for tag, tA, tB, la, lb in (("aligned", False, False, bc.ALIGNED, bc.ALIGNED), ("misaligned", True, True, PTR_OFF, ODD_PITCH)):
        opA, opB = bc.embed(d.A, trans=tA, **la), bc.embed(d.B, trans=tB, **lb)
        rc, part, launches = dev.run_partials(hip, dt, shape, opA, opB, ns)
        assert rc == 0 and launches == 1, (rc, launches)
        acc = dev.sum_slabs(part)
        r = bc.check(acc, want, bound, dt, f"partials {name} {dt} {tag}")
        whole, wl = dev.run_gemm(hip, dt, shape, 1.0, opA, opB)
        if wl == 2:  # the same slabs, finished by splitk_finish_kernel in the same order
            assert np.array_equal(acc, whole), f"partials {name} {dt} {tag}: the slabs do not add up to pthip_gemm's result"
        else:
            assert ns == 1 or row.branch(dt) == "t64"
            if ns == 1:
                assert np.array_equal(acc, whole)
        print(f"partials {name} {dt} {tag}: {ns} slabs, worst |err|/bound = {r:.3g}")
    # a wrong slab count is refused with an error, not a launch
    for wrong in (ns + 1, ns - 1, 0):
        rc, _, launches = dev.run_partials(hip, dt, shape, opA, opB, wrong)
        assert rc != 0 and launches == 0, (wrong, rc, launches)
        assert b"slab count" in hip.lib().pthip_last_error()


# ---------------------------------------------------------------------------------------------------------------
# pthip_gemv
# ---------------------------------------------------------------------------------------------------------------
# (a case whose threshold is in bytes runs in one dtype; the other has a case of its own)
@pytest.mark.parametrize("case,dt", [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in bc.GEMV_CASES for dt in bc.DTYPES if c.only in ("", dt)])
def test_gemv(hip, case, dt):
    d = bc.gemv_data(case, dt)
    worst = 0.0
    for tag, alpha, beta, ymode, sy in (("y NULL", 1.0, 0.0, "null", 1), ("NaN y", bc.ALPHA, 0.0, "nan", 1), ("y", bc.ALPHA, bc.BETA, "vals", 1),
                                        ("sy=2", bc.ALPHA, bc.BETA, "vals", 2), ("sy=-1", 1.0, -bc.BETA, "vals", -1)):
        got, launches = dev.run_gemv(hip, d, alpha, beta, ymode, sy)
        assert launches == case.launches, f"gemv {case.name} {dt} {tag}: {launches} launches, the table says {case.launches}"
        want, bound = bc.gemv_expect(d.A, d.x, alpha, beta, d.y, dt)
        worst = max(worst, bc.check(got, want, bound, dt, f"gemv {case.name} {dt} {tag}"))
        if tag == "y":
            again, _ = dev.run_gemv(hip, d, alpha, beta, ymode, sy)
            assert np.array_equal(got, again), f"gemv {case.name} {dt}: two runs differ"
    wsb = int(hip.lib().pthip_gemv_workspace(hip.np_dtype_code(dt), case.M, case.N, d.sA0, d.sA1))
    assert (wsb > 0) == (case.kind == "col")
    print(f"gemv {case.name} {dt}: worst |err|/bound = {worst:.3g}, workspace {wsb} bytes")


@pytest.mark.parametrize("dt", bc.DTYPES)
def test_gemv_finish(hip, dt):
    rng = np.random.default_rng(11)
    for M in (7, 130, 1):
        for nparts in (1, 3, 64, 65, 300):
            part = rng.standard_normal((nparts, M)).astype(dt)
            y = rng.standard_normal(M).astype(dt)
            for alpha, beta, yv, sy in ((1.0, 0.0, None, 1), (bc.ALPHA, 0.0, np.full(M, np.nan, dt), 1), (bc.ALPHA, bc.BETA, y, 1), (bc.ALPHA, bc.BETA, y, -1),
                                        (1.0, -bc.BETA, y, 2)):
                got, launches = dev.run_finish(hip, dt, part, alpha, beta, yv, sy)
                assert launches == 1
                want, bound = bc.finish_expect(part, alpha, beta, y, dt)
                bc.check(got, want, bound, dt, f"gemv_finish M={M} nparts={nparts} alpha={alpha} beta={beta} sy={sy}")


@pytest.mark.parametrize("dt", bc.DTYPES)
def test_ger(hip, dt):
    rng = np.random.default_rng(13)
    for M, N in ((7, 45), (1, 1), (701, 800)):  # M * N no multiple of 256; the last needs the grid-stride loop
        A = rng.standard_normal((1, M, N)).astype(dt)
        x, y = rng.standard_normal(M).astype(dt), rng.standard_normal(N).astype(dt)
        want, bound = bc.ger_expect(A[0], x, y, bc.ALPHA, dt)
        for tag, op, sx, sy in (("row-major", bc.embed(A, **bc.ALIGNED), 1, 1), ("transposed, odd pitch", bc.embed(A, trans=True, **ODD_PITCH), -1, 2),
                                ("off by one", bc.embed(A, **PTR_OFF), 3, -1), ("transposed", bc.embed(A, trans=True, **bc.ALIGNED), -2, -3)):
            got, launches = dev.run_ger(hip, dt, op, x, sx, y, sy, bc.ALPHA)
            assert launches == 1
            bc.check(got, want, bound, dt, f"ger {M}x{N} {tag}")
    # A strided in both dimensions: A = P[::2, ::3]
    M, N = 9, 70
    A = rng.standard_normal((M, N)).astype(dt)
    x, y = rng.standard_normal(M).astype(dt), rng.standard_normal(N).astype(dt)
    parent = np.full((2 * M, 3 * N + 1), np.nan, dt)
    parent[::2, :3 * N:3] = A
    op = bc.Operand(parent.reshape(-1), 0, 0, 2 * (3 * N + 1), 3, (1, M, N))
    got, _ = dev.run_ger(hip, dt, op, x, 1, y, 1, bc.ALPHA)
    want, bound = bc.ger_expect(A, x, y, bc.ALPHA, dt)
    bc.check(got, want, bound, dt, "ger strided")


@pytest.mark.parametrize("dt", ["int8", "uint8", "int16", "int32", "int64", "uint64"])
def test_imatmul_wraps_like_numpy(hip, dt):
    """bit-exact against np.dot's wrap-around arithmetic; the products overflow every width"""
    rng = np.random.default_rng(17)
    info = np.iinfo(dt)
    M, N, K = 37, 21, 300
    A = rng.integers(info.min, info.max, size=(M, K), dtype=dt, endpoint=True)
    B = rng.integers(info.min, info.max, size=(K, N), dtype=dt, endpoint=True)
    want = (A.astype(np.uint64) @ B.astype(np.uint64)).astype(dt)  # modulo 2^64, then truncated: modulo 2^width
    if np.dtype(dt).itemsize < 8:
        assert np.array_equal(want, np.dot(A, B))
    lib = hip.lib()
    for tA, tB in ORIENT:
        Ah = np.ascontiguousarray(A.T) if tA else A
        Bh = np.ascontiguousarray(B.T) if tB else B
        dA, pA = dev.upload(Ah.reshape(-1), 0)
        dB, pB = dev.upload(Bh.reshape(-1), 0)
        sA = (1, M) if tA else (K, 1)
        sB = (1, K) if tB else (N, 1)
        out = dev.Out(M * N, dt)
        before = lib.pthip_launch_count()
        hip.check(lib.pthip_imatmul(hip.np_dtype_code(dt), M, N, K, pA, sA[0], sA[1], pB, sB[0], sB[1], out.ptr))
        assert lib.pthip_launch_count() - before == 1
        assert np.array_equal(out.fetch((M, N)), want), (dt, tA, tB)


# ---------------------------------------------------------------------------------------------------------------
# the PTHIP_* A/B switches: a fresh child process per setting
# ---------------------------------------------------------------------------------------------------------------
def _g(names, dts=bc.DTYPES, kind="gemm"):
    return tuple(f"{kind}:{n}:{dt}" for n in names.split() for dt in dts)


F32, F64 = ("float32",), ("float64",)
GEMV_ROW_JOBS = _g("row_vec_xlds row_vec_direct row_scalar_xlds row_scalar_direct row_sx2 row_sx_neg row_4rows_6 row_4rows_7 row_4rows_8 row_n0 row_m1",
                   kind="gemv")
# (id, environment, jobs, jobs whose output must equal the default's bit for bit, launches expected in the child or None)
SWITCHES = (
    # (Bit equality is asserted only where the sum is carried by MFMA instructions, which leave the compiler no choice of
    # rounding, and the epilogue is the same two statements.)
    # sgemm_kernel<.., 16> instead of <.., 32> / the persistent kernel: every kernel walks k in groups of 4 in the same
    # MFMA sequence per element (k, k+2 | k+1, k+3), zero padding adds +0, and the split plan does not depend on the tile
    # depth: bit-identical.  Not asserted for the 256 x 256 row (a separate kernel with its own epilogue expression).
    ("sgemm_bk16", {"PTHIP_SGEMM_BK": "16"}, _g("plain split split_ragged remap_on persistent persistent_k33 persistent_k17 persistent_interior s256", F32),
     _g("plain split split_ragged remap_on persistent persistent_k33 persistent_k17 persistent_interior", F32), None),
    # one tile per workgroup instead of the persistent walk: same MFMA sequence, same epilogue statements
    ("sgemm_persist0", {"PTHIP_SGEMM_PERSIST": "0"}, _g("persistent persistent_k33 persistent_k17 persistent_interior remap_on", F32),
     _g("persistent persistent_k33 persistent_k17 persistent_interior remap_on", F32), 1),
    # 128 x 128 tiles instead of 256 x 256: same k order, but the epilogues are different expressions (`alpha*acc + beta*C`
    # in one statement there, two here) that the compiler may contract differently: bound only
    ("sgemm_256_0", {"PTHIP_SGEMM_256": "0"}, _g("s256", F32), (), 1),
    # the 256 x 256 kernel without the fragment prefetch: the same template, the same MFMA sequence and epilogue
    ("sgemm_256_pf0", {"PTHIP_SGEMM_256_PF": "0"}, _g("s256", F32), _g("s256", F32), 1),
    # fp64 without 64 x 64 tiles: the 128-tile instance of the same template sums k in the same order where the plan has
    # no slabs; `t64_for_split` becomes split-K + finish (another order: bound only)
    ("dgemm_t64_0", {"PTHIP_DGEMM_T64": "0"}, _g("t64_batched t64_square t64_for_split plain", F64), _g("t64_batched t64_square plain", F64), None),
    # the long-operand kernels off: the MFMA kernels sum in another order: bound only
    ("gemm_skinny0", {"PTHIP_GEMM_SKINNY": "0"}, _g("long_fwd long_bwd", kind="long"), (), None),
    # other slab counts: another order: bound only (pthip_gemm_nslabs must agree with what pthip_gemm_partials accepts)
    ("maxsplit2", {"PTHIP_GEMM_MAXSPLIT": "2"}, _g("skinny_split_ragged skinny_split_52 split split_ragged t64_for_split skinny_long"), (), None),
    ("mink16_wgs1024", {"PTHIP_GEMM_MINK": "16", "PTHIP_GEMM_WGS": "1024"}, _g("skinny_split_ragged skinny_split_52 skinny_split_m1 split plain skinny_long"),
     (), None),
    # Gemv knobs: x through the caches / through LDS, and the rows in flight per wave.  Each lane walks the row in the same
    # order under every setting, but the dot product is plain C++ (`acc += a * x`) in a separately compiled instantiation
    # per setting, and whether each multiply-add is fused is the compiler's choice per instantiation (measured: ROWS=1 and
    # ROWS=4 differ in the last bit for float32 (16387, 8)): bound only
    ("gemv_xlds0", {"PTHIP_GEMV_XLDS": "0"}, GEMV_ROW_JOBS, (), 1),
    ("gemv_xlds1", {"PTHIP_GEMV_XLDS": "1"}, GEMV_ROW_JOBS, (), 1),
    ("gemv_rows1", {"PTHIP_GEMV_ROWS": "1"}, GEMV_ROW_JOBS, (), 1),
    ("gemv_rows2", {"PTHIP_GEMV_ROWS": "2"}, GEMV_ROW_JOBS, (), 1),
    ("gemv_rows4", {"PTHIP_GEMV_ROWS": "4"}, GEMV_ROW_JOBS, (), 1),
)
# what the changed plans must report in the child (Python restatement of split_plan with the switch's values)
PLAN_ARGS = {"maxsplit2": dict(cap=2), "mink16_wgs1024": dict(mink=16, wgs=1024)}

_DEFAULT = {}


def _default(hip, spec):
    """the same job in this process (no switch set), run once per session"""
    if spec not in _DEFAULT:
        _DEFAULT[spec] = dev.job(hip, spec)
    return _DEFAULT[spec]


def _job_expect(spec):
    kind, name, dt = spec.split(":")
    if kind == "gemv":
        d = bc.gemv_data(bc.GEMV_BY_NAME[name], dt)
        return bc.gemv_expect(d.A, d.x, bc.ALPHA, bc.BETA, d.y, dt)
    if kind == "long":
        key = ("long", name, dt)
        if key not in _DATA:
            _DATA[key] = bc.GemmData(dev.long_row(name)[0], dt)
        d = _DATA[key]
    else:
        d = gemm_data(name, dt)
    return d.expect(bc.ALPHA, bc.BETA, d.C), d.expect(1.0, 0.0)


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s[0])
def test_switch(hip, tmp_path, switch):
    sid, env_add, jobs, biteq, child_launches = switch
    assert all(k not in os.environ for k in env_add), "the switches under test must not be set for the suite itself"
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_blas_tiers_worker.py"), out, *jobs], env=dict(os.environ, **env_add),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    for spec in jobs:
        kind, name, dt = spec.split(":")
        got, route = z[spec], z[spec + ":route"]
        if kind == "gemv":
            want, bound = _job_expect(spec)
        else:
            (want, bound), (pwant, pbound) = _job_expect(spec)
        ratio = bc.check(got, want, bound, dt, f"{sid} {spec}")
        base = _default(hip, spec)
        if child_launches is not None:
            assert route[1] == child_launches, (sid, spec, route)
        if kind == "gemm":
            row = bc.GEMM_BY_NAME[name]
            plan = bc.split_plan(*row.shape, **PLAN_ARGS.get(sid, {}))[0]
            assert route[0] == plan, f"{sid} {spec}: pthip_gemm_nslabs {route[0]}, the plan restated gives {plan}"
            if row.K > 0:
                assert route[2] == 1, f"{sid} {spec}: pthip_gemm_partials does not accept pthip_gemm_nslabs' count (or accepts another)"
                bc.check(z[spec + ":psum"], pwant, pbound, dt, f"{sid} {spec} partials")
            if sid in PLAN_ARGS and plan > 1 and row.branch(dt) in bc.SPLIT_BRANCHES:
                assert route[1] == 2, (sid, spec, route)
            if sid == "dgemm_t64_0":
                assert route[1] == (2 if plan > 1 else 1), (sid, spec, route)
            if sid == "sgemm_bk16":
                assert route[1] == (2 if plan > 1 else 1), (sid, spec, route)
        if kind == "long":
            # in this process csrc/gemm_skinny.hip takes the product in one launch (forward) or slabs + finish (backward)
            assert base[spec + ":route"][1] in (1, 2)
            bc.check(base[spec], want, bound, dt, f"default {spec}")
        if spec in biteq:
            assert np.array_equal(got, base[spec]), f"{sid} {spec}: differs from the default although the summation order is the same"
        print(f"{sid} {spec}: route {route.tolist()}, worst |err|/bound = {ratio:.3g}")
