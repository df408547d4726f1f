"""GPU: every kernel tier behind ``pthip_softmax`` / ``pthip_logsumexp_rows`` / ``pthip_logsumexp_cols`` /
``pthip_softmax_cols`` (csrc/softmax.hip) through the C ABI, against the high-precision reference and the derived bound of
tests/softmax_cases.py (no tuned factor; the worst ``|err| / bound`` per tier is printed, profiles/softmax_tiers.md).

Each row of the table is the smallest shape that reaches one kernel instance at one of its edges (tests/test_softmax_cases.py
proves the coverage on the CPU).  Every row runs in float64 and float32, with three generators (``flat``: every element
counts; ``ramp``: 800 / 110 units of dynamic range, underflow, ``-inf`` entries, the maximum last; ``shifted``), with aligned
pointers and with x, out or both one element behind a 16-byte boundary (another instance of the same shape), and the test
asserts the number of launches the call made.  Operands lie in NaN-padded parents and outputs between sentinels.

Non-finite slices (all ``-inf``, ``+inf`` first / last, NaN last, NaN in the element every clamped load re-reads, ``-inf``
inside a finite slice) are held to the stated rules per kernel family, with every other slice bit-identical to the call
without them.

The six ``PTHIP_*`` switches are read once into ``static const``s: ``test_switch`` runs the rows they affect in a fresh
child process per setting (tests/_softmax_tiers_worker.py), one at a time, each under its own timeout, and none after an
abnormal exit.  The three grid caps and the two staging knobs of the thread-per-row log-sum-exp cannot change a row's
arithmetic (a row is summed by the same lanes in the same order whichever wave or workgroup takes it): bit-identical to
the default process.  ``PTHIP_COL_WG_PER_CU`` changes the number of splits: bound only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import softmax_cases as sc
import _softmax_tiers_worker as dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}  # tier -> worst |err| / bound seen


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def _note(tier, ratio):
    WORST[tier] = max(WORST.get(tier, 0.0), ratio)


def _sweep(hip, case, index, dt):
    lines = []
    for gen in sc.GENS:
        x = sc.values(case, dt, gen)
        st = sc.Stats(x)
        exs = {}  # (the aligned and the misaligned route mostly share their constants: one expectation for both)
        for what in sc.whats(case):
            for mis in ("aligned", sc.misalignment(case, index)):
                r = sc.route_of(case, dt, what, mis)
                tier = sc.tier_name(case, dt, r, what)
                tag = f"{case.entry} {case.name} {dt} {gen} {what} {mis} [{tier}]"
                rc, got, launches = dev.run(hip, case, what, x, mis)
                hip.check(rc)
                assert launches == dev.expected_launches(case, what), f"{tag}: {launches} launches"
                key = (what, sc.c_exp_of(case, dt, r), sc.levels_of(case, dt, r))
                if key not in exs:
                    exs[key] = sc.expect(st, *key[:1], dt, *key[1:])
                ratio = sc.check(got, exs[key], dt, tag)
                _note(tier, ratio)
                lines.append(f"{tag}: worst |err|/bound = {ratio:.3g}")
    print("\n".join(lines))


def _indexed(cases):
    return [pytest.param(c, i, dt, id=f"{c.name}-{dt}") for i, c in enumerate(cases) for dt in sc.dtypes_of(c)]


@pytest.mark.parametrize("case,index,dt", _indexed(sc.SOFTMAX_CASES))
def test_softmax(hip, case, index, dt):
    _sweep(hip, case, index, dt)


@pytest.mark.parametrize("case,index,dt", _indexed(sc.LSE_ROWS_CASES))
def test_logsumexp_rows(hip, case, index, dt):
    _sweep(hip, case, index, dt)


@pytest.mark.parametrize("case,index,dt", _indexed(sc.COL_CASES))
def test_cols(hip, case, index, dt):
    _sweep(hip, case, index, dt)
    # the workspace: what the restated geometry needs, and one byte less is refused before anything is launched
    lib = hip.lib()
    wsb = int(lib.pthip_colstat_workspace(hip.np_dtype_code(dt), *case.shape))
    assert wsb == sc.colstat_workspace(dt, *case.shape)
    x = sc.values(case, dt, "flat")
    for what in ("lse", "softmax"):
        rc, _, launches = dev.run(hip, case, what, x, "aligned", ws_short=1)
        assert rc != 0 and launches == 0, (what, rc, launches)
        assert b"workspace too small" in lib.pthip_last_error()


@pytest.mark.parametrize("case,dt", [pytest.param(c, dt, id=f"{c.entry}-{c.name}-{dt}") for c in sc.NONFINITE_CASES for dt in sc.DTYPES])
def test_nonfinite(hip, case, dt):
    S = sc.slices(case, dt, "flat")
    P, planted = sc.plant_nonfinite(case, S)
    x, xp = sc.arrange(case, S), sc.arrange(case, P)
    st = sc.Stats(xp)
    keep = np.ones(case.nslices, bool)
    keep[list(planted)] = False

    def by_slice(a):  # slices first
        if case.entry != "cols":
            return a
        return np.moveaxis(a, 1, -1).reshape(case.nslices, -1) if a.ndim == 3 else a.reshape(case.nslices)

    for what in sc.whats(case):
        for mis in ("aligned", "x"):
            r = sc.route_of(case, dt, what, mis)
            tag = f"nonfinite {case.entry} {case.name} {dt} {what} {mis}"
            rc, clean, _ = dev.run(hip, case, what, x, mis)
            hip.check(rc)
            rc, got, _ = dev.run(hip, case, what, xp, mis)
            hip.check(rc)
            ex = sc.expect(st, what, dt, sc.c_exp_of(case, dt, r), sc.levels_of(case, dt, r))
            sc.check(got, ex, dt, tag)
            a, b = by_slice(got)[keep], by_slice(clean)[keep]
            assert np.array_equal(a, b), f"{tag}: a slice next to a planted one changed"


@pytest.mark.parametrize("case", sc.DETERMINISM_CASES, ids=lambda c: f"{c.entry}-{'x'.join(map(str, c.shape))}")
def test_two_runs_are_bit_equal(hip, case):
    for dt in sc.DTYPES:
        x = sc.values(case, dt, "flat")
        for what in sc.whats(case):
            a = dev.run(hip, case, what, x)[1]
            b = dev.run(hip, case, what, x)[1]
            assert a is not None and np.array_equal(a, b), f"{case.entry} {case.shape} {dt} {what}: two runs differ"


# ---------------------------------------------------------------------------------------------------------------
# the PTHIP_* switches: a fresh child process per setting
# ---------------------------------------------------------------------------------------------------------------
# (id, environment, cases, geometry of the restated route under the switch, bit-identical to the default process?)
SWITCHES = (
    ("softmax_wg1", {"PTHIP_SOFTMAX_WG_PER_CU": "1"}, sc.SOFTMAX_CHILD_CASES, {"per_cu": 1}, True),
    ("lse_wave_wg1", {"PTHIP_LSE_WAVE_WG_PER_CU": "1"}, sc.LSE_WAVE_CHILD_CASES, {"wave_per_cu": 1}, True),
    ("lse_rows_wg1", {"PTHIP_LSE_ROWS_WG_PER_CU": "1"}, sc.LSE_STREAM_CHILD_CASES, {"rows_per_cu": 1}, True),
    ("lse_small_vec1", {"PTHIP_LSE_SMALL_VEC": "1"}, sc.LSE_SMALL_CHILD_CASES, {}, True),
    ("lse_small_lds60k", {"PTHIP_LSE_SMALL_LDS_MIN": "61440"}, sc.LSE_SMALL_CHILD_CASES, {}, True),
    ("col_wg8", {"PTHIP_COL_WG_PER_CU": "8"}, sc.COL_CHILD_CASES, {"per_cu": 8}, False),
)


def _groups():
    """a child per switch, large case and dtype (their long-double references take seconds each); the small cases of a
    switch share one"""
    out = []
    for sid, env_add, cases, route_kw, biteq in SWITCHES:
        big = [c for c in cases if int(np.prod(c.shape)) >= 10 ** 6]
        small = tuple(c for c in cases if c not in big)
        for grp, dts in [((c,), (dt,)) for c in big for dt in sc.dtypes_of(c)] + ([(small, sc.DTYPES)] if small else []):
            name = f"{grp[0].name}-{dts[0]}" if len(grp) == 1 else "small"
            out.append(pytest.param((sid, env_add, grp, dts, route_kw, biteq), id=f"{sid}-{name}"))
    return out


_ABNORMAL = []


def _specs(cases, dts):
    out = []
    for c in cases:
        i = sc.CHILD_CASES.index(c)
        for dt in (d for d in sc.dtypes_of(c) if d in dts):
            for gen in sc.GENS:
                for mis in ("aligned", sc.misalignment(c, i)):
                    out += [dev.spec_of(c, dt, gen, mis, what) for what in sc.whats(c)]
    return out


@pytest.mark.parametrize("switch", _groups())
def test_switch(hip, tmp_path, switch):
    sid, env_add, cases, dts, route_kw, biteq = switch
    if _ABNORMAL:
        pytest.fail(f"not started: the child of {_ABNORMAL[0]} ended abnormally")
    assert all(k not in os.environ for k in env_add), "the switches under test must not be set for the suite itself"
    specs = _specs(cases, dts)
    out = str(tmp_path / "out.json")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_softmax_tiers_worker.py"), out, json.dumps(route_kw), *specs],
                           env=dict(os.environ, **env_add), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _ABNORMAL.append(sid)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _ABNORMAL.append(sid)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    by_name = {(c.entry, c.name): c for c in cases}
    last = [None, None]  # (the operand of the previous job: the jobs of a case are adjacent)
    for spec in specs:
        entry, name, dt, gen, mis, what = spec.split(":")
        case = by_name[entry, name]
        got = res[spec]
        assert got["ratio"] <= 1.0
        assert got["launches"] == dev.expected_launches(case, what), (sid, spec, got)
        _note(f"{got['tier']} under {sid}", got["ratio"])
        if biteq:
            if last[0] != (entry, name, dt, gen):
                last[:] = (entry, name, dt, gen), sc.values(case, dt, gen)
            rc, base, _ = dev.run(hip, case, what, last[1], mis)
            hip.check(rc)
            assert sc.digest(base) == got["digest"], f"{sid} {spec}: differs from the default process although a row's arithmetic is the same"
    print(f"{sid}: {len(specs)} runs, worst |err|/bound = {max(res[s]['ratio'] for s in specs):.3g}")


def test_generated_softmax_tile_agrees_on_an_infinite_column(hip, tmp_path):
    """``softmax(x, axis=0)`` on the generated N-d tile (``PTHIP_SOFTMAX_COLS=0``: dispatch/extra.py ``_softmax_any_axes``,
    ``exp(x - lse)``): a column with a ``+inf`` entry is all NaN as in the reference, and as on the column kernels"""
    if _ABNORMAL:
        pytest.fail(f"not started: the child of {_ABNORMAL[0]} ended abnormally")
    out = str(tmp_path / "graph.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_softmax_tiers_worker.py"), out, "graph"], env=dict(os.environ, PTHIP_SOFTMAX_COLS="0"),
                       capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _ABNORMAL.append("softmax_cols0")
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    seen = 0
    for dt in sc.DTYPES:
        clean, got = z[f"clean:{dt}"], z[f"planted:{dt}"]
        calls, declined = (int(v) for v in z[f"route:{dt}"])  # (running totals of the child)
        assert calls > seen and declined == 0, f"{dt}: the graph did not run on the generated tile ({calls - seen} calls, {declined} declined)"
        seen = calls
        assert np.isnan(got[:, 2]).all(), f"{dt}: the finite entries of a column with +inf: {got[:5, 2]}"
        assert np.isnan(got[:, 1]).all() and np.isnan(got[:, 3]).all()
        keep = [0, 5]
        assert np.array_equal(got[:, keep], clean[:, keep])
        np.testing.assert_allclose(clean.sum(axis=0), 1.0, rtol=0, atol=1e-5 if dt == "float32" else 1e-12)


def test_zz_report():
    """the worst ratio per tier of this run (the table of profiles/softmax_tiers.md)"""
    for tier in sorted(WORST):
        print(f"TIER {tier}: {WORST[tier]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
