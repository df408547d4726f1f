"""CPU self-test of tests/softmax_cases.py: the bound of the softmax / log-sum-exp sweep is attainable (plain NumPy in
the working dtype, float64 accumulator, passes on every row and generator), every mutation a wrong kernel could produce
fails it wherever its effect is above twice the bound, the restated routes reach every kernel instance of
csrc/softmax.hip at least twice and every coverage condition of the table holds, and the staging magic of the
thread-per-row kernels is exact.  A checker that cannot fail is worth nothing: this is the test of that."""
import numpy as np
import pytest

import softmax_cases as sc

ERR = dict(all="ignore")


def np_eval(S, what, mut=None, geom=None):
    """``what`` of the (nslices, n) values in their own dtype, float64 sum, as a correct kernel forms it.  ``mut`` spoils
    slice 0 the way a wrong kernel would."""
    T = S.dtype.type
    with np.errstate(**ERR):
        x = S.copy()
        if mut == "next_row":
            x[0, -1] = S[1, -1]
        m = x.max(axis=1, keepdims=True)
        # (the log-sum-exp graph shifts by 0 where the max is infinite; Softmax / LogSoftmax subtract the max itself,
        # pytensor/tensor/special.py, so inf - inf = NaN reaches their sum)
        sh = np.where(np.isinf(m), T(0), m) if what == "lse" else m.copy()
        if mut == "shift_inf":
            sh = m.copy()
        e = np.exp(x - sh)
        s = e.sum(axis=1, keepdims=True, dtype=np.float64)
        if mut == "drop":
            s[0] -= e[0][e[0] > 0].min()
        elif mut == "twice":
            s[0] += e[0, 0]
        elif mut == "omit_split":
            s[0] -= e[0, geom[0]:geom[1]].sum(dtype=np.float64)
        elif mut == "pad":
            s[0] += np.nan
        sho = sh.copy()
        if mut == "nbr_max":
            sho[0] = sh[1]
        if what == "lse":
            return (np.log(s).astype(T) + sho)[:, 0]
        if what == "softmax":
            return (np.exp(x - sho) * (T(1) / s.astype(T))).astype(T)
        return ((x - sho) - np.log(s.astype(T))).astype(T)


def _params(cases):
    return [pytest.param(c, dt, id=f"{c.entry}-{c.name}-{dt}") for c in cases for dt in sc.dtypes_of(c)]


def _worst_route(case, dt, what):
    """(c_exp, levels) as the GPU test uses them, the smaller of the aligned and the misaligned route's: the stricter"""
    rs = [sc.route_of(case, dt, what, mis) for mis in ("aligned", "both")]
    return min(sc.c_exp_of(case, dt, r) for r in rs), min(sc.levels_of(case, dt, r) for r in rs)


@pytest.mark.parametrize("case,dt", _params(sc.ALL_CASES + sc.CHILD_CASES))
def test_numpy_passes_and_mutations_fail(case, dt):
    for gen in sc.GENS:
        S = sc.slices(case, dt, gen)
        # the whole operand, clean: only where it is cheap in long double; the first slices otherwise (a slice is independent
        # of the others and the checker is elementwise)
        Sc = S if S.size <= 300000 else S[:max(2, 300000 // S.shape[1])]
        st = sc.Stats(Sc)
        for what in sc.whats(case):
            c_exp, lv = _worst_route(case, dt, what)
            ex = sc.expect(st, what, dt, c_exp, lv)
            r = sc.check(np_eval(Sc, what), ex, dt, f"{case.name} {dt} {gen} {what}")
            assert r <= 1.0
    # mutations, on the generator made for them
    S = sc.slices(case, dt, "flat")
    if S.shape[0] < 2:
        S = np.concatenate([S, S[:1] * S.dtype.type(0.5)])
    S2 = S[:2]
    st = sc.Stats(S2)
    n = S2.shape[1]
    geom = None
    if case.entry == "cols":
        g = sc.col_geometry(dt, *case.shape, True)
        geom = (0, g.rows_per) if g.nsplit > 1 else None
    elif case.entry == "lse_rows":
        r = sc.lse_rows_route(dt, *case.shape, True)
        geom = (n - (n - 1) % (64 * r.V * sc.STREAM_U) - 1, n) if r.kernel == "stream" else None
    for what in sc.whats(case):
        c_exp, lv = _worst_route(case, dt, what)
        ex = sc.expect(st, what, dt, c_exp, lv)
        clean = np_eval(S2, what)
        for mut in ("drop", "twice", "next_row", "nbr_max", "omit_split", "pad"):
            if (mut == "omit_split" and geom is None) or (n == 1 and mut in ("drop", "next_row")):
                continue
            bad = np_eval(S2, what, mut, geom)
            with np.errstate(**ERR):
                effect = np.abs(bad.astype(ex.want.dtype) - clean.astype(ex.want.dtype))
                applies = bool(np.any(~(effect <= 2 * ex.bound)))
            # every mutation is above the resolution of the format on every row of the table, except a single exchanged
            # or dropped element of a float32 sum of thousands
            if np.dtype(dt) == np.float64 or n <= 1000 or mut in ("pad", "omit_split", "nbr_max"):
                assert applies, f"{case.name} {dt} {what}: mutation {mut} is below twice the bound: the generator does not expose it"
            if applies:
                with pytest.raises(AssertionError):
                    sc.check(bad, ex, dt, f"{mut}")


@pytest.mark.parametrize("case,dt", _params(sc.NONFINITE_CASES))
def test_nonfinite_rules(case, dt):
    S, planted = sc.plant_nonfinite(case, sc.slices(case, dt, "flat"))
    st = sc.Stats(S)
    for what in sc.whats(case):
        c_exp, lv = _worst_route(case, dt, what)
        ex = sc.expect(st, what, dt, c_exp, lv)
        got = np_eval(S, what)
        sc.check(got, ex, dt, f"{case.name} {what}")
        if what == "lse":
            assert got[1] == -np.inf and got[3] == np.inf and got[5] == np.inf and np.isnan(got[7]) and np.isfinite(got[8])
            bad = np_eval(S, what, "shift_inf")  # exp(x - inf): NaN where the rule says -inf / +inf
            with pytest.raises(AssertionError):
                sc.check(bad, ex, dt, "shift_inf")
        else:
            assert np.isnan(got[[1, 3, 5, 7]]).all() or what == "log_softmax"
            assert np.isfinite(got[8, 1]) and np.isfinite(got[0]).all()
        if what == "softmax":
            # the suspected column-kernel result: finite entries of a +inf slice come out 0 instead of NaN
            bad = got.copy()
            bad[3, 1:] = 0
            with pytest.raises(AssertionError):
                sc.check(bad, ex, dt, "zero for NaN")


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
def _runs(cases, child=False, **kw):
    """(case, dt, what, mis, route) of every run the GPU test makes of ``cases``: one of the three tables of the default
    process, numbered from 0 as tests/test_gpu_tiers_softmax.py ``_indexed`` does, or (``child``) cases of a switch,
    numbered by their place in ``CHILD_CASES`` as its ``_specs`` does"""
    assert child or cases in (sc.SOFTMAX_CASES, sc.LSE_ROWS_CASES, sc.COL_CASES)
    for i, c in enumerate(cases):
        if child:
            i = sc.CHILD_CASES.index(c)
        for dt in sc.dtypes_of(c):
            for what in sc.whats(c):
                for mis in ("aligned", sc.misalignment(c, i)):
                    yield c, dt, what, mis, sc.route_of(c, dt, what, mis, **kw)


def _default_runs():
    for table in (sc.SOFTMAX_CASES, sc.LSE_ROWS_CASES, sc.COL_CASES):
        yield from _runs(table)


def test_every_kernel_instance_is_reached_twice():
    seen = {}
    for c, dt, what, mis, r in _default_runs():
        t = sc.tier_name(c, dt, r, what)
        seen[t] = seen.get(t, 0) + 1
    want = []
    for dt in sc.DTYPES:
        VW = sc.vec_elems(dt)
        for log in ("", ", LOG"):
            want += [f"softmax_small<{dt}{log}, 16>", f"softmax_block<{dt}{log}>", f"softmax_wave<{dt}{log}>"]
            want += [f"softmax_wave_reg<{dt}{log}, {vpl}, {v}>" for vpl, v in ((2, VW), (8, VW), (16, VW), (4, 1), (16, 1), (32, 1))]
        want += [f"lse_rows_small<{dt}, {c}>" for c in (8, 16, 32)]
        want += [f"lse_rows_wave<{dt}, {vpl}, {v}>" for vpl, v in ((2, VW), (4, VW), (8, VW), (16, VW), (4, 1), (16, 1))]
        want += [f"lse_rows_stream<{dt}, V={v}>" for v in (1, VW)]
        want += [f"col_{w}<{dt}, V={v}, {t}>" for w in ("lse", "softmax", "log_softmax") for v in (1, VW) for t in ("one tile", "tiled")]
    missing = [t for t in want if seen.get(t, 0) < 2]
    assert not missing, f"instances reached fewer than twice: {missing}"
    assert set(seen) <= set(want), f"the restatement names an instance the file does not have: {set(seen) - set(want)}"


def _rows_conditions():
    cond = {}
    runs = list(_runs(sc.SOFTMAX_CASES))
    for dt in sc.DTYPES:
        VW = sc.vec_elems(dt)
        mine = [(c, what, mis, r) for c, d, what, mis, r in runs if d == dt]
        small = [(c, mis, r) for c, what, mis, r in mine if r.kernel == "small"]
        for vec in (0, 1):
            cond[f"softmax {dt} small, 16-byte staging {'on' if vec else 'off'}"] = any(r.V == vec for c, mis, r in small)
        cond[f"softmax {dt} small: the last workgroup's chunk is no whole number of packs, staging on"] = any(
            r.V == 1 and ((c.shape[0] % 256) * c.shape[1]) % VW for c, mis, r in small)
        for cols in (1, 2, 3, 15, 16):
            for rows in (1, 255, 256, 257, 513):
                cond[f"softmax {dt} small {rows}x{cols}"] = any(c.shape == (rows, cols) for c, mis, r in small)
        regs = [(c, r) for c, what, mis, r in mine if r.kernel == "reg"]
        for inst, lo, hi in (((2, VW), 16 + VW, 128 * VW), ((8, VW), 128 * VW + VW, 512 * VW), ((16, VW), 512 * VW + VW, 1024 * VW),
                             ((4, 1), 17, 256), ((16, 1), 257, 1024), ((32, 1), 1025, 2048)):
            got = {c.shape[1] for c, r in regs if (r.VPL, r.V) == inst}
            # (an unpacked instance takes an odd width, or an even one behind a misaligned pointer)
            cond[f"softmax {dt} reg{inst}: lower edge"] = bool(got & {lo, lo + 1}) if inst[1] == 1 else lo in got
            cond[f"softmax {dt} reg{inst}: upper edge"] = bool(got & {hi, hi - 1}) if inst[1] == 1 else hi in got
        for inst in ((2, VW), (4, 1)):
            rr = {c.shape[0] - r.nwaves for c, r in regs if (r.VPL, r.V) == inst}
            cond[f"softmax {dt} reg{inst}: rows 1, 5, nwaves + 1"] = {c.shape[0] for c, r in regs if (r.VPL, r.V) == inst} >= {1, 5, 3073} and 1 in rr
            cond[f"softmax {dt} reg{inst}: a third row"] = any(c.shape[0] > 2 * r.nwaves for c, r in regs if (r.VPL, r.V) == inst)
        wave = {c.shape for c, what, mis, r in mine if r.kernel == "wave"}
        cond[f"softmax {dt} wave"] = wave >= ({(5, 2049), (512, 4097)} | ({(5, 2050)} if VW == 2 else {(512, 4100)}))
        block = {c.shape for c, what, mis, r in mine if r.kernel == "block"}
        cond[f"softmax {dt} block"] = block >= {(r_, c_) for r_ in (1, 3, 511) for c_ in (4096, 4097)}
        kid = {(r.kernel, r.VPL, r.V) for c, d, what, mis, r in _runs(sc.SOFTMAX_CHILD_CASES, True, per_cu=1) if d == dt and c.shape[0] > 2 * r.nwaves and r.nwaves == 1024}
        cond[f"softmax {dt} child: a third row in reg(16, VW), reg(32, 1) and wave"] = kid >= {("reg", 16, VW), ("reg", 32, 1), ("wave", 0, 0)}
    runs = list(_runs(sc.LSE_ROWS_CASES))
    for dt in sc.DTYPES:
        VW = sc.vec_elems(dt)
        mine = [(c, mis, r) for c, d, what, mis, r in runs if d == dt]
        small = {c.shape for c, mis, r in mine if r.kernel == "small"}
        cond[f"lse {dt} small"] = small >= {(r_, c_) for c_ in (1, 8, 9, 16, 17, 24, 31, 32) for r_ in (1, 256, 257, 70001)}
        for inst, lo, hi in (((2, VW), 32 + VW, 128 * VW), ((4, VW), 128 * VW + VW, 256 * VW), ((8, VW), 256 * VW + VW, 512 * VW),
                             ((16, VW), 512 * VW + VW, 1024 * VW), ((4, 1), 33, 255), ((16, 1), 257, 1023)):
            got = {c.shape[1] for c, mis, r in mine if r.kernel == "wave" and (r.VPL, r.V) == inst}
            cond[f"lse {dt} wave{inst}: both edges"] = {lo, hi} <= got
        cond[f"lse {dt} wave: a second and a third row"] = any(r.kernel == "wave" and c.shape[0] == r.nwaves + 1 for c, mis, r in mine) and any(
            r.kernel == "wave" and c.shape[0] > 2 * r.nwaves for c, mis, r in mine)
        for V in (1, VW):
            st = [(c.shape, r) for c, mis, r in mine if r.kernel == "stream" and r.V == V]
            per = 64 * V * sc.STREAM_U
            cond[f"lse {dt} stream V={V}: G odd and even"] = {r.G % 2 for s, r in st} == {0, 1}
            cond[f"lse {dt} stream V={V}: exactly G visits"] = any(s[1] == r.G * per for s, r in st)
            cond[f"lse {dt} stream V={V}: one pack over"] = any(s[1] == (r.G - 1) * per + V and any(s2[1] == s[1] - V for s2, _ in st) for s, r in st)
            cond[f"lse {dt} stream V={V}: one lane of the last visit live"] = any(s[1] - (r.G - 1) * per <= V for s, r in st)
        kw = {(r.VPL, r.V) for c, d, what, mis, r in _runs(sc.LSE_WAVE_CHILD_CASES, True, wave_per_cu=1) if d == dt and r.kernel == "wave" and c.shape[0] > 2 * r.nwaves}
        cond[f"lse {dt} child: a third row in wave(16, 1) and a packed wave"] = (16, 1) in kw and any(v == VW for _, v in kw)
        ks = {(r.V, r.G % 2) for c, d, what, mis, r in _runs(sc.LSE_STREAM_CHILD_CASES, True, rows_per_cu=1) if d == dt and r.kernel == "stream" and c.shape[0] > 2 * r.nwaves}
        cond[f"lse {dt} child: stream rows from both buffers, V = 1 and VW"] = ks >= {(1, 0), (1, 1)} and any(v == VW for v, _ in ks)
    cond["lse float32 stream: more rows than the 8192 waves of the default grid"] = any(
        d == "float32" and r.kernel == "stream" and c.shape[0] > r.nwaves == 8192 and r.G % 2 for c, d, what, mis, r in runs)
    cond["lse float64 small: 24 columns are the first past 48 KB of LDS"] = sc.lse_small_lds("float64", 24) > 48 * 1024 >= sc.lse_small_lds("float64", 23)
    return cond


def _col_conditions():
    cond = {}
    for dt in sc.DTYPES:
        VW = sc.vec_elems(dt)
        runs = [(c, mis, g) for c, d, what, mis, g in _runs(sc.COL_CASES) if d == dt and what == "softmax"]
        one = [(c, mis, g) for c, mis, g in runs if g.ctiles == 1]
        many = [(c, mis, g) for c, mis, g in runs if g.ctiles > 1]
        cond[f"cols {dt}: TX divides 256"] = any(256 % g.TX == 0 and g.TX > 1 for c, mis, g in one)
        for cp in (5, 7, 100):
            cond[f"cols {dt}: TX = {cp}"] = any(g.TX == cp for c, mis, g in one)
        cond[f"cols {dt}: TY = 1"] = any(g.TY == 1 and 129 <= g.TX <= 256 for c, mis, g in one)
        cond[f"cols {dt}: one tile, V = VW"] = any(g.V == VW for c, mis, g in one)
        cond[f"cols {dt}: V = 1 through an odd C"] = any(g.V == 1 and c.shape[2] % VW for c, mis, g in runs)
        cond[f"cols {dt}: V = 1 through a misaligned pointer"] = any(g.V == 1 and c.shape[2] % VW == 0 and mis != "aligned" for c, mis, g in runs)
        cond[f"cols {dt}: tiles, a multiple of 64 packs"] = any((c.shape[2] // g.V) % 64 == 0 for c, mis, g in many)
        cond[f"cols {dt}: tiles, a partial last tile"] = any((c.shape[2] // g.V) % 64 for c, mis, g in many)
        cond[f"cols {dt}: tiles, V = 1 and V = VW"] = {g.V for c, mis, g in many} == {1, VW}
        cond[f"cols {dt}: R = 2"] = any(c.shape[1] == 2 for c, mis, g in runs)
        cond[f"cols {dt}: R < TY"] = any(c.shape[1] < g.TY for c, mis, g in runs)
        cond[f"cols {dt}: the last split is short"] = any(c.shape[1] % g.rows_per for c, mis, g in runs)
        cond[f"cols {dt}: the last split has fewer rows than TY"] = any(0 < c.shape[1] - (g.nsplit - 1) * g.rows_per < g.TY and g.nsplit > 1 for c, mis, g in runs)
        for v, U in ((1, 8), (VW, sc.col_visit_u(dt, VW))):
            par = {sc.ceil_div(sc.ceil_div(min(g.rows_per, c.shape[1]), g.TY), U) % 2 for c, mis, g in runs if g.V == v}
            cond[f"cols {dt} V={v}: a visit count ending in each buffer"] = par == {0, 1}
        cond[f"cols {dt}: nsplit = 1"] = any(g.nsplit == 1 for c, mis, g in runs)
        cond[f"cols {dt}: 2 <= nsplit <= L"] = any(2 <= g.nsplit <= g.L for c, mis, g in runs)
        cond[f"cols {dt}: nsplit > L"] = any(g.nsplit > g.L for c, mis, g in runs)
        cond[f"cols {dt}: L cut by the column count"] = any(g.L < 64 and g.L < g.nsplit for c, mis, g in runs)
        cond[f"cols {dt}: batch 1 and 3"] = {c.shape[0] for c, mis, g in runs} >= {1, 3}
        kid = [g for c, d, what, mis, g in _runs(sc.COL_CHILD_CASES, True, per_cu=8) if d == dt]
        cond[f"cols {dt} child: nsplit > 8 L"] = any(g.nsplit > 8 * g.L for g in kid)
    g = sc.col_geometry("float64", 1, 16400, 255, True, per_cu=8)
    cond["cols child: 16400 x 255 gives 1025 splits on 64 finish lanes"] = (g.nsplit, g.L) == (1025, 64)
    return cond


def test_the_table_meets_every_coverage_condition():
    cond = {**_rows_conditions(), **_col_conditions()}
    missed = [k for k, v in cond.items() if not v]
    assert not missed, "conditions the table misses:\n  " + "\n  ".join(missed)
    assert len(cond) > 150


def test_operands_stay_small():
    for c in sc.ALL_CASES + sc.CHILD_CASES + sc.NONFINITE_CASES + sc.DETERMINISM_CASES:
        for dt in sc.dtypes_of(c):
            assert int(np.prod(c.shape)) * np.dtype(dt).itemsize <= 70e6, c
    for c in sc.NONFINITE_CASES:
        assert c.nslices >= 12
    fam = {(c.entry, sc.route_of(c, "float64", sc.whats(c)[-1], "aligned")[0 if c.entry != "cols" else 3]) for c in sc.NONFINITE_CASES}
    assert fam >= {("softmax", "small"), ("softmax", "reg"), ("softmax", "wave"), ("softmax", "block"), ("lse_rows", "small"), ("lse_rows", "wave"),
                   ("lse_rows", "stream"), ("cols", 1)} and any(e == "cols" and t > 1 for e, t in fam)


def test_workspace_restatement_covers_both_pack_widths():
    for c in sc.COL_CASES:
        for dt in sc.DTYPES:
            for al in (True, False):
                g = sc.col_geometry(dt, *c.shape, al)
                b, R, Cc = c.shape
                assert sc.colstat_workspace(dt, *c.shape) >= (b * g.nsplit * Cc + b * Cc) * 16 + 256


def test_staging_magic_is_exact():
    """idx / cols as (idx * ceil(2^20 / cols)) >> 20 in 32-bit unsigned arithmetic, for every index of a 256-row chunk"""
    for cols in range(1, 33):
        idx = np.arange(256 * cols, dtype=np.uint64)
        magic = np.uint64(sc.staging_magic(cols))
        prod = idx * magic
        assert prod.max() < 2 ** 32  # no wrap in the kernel's unsigned multiply
        assert np.array_equal((prod & np.uint64(0xFFFFFFFF)) >> np.uint64(20), idx // np.uint64(cols)), cols
