"""GPU: the software-pipelined row loop of ``gchain`` (csrc/gchain_device.h) against the plain loop it replaces.

Both forms run config #4's graph on the same inputs; the pipelined outputs must equal the plain ones bit for bit
(same add tree per row, same order of rows in the ``A.T@w`` accumulators and the bins, same lanes in the block combine),
both must meet the oracle at the bound of ``test_c4_group_counts_across_the_scatter_bin_limit`` (rtol 1e-11,
atol 2e-11 * scale), and a second call must repeat the first exactly.  Shapes are the smallest at which the loop takes
another path: group and half-group edges, waves without a group, one to three groups per wave, every kernel instance
(pack, chunks, rows per group, float32), the bin-count edges, the LDS gather table at and past its limit.

The dispatcher runs the pipelined loop only for the instances it was timed on (``fused._pipelined``); the other cases stay
here, where both settings of the switch then select the plain loop, so that they are in place when the set is widened.
"""
import numpy as np
import pytest

import np_graph
from util import load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def _inputs(N, K, G, dtype="float64"):
    from pytensor_amd import configs

    g, _, _, _, meta = load_case("c4_hier" if dtype == "float64" else "c4_hier_f32")
    vals = configs.c4_inputs(N=N, K=K, G=G)
    if dtype != "float64":
        vals = {k: (np.asarray(a, dtype=dtype) if np.asarray(a).dtype.kind == "f" else a) for k, a in vals.items()}
    return g, vals, meta["input_names"]


def _run(g, inputs, pipe, monkeypatch, calls=1):
    """Outputs of ``calls`` evaluations with the switch set, and the names of the gchain kernels that ran."""
    from pytensor_amd.dispatch import fused
    from pytensor_amd.executor import HipExecutable

    monkeypatch.setattr(fused, "PTHIP_GCHAIN_PIPE", pipe)
    exe = HipExecutable(g)
    outs = [exe(*inputs) for _ in range(calls)]
    exe.profile_nodes(inputs, reps=1)
    names = [k for k in exe.last_kernel_times if k.startswith("gchain_")]
    return outs, names


def _check(monkeypatch, N, K, G, dtype="float64", pipelined=True, gidx=None):
    g, vals, names = _inputs(N, K, G, dtype)
    if gidx is not None:
        vals["gidx"] = gidx(vals["gidx"])
    inputs = [vals[k] for k in names]
    (on, again), k_on = _run(g, inputs, True, monkeypatch, calls=2)
    (off,), k_off = _run(g, inputs, False, monkeypatch)
    assert len(k_on) == 1 and len(k_off) == 1, (k_on, k_off)
    assert ("_pipe" in k_on[0]) == pipelined, k_on
    assert "_pipe" not in k_off[0], k_off
    want = np_graph.run_graph(g, inputs)
    for k, (a, a2, b, w) in enumerate(zip(on, again, off, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"out{k}: pipelined vs plain loop")
        np.testing.assert_array_equal(a, a2, err_msg=f"out{k}: second call")
        scale = max(1.0, float(np.max(np.abs(w))))
        if dtype == "float64":
            rtol, atol = 1e-11, 2e-11 * scale
        else:
            # A float32 graph against its float32 NumPy evaluation.  The float64 bound cannot hold: every output is a sum
            # of up to N float32 terms, formed in another order on either side, and a float32 sum of N terms is off by up
            # to N * u * sum|term| (u = 2^-24) whatever the order.  The bound keeps the shape of the one above — rtol r,
            # atol 2 r * scale, the 2 for the two sides — with r = N * u (2.4e-5 at N = 401; the golden case of this graph,
            # 3000 terms, is held to 2e-4).  One row of 401 dropped or doubled moves a sum by about 1/401 of it, a
            # hundred times this.
            r = N * 2.0**-24
            rtol, atol = r, 2 * r * scale
        err = float(np.max(np.abs(np.asarray(a, dtype="float64") - np.asarray(w, dtype="float64"))))
        print(f"N={N} K={K} G={G} {dtype} out{k}: max|err| {err:.3e} scale {scale:.3e}")
        np.testing.assert_allclose(a, w, rtol=rtol, atol=atol, err_msg=f"out{k}: pipelined vs oracle")
        np.testing.assert_allclose(b, w, rtol=rtol, atol=atol, err_msg=f"out{k}: plain loop vs oracle")


@pytest.mark.parametrize("N", [1, 15, 16, 17, 31, 32, 33, 129])
def test_group_and_half_group_edges(hip, monkeypatch, N):
    """N = 33: one workgroup whose waves 2 and 3 own no group; N <= 16: a second half that holds no row."""
    _check(monkeypatch, N, 128, 128)


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_groups_per_wave(hip, monkeypatch, groups):
    """One workgroup: every wave walks ``groups`` groups (wave 0 one more, of 5 rows) — the last group, odd and even
    trip counts of the two-stage loop, a half whose successor is the first half of the next group."""
    from pytensor_amd.dispatch import fused

    monkeypatch.setattr(fused, "CHAIN_GRID", 1)
    _check(monkeypatch, 32 * 4 * groups + 5, 128, 128)


@pytest.mark.parametrize(
    "K,dtype,pipelined",
    [
        (2, "float64", True),  # one pack: most lanes hold nothing
        (64, "float64", True),
        (127, "float64", False),  # pack 1: measured no gain, plain loop
        (256, "float64", False),  # C = 2, RG = 16: measured no gain, plain loop
        (1024, "float64", False),  # C = 8, RG = 4: two half buffers do not fit two waves per SIMD
        (2048, "float64", False),  # RG = 2, multiplier in LDS
        (128, "float32", False),  # the four-column pack: not timed, plain loop
    ],
)
def test_instances(hip, monkeypatch, K, dtype, pipelined):
    _check(monkeypatch, 401, K, 128, dtype, pipelined)


@pytest.mark.parametrize("G", [1, 63, 64, 65, 256, 300])
def test_bin_counts(hip, monkeypatch, G):
    """Bins in one, two and four accumulator registers; G = 300 stores the scattered output (late scatter).  Two bin
    groups (65 .. 128 bins) is the form that was timed and runs pipelined."""
    _check(monkeypatch, 401, 128, G, pipelined=(G == 65))


def test_gather_table_at_and_past_the_lds_limit(hip, monkeypatch):
    from pytensor_amd.dispatch import fused

    # (config #4's table has one entry per bin, so one entry past the limit is also a third bin group)
    _check(monkeypatch, 401, 128, fused.GATHER_LDS_ENTRIES, pipelined=True)
    _check(monkeypatch, 401, 128, fused.GATHER_LDS_ENTRIES + 1, pipelined=False)


def test_negative_index_wraps(hip, monkeypatch):
    def wrap(gidx):
        gidx = gidx.copy()
        gidx[[0, 17, 400]] = -1
        return gidx

    _check(monkeypatch, 401, 128, 128, gidx=wrap)


@pytest.mark.parametrize("pipe", [True, False])
def test_index_past_the_table_is_index_error(hip, monkeypatch, pipe):
    from pytensor_amd.dispatch import fused
    from pytensor_amd.executor import HipExecutable

    g, vals, names = _inputs(401, 128, 128)
    good = [vals[k] for k in names]
    bad_idx = vals["gidx"].copy()
    bad_idx[200] = 128
    bad = [bad_idx if k == "gidx" else vals[k] for k in names]
    monkeypatch.setattr(fused, "PTHIP_GCHAIN_PIPE", pipe)
    exe = HipExecutable(g)
    first = exe(*good)
    with pytest.raises(IndexError):
        exe(*bad)
    for a, b in zip(exe(*good), first):  # the flag was cleared: the next valid call is clean
        np.testing.assert_array_equal(a, b)
