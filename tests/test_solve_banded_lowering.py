"""CPU: ``solve(A, b, assume_a="banded")`` and its gradient lower whole under ``mode="hip"`` (no host node), the
lowered graph — run by the oracle — reproduces the reference's C linker, and ``dispatch/lu.py::banded_tier`` sends
n <= 64 to the dense one-launch tier and everything above to the band kernels (csrc/gbsv.hip)."""
import os
import re

import numpy as np
import pytest

import make_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_ref = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")


def banded_input(n, kl0, ku0, rng, batch=None):
    """A = 0.01 G mask(kl0, ku0) + diag(1 + U(0, 1)) with the row pairs (0, 1), (2, 3), ... swapped: every second
    pivot is a genuine interchange and the band widens to about (kl0 + 1, ku0 + 1)"""
    lead = () if batch is None else (batch,)
    i, j = np.indices((n, n))
    mask = (i - j <= kl0) & (j - i <= ku0)
    A = 0.01 * rng.standard_normal((*lead, n, n)) * mask + (1.0 + rng.random((*lead, n, 1))) * np.eye(n)
    perm = np.arange(n)
    perm[: n - n % 2] = perm[: n - n % 2].reshape(-1, 2)[:, ::-1].ravel()
    return A[..., perm, :]


def test_banded_tier_boundaries():
    from pytensor_amd.dispatch.lu import WAVE_MAX_N, banded_tier

    assert WAVE_MAX_N == 64
    for nb in (0, 1, 2, 100000):
        assert banded_tier(1, nb) == "wave" and banded_tier(63, nb) == "wave" and banded_tier(64, nb) == "wave"
        assert banded_tier(65, nb) == "band" and banded_tier(4096, nb) == "band"


def test_abi_declares_the_band_entry_points():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    for name in ("pthip_band_scan", "pthip_gbsv_workspace", "pthip_gbsv_batched"):
        assert name in ffi.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    # every band of a small matrix fits the LDS; the widest band of a large one does not: one dense slab per item
    lib = ffi.lib()
    assert lib.pthip_gbsv_workspace(ffi.np_dtype_code(np.dtype("float64")), 7, 64) == 0
    assert lib.pthip_gbsv_workspace(ffi.np_dtype_code(np.dtype("float64")), 7, 130) == 7 * 130 * 130 * 8
    assert lib.pthip_gbsv_workspace(ffi.np_dtype_code(np.dtype("float32")), 3, 1025) == 3 * 1025 * 1025 * 4


@pytest.fixture(scope="module")
def pt():
    make_ref.activate()
    import pytensor
    import pytensor.tensor as ptt

    import pytensor_amd

    pytensor_amd.register()
    return pytensor, ptt


def _nodes(f):
    return f.maker.linker.last_ir.nodes


def _banded_solves(nodes):
    out = []
    for n in nodes:
        if n.op == "Solve":
            out.append(("Solve", n.params["assume_a"]))
        elif n.op == "Blockwise" and n.params["core_op"] == "Solve":
            out.append(("Blockwise", n.params["core_params"]["assume_a"]))
    return out


@needs_ref
def test_banded_solve_lowers(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve

    A2, A3, b1, b2 = ptt.dmatrix("A"), ptt.dtensor3("A3"), ptt.dvector("b"), ptt.dmatrix("B")
    for ins, out, kind in [
        ([A2, b1], solve(A2, b1, assume_a="banded"), "Solve"),
        ([A2, b2], solve(A2, b2, assume_a="banded"), "Solve"),
        ([A3, b2], solve(A3, b2, assume_a="banded", b_ndim=1), "Blockwise"),
    ]:
        f = pytensor.function(ins, out, mode="hip")
        nodes = _nodes(f)
        assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
        assert _banded_solves(nodes) == [(kind, "banded")], [n.op for n in nodes]


@needs_ref
def test_banded_solve_gradient_lowers(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve

    for A, b, b_ndim in [(ptt.dmatrix("A"), ptt.dvector("b"), 1), (ptt.dtensor3("A"), ptt.dmatrix("b"), 1), (ptt.dmatrix("A"), ptt.dmatrix("b"), 2)]:
        cost = (solve(A, b, assume_a="banded", b_ndim=b_ndim) ** 2).sum()
        f = pytensor.function([A, b], pytensor.grad(cost, [A, b]), mode="hip")
        nodes = _nodes(f)
        assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
        solves = _banded_solves(nodes)
        # the solve and the pullback's solve on A.mT, both banded
        assert len(solves) >= 2 and all(a == "banded" for _, a in solves), solves


@needs_ref
def test_lowered_graph_matches_the_c_linker(pt):
    pytensor, ptt = pt
    import np_graph
    from pytensor.tensor.linalg import solve

    rng = np.random.default_rng(0)
    A2, A3, b1, b2 = ptt.dmatrix("A"), ptt.dtensor3("A3"), ptt.dvector("b"), ptt.dmatrix("B")
    x = solve(A2, b1, assume_a="banded")
    # (B is (4, n): the right-hand sides of the stack, and transposed the (n, 4) block of the unbatched solve)
    outs = [x, solve(A2, b2.T, assume_a="banded"), solve(A3, b2, assume_a="banded", b_ndim=1), *pytensor.grad((x**2).sum(), [A2, b1])]
    n = 9
    vals = {"A": banded_input(n, 2, 1, rng), "A3": banded_input(n, 1, 3, rng, batch=4), "b": rng.standard_normal(n), "B": rng.standard_normal((4, n))}
    ins = [A2, A3, b1, b2]
    f = pytensor.function(ins, outs, mode="hip")
    g = f.maker.linker.last_ir
    assert not any(nd.op == "HostPerform" for nd in g.nodes)
    want = pytensor.function(ins, outs, mode="CVM")(*[vals[i.name] for i in ins])
    got = np_graph.run_graph(g, [vals[i.name] for i in f.maker.fgraph.inputs])
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11, err_msg=f"output {k}")
