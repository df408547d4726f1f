"""CPU: the batched general solve / inverse tiers (``dispatch/lu.py::solve_tier``), their C ABI, and the graphs
that use them under ``mode="hip"`` — ``solve`` and ``inv`` of a stack and the batched generalised ``eigh`` lower with
no host fallback."""
import os
import re

import numpy as np
import pytest

import make_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_ref = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")


def test_solve_tier_boundaries():
    from pytensor_amd.dispatch.lu import WAVE_MAX_N, solve_tier

    assert WAVE_MAX_N == 64
    for nb in (1, 2, 100000):
        assert solve_tier(1, nb) == "wave" and solve_tier(64, nb) == "wave"
    assert solve_tier(65, 2) == "composed" and solve_tier(4096, 257) == "composed"
    assert solve_tier(65, 1) == "loop" and solve_tier(65, 0) == "loop"


def test_batch_dims_fold_into_one_stride_per_operand():
    from pytensor_amd.dispatch.lu import _collapse_batch

    n2 = 16
    # a contiguous stack against a contiguous stack: one launch
    assert _collapse_batch((5, 7), (7 * n2, n2), (7 * 4, 4)) == ([], 35, [n2, 4])
    # A (n, n) against b (65, n): the matrix is shared (stride 0)
    assert _collapse_batch((65,), (0,), (4,)) == ([], 65, [0, 4])
    # A (5, 1, n, n) against b (1, 7, n, 3): the 7 fold (A shared), the 5 are walked
    outer, inner, st = _collapse_batch((5, 7), (n2, 0), (0, 12))
    assert (inner, st) == (7, [0, 12]) and outer == [(5, [n2, 0])]
    # every second matrix of a larger stack; no batch at all
    assert _collapse_batch((4,), (2 * n2,), (4,)) == ([], 4, [2 * n2, 4])
    assert _collapse_batch((), (), ()) == ([], 1, [0, 0])


def test_abi_declares_the_batched_solve_entry_points():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    for name in ("pthip_gesv_batched", "pthip_laswp_batched"):
        assert name in ffi.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    assert len(ffi.SIGNATURES["pthip_gesv_batched"][1]) == 12


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


@needs_ref
def test_batched_solve_inverse_and_generalised_eigh_lower(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import eigh, inv, solve

    A3, B3, b2 = ptt.tensor3("A"), ptt.tensor3("B"), ptt.matrix("b")
    for ins, out, core in [
        ([A3, b2], solve(A3, b2), "Solve"),
        ([A3], inv(A3), "MatrixInverse"),
        ([A3, B3], list(eigh(A3, B3)), "Eigh"),
    ]:
        f = pytensor.function(ins, out, mode="hip")
        nodes = _nodes(f)
        assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
        assert any(n.op == "Blockwise" and n.params["core_op"] == core for n in nodes), [n.op for n in nodes]


@needs_ref
def test_batched_solve_gradient_lowers(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve

    A3, b2, w = ptt.tensor3("A"), ptt.matrix("b"), ptt.matrix("w")
    cost = (solve(A3, b2, b_ndim=1) * w).sum()
    f = pytensor.function([A3, b2, w], pytensor.grad(cost, [A3, b2]), mode="hip")
    assert not any(n.op == "HostPerform" for n in _nodes(f))
