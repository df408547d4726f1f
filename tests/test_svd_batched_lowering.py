"""CPU: the batched SVD tiers (``dispatch/decomp.py::svd_tier``), the C ABI of the one-launch kernel, and the graphs
that use them under ``mode="hip"`` — ``svd``, ``pinv`` and ``qr`` of a stack, and the gradients of ``svd``, lower
to ``Blockwise`` nodes with no host fallback."""
import os
import re

import pytest

import make_ref
from pytensor_amd.dispatch.decomp import SVD_WAVE_MAX, svd_tier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_ref = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")


def test_svd_tier_boundaries():
    W = SVD_WAVE_MAX
    assert W in (32, 64)
    for nb in (1, 2, 100000):
        for m, n in [(1, 1), (W, W), (W, 1), (1, W)]:
            assert svd_tier(m, n, nb) == "wave", (m, n, nb)
        for m, n in [(W + 1, 1), (1, W + 1), (2048, 4096)]:
            assert svd_tier(m, n, nb) == "rows", (m, n, nb)


def test_abi_declares_the_batched_svd_entry_point():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    assert "pthip_gesvj_batched" in ffi.SIGNATURES and re.search(r"\bpthip_gesvj_batched\s*\(", header)
    # dtype, batch, m, n, job, A and its three strides, rcond, U, S, Vt, pinv
    assert len(ffi.SIGNATURES["pthip_gesvj_batched"][1]) == 14


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
def test_batched_svd_pinv_and_qr_lower(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import pinv, qr, svd

    A3 = ptt.tensor3("A")
    for out, core in [
        (list(svd(A3, full_matrices=False)), "SVD"),
        (svd(A3, compute_uv=False), "SVD"),
        (pinv(A3), "MatrixPinv"),
        (list(qr(A3)), "QR"),
    ]:
        f = pytensor.function([A3], out, mode="hip")
        nodes = _nodes(f)
        assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
        assert any(n.op == "Blockwise" and n.params["core_op"] == core for n in nodes), [n.op for n in nodes]


@needs_ref
def test_batched_svd_gradients_lower(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import svd

    A3, w, W = ptt.tensor3("A"), ptt.matrix("w"), ptt.tensor3("W")
    cost = (w * svd(A3, compute_uv=False)).sum()
    f = pytensor.function([A3, w], pytensor.grad(cost, A3), mode="hip")
    assert not any(n.op == "HostPerform" for n in _nodes(f))
    U, s, Vt = svd(A3, full_matrices=False)
    cost = ((U @ Vt) * W).sum() + s.sum()
    f = pytensor.function([A3, W], pytensor.grad(cost, A3), mode="hip")
    assert not any(n.op == "HostPerform" for n in _nodes(f))
