"""CPU: the whole-chip SVD tier (``dispatch/decomp.py::svd_tier`` -> "block", ``pthip_svd_block``) — the shapes it
takes, the boundaries below it that must not move, its C ABI, and the ``svd`` / ``pinv`` / ``lstsq`` graphs that reach
it through ``svd_device`` lowering with no host fallback."""
import os
import re

import pytest

import make_ref
from pytensor_amd.dispatch import decomp
from pytensor_amd.dispatch.decomp import SVD_WAVE_MAX, svd_tier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_ref = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")


def test_block_tier_takes_what_was_refused():
    assert decomp.SVD_ROWS_MAX == 2048
    for nb in (1, 3):
        assert svd_tier(2049, 2049, nb) == "block"
        assert svd_tier(5000, 2049, nb) == "block"
        assert svd_tier(2049, 5000, nb) == "block"


def test_boundaries_below_the_block_tier_hold():
    W = SVD_WAVE_MAX
    assert W in (32, 64)
    for nb in (1, 2, 100000):
        for m, n in [(1, 1), (W, W), (W, 1), (1, W)]:
            assert svd_tier(m, n, nb) == "wave", (m, n, nb)
        for m, n in [(W + 1, 1), (1, W + 1), (2048, 4096), (4096, 2048), (2048, 2048), (100000, 2048)]:
            assert svd_tier(m, n, nb) == "rows", (m, n, nb)


def test_abi_declares_the_block_svd_entry_point():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    assert "pthip_svd_block" in ffi.SIGNATURES and re.search(r"\bpthip_svd_block\s*\(", header)
    # dtype, batch, r, c, vectors, rows_out, X, S, Wt, Pt
    assert len(ffi.SIGNATURES["pthip_svd_block"][1]) == 10
    assert "pthip_svd_block_sweeps" in ffi.SIGNATURES and re.search(r"\bpthip_svd_block_sweeps\s*\(", header)
    assert len(ffi.SIGNATURES["pthip_svd_block_sweeps"][1]) == 0


@pytest.fixture(scope="module")
def pt():
    make_ref.activate()
    import pytensor
    import pytensor.tensor as ptt

    import pytensor_amd

    pytensor_amd.register()
    return pytensor, ptt


@needs_ref
def test_svd_pinv_and_lstsq_lower_without_a_host_node(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import lstsq, pinv, svd

    A, B, A3 = ptt.matrix("A"), ptt.matrix("B"), ptt.tensor3("A3")
    for ins, out in [
        ([A], list(svd(A, full_matrices=False))),
        ([A], list(svd(A, full_matrices=True))),
        ([A], svd(A, compute_uv=False)),
        ([A], pinv(A)),
        ([A, B], list(lstsq(A, B, -1.0))),
        ([A3], list(svd(A3, full_matrices=False))),
        ([A3], pinv(A3)),
    ]:
        f = pytensor.function(ins, out, mode="hip")
        nodes = f.maker.linker.last_ir.nodes
        assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
