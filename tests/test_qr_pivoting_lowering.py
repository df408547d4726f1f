"""CPU: ``pt.linalg.qr(x, pivoting=True)`` under ``mode="hip"`` lowers to the ``QR`` IR op with ``pivoting`` set (one
more output, the int32 permutation, last), a stack of matrices to its ``Blockwise``, with no host fallback; unpivoted
nodes keep the params they always had; the C ABI declares ``pthip_geqp3``."""
import os
import re

import numpy as np
import pytest

import make_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_ref = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")

N_OUT = {"full": 3, "economic": 3, "r": 2, "raw": 4}


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


def _last_output(f, node):
    return f.maker.linker.last_ir.vars[node.outputs[-1]]


def _outputs(r):
    return list(r) if isinstance(r, (list, tuple)) else [r]


@needs_ref
@pytest.mark.parametrize("mode", list(N_OUT))
def test_single_matrix_lowers(pt, mode):
    pytensor, ptt = pt
    x = ptt.matrix("x")
    f = pytensor.function([x], _outputs(ptt.linalg.qr(x, mode=mode, pivoting=True)), mode="hip")
    nodes = _nodes(f)
    assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
    (qr,) = [n for n in nodes if n.op == "QR"]
    assert qr.params == {"mode": mode, "pivoting": True}
    assert len(qr.outputs) == N_OUT[mode]
    assert _last_output(f, qr).dtype == "int32" and len(_last_output(f, qr).shape) == 1


@needs_ref
@pytest.mark.parametrize("mode", list(N_OUT))
def test_stack_lowers_to_blockwise(pt, mode):
    pytensor, ptt = pt
    x = ptt.tensor3("x")
    f = pytensor.function([x], _outputs(ptt.linalg.qr(x, mode=mode, pivoting=True)), mode="hip")
    nodes = _nodes(f)
    assert not any(n.op == "HostPerform" for n in nodes), [n.op for n in nodes]
    (bw,) = [n for n in nodes if n.op == "Blockwise"]
    assert bw.params["core_op"] == "QR" and bw.params["core_params"] == {"mode": mode, "pivoting": True}
    assert bw.params["signature"].endswith(",(n)")
    assert len(bw.outputs) == N_OUT[mode]
    assert _last_output(f, bw).dtype == "int32" and len(_last_output(f, bw).shape) == 2


@needs_ref
def test_unpivoted_params_are_unchanged(pt):
    pytensor, ptt = pt
    x, x3 = ptt.matrix("x"), ptt.tensor3("x3")
    f = pytensor.function([x], _outputs(ptt.linalg.qr(x, mode="economic")), mode="hip")
    (qr,) = [n for n in _nodes(f) if n.op == "QR"]
    assert qr.params == {"mode": "economic"} and len(qr.outputs) == 2
    f = pytensor.function([x3], _outputs(ptt.linalg.qr(x3, mode="r")), mode="hip")
    (bw,) = [n for n in _nodes(f) if n.op == "Blockwise"]
    assert bw.params["core_params"] == {"mode": "r"}


def test_abi_declares_geqp3():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    assert "pthip_geqp3" in ffi.SIGNATURES and re.search(r"\bpthip_geqp3\s*\(", header)
    assert len(ffi.SIGNATURES["pthip_geqp3"][1]) == 7
    decl = re.search(r"\bpthip_geqp3\s*\(([^)]*)\)", header).group(1)
    assert len(decl.split(",")) == 7


def test_lds_bound_matches_the_kernel_source():
    """``geqp3_lds_fits`` restates the bound of csrc/decomp.hip: the same constant, and the edges the GPU tests sit on"""
    from pytensor_amd.dispatch import decomp

    src = open(os.path.join(ROOT, "pytensor_amd", "csrc", "decomp.hip")).read()
    m = re.search(r"QR_LDS_MAX = (\d+) \* 1024 - (\d+) \* 1024;", src)
    assert (int(m.group(1)) - int(m.group(2))) * 1024 == decomp.QR_LDS_MAX
    assert decomp.geqp3_lds_fits(136, 136, 8) and not decomp.geqp3_lds_fits(137, 137, 8)
    assert decomp.geqp3_lds_fits(193, 193, 4) and not decomp.geqp3_lds_fits(194, 194, 4)
    assert not decomp.geqp3_lds_fits(600, 3, 8)  # (m beyond 512: the reflector stage of the LDS form)
    assert np.dtype("int32").itemsize == 4
