"""CPU: ``attnfuse.fuse_attention`` on graphs lowered with the ``hip`` mode's rewrites (reference copy ``oracle/_ref``)."""
import pytest

import make_ref

pytestmark = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")


@pytest.fixture(scope="module")
def pt():
    make_ref.activate()
    import pytensor
    import pytensor.tensor as ptt

    import pytensor_amd

    pytensor_amd.register()
    return pytensor, ptt


def lowered_ops(pt, nd=3, dtype="float16", scale="mul", log=False, mask=False, keep_p=False, grad=False):
    """op names after ``run_pipeline`` of ``softmax(scale(q @ k^T) [+ m]) @ v`` (or of its gradient)"""
    pytensor, ptt = pt
    from pytensor_amd.passes import run_pipeline

    q, k, v, m = (ptt.tensor(n, dtype=dtype, shape=(None,) * nd) for n in "qkvm")
    c = ptt.scalar("c", dtype=dtype)
    s = ptt.matmul(q, k.swapaxes(-1, -2)) if nd == 3 else ptt.dot(q, k.T)
    s = {"mul": lambda: s * ptt.constant(0.25, dtype=dtype), "div": lambda: s / c, None: lambda: s}[scale]()
    p = (ptt.special.log_softmax if log else ptt.special.softmax)(s + m if mask else s, axis=-1)
    o = ptt.matmul(p, v) if nd == 3 else ptt.dot(p, v)
    outs = pytensor.grad(o.sum(), [q, k, v]) if grad else [o] + ([p] if keep_p else [])
    f = pytensor.function([q, k, v] + ([m] if mask else []) + ([c] if scale == "div" else []), outs, mode="hip")
    g, _ = run_pipeline(f.maker.linker.last_ir)
    att = [n for n in g.nodes if n.op == "Attention"]
    assert all(len(n.inputs) == (3 if scale is None else 4) and n.params["scale"] == scale for n in att)
    return [n.op for n in g.nodes]


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("scale", ["mul", "div", None])
def test_attention_chain_becomes_one_node(pt, nd, scale):
    ops = lowered_ops(pt, nd=nd, scale=scale)
    assert ops.count("Attention") == 1 and not {"Softmax", "BatchedDot", "Dot22", "Dot22Scalar"} & set(ops), ops


@pytest.mark.parametrize("kw", [dict(dtype="float32"), dict(log=True), dict(mask=True), dict(keep_p=True), dict(grad=True)], ids=str)
def test_everything_else_is_left_alone(pt, kw):
    ops = lowered_ops(pt, **kw)
    assert "Attention" not in ops and "Softmax" in ops, ops


def test_the_switch_turns_the_pass_off(pt, monkeypatch):
    monkeypatch.setenv("PTHIP_ATTENTION", "0")
    assert "Attention" not in lowered_ops(pt)
