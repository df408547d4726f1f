"""CPU: Bessel functions of real order and Owen's T under ``mode="hip"`` — each graph lowers into a fused
``Elemwise`` whose kernel carries the device helper it needs, and only that one.  Hyp2F1 stays refused."""
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


def _graphs(pytensor, ptt):
    x, v, h = ptt.dvector("x"), ptt.dvector("v"), ptt.dvector("h")
    n = ptt.lvector("n")
    return {
        "grad_i1": ([x], pytensor.grad(ptt.i1(x).sum(), x), "Ive"),
        "ive": ([v, x], ptt.ive(v, x), "Ive"),
        "iv": ([v, x], ptt.iv(v, x), "Ive"),
        "log_iv": ([v, x], ptt.log(ptt.iv(v, x)), "Ive"),
        "kve": ([v, x], ptt.kve(v, x), "Kve"),
        "kv": ([v, x], ptt.kv(v, x), "Kve"),
        "kn": ([n, x], ptt.kn(n, x), "Kve"),
        "jv": ([v, x], ptt.jv(v, x), "Jv"),
        "owens_t": ([h, x], ptt.owens_t(h, x), "Owens_t"),
        "grad_jv": ([v, x], pytensor.grad(ptt.jv(v, x).sum(), x), "Jv"),
        "grad_log_kv": ([v, x], pytensor.grad(ptt.log(ptt.kv(v, x)).sum(), x), "Kve"),
        "grad_owens_t": ([h, x], pytensor.grad(ptt.owens_t(h, x).sum(), [h, x]), None),  # exp / erf only
        "f32_jv": ([ptt.fvector("v32"), ptt.fvector("x32")], None, "Jv"),
    }


def _scalar_ops(f):
    from pytensor_amd import codegen_scalar

    g = f.maker.linker.last_ir
    ops = [n.op for n in g.nodes]
    assert "HostPerform" not in ops, ops
    return {op for n in g.nodes if n.op == "Elemwise" for op in codegen_scalar.body_ops(n.params["scalar"])}


@pytest.mark.parametrize("name", ["grad_i1", "ive", "iv", "log_iv", "kve", "kv", "kn", "jv", "owens_t", "grad_jv", "grad_log_kv", "grad_owens_t", "f32_jv"])
def test_graph_lowers_into_a_fused_elemwise(pt, name):
    pytensor, ptt = pt
    ins, out, op = _graphs(pytensor, ptt)[name]
    if out is None:
        out = ptt.jv(ins[0], ins[1])
        assert out.dtype == "float32"
    f = pytensor.function(ins, out, mode="hip")
    ops = _scalar_ops(f)
    assert op is None or op in ops


def test_scan_step_with_jv_lowers(pt):
    pytensor, ptt = pt
    x = ptt.dvector("x")
    ys, _ = pytensor.scan(lambda k, acc: acc + ptt.jv(k, x), sequences=[ptt.arange(3.0)], outputs_info=[ptt.zeros_like(x)])
    f = pytensor.function([x], ys[-1], mode="hip")
    ops = [n.op for n in f.maker.linker.last_ir.nodes]
    assert "HostPerform" not in ops


def test_hyp2f1_is_still_refused(pt):
    pytensor, ptt = pt
    x = ptt.dvector("x")
    with pytest.raises(NotImplementedError, match="Hyp2F1"):
        pytensor.function([x], ptt.hyp2f1(0.5, 1.0, 1.5, ptt.sigmoid(x)), mode="hip")


def test_kernel_source_carries_only_the_helpers_it_uses(pt):
    pytensor, ptt = pt
    from pytensor_amd import codegen_scalar

    x, v, h = ptt.dvector("x"), ptt.dvector("v"), ptt.dvector("h")
    f = pytensor.function([v, x, h], [ptt.jv(v, x), ptt.ive(v, x), ptt.kve(v, x), ptt.owens_t(h, x)], mode="hip")
    bodies = [n.params["scalar"] for n in f.maker.linker.last_ir.nodes if n.op == "Elemwise"]
    assert {op for b in bodies for op in codegen_scalar.body_ops(b)} >= {"Jv", "Ive", "Kve", "Owens_t"}
    full = codegen_scalar.prelude_for(*bodies)
    for fn in ("double pt_jv(", "double pt_ive(", "double pt_kve(", "double pt_owens_t("):
        assert fn in full
    plain = pytensor.function([x], ptt.exp(x) * ptt.i0(x), mode="hip")
    src = codegen_scalar.prelude_for(*[n.params["scalar"] for n in plain.maker.linker.last_ir.nodes if n.op == "Elemwise"])
    assert "pt_jv" not in src and "pt_owens_t" not in src and "pt_sf_" not in src
    # an Owen's T body does not carry the Bessel code, nor the reverse
    ot = [b for b in bodies if "Owens_t" in set(codegen_scalar.body_ops(b))]
    jv = [b for b in bodies if "Jv" in set(codegen_scalar.body_ops(b))]
    assert "pt_jv" not in codegen_scalar.prelude_for(*ot) and "pt_owens_t" not in codegen_scalar.prelude_for(*jv)


def test_flat_kernel_compiles_for_gfx950(pt):
    pytensor, ptt = pt
    from pytensor_amd import codegen, ffi

    x, v, h = ptt.dvector("x"), ptt.dvector("v"), ptt.dvector("h")
    f = pytensor.function([v, x, h], [ptt.jv(v, x), ptt.owens_t(h, x)], mode="hip")
    for n in f.maker.linker.last_ir.nodes:
        b = n.params["scalar"]
        code = ffi.jit_compile(codegen.flat_kernel_source("k_special", b, "V" * len(b["in_dtypes"]), 2), "k_special.hip")
        assert len(code) > 0
