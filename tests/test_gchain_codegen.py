"""CPU: every ``gchain`` instance the pipelined row loop is generated for compiles for gfx950 without scratch memory
and within the LDS budget of ``dispatch/fused.py`` (static LDS of the kernel plus the largest gather table it may be
launched with).  Needs the built ``libpthip.so`` (hiprtc), no GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chain():
    """config #4's GemvChain node after the fusion passes."""
    from pytensor_amd.ir import Graph
    from pytensor_amd.passes import run_pipeline

    d = json.load(open(os.path.join(ROOT, "tests", "golden", "c4_hier.json")))
    graph, _ = run_pipeline(Graph.from_dict(d), True, tail=True)
    (node,) = [n for n in graph.nodes if n.op == "GemvChain"]
    return node.params


def _note_int(code: bytes, key: bytes) -> int:
    """The integer stored under ``key`` in the code object's metadata note (a MessagePack map; one kernel per object)."""
    at = code.index(bytes([0xA0 + len(key)]) + key) + 1 + len(key)  # (a fixstr: one length byte, then the text)
    assert code.count(key) == 1
    t = code[at]
    if t <= 0x7F:
        return t
    width = {0xCC: 1, 0xCD: 2, 0xCE: 4, 0xCF: 8}[t]
    return int.from_bytes(code[at + 1 : at + 1 + width], "big")


def _metadata(code: bytes):
    """(private segment bytes, static LDS bytes) of the one kernel in ``code``."""
    return _note_int(code, b".private_segment_fixed_size"), _note_int(code, b".group_segment_fixed_size")


# (C, RG, pack, dtype, full, scatter output in bins | None: stored for the late scatter, bin groups)
CASES = [
    (1, 32, 2, "float64", True, True, 2),  # config #4
    (1, 32, 2, "float64", True, True, 1),
    (1, 32, 2, "float64", True, True, 4),
    (1, 32, 2, "float64", True, False, 2),  # more than 256 bins: the scattered output is stored
    (1, 32, 2, "float64", False, True, 2),  # K = 2, 64: lanes past the end of the row
    (1, 32, 1, "float64", False, True, 2),  # K = 127
    (2, 16, 2, "float64", True, True, 2),  # K = 256
    (4, 8, 2, "float64", False, True, 2),  # K = 500
    (8, 4, 2, "float64", True, True, 2),  # K = 1024: the smallest RG the pipelined form exists for
    (16, 2, 2, "float64", True, True, 2),  # K = 2048: multiplier in LDS, plain loop only
    (2, 16, 4, "float32", True, True, 2),  # float32, K = 128: the four-column pack
]


@pytest.mark.parametrize("pipe", [True, False])
@pytest.mark.parametrize("C,RG,pack,dtype,full,binned,sgroups", CASES)
def test_instance_compiles_without_scratch_within_the_lds_budget(chain, C, RG, pack, dtype, full, binned, sgroups, pipe):
    from pytensor_amd import codegen_gchain, kernel_cache
    from pytensor_amd.dispatch import fused

    p = chain
    body, spec = p["scalar"], p["reduce"]
    if dtype != "float64":
        d = json.load(open(os.path.join(ROOT, "tests", "golden", "c4_hier_f32.json")))
        from pytensor_amd.ir import Graph
        from pytensor_amd.passes import run_pipeline

        graph, _ = run_pipeline(Graph.from_dict(d), True, tail=True)
        (node,) = [n for n in graph.nodes if n.op == "GemvChain"]
        p = node.params
        body, spec = p["scalar"], p["reduce"]
    rs = [None if r is None else (r["op"], r["acc_dtype"]) for r in spec]
    out_store = list(p.get("out_store") or [s is None for s in spec])
    scatter_out = p["scatter_out"] if binned else None
    if not binned:
        out_store[p["scatter_out"]] = True
    gather = set(p.get("gather") or [])
    e_modes = ["R" if k == p["r_pos"] else ("G" if k in gather else "S") for k in range(len(body["in_dtypes"]))]
    name = f"gchain_t_c{C}_g{RG}_p{pack}_{dtype}_{int(full)}{int(binned)}{sgroups}_{int(pipe)}"
    args = (body, e_modes, rs, p["w_out"], C, RG, p["store_r"], True, out_store, scatter_out, sgroups, pack, dtype, pipe, pipe and full)
    if pipe and RG < 4:
        with pytest.raises(AssertionError):  # (no pipelined form: a half would be less than two rows)
            codegen_gchain.gemv_chain_source(name, *args)
        return
    src = codegen_gchain.gemv_chain_source(name, *args)
    key = kernel_cache.compile_source(src, name)
    private, lds = _metadata(kernel_cache._code[key])
    assert private == 0, "the kernel spills to scratch memory"
    table = fused.GATHER_LDS_ENTRIES * 8 if pipe else 0  # the largest gather table it may be launched with (dynamic LDS)
    # the budget is the pipelined form's (three workgroups per CU); the plain loop is held to the LDS of a CU only
    assert lds + table <= (fused.CHAIN_LDS_BUDGET if pipe else 160 * 1024), (lds, table)
