"""float16 attention: ``softmax(scale * q @ kT) @ v`` as one node.

The reference lowers an attention layer to a chain of four or five ``Apply`` nodes

    3-D:  BatchedDot(q, kT) -> [Elemwise: * or / an all-broadcast scalar] -> Softmax{axis=[2]} -> BatchedDot(p, v)
    2-D:  Dot22(q, kT) | Dot22Scalar(q, kT, s)                            -> Softmax{axis=[1]} -> Dot22(p, v)

(blas/batched.py:18, blas/gemm.py:248,298, special.py:26), each of which writes and reads the S x T score matrix.
``fuse_attention`` folds the chain into one ``Attention`` node — inputs ``q``, ``kT`` (the first product's right
operand as the graph has it: a (.., D, T) view), ``v`` and the optional scale — that csrc/hattention.hip runs in one
launch without the scores ever reaching memory (dispatch/blas.py ``attention``).

Matched only when every variable is float16, the softmax is the plain one over the last axis, the softmax is the
LEFT operand of the second product, and no intermediate has another consumer or is a graph output.  Everything else —
an additive mask, ``where``, a log-softmax, the gradient graph (its softmax output has several consumers), float32 /
float64, the 4-D form (``Reshape`` nodes around each ``BatchedDot``) — stays as it is.  ``PTHIP_ATTENTION=0``
switches the pass off.
"""

from __future__ import annotations

import os

from pytensor_amd.gemmfuse import _map_scan_inner
from pytensor_amd.inline import _copy, _index, _scalar_like
from pytensor_amd.ir import Graph, Node

_FIRST = ("BatchedDot", "Dot22", "Dot22Scalar")


def _scale_of(g: Graph, E: Node, scores: int):
    """``(scale var, "mul" | "div")`` when the Elemwise node ``E`` is exactly ``scores * c``, ``c * scores`` or
    ``scores / c`` with ``c`` of all-broadcastable shape; else ``None``"""
    if E.op != "Elemwise" or len(E.inputs) != 2 or len(E.outputs) != 1 or E.inputs.count(scores) != 1:
        return None
    sc = E.params["scalar"]
    if len(sc["body"]) != 1 or sc["outs"] != [["t", 0]]:
        return None
    pos = E.inputs.index(scores)
    other = E.inputs[1 - pos]
    if not _scalar_like(g.vars[other]):
        return None
    op, refs = sc["body"][0]["op"], sc["body"][0]["in"]
    if op == "Mul" and sorted(map(list, refs)) == [["i", 0], ["i", 1]]:
        return other, "mul"
    if op == "TrueDiv" and list(map(list, refs)) == [["i", pos], ["i", 1 - pos]]:
        return other, "div"
    return None


def fuse_attention(g: Graph) -> Graph:
    if os.environ.get("PTHIP_ATTENTION", "1") == "0":
        return g
    g = _map_scan_inner(g, fuse_attention)
    _, consumers = _index(g)
    out_set = set(g.outputs)
    half = lambda *vids: all(g.vars[v].dtype == "float16" for v in vids)

    def sole(vid):
        """the one node reading ``vid`` (once), when nothing else does and it is no graph output"""
        cons = consumers.get(vid, [])
        return g.nodes[cons[0]] if len(cons) == 1 and vid not in out_set else None

    replace, dead = {}, set()
    for k1, P1 in enumerate(g.nodes):
        if P1.op not in _FIRST or k1 in dead or not half(*P1.inputs, *P1.outputs):
            continue
        nd = 3 if P1.op == "BatchedDot" else 2
        if any(g.vars[v].ndim != nd for v in P1.inputs[:2]):
            continue
        scale, how = (P1.inputs[2], "mul") if P1.op == "Dot22Scalar" else (None, None)
        chain, cur = [P1], P1.outputs[0]
        nxt = sole(cur)
        if nxt is not None and scale is None and nxt.op == "Elemwise":
            hit = _scale_of(g, nxt, cur)
            if hit is None or not half(hit[0], nxt.outputs[0]):
                continue
            scale, how = hit
            chain.append(nxt)
            cur = nxt.outputs[0]
            nxt = sole(cur)
        if nxt is None or nxt.op != "Softmax" or nxt.params["log"] or list(nxt.params["axis"]) != [nd - 1]:
            continue
        chain.append(nxt)
        cur = nxt.outputs[0]
        P2 = sole(cur)
        if P2 is None or P2.op != ("BatchedDot" if nd == 3 else "Dot22") or P2.inputs[0] != cur or P2.inputs[1] == cur:
            continue
        if not half(cur, *P2.inputs, *P2.outputs) or g.vars[P2.inputs[1]].ndim != nd:
            continue
        chain.append(P2)
        ids = [k for k, n in enumerate(g.nodes) if any(n is c for c in chain)]
        ins = [P1.inputs[0], P1.inputs[1], P2.inputs[1]] + ([scale] if scale is not None else [])
        replace[ids[-1]] = Node("Attention", {"scale": how}, ins, list(P2.outputs))  # at the second product: v is there
        dead.update(ids[:-1])
    if not replace:
        return g
    return _copy(g, [replace.get(k, n) for k, n in enumerate(g.nodes) if k not in dead])
