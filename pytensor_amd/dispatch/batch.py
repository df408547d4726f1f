"""Batch geometry: broadcast leading dimensions and their strides as what a kernel that takes a batch stride can walk.

The one place that knows it (DESIGN §4 "Stacked core ops"); a leaf module, imported by the linear-algebra and signal
handlers and importing none of them.
"""

from __future__ import annotations

import numpy as np

from pytensor_amd.device import DeviceArray, contiguous_strides, copy_into


def batch_strides(x: DeviceArray, core_ndim: int, bshape):
    """Element strides of ``x``'s leading dims broadcast to ``bshape`` (0 along a broadcast dim)."""
    lead = x.shape[: x.ndim - core_ndim]
    pad = len(bshape) - len(lead)
    return (0,) * pad + tuple(0 if s == 1 else st for s, st in zip(lead, x.strides[: len(lead)]))


def batchify(x: DeviceArray, core_ndim: int, bshape):
    """Broadcast leading dims to ``bshape`` and return a contiguous (batch, *core) array."""
    core = x.shape[x.ndim - core_ndim :]
    lead = x.shape[: x.ndim - core_ndim]
    lead = (1,) * (len(bshape) - len(lead)) + lead
    nb = int(np.prod(bshape)) if bshape else 1
    if lead == tuple(bshape) and x.is_contiguous():
        return x.view((nb, *core), contiguous_strides((nb, *core)))
    out = DeviceArray.empty((*bshape, *core), x.dtype)
    copy_into(out, x.view((*lead, *core), (0,) * (len(lead) - (x.ndim - core_ndim)) + x.strides))
    return out.view((nb, *core), contiguous_strides((nb, *core)))


def merge_batch(bshape, *stride_sets):
    """The batch as the fewest (size, strides per operand) dimensions a kernel can walk: length-1 dimensions dropped,
    neighbours merged where every operand's strides allow it."""
    dims = []
    for d, n in enumerate(bshape):
        if n == 1:
            continue
        st = [ss[d] for ss in stride_sets]
        if dims and all(p == q * n for p, q in zip(dims[-1][1], st)):
            dims[-1] = (dims[-1][0] * n, st)
        else:
            dims.append((n, st))
    return dims


def collapse_batch(bshape, *stride_sets):
    """Fold the batch dims, innermost first, into one count with ONE stride per operand — what a kernel that takes
    a batch stride can walk by itself.  Returns (outer, inner, strides): ``outer`` lists the (size, stride per
    operand) of the leading dims that do not fold (the caller loops them: ``walk_outer``), ``inner`` the folded count.

    Not ``merge_batch`` with its last dimension split off: that merges from the left, so leading dims that merge with
    each other but not into the inner fold ((2, 3, 5) with strides (60, 20, 2)) come back as one outer dim where this
    lists two, and a zero extent folds differently.  The walk is the same; the lists the callers see are not."""
    dims = [(s, [ss[d] for ss in stride_sets]) for d, s in enumerate(bshape) if s != 1]
    inner, st = 1, [0] * len(stride_sets)
    while dims:
        s, sts = dims[-1]
        if inner > 1 and any(a != b * inner for a, b in zip(sts, st)):
            break
        if inner == 1:
            st = list(sts)
        inner *= s
        dims.pop()
    return dims, inner, st


def walk_outer(outer, n_operands: int):
    """(flat index, [element offset per operand]) of every index of the dims ``collapse_batch`` left unfolded, in
    row-major order: one launch each."""
    for f, idx in enumerate(np.ndindex(*[s for s, _ in outer])):
        yield f, [sum(i * sts[k] for i, (_, sts) in zip(idx, outer)) for k in range(n_operands)]


def swap_core(x: DeviceArray) -> DeviceArray:
    """the stack with its two core dimensions swapped (a view)"""
    return x.view((*x.shape[:-2], x.shape[-1], x.shape[-2]), (*x.strides[:-2], x.strides[-1], x.strides[-2]))


def as_contiguous(x: DeviceArray, shape) -> DeviceArray:
    """``x`` (copied if it is not contiguous) viewed in ``shape``"""
    return x.contiguous().view(tuple(shape), contiguous_strides(shape))
