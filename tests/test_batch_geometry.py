"""CPU: ``dispatch/batch.py`` against the helpers it replaced.  The folding rules as they stood in ``dispatch/lu.py``
(``_batch_strides``, ``_collapse_batch``) and ``dispatch/misc.py`` (``_merge_batch``), and the walk over the unfolded
dims as ``_gesv_wave`` / ``_gbsv`` / ``gesvj_device`` wrote it out, are restated here in plain Python; the module's
functions must give exactly what they give on every batch shape of up to four dims with extents in {1, 2, 3, 5}, for
one, two and three operands, each contiguous, broadcast (stride 0, by a length-1 dim or a missing leading dim), sliced
(every second item) or permuted."""
import functools
import itertools

import numpy as np

from pytensor_amd.device import DeviceArray, contiguous_strides
from pytensor_amd.dispatch.batch import batch_strides, collapse_batch, merge_batch, walk_outer

CORE = (4, 3)
KINDS = ("contiguous", "bcast_even", "bcast_odd", "short", "sliced", "permuted")
BSHAPES = [s for nd in range(5) for s in itertools.product((1, 2, 3, 5), repeat=nd)]


def operand(bshape, kind):
    """A (*lead, *CORE) array (no memory behind it: only shapes and strides are read) that broadcasts to ``bshape``"""
    lead = tuple(bshape)
    if kind == "bcast_even":
        lead = tuple(1 if d % 2 == 0 else s for d, s in enumerate(lead))
    elif kind == "bcast_odd":
        lead = tuple(1 if d % 2 == 1 else s for d, s in enumerate(lead))
    elif kind == "short":
        lead = lead[1:]
    st = contiguous_strides((*lead, *CORE))
    if kind == "sliced":
        st = tuple(2 * s for s in st[: len(lead)]) + st[len(lead):]
    elif kind == "permuted":  # the batch dims of a stack stored in the reverse order
        rev = contiguous_strides((*lead[::-1], *CORE))
        st = rev[: len(lead)][::-1] + st[len(lead):]
    return DeviceArray(None, 0, (*lead, *CORE), st, "float64")


def old_batch_strides(x, core_ndim, bshape):
    lead = x.shape[: x.ndim - core_ndim]
    pad = len(bshape) - len(lead)
    return (0,) * pad + tuple(0 if s == 1 else st for s, st in zip(lead, x.strides[: len(lead)]))


def old_collapse_batch(bshape, *stride_sets):
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


def old_merge_batch(bshape, *stride_sets):
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


def old_walk(outer, n_operands):
    for f, idx in enumerate(np.ndindex(*[s for s, _ in outer])):
        yield f, [sum(i * sts[k] for i, (_, sts) in zip(idx, outer)) for k in range(n_operands)]


@functools.lru_cache(maxsize=None)
def cases():
    """(batch shape, operands), built once for the three tests"""
    return [(bshape, [operand(bshape, k) for k in kinds])
            for bshape in BSHAPES for nops in (1, 2, 3)
            for kinds in itertools.combinations_with_replacement(KINDS, nops)]  # (the rules do not care which operand is which)


def test_the_enumeration_reaches_every_outcome():
    """some batches fold whole, some leave dims to walk, and the two folding rules do differ: the reason
    ``collapse_batch`` keeps a loop of its own"""
    whole = walked = differ = 0
    for bshape, xs in cases():
        sets = [old_batch_strides(x, 2, bshape) for x in xs]
        outer, inner, st = old_collapse_batch(bshape, *sets)
        merged = old_merge_batch(bshape, *sets)
        whole += not outer
        walked += len(outer) >= 2
        differ += len(merged) != len(outer) + (inner > 1)
    assert whole > 1000 and walked > 1000 and differ > 0


def test_batch_strides_and_both_foldings_are_the_replaced_ones():
    for bshape, xs in cases():
        sets = [batch_strides(x, 2, bshape) for x in xs]
        assert sets == [old_batch_strides(x, 2, bshape) for x in xs], (bshape, xs)
        assert collapse_batch(bshape, *sets) == old_collapse_batch(bshape, *sets), (bshape, sets)
        assert merge_batch(bshape, *sets) == old_merge_batch(bshape, *sets), (bshape, sets)


def test_walk_outer_is_the_ndindex_arithmetic():
    for bshape, xs in cases():
        sets = [old_batch_strides(x, 2, bshape) for x in xs]
        outer, inner, _ = old_collapse_batch(bshape, *sets)
        walk = list(walk_outer(outer, len(xs)))
        assert walk == list(old_walk(outer, len(xs))), (bshape, sets)
        # every item of the batch is addressed once: the walk times the fold is the batch
        assert len(walk) * inner == int(np.prod(bshape)), (bshape, sets)
