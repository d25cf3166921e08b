"""Rankings: the k hottest cells of a cell list -- host side of hm_cells_top
(include/heatmap_amd.h, "Rankings").

    n, keys, counts = top_cells(keys, counts, 100)     # CUDA tensors, rank order

The order is fixed once: a record ranks before another when its count is
larger, or the counts are equal and its key is smaller, both as unsigned 64-bit
integers; for cells the key is HM_KEY(zoom, row, col), so ties go by zoom, row,
column.  StreamingHeatmap.top / top_tiles / top_groups / top_users answer the
same question straight from the resident log (hm_stream_top,
hm_stream_top_groups); rank_order and join_ranked are the pure host pieces
they share with the tests.  There is no CPU fallback: without a device
top_cells raises DeviceUnavailable.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import device as _dv


def check_k(k) -> int:
    """k as an int in 1..HM_TOP_MAX_K.  Pure: no device."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer 1..%d (got %r)" % (_lib.HM_TOP_MAX_K, k))
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1 (got %d)" % k)
    if k > _lib.HM_TOP_MAX_K:
        raise ValueError("k must be at most %d (got %d): a ranking of more cells is view() and a sort"
                         % (_lib.HM_TOP_MAX_K, k))
    return k


def rank_order(keys, counts) -> np.ndarray:
    """The permutation that puts (keys, counts) -- any integers, read as
    unsigned 64-bit -- into rank order: count descending, then key ascending.
    Pure numpy."""
    k = np.ascontiguousarray(keys).astype(np.int64, copy=False).view(np.uint64).reshape(-1)
    c = np.ascontiguousarray(counts).astype(np.int64, copy=False).view(np.uint64).reshape(-1)
    if k.shape != c.shape:
        raise ValueError("keys and counts must have one entry per record")
    return np.lexsort((k, ~c))


def join_ranked(zoom, row, col, count, side, k):
    """(zoom, row, col, count) int64 arrays of the first k cells in rank order
    among the ranked device cells given and the stream's out-of-square side
    records, side = (zoom, row, col, count) or None.  Cells rank by count
    descending, then zoom, row, col ascending as signed integers (for cells
    inside the square that is HM_KEY order); side cells are never cells of the
    device result, so the first k of the union is the first k overall.  Pure."""
    k = check_k(k)
    cols = [np.asarray(a).astype(np.int64).reshape(-1) for a in (zoom, row, col, count)]
    if side is not None:
        extra = [np.asarray(a).astype(np.int64).reshape(-1) for a in side]
        cols = [np.concatenate([a, b]) for a, b in zip(cols, extra)]
    z, r, c, n = cols
    order = np.lexsort((c, r, z, ~n.view(np.uint64)))[:k]
    return z[order], r[order], c[order], n[order]


def _u64_tensor(x, torch, dev_index):
    return _dv._dev(np.asarray(x).view(np.int64) if isinstance(x, np.ndarray) else x, torch.int64, dev_index)


def top_cells(keys, counts, k, device=0):
    """(n, keys, counts): the first n = min(len(keys), k) records of (keys,
    counts) -- hm_count's keys and counts, count / rollup / window / view
    output, numpy uint64 / int64 arrays or int64 CUDA tensors holding the
    unsigned bits -- in rank order, as int64 CUDA tensors of n entries
    (hm_cells_top).  Repeated keys are not merged.  The call is asynchronous
    on the context's stream."""
    dev_index = int(device)
    torch = _dv._torch()
    k = check_k(k)
    ctx = _dv.context(dev_index)
    kt = _u64_tensor(keys, torch, dev_index)
    ct = _u64_tensor(counts, torch, dev_index)
    if kt.numel() != ct.numel():
        raise ValueError("keys and counts must have one entry per record")
    ko = torch.empty(k, dtype=torch.int64, device="cuda:%d" % dev_index)
    co = torch.empty(k, dtype=torch.int64, device="cuda:%d" % dev_index)
    n = ctypes.c_int64(0)
    rc = ctx.L.hm_cells_top(ctx.ptr, _dv._ptr(kt), _dv._ptr(ct), kt.numel(), k, _dv._ptr(ko), _dv._ptr(co),
                            ctypes.byref(n))
    if rc != _lib.HM_OK:
        _lib.raise_for(rc)
    return n.value, ko[:n.value], co[:n.value]
