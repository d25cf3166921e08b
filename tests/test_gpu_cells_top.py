"""hm_cells_top / heatmap_amd.top.top_cells on the device: the first k records in
rank order (count descending, key ascending, both unsigned 64-bit), exactly
numpy's lexsort on (key, ~count), order included.

Sizes sit at the selection's edges: a wave (64), a block's step (256), the
sort block's capacity and HM_TOP_MAX_K (4096, with the 4096 records a block of
the pass grid is sized by), 2048 and 8192 and their neighbours, and 100003 (a
few dozen blocks, a ragged tail).  k sits at 1, 2, a wave, 100, around n (the
n <= k path sorts the input itself) and at the limit."""
import ctypes

import numpy as np
import pytest

from heatmap_amd import _lib, device, top

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 100003]
MAXK = 4096
SENT = 0x5A5A5A5A5A5A5A5A
TOP = np.uint64(2 ** 64 - 1)


def ks(n):
    return sorted({k for k in (1, 2, 64, 100, n - 1, n, n + 1, MAXK) if 1 <= k <= MAXK})


def distinct_keys(n, rng):
    """n distinct keys that use all 64 bits, in random order"""
    k = np.unique(rng.integers(0, 2 ** 64 - 1, n + 64, dtype=np.uint64, endpoint=True))
    assert len(k) >= n
    k = rng.permutation(k)[:n]
    if n >= 2:
        k[0], k[1] = TOP, np.uint64(0)      # both ends of the key range are present
    return k


def u(rng, lo, hi, n):
    return rng.integers(lo, hi, n, dtype=np.uint64, endpoint=True)


# name -> (counts(n, k, rng), whether ties at the threshold must outnumber the records still wanted)
def _exact(n, k, rng):
    """k // 2 records above the threshold, exactly k - k // 2 at it, the rest below"""
    c = np.ones(n, dtype=np.uint64)
    c[:min(k, n)] = 5
    c[:min(k, n) // 2] = 9
    return rng.permutation(c)


def _huge(n, k, rng):
    c = np.full(n, 3, dtype=np.uint64)
    if n:
        c[rng.integers(0, n)] = TOP
    return c


PATTERNS = {
    "all equal": (lambda n, k, rng: np.full(n, 7, dtype=np.uint64), lambda n, k: k < n),
    "distinct high": (lambda n, k, rng: np.uint64(2 ** 63) + rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(
        max(1, (2 ** 63 - 1) // max(n, 1)))), None),
    "one to five": (lambda n, k, rng: u(rng, 1, 5, n), lambda n, k: n >= 2047 and k <= 100),
    "top byte": (lambda n, k, rng: (u(rng, 0, 255, n) << np.uint64(56)) | np.uint64(0x00AB00CD00EF0011),
                 lambda n, k: n >= 8191 and k <= 2),
    "bottom byte": (lambda n, k, rng: u(rng, 0, 255, n) | np.uint64(0xF0AB00CD00EF0000),
                    lambda n, k: n >= 8191 and k <= 2),
    "one huge among ties": (_huge, lambda n, k: 2 <= k < n),
    "zeros": (lambda n, k, rng: u(rng, 0, 2, n), lambda n, k: n >= 2047 and k <= 100),
    "ties exactly as wanted": (_exact, None),
}


def run(ctx, kt, ct, n, k, torch):
    """(status, n_out, keys_out, counts_out as uint64 host arrays of k entries)"""
    ko = torch.full((k,), SENT, dtype=torch.int64, device=kt.device)
    co = torch.full((k,), SENT, dtype=torch.int64, device=kt.device)
    m = ctypes.c_int64(-7)
    rc = ctx.L.hm_cells_top(ctx.ptr, device._ptr(kt), device._ptr(ct), n, k, device._ptr(ko), device._ptr(co),
                            ctypes.byref(m))
    return rc, m.value, ko.cpu().numpy().view(np.uint64), co.cpu().numpy().view(np.uint64)


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


@pytest.mark.parametrize("name", list(PATTERNS))
def test_first_k_in_rank_order(gpu, name):
    import torch

    make, must_tie = PATTERNS[name]
    ctx = device.context(0)
    rng = np.random.default_rng(list(PATTERNS).index(name) + 11)
    for n in SIZES:
        keys = distinct_keys(n, rng)
        fixed = None if name == "ties exactly as wanted" else make(n, 0, rng)
        for k in ks(n):
            counts = make(n, k, rng) if fixed is None else fixed
            kt, ct = dev(keys, torch), dev(counts, torch)
            order = np.lexsort((keys, ~counts))[:k]
            m = min(n, k)
            if k < n:
                t = counts[order[-1]]
                above, ties = int((counts > t).sum()), int((counts == t).sum())
                if name == "ties exactly as wanted":
                    assert ties == k - above and above == k // 2
                elif must_tie is not None and must_tie(n, k):
                    assert ties > k - above, (n, k)        # the key walk has something to cut
            rc, got_m, gk, gc = run(ctx, kt, ct, n, k, torch)
            assert rc == _lib.HM_OK and got_m == m, (n, k)
            assert np.array_equal(gk[:m], keys[order]) and np.array_equal(gc[:m], counts[order]), (n, k)
            assert (gk[m:] == SENT).all() and (gc[m:] == SENT).all(), (n, k)      # beyond *n_out: untouched
            # the inputs are as they were
            assert np.array_equal(kt.cpu().numpy().view(np.uint64), keys), (n, k)
            assert np.array_equal(ct.cpu().numpy().view(np.uint64), counts), (n, k)
            # again: bit-identical; a shuffled copy of the input: the identical output
            rc2, _, gk2, gc2 = run(ctx, kt, ct, n, k, torch)
            assert rc2 == _lib.HM_OK and np.array_equal(gk2, gk) and np.array_equal(gc2, gc), (n, k)
            p = rng.permutation(n)
            rc3, _, gk3, gc3 = run(ctx, dev(keys[p], torch), dev(counts[p], torch), n, k, torch)
            assert rc3 == _lib.HM_OK and np.array_equal(gk3, gk) and np.array_equal(gc3, gc), (n, k)


def test_repeated_keys_rank_each_by_itself(gpu):
    """keys that repeat are not merged: equal (count, key) records are the same
    record, so the first k are still unique -- also when the cut falls between
    copies of one key"""
    import torch

    ctx = device.context(0)
    rng = np.random.default_rng(77)
    for n, nkeys, hi in ((1000, 7, 2), (8193, 50, 1), (100003, 3, 0), (5000, 1, 0)):
        keys = rng.integers(0, nkeys, n).astype(np.uint64) << np.uint64(40)
        counts = u(rng, 0, hi, n)
        kt, ct = dev(keys, torch), dev(counts, torch)
        order = np.lexsort((keys, ~counts))
        for k in (1, 2, 64, 100, 999, MAXK):
            m = min(n, k)
            t, tk = counts[order[m - 1]], keys[order[m - 1]]
            same = int(((counts == t) & (keys == tk)).sum())
            assert same > 1                                  # the last record taken has copies
            rc, got_m, gk, gc = run(ctx, kt, ct, n, k, torch)
            assert rc == _lib.HM_OK and got_m == m, (n, k)
            assert np.array_equal(gk[:m], keys[order[:m]]) and np.array_equal(gc[:m], counts[order[:m]]), (n, k)
            assert (gk[m:] == SENT).all() and (gc[m:] == SENT).all(), (n, k)


def test_top_cells_wrapper_and_count_output(gpu):
    """the Python wrapper over numpy and tensor input, on real hm_count cells"""
    import torch

    from heatmap_amd import synth

    lat, lon = synth.generate("hotspots", 50000, seed=3)
    cnt = device.count(lat, lon, None, 0, 18)
    keys = (cnt.zoom.astype(np.uint64) << np.uint64(58)) | (cnt.row.astype(np.uint64) << np.uint64(29)) | \
        cnt.col.astype(np.uint64)
    counts = cnt.count.astype(np.uint64)
    order = top.rank_order(keys, counts)
    for k in (1, 100, MAXK):
        for a, b in ((keys, counts), (dev(keys, torch), dev(counts, torch))):
            n, tk, tc = top.top_cells(a, b, k)
            assert n == min(k, len(keys)) and tk.is_cuda and tk.numel() == n
            assert np.array_equal(tk.cpu().numpy().view(np.uint64), keys[order[:k]])
            assert np.array_equal(tc.cpu().numpy().view(np.uint64), counts[order[:k]])
    assert counts[order[0]] == 50000 and keys[order[0]] == 0          # the zoom-0 cell leads
    n, tk, tc = top.top_cells(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 5)
    assert n == 0 and tk.numel() == 0
    with pytest.raises(ValueError):
        top.top_cells(keys, counts[:-1], 5)
    with pytest.raises(ValueError, match=r"view\(\)"):
        top.top_cells(keys, counts, MAXK + 1)


def test_bad_arguments_leave_the_outputs(gpu):
    import torch

    ctx = device.context(0)
    L = ctx.L
    buf = torch.arange(64, dtype=torch.int64, device="cuda:0")
    kin, cin = buf[0:16], buf[16:32]
    out = torch.full((32,), SENT, dtype=torch.int64, device="cuda:0")
    ko, co = out[0:8], out[8:16]
    P = device._ptr
    m = ctypes.c_int64(-7)
    table = [
        (None, P(kin), P(cin), 16, 4, P(ko), P(co), ctypes.byref(m)),          # no context
        (ctx.ptr, P(kin), P(cin), 16, 4, P(ko), P(co), None),                  # no n_out
        (ctx.ptr, P(kin), P(cin), -1, 4, P(ko), P(co), ctypes.byref(m)),       # n < 0
        (ctx.ptr, P(kin), P(cin), 16, 0, P(ko), P(co), ctypes.byref(m)),       # k = 0
        (ctx.ptr, P(kin), P(cin), 16, -3, P(ko), P(co), ctypes.byref(m)),
        (ctx.ptr, P(kin), P(cin), 16, MAXK + 1, P(ko), P(co), ctypes.byref(m)),
        (ctx.ptr, None, P(cin), 16, 4, P(ko), P(co), ctypes.byref(m)),         # nulls with n > 0
        (ctx.ptr, P(kin), None, 16, 4, P(ko), P(co), ctypes.byref(m)),
        (ctx.ptr, P(kin), P(cin), 16, 4, None, P(co), ctypes.byref(m)),
        (ctx.ptr, P(kin), P(cin), 16, 4, P(ko), None, ctypes.byref(m)),
        (ctx.ptr, P(kin), P(cin), 16, 4, P(kin), P(co), ctypes.byref(m)),      # outputs on the inputs
        (ctx.ptr, P(kin), P(cin), 16, 4, P(ko), P(cin), ctypes.byref(m)),
        (ctx.ptr, P(kin), P(cin), 16, 4, P(buf[14:18]), P(co), ctypes.byref(m)),   # straddling both inputs
        (ctx.ptr, P(kin), P(cin), 16, 8, P(buf[32:40]), P(buf[28:36]), ctypes.byref(m)),   # counts_out into counts
        (ctx.ptr, P(buf[0:16]), P(buf[40:56]), 16, 8, P(buf[16:24]), P(buf[36:44]), ctypes.byref(m)),
    ]
    for args in table:
        assert L.hm_cells_top(*args) == _lib.HM_E_ARG, args[3:5]
    torch.cuda.synchronize()
    assert m.value == -7
    assert (out.cpu().numpy().view(np.uint64) == SENT).all()
    assert np.array_equal(buf.cpu().numpy(), np.arange(64))
    # adjacent ranges do not overlap; n = 0 is fine with nothing at all
    assert L.hm_cells_top(ctx.ptr, P(buf[0:16]), P(buf[16:32]), 16, 8, P(buf[32:40]), P(buf[40:48]),
                          ctypes.byref(m)) == _lib.HM_OK and m.value == 8
    assert L.hm_cells_top(ctx.ptr, None, None, 0, 4, None, None, ctypes.byref(m)) == _lib.HM_OK and m.value == 0
    torch.cuda.synchronize()
