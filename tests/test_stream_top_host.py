"""The host side of rankings (hm_cells_top, hm_stream_top, hm_stream_top_groups;
heatmap_amd.top and StreamingHeatmap.top*) on the CPU.

csrc/hm_top_select.h is plain C and is the digit walk the selection kernels
run: a shim around it is built here with the host compiler and a Python loop
plays the passes -- numpy counts the records that agree with the decided bits
by their next digit, the header picks the digit -- until the value is complete.
The threshold, the records above it and the tie key it reaches must be the
ones numpy's sort gives.  rank_order, join_ranked and check_k are pure
functions of heatmap_amd.top and are checked against a brute-force sort."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")
HEADER = os.path.join(REPO, "include", "heatmap_amd.h")
MAXK = 4096
SHIM = """
#include "hm_top_select.h"
void pick(const uint64_t* hist, int nbins, uint64_t want, int descending, uint64_t* out)
{
    const HmTopPick p = hm_top_pick(hist, nbins, want, descending);
    out[0] = p.digit, out[1] = p.beyond, out[2] = p.want, out[3] = p.size;
}
void walk_begin(uint64_t vor, uint64_t vand, uint64_t want, HmTopWalk* w) { *w = hm_top_walk_begin(vor, vand, want); }
uint64_t walk_step(HmTopWalk* w, const uint64_t* hist, int descending) { return hm_top_walk_step(w, hist, descending); }
uint64_t walk_mask(int shift) { return hm_top_mask(shift); }
int digit_bits(void) { return HM_TOP_DIGIT_BITS; }
int bins(void) { return HM_TOP_BINS; }
"""


class Walk(ctypes.Structure):
    _fields_ = [("prefix", ctypes.c_uint64), ("want", ctypes.c_uint64), ("beyond", ctypes.c_uint64),
                ("diff", ctypes.c_uint64), ("base", ctypes.c_uint64), ("shift", ctypes.c_int32), ("pad", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("top_select")
    src, lib = d / "shim.c", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                    str(src), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.pick.argtypes = [u64p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, u64p]
    L.pick.restype = None
    L.walk_begin.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(Walk)]
    L.walk_begin.restype = None
    L.walk_step.argtypes = [ctypes.POINTER(Walk), u64p, ctypes.c_int]
    L.walk_step.restype = ctypes.c_uint64
    L.walk_mask.argtypes = [ctypes.c_int]
    L.walk_mask.restype = ctypes.c_uint64
    return L


def walk(shim, v, want, descending):
    """(value, records ranking before it, records equal to it, rank left among
    those, passes): the walk over the u64 array v to the record of rank want"""
    u64p = ctypes.POINTER(ctypes.c_uint64)
    v = np.ascontiguousarray(v, dtype=np.uint64)
    w = Walk()
    shim.walk_begin(int(np.bitwise_or.reduce(v)), int(np.bitwise_and.reduce(v)), want, ctypes.byref(w))
    size, passes = len(v), 0
    while w.shift >= 0:
        assert passes < 8
        mask = np.uint64(shim.walk_mask(w.shift))
        live = v[(v & mask) == np.uint64(w.prefix)]
        hist = np.bincount(((live >> np.uint64(w.shift)) & np.uint64(shim.bins() - 1)).astype(np.int64),
                           minlength=shim.bins()).astype(np.uint64)
        size = shim.walk_step(ctypes.byref(w), hist.ctypes.data_as(u64p), int(descending))
        passes += 1
    return w.prefix, w.beyond, size, w.want, passes


def select(shim, keys, counts, k):
    """(T, records above T, tie key or None, passes): the whole selection of
    the first k of n > k records, as the kernels chain the two walks"""
    t, above, ties, need, p1 = walk(shim, counts, k, True)
    if ties <= need:
        return t, above, None, p1
    tk, _, one, left, p2 = walk(shim, keys[counts == np.uint64(t)], need, False)
    assert one == 1 and left == 1      # distinct keys: the walk ends on one record
    return t, above, tk, p1 + p2


def expect(keys, counts, k):
    order = np.lexsort((keys, ~counts))
    t = counts[order[k - 1]]
    above = int((counts > t).sum())
    ties = int((counts == t).sum())
    return int(t), above, (int(keys[order[k - 1]]) if ties > k - above else None)


def patterns(n, rng):
    u = lambda lo, hi: rng.integers(lo, hi, n, dtype=np.uint64, endpoint=True)
    yield "random", u(0, 2 ** 64 - 1)
    yield "high", u(2 ** 63, 2 ** 64 - 1)
    yield "equal", np.full(n, 0x8000000000000123, dtype=np.uint64)
    yield "zero", np.zeros(n, dtype=np.uint64)
    yield "small", u(1, 5)
    yield "top byte", (u(0, 255) << np.uint64(56)) | np.uint64(0x00AB00CD00EF0011)
    yield "bottom byte", u(0, 255) | np.uint64(0xF0AB00CD00EF0000)


def test_digit_geometry(shim):
    assert shim.digit_bits() == 8 and shim.bins() == 256
    assert shim.walk_mask(56) == 0 and shim.walk_mask(48) == 0xFF00000000000000 and shim.walk_mask(0) == 2 ** 64 - 256


def test_pick_against_a_scan(shim):
    rng = np.random.default_rng(5)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    for nb in (1, 2, 16, 256):
        for _ in range(20):
            hist = (rng.integers(0, 4, nb) * rng.integers(0, 1000, nb)).astype(np.uint64)
            if not hist.sum():
                hist[rng.integers(0, nb)] = 3
            for desc in (0, 1):
                walked = hist[::-1] if desc else hist
                cum = np.cumsum(walked)
                for want in {1, int(hist.sum()), int(rng.integers(1, int(hist.sum()) + 1))}:
                    out = (ctypes.c_uint64 * 4)()
                    shim.pick(hist.ctypes.data_as(u64p), nb, want, desc, out)
                    j = int(np.searchsorted(cum, want))                  # first bin with cum >= want
                    d = nb - 1 - j if desc else j
                    before = int(cum[j] - walked[j])
                    assert list(out) == [d, before, want - before, int(walked[j])]


@pytest.mark.parametrize("n", [1, 2, 65, 100000])
def test_walks_against_numpy(shim, n):
    rng = np.random.default_rng(n)
    for name, v in patterns(n, rng):
        for want in sorted({1, n, (n + 1) // 2, min(n, 100)}):
            for desc in (True, False):
                s = np.sort(v)[::-1] if desc else np.sort(v)
                t = s[want - 1]
                value, before, same, left, passes = walk(shim, v, want, desc)
                assert value == int(t), (name, want, desc)
                assert before == int((v > t).sum() if desc else (v < t).sum()), (name, want, desc)
                assert same == int((v == t).sum()) and left == want - before, (name, want, desc)
                # shared leading bits cost no pass: equal values none, one differing byte one
                if name in ("equal", "zero"):
                    assert passes == 0
                if name in ("top byte", "bottom byte", "small"):
                    assert passes <= 1


@pytest.mark.parametrize("n", [2, 65, 100000])
def test_selection_against_numpy(shim, n):
    rng = np.random.default_rng(1000 + n)
    keys = rng.permutation(np.unique(rng.integers(0, 2 ** 64 - 1, 2 * n, dtype=np.uint64, endpoint=True))[:n])
    assert len(keys) == n
    for name, counts in patterns(n, rng):
        for k in sorted({1, 2, 64, 100, n - 1} & set(range(1, n))):
            t, above, tk, passes = select(shim, keys, counts, k)
            assert (t, above, tk) == expect(keys, counts, k), (name, k)
            assert passes <= 16
            take = (counts > np.uint64(t)) | ((counts == np.uint64(t)) & (keys <= np.uint64(2 ** 64 - 1 if tk is None else tk)))
            assert int(take.sum()) == k, (name, k)


# ------------------------------------------------------------ the pure host

def brute(recs, k):
    """recs: (zoom, row, col, count) tuples of Python ints"""
    return sorted(recs, key=lambda t: (-t[3], t[0], t[1], t[2]))[:k]


def test_rank_order_is_count_descending_then_key():
    from heatmap_amd import top

    rng = np.random.default_rng(3)
    keys = rng.permutation(np.unique(rng.integers(0, 2 ** 64 - 1, 600, dtype=np.uint64, endpoint=True))[:500])
    for counts in (rng.integers(0, 4, 500).astype(np.uint64), rng.integers(2 ** 63, 2 ** 64 - 1, 500, dtype=np.uint64),
                   np.zeros(500, np.uint64)):
        want = sorted(range(500), key=lambda i: (-int(counts[i]), int(keys[i])))
        assert top.rank_order(keys, counts).tolist() == want
        # signed views of the same bits (what the CUDA tensors hold) rank the same
        assert top.rank_order(keys.view(np.int64), counts.view(np.int64)).tolist() == want
    assert top.rank_order([], []).tolist() == []
    with pytest.raises(ValueError):
        top.rank_order([1, 2], [1])


def test_join_ranked_with_side_records():
    from heatmap_amd import top

    rng = np.random.default_rng(4)
    inside = {(18, int(r), int(c)): int(n) for r, c, n in zip(rng.integers(0, 1 << 18, 300), rng.integers(0, 1 << 18, 300),
                                                              rng.integers(1, 6, 300))}
    dev = brute([(*cell, n) for cell, n in inside.items()], 4096)     # the device's part: ranked already
    side = [(18, -3, 5, 4), (18, -3, -7, 4), (18, 1 << 18, 2, 5), (18, 7, -1, 1), (18, -1, 1 << 18, 9), (17, -2, 0, 5)]
    cols = lambda recs: tuple(np.array([t[j] for t in recs], dtype=np.int64) for j in range(4))
    for k in (1, 3, 10, 100, 306, 4096):
        got = top.join_ranked(*cols(dev[:k]), cols(side), k)
        assert list(zip(*(a.tolist() for a in got))) == brute(dev + side, k)
        got = top.join_ranked(*cols(dev[:k]), None, k)
        assert list(zip(*(a.tolist() for a in got))) == dev[:k]
    # negative rows and columns rank as signed integers, before row 0 of their zoom and after a smaller zoom
    got = top.join_ranked(*cols([(18, 0, 0, 5)]), cols(side), 10)
    assert list(zip(*(a.tolist() for a in got)))[:4] == [(18, -1, 1 << 18, 9), (17, -2, 0, 5), (18, 0, 0, 5),
                                                         (18, 1 << 18, 2, 5)]
    empty = top.join_ranked([], [], [], [], None, 5)
    assert all(len(a) == 0 for a in empty)


def test_check_k():
    from heatmap_amd import _lib, top

    assert top.check_k(1) == 1 and top.check_k(np.int64(MAXK)) == MAXK
    for bad in (0, -1, MAXK + 1, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            top.check_k(bad)
    with pytest.raises(ValueError, match=r"view\(\)"):
        top.check_k(MAXK + 1)
    assert _lib.HM_TOP_MAX_K == MAXK


# ------------------------------------------------------------------ the ABI

NEW = ("hm_cells_top", "hm_stream_top", "hm_stream_top_groups")


def test_the_three_names_are_declared_exported_and_listed():
    from heatmap_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    L = _lib.load()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in exported and name in _lib.EXPORTS
        assert getattr(L, name).argtypes
    m = re.search(r"^#define HM_TOP_MAX_K (\d+)$", src, flags=re.M)
    assert m and int(m.group(1)) == _lib.HM_TOP_MAX_K == MAXK
    assert re.search(r"^#define HM_ABI_VERSION 7$", src, flags=re.M)
    import heatmap_amd.build as build
    assert "hm_top.hip" in build.SOURCES


def test_null_handles_answer_e_arg():
    """before any device call: so also on a machine without a GPU"""
    from heatmap_amd import _lib

    L = _lib.load()
    k64 = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    c64 = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    g32 = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    n, m = ctypes.c_int64(77), ctypes.c_int64(78)
    pk, pc, pg = (ctypes.cast(o, ctypes.c_void_p) for o in (k64, c64, g32))
    rect = (ctypes.c_int64 * 5)(3, 0, 8, 0, 8)
    assert L.hm_cells_top(None, pk, pc, 4, 2, pk, pc, ctypes.byref(n)) == _lib.HM_E_ARG
    assert L.hm_cells_top(None, None, None, 0, 2, None, None, ctypes.byref(n)) == _lib.HM_E_ARG
    for lo, hi in ((-1, -1), (0, 5)):
        for k in (1, MAXK, 0, MAXK + 1):
            assert L.hm_stream_top(None, lo, hi, _lib.HM_VIEW_MERGED, rect, 1, k, pk, pc, ctypes.byref(n),
                                   ctypes.byref(m)) == _lib.HM_E_ARG
            assert L.hm_stream_top_groups(None, lo, hi, rect, 1, k, pg, pc, ctypes.byref(n),
                                          ctypes.byref(m)) == _lib.HM_E_ARG
    assert list(k64) == [7] * 4 and list(c64) == [7] * 4 and list(g32) == [7] * 4
    assert (n.value, m.value) == (77, 78)


def test_python_argument_checks_need_no_device():
    from heatmap_amd import stream

    s = object.__new__(stream.StreamingHeatmap)      # no device: only the validation paths run
    s.zmin, s.zmax, s._index, s.labels, s._explicit_max = 0, 18, {"all": 0, "u1": 1}, ["all", "u1"], 5
    with pytest.raises(ValueError, match="label per group"):
        s.top_users(3, [(14, 0, 4, 0, 4)])
    with pytest.raises(ValueError, match="zoom 19"):
        s.top_tiles(3, 19)
    with pytest.raises(ValueError, match="within"):
        s.top_tiles(3, 14, within=[])
    with pytest.raises(ValueError, match="not a tile"):
        s.top_tiles(3, 14, within=[(15, 0, 0)])
    with pytest.raises(ValueError, match="user='all'"):
        s.top_tiles(3, 14, user="all")
    with pytest.raises(ValueError, match=r"view\(\)"):
        s.top_tiles(MAXK + 1, 14)
    assert s.top_tiles(3, 14, user="nobody") == []
