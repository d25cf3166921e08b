"""The host side of distinct visitors (hm_stream_visitors;
StreamingHeatmap.visitors / top_visited / tile_visitors, tile_raster with
min_users) on the CPU.

_visitor_records is the pure function that gives the out-of-square side
records their per-cell visitors and the threshold: it is checked against a
brute-force dict of group sets.  csrc/hm_visit.h is plain C and is the
threshold, withheld and table-size arithmetic the kernels run: a shim around it
is built with the host compiler and compared with the same arithmetic in
Python.  The argument checks that need no device are pure functions too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from heatmap_amd import stream as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")
SHIM = """
#include "hm_visit.h"
int keeps(uint32_t visitors, uint64_t min_visitors) { return hm_visit_keeps(visitors, min_visitors); }
uint64_t slots(uint64_t nd) { return hm_visit_slots(nd); }
/* n folded cells judged in turn: out = emitted cells, withheld cells, withheld points */
void sweep(const uint32_t* visitors, const uint64_t* points, int64_t n, uint64_t min_visitors, uint64_t* out)
{
    HmVisitWithheld w = {0, 0};
    uint64_t emitted = 0;
    for (int64_t i = 0; i < n; i++) emitted += (uint64_t)hm_visit_judge(&w, visitors[i], points[i], min_visitors);
    out[0] = emitted, out[1] = w.cells, out[2] = w.points;
}
"""


# ------------------------------------------------------------ _visitor_records

def _brute(x, rects, hours, m):
    """{(zoom, row, col): (points, visitors)} by sets of groups"""
    groups, points = {}, {}
    for g, h, z, r, c, n in x.tolist():
        if not any(z == rz and rlo <= r < rhi and clo <= c < chi for rz, rlo, rhi, clo, chi in rects):
            continue
        if hours is not None and (h == S.UNDATED_HOUR or not hours[0] <= h < hours[1]):
            continue
        groups.setdefault((z, r, c), set()).add(g)
        points[(z, r, c)] = points.get((z, r, c), 0) + n
    return {k: (points[k], len(v)) for k, v in groups.items() if len(v) >= m}


def _as_dict(rec):
    assert rec.dtype == np.int64 and rec.ndim == 2 and rec.shape[1] == 5
    out = {(z, r, c): (p, v) for z, r, c, p, v in rec.tolist()}
    assert len(out) == len(rec)                          # distinct cells
    return out


def _side_records(seed, n=3000):
    """random out-of-square records: few cells, many groups and hours, some
    undated, some without a group, repeated (group, hour, cell) rows"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 12, n)
    g[rng.random(n) < 0.15] = S.NOGROUP
    h = 480000 + rng.integers(0, 10, n)
    h[rng.random(n) < 0.2] = S.UNDATED_HOUR
    z = rng.integers(17, 19, n)
    r = -rng.integers(1, 9, n)                           # above the square
    c = rng.integers(-3, 6, n)
    cnt = rng.integers(1, 1 << 33, n)
    return np.stack([g, h, z, r, c, cnt], axis=1).astype(np.int64)


RECTS = {"one": [(18, -8, 0, -3, 6)],
         "overlapping": [(18, -6, -1, -2, 4), (18, -4, 0, 0, 6)],
         "two zooms": [(17, -8, -2, -3, 2), (18, -3, 0, 1, 6)],
         "misses": [(16, -8, 0, -3, 6), (18, 0, 8, 0, 6)]}
HOURS = [None, (480002, 480005), (479000, 480001), (480009, 490000), (481000, 482000)]


@pytest.mark.parametrize("name", sorted(RECTS))
def test_visitor_records_against_group_sets(name):
    x = _side_records(5)
    rects = RECTS[name]
    seen = set()
    for hours in HOURS:
        every = _brute(x, rects, hours, 1)
        vmax = max((v for _, v in every.values()), default=0)
        for m in sorted({1, max(1, vmax // 2), max(1, vmax), vmax + 1}):
            got = _as_dict(S._visitor_records(x, rects, hours, m))
            assert got == _brute(x, rects, hours, m), (name, hours, m)
            seen.add("some" if got else "none")
        assert not _as_dict(S._visitor_records(x, rects, hours, vmax + 1))
    assert seen == ({"none"} if name == "misses" else {"some", "none"})


def test_visitor_records_rules():
    G, U = S.NOGROUP, S.UNDATED_HOUR
    x = np.array([[1, 10, 18, -1, 3, 2],                 # group 1, twice in the window and once outside it
                  [1, 11, 18, -1, 3, 5],
                  [1, 20, 18, -1, 3, 100],
                  [2, 20, 18, -1, 3, 7],                 # group 2: only outside the window
                  [G, 10, 18, -1, 3, 1],                 # the records without a group: one visitor together
                  [G, 11, 18, -1, 3, 1],
                  [3, U, 18, -1, 3, 1000],               # undated: alltime only
                  [4, 10, 18, -2, 3, 9]], dtype=np.int64)
    rect = [(18, -4, 0, 0, 8)]
    assert _as_dict(S._visitor_records(x, rect, (10, 12), 1)) == {(18, -1, 3): (9, 2), (18, -2, 3): (9, 1)}
    assert _as_dict(S._visitor_records(x, rect, (10, 12), 2)) == {(18, -1, 3): (9, 2)}
    assert _as_dict(S._visitor_records(x, rect, (10, 12), 3)) == {}
    assert _as_dict(S._visitor_records(x, rect, None, 1)) == {(18, -1, 3): (1116, 4), (18, -2, 3): (9, 1)}
    assert _as_dict(S._visitor_records(x, rect, None, 4)) == {(18, -1, 3): (1116, 4)}
    assert _as_dict(S._visitor_records(x, rect + rect, None, 4)) == {(18, -1, 3): (1116, 4)}   # a cell twice: once
    empty = S._visitor_records(np.zeros((0, 6), np.int64), rect, None, 1)
    assert empty.shape == (0, 5) and empty.dtype == np.int64


# ------------------------------------------------------------ argument checks

def test_threshold_arguments():
    assert S._check_min_visitors(1) == 1 and S._check_min_visitors(np.int64(7)) == 7
    for bad in (0, -1, 1.0, "2", None, True):
        with pytest.raises(ValueError):
            S._check_min_visitors(bad)
    assert S._min_users_arg(None, None) is None and S._min_users_arg(None, "u1") is None
    assert S._min_users_arg(5, None) == 5
    with pytest.raises(ValueError, match="k-anonymous"):
        S._min_users_arg(5, "u1")
    for bad in (0, -2, 2.5, False):
        with pytest.raises(ValueError, match="min_users"):
            S._min_users_arg(bad, None)


def test_haloed_rects():
    assert S._haloed_rects([(3, 2, 5)], 4, 0) == S.tile_rects([(3, 2, 5)], 4)
    assert S._haloed_rects([(0, 0, 0), (3, 2, 5)], 3, 2) == [(3, -2, 10, -2, 10), (6, 14, 26, 38, 50)]


# ------------------------------------------------------------ hm_visit.h

@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("visit")
    src, lib = d / "shim.c", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                    str(src), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    L.keeps.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    L.slots.argtypes = [ctypes.c_uint64]
    L.slots.restype = ctypes.c_uint64
    L.sweep.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64,
                        ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.sweep.restype = None
    return L


def test_header_threshold(shim):
    for v, m, want in ((1, 1, 1), (1, 2, 0), (5, 5, 1), (4, 5, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1),
                       (0xFFFFFFFF, 1 << 32, 0), (7, (1 << 32) + 3, 0), (3, (1 << 63) - 1, 0)):
        assert shim.keeps(v, m) == want, (v, m)          # the threshold is compared in 64 bits, never truncated


def test_header_sweep_sums_in_64_bits(shim):
    rng = np.random.default_rng(11)
    vis = rng.integers(1, 9, 5000).astype(np.uint32)
    pts = rng.integers(1, 1 << 41, 5000).astype(np.uint64)
    pts[:2] = 1 << 40
    out = (ctypes.c_uint64 * 3)()
    for m in (1, 2, 5, 8, 9, 1 << 40):
        shim.sweep(vis.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                   pts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(vis), m, out)
        low = vis.astype(np.uint64) < np.uint64(m)
        assert list(out) == [int((~low).sum()), int(low.sum()), sum(int(p) for p in pts[low])], m
    assert sum(int(p) for p in pts) > 1 << 52            # far beyond what 32 bits hold


def test_header_table_size(shim):
    for nd in (0, 1, 511, 512, 513, 1023, 1024, 1025, 4096, 4097, 99999, (1 << 30) + 1):
        s = shim.slots(nd)
        assert s >= 1024 and s & (s - 1) == 0 and s >= 2 * nd
        assert s == 1024 or s < 4 * nd                   # and no larger than needed
