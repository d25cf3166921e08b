"""CPU: the host side of the stream's viewport and tile queries -- the selection
of the out-of-square side records (stream._view_records) and the tile ->
rectangle map (stream.tile_rects) against brute-force loops, and the argument
check of hm_stream_view that needs no GPU."""
import os
import subprocess
import sys

import numpy as np

from heatmap_amd.stream import ALLGROUPS, NOGROUP, UNDATED_HOUR, _view_records, tile_rects

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H0 = 480000


def _records(seed=4, n=600):
    """(group, hour or UNDATED_HOUR, zoom, row, col, count) records around the
    edges of the square: rows -3..0 and columns 2^z - 1 .. 2^z + 2, few distinct
    cells, so several hours and groups share one."""
    rng = np.random.default_rng(seed)
    g = rng.choice([1, 2, 3, NOGROUP], n)
    h = np.where(rng.random(n) < 0.2, UNDATED_HOUR, H0 + rng.integers(0, 8, n))
    z = rng.integers(0, 4, n)
    r = rng.integers(-3, 1, n)
    c = (1 << z) - 1 + rng.integers(0, 4, n)
    cnt = rng.integers(1, 50, n)
    rec = np.stack([g, h, z, r, c, cnt], axis=1).astype(np.int64)
    u, inv = np.unique(rec[:, :5], axis=0, return_inverse=True)
    tot = np.zeros(len(u), np.int64)
    np.add.at(tot, inv.reshape(-1), rec[:, 5])
    return np.concatenate([u, tot[:, None]], axis=1)


def _brute(x, rects, hours, group):
    out = {}
    for g, h, z, r, c, n in x.tolist():
        if not any(z == rz and rlo <= r < rhi and clo <= c < chi for rz, rlo, rhi, clo, chi in rects):
            continue
        if hours is not None and (h == UNDATED_HOUR or not (hours[0] <= h < hours[1])):
            continue
        if group not in ("merged", "each") and g != group:
            continue
        k = (ALLGROUPS if group == "merged" else g, z, r, c)
        out[k] = out.get(k, 0) + n
    return out


def _as_dict(rec):
    d = {tuple(row[:4]): row[4] for row in rec.tolist()}
    assert len(d) == len(rec)       # summed: one record per (group, cell)
    return d


RECTS = [
    [(2, -3, 1, 3, 7)],                                    # all of zoom 2's records: reaches outside the square
    [(3, -1, 0, 8, 9)],                                    # one cell outside
    [(1, -2, 0, 1, 3), (1, -3, -1, 2, 4), (3, -3, 1, 7, 9)],   # overlapping rectangles of one zoom, and another zoom
    [(0, 0, 1, 0, 1), (2, 0, 4, 0, 4)],                    # wholly inside the square (col 2^z - 1 records only)
    [(3, 5, 9, 0, 3)],                                     # no record there
]


def test_view_records_match_brute_force():
    x = _records()
    assert (x[:, 1] == UNDATED_HOUR).any() and (x[:, 0] == NOGROUP).any()
    nonempty = 0
    for rects in RECTS:
        for hours in (None, (H0, H0 + 1), (H0 + 2, H0 + 5), (H0 - 10, H0 + 100), (H0 + 8, H0 + 20), (UNDATED_HOUR, H0)):
            for group in ("merged", "each", 2, NOGROUP, 77):
                want = _brute(x, rects, hours, group)
                got = _view_records(x, rects, hours, group)
                assert got.shape[1] == 5
                assert _as_dict(got) == want, (rects, hours, group)
                nonempty += bool(want)
    assert nonempty > 40
    # a cell in two overlapping rectangles is counted once
    one = _view_records(x, [(1, -2, 0, 1, 3)], None, "merged")
    two = _view_records(x, [(1, -2, 0, 1, 3), (1, -2, 0, 1, 3), (1, -2, -1, 2, 3)], None, "merged")
    assert len(one) and np.array_equal(one, two)
    # lo is inclusive, hi exclusive
    cell = _view_records(x, [(3, -1, 0, 8, 9)], None, "merged")
    assert cell[:, 1:4].tolist() == [[3, -1, 8]]
    # undated records: in the alltime view, in no window
    und = x[x[:, 1] == UNDATED_HOUR]
    everything = [(z, -10, 10, 0, 100) for z in range(4)]
    assert _view_records(und, everything, None, "merged")[:, 4].sum() == und[:, 5].sum()
    assert len(_view_records(und, everything, (UNDATED_HOUR, H0 + 100), "merged")) == 0
    # merged == the per-group records summed
    each = _view_records(x, everything, (H0, H0 + 8), "each")
    merged = _view_records(x, everything, (H0, H0 + 8), "merged")
    assert (merged[:, 0] == ALLGROUPS).all() and merged[:, 4].sum() == each[:, 4].sum()


def test_view_records_empty():
    x = np.zeros((0, 6), np.int64)
    for group in ("merged", "each", 3):
        assert _view_records(x, [(2, 0, 4, 0, 4)], None, group).shape == (0, 5)
        assert _view_records(x, [(2, 0, 4, 0, 4)], (0, 10), group).shape == (0, 5)


def test_tile_rects_match_loop():
    rng = np.random.default_rng(9)
    for d in (1, 3, 5):
        tiles = [(int(tz), int(rng.integers(0, 1 << tz)), int(rng.integers(0, 1 << tz)))
                 for tz in rng.integers(1, 14, 50)]
        rects = tile_rects(tiles, d)
        assert len(rects) == len(tiles)
        for (tz, tr, tc), (z, rlo, rhi, clo, chi) in zip(tiles, rects):
            # the rectangle holds exactly the cells whose row tile (cell >> d) is the tile
            assert z == tz + d and rhi - rlo == 1 << d and chi - clo == 1 << d
            for r in (rlo - 1, rlo, rhi - 1, rhi):
                assert ((r >> d) == tr) == (rlo <= r < rhi)
            for c in (clo - 1, clo, chi - 1, chi):
                assert ((c >> d) == tc) == (clo <= c < chi)
    assert tile_rects([], 5) == []
    assert tile_rects([(1, 1, 0)], 5) == [(6, 32, 64, 0, 32)]


def test_null_stream_is_an_argument_error():
    """hm_stream_view(NULL, ...) answers HM_E_ARG before anything touches a
    device (a child process: the library is loaded without a GPU)."""
    code = r"""
import ctypes
from heatmap_amd import _lib
L = _lib.load()
n = ctypes.c_int64(7)
rects = (ctypes.c_int64 * 5)(3, 0, 8, 0, 8)
print("VIEW", L.hm_stream_view(None, -1, -1, -1, rects, 1, None, None, None, 0, ctypes.byref(n)))
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert "VIEW 16" in r.stdout, r.stdout + r.stderr
