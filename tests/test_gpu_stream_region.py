"""Region queries on the resident streaming heatmap (hm_stream_region_series /
_view / _visitors; StreamingHeatmap.region_totals / region_series /
region_view / region_visitors) vs the CPU model of tests/stream_model.py.

Points are tile centres (stream_model.centre), so a point's cell at every zoom
is integer arithmetic.  Region membership is taken from the mask that built
the region, or from RegionSet.cells() where a polygon built it (that path is
checked on the CPU, tests/test_region_host.py).  Every comparison is exact.

Data: a stream of zooms 0..10; 4 batches of 4000 points in a few clusters (two
of them in the corners of the square, so the first and last rows and columns
hold cells) over a thin uniform background, hours BASE .. BASE + 11 with
consecutive batches overlapping in hours, 10% dropped by keep, 24 group ids
drawn with a skew; one dated batch without ids (NOGROUP) and one undated batch
without ids.  Checked on a log that still holds repeated keys ('raw') and on a
compacted one ('compact').

The totals sink keeps its accumulators in LDS up to HMS_RG_TOT_LDS frames x
regions and reduces across the wave above; the bound is read from
csrc/hm_pipeline.h, and the cases F * R = bound and bound + 1 straddle it."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import stream_model as sm
from heatmap_amd import _lib, device
from heatmap_amd.region import RegionSet
from heatmap_amd.stream import ALLGROUPS, NOGROUP, StreamingHeatmap

pytestmark = pytest.mark.gpu
BASE = 480000
ZMIN, ZMAX = 0, 10
SIDE = 1 << ZMAX
NG = 24
ALL = (BASE, BASE + 12)
SENT = 0x5A5A5A5A5A5A5A5A
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOT_LDS = int(re.search(r"#define HMS_RG_TOT_LDS (\d+)",
                        open(os.path.join(REPO, "heatmap_amd", "csrc", "hm_pipeline.h")).read()).group(1))


# ------------------------------------------------------------------- data

def _points(rng, n):
    centres = np.array([[2, 3], [1021, 1020], [500, 500], [300, 700], [520, 480]])
    which = rng.integers(0, len(centres), n)
    p = centres[which] + np.rint(rng.normal(0, 6, (n, 2))).astype(np.int64)
    bg = rng.random(n) < 0.15
    p[bg] = rng.integers(0, SIDE, (int(bg.sum()), 2))
    p = np.clip(p, 0, SIDE - 1)
    return p[:, 0], p[:, 1]


class Data:
    def __init__(self):
        self.batches = []
        for b in range(4):
            rng = np.random.default_rng(700 + b)
            rows, cols = _points(rng, 4000)
            hour = (BASE + 2 * b + rng.integers(0, 6, 4000)).astype(np.uint32)   # 0-5, 2-7, 4-9, 6-11
            keep = (rng.random(4000) > 0.1).astype(np.uint8)
            group = np.floor(NG * rng.random(4000) ** 3).astype(np.uint32)
            self.batches.append((rows, cols, keep, hour, group))
        rng = np.random.default_rng(710)
        rows, cols = _points(rng, 1000)
        self.batches.append((rows, cols, None, (BASE + 3 + rng.integers(0, 4, 1000)).astype(np.uint32), None))
        rows, cols = _points(rng, 1000)
        self.batches.append((rows, cols, None, None, None))
        self.model = sm.StreamModel(ZMIN, ZMAX)
        for rows, cols, keep, hour, group in self.batches:
            self.model.add(rows, cols, keep, hour, group)

    def stream(self, ids=True, nbatches=None):
        s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1 << 16)
        for rows, cols, keep, hour, group in self.batches[:nbatches]:
            lat, lon = sm.centre(rows, cols, ZMAX)
            s.add(lat, lon, keep, hour, group=group if ids else None)
        return s


@pytest.fixture(scope="module")
def data(gpu):
    return Data()


@pytest.fixture(scope="module", params=["raw", "compact"])
def stream(request, data):
    s = data.stream()
    if request.param == "compact":
        s.cells()
    yield s
    s.close()


# ------------------------------------------------------------ region sets

class Reg:
    """A region set and its membership: `img` (an integer image of the whole
    square, value v > 0: region v - 1) or `stack` (bool [R, side, side])."""

    def __init__(self, rs, img=None, stack=None):
        self.rs, self.img, self.stack = rs, img, stack

    def pairs(self, rows, cols):
        """(record index, region) of every (record, region that holds its cell)"""
        if self.img is not None:
            v = self.img[rows, cols]
            i = np.flatnonzero(v > 0)
            return i, v[i] - 1
        ii, rr = [], []
        for j in range(self.stack.shape[0]):
            i = np.flatnonzero(self.stack[j, rows, cols])
            ii.append(i), rr.append(np.full(len(i), j))
        return np.concatenate(ii), np.concatenate(rr)


def _stack_reg(zoom, stack):
    return Reg(RegionSet.from_mask(zoom, 0, 0, stack), stack=stack)


def _img_reg(zoom, img):
    return Reg(RegionSet.from_mask(zoom, 0, 0, img), img=img)


def _poly_reg(zoom, regions):
    rs = RegionSet.from_tile_polygons(regions, zoom)
    stack = np.zeros((rs.nregions, 1 << zoom, 1 << zoom), dtype=bool)
    for j in range(rs.nregions):
        r, c = rs.cells(j)
        stack[j, r, c] = True
    return Reg(rs, stack=stack)


def _edge_stack():
    """zoom 10: rows 0 and 2^z - 1, spans touching column 0 and 2^z, a width-1
    span, covered rows without a span, abutting and overlapping regions"""
    st = np.zeros((3, SIDE, SIDE), dtype=bool)
    st[0, 0:3, 0:6] = True            # touches row 0 and column 0
    st[0, 0:2, SIDE - 5:SIDE] = True  # touches column 2^z
    st[0, 1, 500] = True              # width 1
    st[0, 490:515, 470:500] = True
    st[1, 490:515, 500:530] = True    # abuts region 0: col_hi == col_lo
    st[1, SIDE - 4:SIDE, SIDE - 8:SIDE] = True   # the last rows and columns
    st[2, 480:505, 485:510] = True    # overlaps both
    st[2, 0:1, 0:SIDE] = True         # a whole row
    return st


def _mid_stack():
    """zoom 5: a region with a hole, one abutting it, one overlapping both"""
    st = np.zeros((3, 32, 32), dtype=bool)
    st[0, 10:22, 8:20] = True
    st[0, 13:18, 11:16] = False       # the hole
    st[1, 12:20, 20:27] = True
    st[2, 14:17, 0:32] = True
    return st


def _grid_img(nregions):
    """zoom 10: 16 x 16 blocks numbered row-major, the numbers capped at nregions"""
    ids = np.arange(SIDE)[:, None] // 16 * 64 + np.arange(SIDE)[None] // 16
    return np.minimum(ids, nregions - 1) + 1


REGS = {}


def reg(name):
    if name not in REGS:
        REGS[name] = {
            "z0": lambda: _stack_reg(0, np.ones((1, 1, 1), dtype=bool)),
            "edge": lambda: _stack_reg(ZMAX, _edge_stack()),
            "mid": lambda: _stack_reg(5, _mid_stack()),
            "checker": lambda: _stack_reg(6, (np.indices((64, 64)).sum(0) % 2 == 0)[None]),
            "grid4096": lambda: _img_reg(ZMAX, _grid_img(_lib.HM_REGION_MAX_REGIONS)),
            "at_bound": lambda: _img_reg(ZMAX, _grid_img(TOT_LDS)),
            "over_bound": lambda: _img_reg(ZMAX, _grid_img(TOT_LDS + 1)),
            "poly": lambda: _poly_reg(8, [[np.array([[100.3, 110.2], [160.9, 118.4], [150.2, 170.7], [120.5, 140.1],
                                                      [95.6, 165.3]]),
                                           np.array([[120.0, 120.0], [135.0, 120.0], [135.0, 132.0], [120.0, 132.0]])],
                                          [np.array([[-5.0, -5.0], [20.5, -3.0], [14.2, 30.8]]),
                                           np.array([[240.0, 250.0], [258.0, 251.0], [250.0, 259.0]])]]),
        }[name]()
    return REGS[name]


# ------------------------------------------------------------------ model

def _select(model, zoom, hours, group):
    """the model's records (group, hour, zoom, row, col, count) of one zoom, of the hours and the group"""
    rec = model.rec[model.rec[:, 2] == zoom]
    if hours is not None:
        h = rec[:, 1]
        rec = rec[(h != sm.UNDATED_HOUR) & (h >= hours[0]) & (h < hours[1])]
    if group is not None:
        rec = rec[rec[:, 0] == group]
    return rec


def want_series(model, rg, lo, hi, fh, group=None):
    nf = -((lo - hi) // fh)
    out = np.zeros((nf, rg.rs.nregions), dtype=np.int64)
    rec = _select(model, rg.rs.zoom, (lo, hi), group)
    i, r = rg.pairs(rec[:, 3], rec[:, 4])
    np.add.at(out, ((rec[i, 1] - lo) // fh, r), rec[i, 5])
    return out


def want_totals(model, rg, hours=None, group=None):
    out = np.zeros(rg.rs.nregions, dtype=np.int64)
    rec = _select(model, rg.rs.zoom, hours, group)
    i, r = rg.pairs(rec[:, 3], rec[:, 4])
    np.add.at(out, r, rec[i, 5])
    return out


def want_view(model, rg, hours, group):
    """sorted (group, zoom, row, col, count) records of a region view"""
    rec = _select(model, rg.rs.zoom, hours, None if group in ("merged", "each") else int(group))
    i, _ = rg.pairs(rec[:, 3], rec[:, 4])
    rec = rec[np.unique(i)][:, [0, 2, 3, 4, 5]]
    if group == "merged":
        rec[:, 0] = ALLGROUPS
    return sm.sum_records(rec)


def want_visitors(model, rg, hours, m):
    R = rg.rs.nregions
    rec = _select(model, rg.rs.zoom, hours, None)
    i, r = rg.pairs(rec[:, 3], rec[:, 4])
    pts = np.zeros(R, dtype=np.int64)
    np.add.at(pts, r, rec[i, 5])
    pairs = np.unique(np.stack([r, rec[i, 0]], axis=1), axis=0)
    vis = np.bincount(pairs[:, 0], minlength=R).astype(np.int64)
    low = (vis >= 1) & (vis < m)
    wr, wp = int(low.sum()), int(pts[low].sum())
    pts[vis < m] = 0
    vis[vis < m] = 0
    return pts, vis, wr, wp


def got_view(s, rs, hours, group):
    g, z, r, c, n = s.region_view(rs, hours, group)
    return sm.sort_records(np.stack([g.astype(np.int64), z.astype(np.int64), r, c, n], axis=1))


def raw_series(s, rs, lo, hi, fh, gw, frames):
    """hm_stream_region_series itself: any group word, a sentinel behind the output"""
    import torch

    st, keep = s._region_table(rs)
    out = torch.full((frames * rs.nregions + 4,), SENT, dtype=torch.int64, device="cuda")
    rc = s.ctx.L.hm_stream_region_series(s.ptr, lo, hi, fh, gw, ctypes.byref(st), device._ptr(out))
    o = out.cpu().numpy()
    assert (o[frames * rs.nregions:] == SENT).all()
    return rc, o[:frames * rs.nregions].reshape(frames, rs.nregions)


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("name", ["z0", "edge", "mid", "checker", "poly", "grid4096", "at_bound", "over_bound"])
def test_totals(stream, data, name):
    """alltime (undated batch included) and a window (excluded), every shape:
    zoom zmin, zmax and between; R = 1, 3, the LDS bound, bound + 1 and the
    most regions a set holds"""
    rg = reg(name)
    assert rg.rs.nregions in (1, 2, 3, TOT_LDS, TOT_LDS + 1, _lib.HM_REGION_MAX_REGIONS)
    got = stream.region_totals(rg.rs).cpu().numpy()
    want = want_totals(data.model, rg)
    assert want.sum() > 0 and np.array_equal(got, want)
    win = (BASE + 2, BASE + 9)
    got = stream.region_totals(rg.rs, win).cpu().numpy()
    want_w = want_totals(data.model, rg, win)
    assert np.array_equal(got, want_w) and want_w.sum() < want.sum()
    assert np.array_equal(stream.region_series(rg.rs, win, 3).sum(0).cpu().numpy(), want_w)


def test_shapes_the_edge_set_is_built_for():
    rs = reg("edge").rs
    assert rs.row_lo == 0 and rs.nrows == SIDE and rs.col_lo.min() == 0 and rs.col_hi.max() == SIDE
    assert ((rs.col_hi - rs.col_lo) == 1).any() and (np.diff(rs.row_ptr.astype(np.int64)) == 0).any()
    rows = rs.rows()
    m = rows == 495
    assert rs.col_hi[m][rs.region[m] == 0][0] == rs.col_lo[m][rs.region[m] == 1][0] == 500   # abutting
    assert np.diff(reg("checker").rs.row_ptr.astype(np.int64)).tolist() == [32] * 64
    assert reg("at_bound").rs.nregions == TOT_LDS and reg("over_bound").rs.nregions == TOT_LDS + 1


@pytest.mark.parametrize("fh", [1, 5, 12])
def test_series_frames(stream, data, fh):
    """F * R = 36, 9 and 3 on the three-region sets; 12 x 4096 far above the LDS bound"""
    for name in ("edge", "mid"):
        rg = reg(name)
        got = stream.region_series(rg.rs, ALL, fh).cpu().numpy()
        assert got.shape == (math.ceil(12 / fh), 3)
        assert np.array_equal(got, want_series(data.model, rg, *ALL, fh))
    rg = reg("grid4096")
    assert np.array_equal(stream.region_series(rg.rs, ALL, fh).cpu().numpy(), want_series(data.model, rg, *ALL, fh))


def test_series_windows_around_the_base(stream, data):
    rg = reg("mid")
    for lo, hi, fh in [(BASE - 7, BASE + 5, 5), (BASE - 7, BASE + 5, 1), (BASE + 9, BASE + 40, 7), (BASE - 3, BASE + 30, 12)]:
        got = stream.region_series(rg.rs, (lo, hi), fh).cpu().numpy()
        assert np.array_equal(got, want_series(data.model, rg, lo, hi, fh)), (lo, hi, fh)
    got = stream.region_series(rg.rs, (BASE - 20, BASE - 10), 3).cpu().numpy()       # wholly before the stream
    assert got.shape == (4, 3) and not got.any()
    assert not stream.region_totals(rg.rs, (BASE + 12, BASE + 20)).cpu().numpy().any()   # wholly after the data


def test_series_groups(stream, data):
    """merged, one id, NOGROUP, an id never seen; HM_VIEW_EACH is refused"""
    for name in ("edge", "over_bound"):
        rg = reg(name)
        for gw, group in ((_lib.HM_VIEW_MERGED, None), (0, 0), (7, 7), (NOGROUP, NOGROUP), (1000, 1000)):
            rc, got = raw_series(stream, rg.rs, *ALL, 4, gw, 3)
            assert rc == _lib.HM_OK
            want = want_series(data.model, rg, *ALL, 4, group)
            assert np.array_equal(got, want), (name, gw)
            assert want.any() == (gw != 1000)
            rc, got = raw_series(stream, rg.rs, _lib.HM_STREAM_ALLTIME, _lib.HM_STREAM_ALLTIME, 1, gw, 1)
            assert rc == _lib.HM_OK and np.array_equal(got[0], want_totals(data.model, rg, None, group))
    rs = reg("mid").rs
    assert raw_series(stream, rs, *ALL, 4, _lib.HM_VIEW_EACH, 3)[0] == _lib.HM_E_ARG
    assert raw_series(stream, rs, BASE + 5, BASE + 5, 1, _lib.HM_VIEW_MERGED, 1)[0] == _lib.HM_E_ARG
    assert raw_series(stream, rs, *ALL, 0, _lib.HM_VIEW_MERGED, 1)[0] == _lib.HM_E_ARG
    rc, got = raw_series(stream, rs, _lib.HM_STREAM_ALLTIME, _lib.HM_STREAM_ALLTIME, 0, _lib.HM_VIEW_MERGED, 1)
    assert rc == _lib.HM_OK and np.array_equal(got[0], want_totals(data.model, reg("mid")))   # frame_hours not read


def test_user_labels(data):
    """user= is a label as in tile_raster: a label never seen gives zeros, 'all' is refused"""
    rows, cols, keep, hour, group = data.batches[0]
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1 << 16)
    s.add(*sm.centre(rows, cols, ZMAX), keep, hour, user_id=["u%d" % g for g in group])
    m = sm.StreamModel(ZMIN, ZMAX)
    m.add(rows, cols, keep, hour, np.array([s._index.get("u%d" % g, -5) for g in group]))
    rg = reg("edge")
    for label in ("u0", "u3"):
        gid = s._index[label]
        assert np.array_equal(s.region_series(rg.rs, ALL, 5, user=label).cpu().numpy(),
                              want_series(m, rg, *ALL, 5, gid))
        assert np.array_equal(s.region_totals(rg.rs, user=label).cpu().numpy(), want_totals(m, rg, None, gid))
    assert not s.region_series(rg.rs, ALL, 5, user="nobody").cpu().numpy().any()
    assert not s.region_totals(rg.rs, user="nobody").cpu().numpy().any()
    with pytest.raises(ValueError, match="'all'"):
        s.region_totals(rg.rs, user="all")
    with pytest.raises(ValueError, match="alltime has no first frame"):
        s.region_series(rg.rs, None)
    with pytest.raises(ValueError, match="zoom"):
        s.region_totals(RegionSet.from_rects([(11, 0, 1, 0, 1)]))
    s.close()


@pytest.mark.parametrize("name", ["edge", "mid", "poly", "z0"])
def test_view_is_the_models_cells(stream, data, name):
    rg = reg(name)
    for hours in (None, (BASE + 2, BASE + 9)):
        for group in ("merged", "each", 2, NOGROUP):
            got = got_view(stream, rg.rs, hours, group)
            want = want_view(data.model, rg, hours, group)
            assert len(want) and np.array_equal(got, want), (name, hours, group, len(got), len(want))
    c = stream.region_counts(rg.rs)
    want = want_view(data.model, rg, None, "merged")
    got = sm.sort_records(np.stack([np.asarray(x).astype(np.int64) for x in (c.zoom, c.row, c.col, c.count)], axis=1))
    assert np.array_equal(got, want[:, 1:])


def test_view_capacity_and_sentinels(stream, data):
    import torch

    rg = reg("edge")
    want = want_view(data.model, rg, None, "each")
    n = len(want)
    st, keep = stream._region_table(rg.rs)

    def call(cap):
        k, c = (torch.full((n + 8,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        g = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        no = ctypes.c_int64(-1)
        rc = stream.ctx.L.hm_stream_region_view(stream.ptr, _lib.HM_STREAM_ALLTIME, _lib.HM_STREAM_ALLTIME,
                                                _lib.HM_VIEW_EACH, ctypes.byref(st), device._ptr(k), device._ptr(c),
                                                device._ptr(g), cap, ctypes.byref(no))
        return rc, no.value, k.cpu().numpy(), c.cpu().numpy(), g.cpu().numpy()

    rc, m, k, c, g = call(n + 8)
    assert (rc, m) == (_lib.HM_OK, n)
    assert (k[n:] == SENT).all() and (c[n:] == SENT).all() and (g[n:] == 0x5A5A5A5A).all()
    z, r, q = device.decode_keys(k[:n].view(np.uint64))
    got = sm.sort_records(np.stack([g[:n].view(np.uint32).astype(np.int64), z.astype(np.int64), r, q, c[:n]], axis=1))
    assert np.array_equal(got, want)
    rc, m, k, c, g = call(n - 1)
    assert (rc, m) == (_lib.HM_E_CAPACITY, n)
    rc, m, k, c, g = call(n)
    assert (rc, m) == (_lib.HM_OK, n) and (k[n:] == SENT).all()


def test_view_of_rectangles_is_view(stream):
    for rects in ([(ZMAX, 480, 520, 470, 530)], [(5, 0, 32, 0, 32)], [(ZMAX, -3, 9, -3, 12), (ZMAX, 1015, 1030, 1000, 1030)],
                  [(0, 0, 1, 0, 1)]):
        rs = RegionSet.from_rects(rects)
        for hours, group in ((None, "merged"), ((BASE + 1, BASE + 8), "each"), (None, 3)):
            a = sm.sort_records(np.stack([np.asarray(x).astype(np.int64) for x in stream.view(rects, hours, group)], axis=1))
            b = got_view(stream, rs, hours, group)
            assert len(a) and np.array_equal(a, b), (rects, hours, group)


@pytest.mark.parametrize("m", [1, 3, 25])
def test_visitors(stream, data, m):
    for name in ("edge", "mid", "grid4096"):
        rg = reg(name)
        for hours in (None, (BASE + 2, BASE + 9)):
            pts, vis, wr, wp = stream.region_visitors(rg.rs, hours, m)
            want = want_visitors(data.model, rg, hours, m)
            assert np.array_equal(pts, want[0]) and np.array_equal(vis, want[1]), (name, hours)
            assert (wr, wp) == want[2:], (name, hours)
            if m == 25:                                   # 24 ids and NOGROUP: only a region all of them visited stays
                assert (vis[vis > 0] == 25).all() and (name != "grid4096" or wr > 1000)
            if m == 1:
                assert wr == 0 and vis.max() > 3


def test_visitors_without_ids(data):
    """a stream fed without ids: one visitor per non-empty region"""
    s = data.stream(ids=False, nbatches=2)
    m = sm.StreamModel(ZMIN, ZMAX)
    for rows, cols, keep, hour, _ in data.batches[:2]:
        m.add(rows, cols, keep, hour, None)
    for name in ("mid", "at_bound"):
        rg = reg(name)
        pts, vis, wr, wp = s.region_visitors(rg.rs)
        want = want_totals(m, rg)
        assert np.array_equal(pts, want) and np.array_equal(vis, (want > 0).astype(np.int64)) and (wr, wp) == (0, 0)
        pts, vis, wr, wp = s.region_visitors(rg.rs, None, 2)
        assert not pts.any() and not vis.any() and (wr, wp) == (int((want > 0).sum()), int(want.sum()))
    s.close()


def test_totals_against_series_and_view(stream):
    for name in ("edge", "poly", "grid4096"):
        rs = reg(name).rs
        for hours in (ALL, (BASE + 3, BASE + 10)):
            t = stream.region_totals(rs, hours).cpu().numpy()
            assert np.array_equal(t, stream.region_series(rs, hours, 1).sum(0).cpu().numpy())
    rg = reg("grid4096")                                  # regions that do not overlap
    for hours in (None, (BASE + 3, BASE + 10)):
        _, z, r, c, n = stream.region_view(rg.rs, hours)
        want = np.zeros(rg.rs.nregions, dtype=np.int64)
        np.add.at(want, rg.img[r, c] - 1, n)
        assert np.array_equal(stream.region_totals(rg.rs, hours).cpu().numpy(), want)


def test_empty_stream_and_empty_table(stream, data):
    empty = RegionSet.from_mask(5, 0, 0, np.zeros((2, 4, 4), dtype=bool))
    assert empty.nspans == 0 and empty.nregions == 2
    s0 = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1 << 12)
    for s, rs in ((stream, empty), (s0, empty), (s0, reg("mid").rs)):
        assert not s.region_totals(rs).cpu().numpy().any()
        got = s.region_series(rs, ALL, 5).cpu().numpy()
        assert got.shape == (3, rs.nregions) and not got.any()
        assert s.region_view_device(rs)[0] == 0
        pts, vis, wr, wp = s.region_visitors(rs, None, 2)
        assert len(pts) == len(vis) == rs.nregions and not pts.any() and not vis.any() and (wr, wp) == (0, 0)
    s0.close()


def test_bad_tables_are_refused_and_leave_the_stream_right(stream, data):
    import torch

    rg = reg("mid")
    rs = rg.rs
    out = torch.full((rs.nregions,), SENT, dtype=torch.int64, device="cuda")
    vis = torch.full((rs.nregions,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    no = ctypes.c_int64(-1)
    A = _lib.HM_STREAM_ALLTIME
    row = int(np.flatnonzero(np.diff(rs.row_ptr.astype(np.int64)) >= 2)[0])
    j = int(rs.row_ptr[row])
    unsorted = rs.col_lo.copy()
    unsorted[j], unsorted[j + 1] = unsorted[j + 1], unsorted[j]
    hi_unsorted = rs.col_hi.copy()
    hi_unsorted[j], hi_unsorted[j + 1] = hi_unsorted[j + 1], hi_unsorted[j]
    bad_region = rs.region.copy()
    bad_region[5] = rs.nregions
    short_ptr = rs.row_ptr.copy()
    short_ptr[-1] -= 1
    u32p = ctypes.POINTER(ctypes.c_uint32)
    for arrays, index in (((rs.row_ptr, unsorted, hi_unsorted, rs.region), j + 1),
                          ((rs.row_ptr, rs.col_lo, rs.col_hi, bad_region), 5),
                          ((short_ptr, rs.col_lo, rs.col_hi, rs.region), rs.nrows)):
        st = _lib.hm_regions(rs.zoom, rs.row_lo, rs.nrows, rs.nspans, rs.nregions,
                             *(np.ascontiguousarray(a).ctypes.data_as(u32p) for a in arrays))
        L = stream.ctx.L
        assert L.hm_stream_region_series(stream.ptr, A, A, 1, _lib.HM_VIEW_MERGED, ctypes.byref(st),
                                         device._ptr(out)) == _lib.HM_E_ARG
        assert stream.ctx.last_error() == (index, _lib.HM_E_ARG)
        assert L.hm_stream_region_view(stream.ptr, A, A, _lib.HM_VIEW_MERGED, ctypes.byref(st), None, None, None, 0,
                                       ctypes.byref(no)) == _lib.HM_E_ARG
        assert L.hm_stream_region_visitors(stream.ptr, A, A, ctypes.byref(st), 1, device._ptr(out), device._ptr(vis),
                                           None) == _lib.HM_E_ARG
        assert (out.cpu().numpy() == SENT).all() and (vis.cpu().numpy() == 0x5A5A5A5A).all() and no.value == -1
        assert np.array_equal(stream.region_totals(rs).cpu().numpy(), want_totals(data.model, rg))
    assert np.array_equal(got_view(stream, rs, None, "merged"), want_view(data.model, rg, None, "merged"))
