"""Viewport and tile queries on the resident streaming heatmap (hm_stream_view,
StreamingHeatmap.view / tile_rows) vs the oracle: a view equals one oracle
count over the selected points (hours, groups), filtered by rectangle in numpy.
Every non-empty rectangle is placed on the oracle's own cells (around its
heaviest cell of that zoom) and the expected set is asserted non-empty.

The main stream's log holds well over 4 x 8192 cells, so the filter kernel runs
several blocks and a ragged last chunk; the tiny stream is one partial chunk of
one block; the zooms 6-12 stream has pyramid offsets that do not start at 0."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, synth
from heatmap_amd.stream import ALLGROUPS, NOGROUP, StreamingHeatmap, tile_rects

pytestmark = pytest.mark.gpu
BASE = 480000  # epoch hour (2024-10-04)
ZMIN, ZMAX = 0, 18
USERS = ["u1", "u2", "u3", "xhidden", "xother"]


def _in_rects(z, r, c, rects):
    m = np.zeros(z.size, dtype=bool)
    for rz, rlo, rhi, clo, chi in rects:
        m |= (z == rz) & (r >= rlo) & (r < rhi) & (c >= clo) & (c < chi)
    return m


def _expect(ref, rects):
    """the oracle's cells (zoom, row, col, count) inside any of the rectangles"""
    assert ref["status"] == 0
    z, r, c, n = (np.asarray(ref[k]).astype(np.int64) for k in ("zoom", "row", "col", "count"))
    m = _in_rects(z, r, c, rects)
    return z[m], r[m], c[m], n[m]


def _check(got, want, nonempty=True):
    """got, want: (zoom, row, col, count) in any order; want's cells are distinct"""
    g = [np.asarray(a).astype(np.int64) for a in got]
    w = [np.asarray(a).astype(np.int64) for a in want]
    if nonempty:
        assert w[0].size > 0
    assert g[0].size == w[0].size
    og, ow = np.lexsort((g[2], g[1], g[0])), np.lexsort((w[2], w[1], w[0]))
    for a, b, name in zip(g, w, ("zoom", "row", "col", "count")):
        assert np.array_equal(a[og], b[ow]), name


def _heaviest(ref, z):
    m = np.asarray(ref["zoom"]) == z
    assert m.any()
    i = int(np.argmax(np.where(m, np.asarray(ref["count"]).astype(np.int64), -1)))
    return int(ref["row"][i]), int(ref["col"][i])


def _around(ref, z, half):
    """the 2*half square around the oracle's heaviest cell of zoom z (unclipped)"""
    r, c = _heaviest(ref, z)
    return (z, r - half, r + half, c - half, c + half)


def _raw_view(s, rects, lo=-1, hi=-1, group=_lib.HM_VIEW_MERGED, nrects=None, capacity=0):
    """hm_stream_view through ctypes with no output arrays: (status, *n_out)"""
    flat = [int(v) for r in rects for v in r] or [0]
    ra = (ctypes.c_int64 * len(flat))(*flat)
    n = ctypes.c_int64(-7)
    rc = s.ctx.L.hm_stream_view(s.ptr, lo, hi, group, ra, len(rects) if nrects is None else nrects, None, None, None,
                                capacity, ctypes.byref(n))
    return rc, n.value


class Data:
    """6 batches x 20 000 'hotspots' points; a batch's hours overlap the next
    one's (hours BASE .. BASE + 17), 10% dropped by keep, three user groups and
    two 'x...' ids (no group): the data of tests/test_gpu_stream_window.py."""

    def __init__(self, nb=6, n=20000, seed=7):
        self.batches = []
        for b in range(nb):
            lat, lon = synth.generate("hotspots", n, seed=seed, start=b * n)
            rng = np.random.default_rng(seed * 100 + b)
            hour = (BASE + 3 * b + rng.integers(0, 3, n)).astype(np.uint32)
            keep = (rng.random(n) > 0.1).astype(np.uint8)
            users = [USERS[i] for i in rng.integers(0, len(USERS), n)]
            self.batches.append((lat, lon, keep, hour, users))
        self.lat = np.concatenate([b[0] for b in self.batches])
        self.lon = np.concatenate([b[1] for b in self.batches])
        self.keep = np.concatenate([b[2] for b in self.batches])
        self.hour = np.concatenate([b[3] for b in self.batches]).astype(np.int64)
        self.users = np.array(sum((b[4] for b in self.batches), []))
        self._memo = {}

    def stream(self, users=True, base=BASE, **kw):
        s = StreamingHeatmap(ZMIN, ZMAX, base_hour=base, **kw)
        for lat, lon, keep, hour, us in self.batches:
            s.add(lat, lon, keep, hour, user_id=us if users else None)
        return s

    def ref(self, lo=BASE, hi=BASE + 18, extra=None):
        """oracle.count over keep & (lo <= hour < hi) [& extra], computed once"""
        key = (lo, hi, None if extra is None else extra.tobytes())
        if key not in self._memo:
            m = (self.keep == 1) & (self.hour >= lo) & (self.hour < hi)
            if extra is not None:
                m &= extra
            self._memo[key] = oracle.count(self.lat, self.lon, m.astype(np.uint8), ZMIN, ZMAX)
        return self._memo[key]


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def main(gpu, data):
    """the main stream with user groups; the tests that use it leave it as it is"""
    s = data.stream()
    assert s.cells()[0] > 4 * 8192
    yield s
    s.close()


# ------------------------------------------------------------- rectangles

def test_every_zoom_whole(main, data):
    """(1) 'all of zoom z', alltime == the oracle's zoom-z cells: both ends of
    every zoom's id interval against its neighbour zooms."""
    ref = data.ref()
    for z in range(ZMIN, ZMAX + 1):
        rect = [(z, 0, 1 << z, 0, 1 << z)]
        want = _expect(ref, rect)
        assert (want[0] == z).all() and want[0].size == int((np.asarray(ref["zoom"]) == z).sum())
        w = main.view_counts(rect)
        _check((w.zoom, w.row, w.col, w.count), want)


def test_one_cell_and_its_neighbours(main, data):
    """(2) the heaviest zoom-18 cell alone; rectangles that end at it (hi
    exclusive) and start at it (lo inclusive), by row and by column."""
    ref = data.ref()
    r, c = _heaviest(ref, 18)
    g, z, rr, cc, n = main.view([(18, r, r + 1, c, c + 1)])
    want = _expect(ref, [(18, r, r + 1, c, c + 1)])
    assert want[0].size == 1 and (g == ALLGROUPS).all()
    _check((z, rr, cc, n), want)
    w = 64
    for rect, holds in (((18, r - w, r, c - w, c + w), False), ((18, r, r + w, c - w, c + w), True),
                        ((18, r - w, r + w, c - w, c), False), ((18, r - w, r + w, c, c + w), True),
                        ((18, r - w, r + 1, c - w, c + 1), True), ((18, r + 1, r + w, c - w, c + w), False),
                        ((18, r - w, r + w, c + 1, c + w), False)):
        want = _expect(ref, [rect])
        assert bool(((want[1] == r) & (want[2] == c)).any()) == holds
        v = main.view_counts([rect])
        _check((v.zoom, v.row, v.col, v.count), want)


def _tile13(data, lo, hi):
    r, c = _heaviest(data.ref(lo, hi), 13)
    return (13, r >> 5 << 5, (r >> 5 << 5) + 32, c >> 5 << 5, (c >> 5 << 5) + 32)


def test_window_merged_each_and_one_group(main, data):
    """(3) a 32 x 32 zoom-13 rectangle over the hours [BASE+4, BASE+8): merged;
    per group == the oracle with that user's mask, 'x...' users under NOGROUP,
    the groups' counts summing to the merged ones; one group id alone."""
    lo, hi = BASE + 4, BASE + 8
    rect = [_tile13(data, lo, hi)]
    g, z, r, c, n = main.view(rect, (lo, hi))
    assert (g == ALLGROUPS).all()
    merged = _expect(data.ref(lo, hi), rect)
    _check((z, r, c, n), merged)
    g, z, r, c, n = main.view(rect, (lo, hi), "each")
    ids = {u: main.labels.index(u) for u in ("u1", "u2", "u3")}
    assert sorted(np.unique(g).tolist()) == sorted(list(ids.values()) + [NOGROUP])
    for u, gid in ids.items():
        m = g == gid
        _check((z[m], r[m], c[m], n[m]), _expect(data.ref(lo, hi, data.users == u), rect))
    m = g == NOGROUP
    _check((z[m], r[m], c[m], n[m]), _expect(data.ref(lo, hi, np.char.startswith(data.users, "x")), rect))
    key = (r.astype(np.int64) << 32) | c.astype(np.int64)
    uk, inv = np.unique(key, return_inverse=True)
    tot = np.zeros(uk.size, np.int64)
    np.add.at(tot, inv.reshape(-1), n.astype(np.int64))
    _check((np.full(uk.size, 13), uk >> 32, uk & 0xFFFFFFFF, tot), merged)
    g, z, r, c, n = main.view(rect, (lo, hi), ids["u2"])
    assert (g == ids["u2"]).all()
    _check((z, r, c, n), _expect(data.ref(lo, hi, data.users == "u2"), rect))
    g, z, r, c, n = main.view(rect, (lo, hi), NOGROUP)
    assert (g == NOGROUP).all()
    _check((z, r, c, n), _expect(data.ref(lo, hi, np.char.startswith(data.users, "x")), rect))


def test_many_rectangles_overlapping(main, data):
    """(4) 32 rectangles over 8 zooms, four per zoom around the heaviest cell,
    three of them overlapping: each cell once, the union computed on the host.
    33 and 0 rectangles are argument errors."""
    ref = data.ref()
    rects = []
    for z in (4, 6, 8, 10, 12, 14, 16, 18):
        r, c = _heaviest(ref, z)
        h = 2 if z <= 6 else 6
        rects += [(z, r - h, r + h, c - h, c + h), (z, r - 1, r + h + 3, c - 1, c + h + 3),
                  (z, r - h - 2, r + 1, c - h, c + 2), (z, r + 3 * h, r + 5 * h, c - h, c + h)]
    assert len(rects) == 32
    want = _expect(ref, rects)
    singly = sum(_expect(ref, [q])[0].size for q in rects)
    assert singly > want[0].size > 32           # the rectangles do overlap on cells that exist
    assert len(np.unique(want[0])) == 8
    v = main.view_counts(rects)
    _check((v.zoom, v.row, v.col, v.count), want)
    n, keys, _, _ = main.view_device(rects)
    assert len(np.unique(keys[:n].cpu().numpy())) == n == want[0].size
    assert _raw_view(main, rects + [rects[0]])[0] == _lib.HM_E_ARG
    assert _raw_view(main, [])[0] == _lib.HM_E_ARG
    assert _raw_view(main, rects, nrects=-1)[0] == _lib.HM_E_ARG
    for bad in (rects + [rects[0]], []):
        with pytest.raises(ValueError):
            main.view(bad)


def test_clipping_empties_and_bad_arguments(main, data):
    """(5) bounds below 0 and beyond 2^z are clipped; rectangles outside the
    square, in an empty region, or a window without data give nothing; bad
    rectangles, zooms and hour pairs are argument errors."""
    ref = data.ref()
    z, side = 10, 1 << 10
    r, c = _heaviest(ref, z)
    wide = (z, -5, r + 3, c - 3, side + 7)
    clipped = (z, 0, r + 3, c - 3, side)
    want = _expect(ref, [clipped])
    v = main.view_counts([wide])
    _check((v.zoom, v.row, v.col, v.count), want)
    v = main.view_counts([clipped])
    _check((v.zoom, v.row, v.col, v.count), want)
    empty = (18, 0, 16, 0, 16)
    assert _expect(ref, [empty])[0].size == 0                    # the oracle shows nothing there
    for rect in ((z, -8, -1, 0, 10), (z, 0, 10, side, side + 5), (z, side, side + 1, -3, 0), empty):
        assert main.view_device([rect])[0] == 0, rect
        assert _raw_view(main, [rect]) == (_lib.HM_OK, 0), rect
        assert main.view_counts([rect]).count.size == 0
    # an outside rectangle beside a real one changes nothing
    v = main.view_counts([(z, -8, -1, 0, 10), clipped])
    _check((v.zoom, v.row, v.col, v.count), want)
    for lo, hi in ((BASE + 100, BASE + 200), (BASE - 50, BASE), (BASE + 18, BASE + 19)):
        assert main.view_device([clipped], (lo, hi))[0] == 0
        assert _raw_view(main, [clipped], lo, hi) == (_lib.HM_OK, 0)
    # clamped hour bounds: every dated hour
    v = main.view_counts([clipped], (BASE - 1000, BASE + (1 << 40)))
    _check((v.zoom, v.row, v.col, v.count), want)
    for bad in ((z, 5, 5, 0, 4), (z, 6, 2, 0, 4), (z, 0, 4, 7, 7), (z, 0, 4, 9, 1), (ZMAX + 1, 0, 4, 0, 4),
                (-1, 0, 1, 0, 1), (40, 0, 1, 0, 1)):
        assert _raw_view(main, [bad])[0] == _lib.HM_E_ARG, bad
        assert _raw_view(main, [clipped, bad])[0] == _lib.HM_E_ARG, bad
        with pytest.raises(ValueError):
            main.view([bad])
    for lo, hi in ((BASE + 5, BASE + 5), (BASE + 6, BASE + 2), (-1, -2), (-2, -2), (0, 0)):
        assert _raw_view(main, [clipped], lo, hi)[0] == _lib.HM_E_ARG, (lo, hi)
        with pytest.raises(ValueError):
            main.view([clipped], (lo, hi))
    for group in (-3, 1 << 32, 0xFFFFFFFF):
        assert _raw_view(main, [clipped], group=group)[0] == _lib.HM_E_ARG, group
        with pytest.raises(ValueError):
            main.view([clipped], None, group)
    with pytest.raises(ValueError):
        main.view([clipped], None, "all")
    n = ctypes.c_int64(0)
    ra = (ctypes.c_int64 * 5)(*clipped)
    view = main.ctx.L.hm_stream_view
    assert view(main.ptr, -1, -1, -1, None, 1, None, None, None, 0, ctypes.byref(n)) == _lib.HM_E_ARG
    assert view(main.ptr, -1, -1, -1, ra, 1, None, None, None, 0, None) == _lib.HM_E_ARG


def test_capacity_zero_reports_cells_needed(main, data):
    """(6) capacity = 0: HM_E_CAPACITY and the exact number of cells; the
    next view still works (the log is unchanged)."""
    lo, hi = BASE + 4, BASE + 8
    rect = [_tile13(data, lo, hi)]
    want = _expect(data.ref(lo, hi), rect)
    assert want[0].size > 0
    assert _raw_view(main, rect, lo, hi) == (_lib.HM_E_CAPACITY, want[0].size)
    per_group = sum(_expect(data.ref(lo, hi, m), rect)[0].size
                    for m in [data.users == u for u in ("u1", "u2", "u3")] + [np.char.startswith(data.users, "x")])
    assert _raw_view(main, rect, lo, hi, _lib.HM_VIEW_EACH) == (_lib.HM_E_CAPACITY, per_group)
    before = main.cells()[0]
    v = main.view_counts(rect, (lo, hi))
    _check((v.zoom, v.row, v.col, v.count), want)
    assert main.cells()[0] == before


# ------------------------------------------------- a log that changes

def test_repeated_keys_expire_and_later_batch(gpu, data):
    """(7) the same hours added twice (a log with repeated keys): summed; the
    view still matches after expire(cut) and after a later batch."""
    s = data.stream(users=False)
    lat, lon, keep, hour, _ = data.batches[1]           # hours BASE + 3 .. BASE + 5
    s.add(lat, lon, keep, hour)
    lo, hi = BASE + 3, BASE + 6
    again = oracle.count(np.concatenate([data.lat, lat]), np.concatenate([data.lon, lon]),
                         np.concatenate([data.keep * ((data.hour >= lo) & (data.hour < hi)), keep]), ZMIN, ZMAX)
    rects = [_around(again, 13, 16), _around(again, 18, 200), (3, 0, 8, 0, 8)]
    want = _expect(again, rects)
    assert want[3].sum() > _expect(data.ref(lo, hi), rects)[3].sum()
    v = s.view_counts(rects, (lo, hi))
    _check((v.zoom, v.row, v.col, v.count), want)
    cut = BASE + 8
    s.expire(cut)
    v = s.view_counts(rects)
    _check((v.zoom, v.row, v.col, v.count), _expect(data.ref(cut, BASE + 18), rects))
    v = s.view_counts(rects, (BASE, cut))
    assert v.count.size == 0
    nlat, nlon = synth.generate("hotspots", 20000, seed=7, start=6 * 20000)
    s.add(nlat, nlon, None, np.full(20000, BASE + 30, np.uint32))
    alive = np.concatenate([(data.keep == 1) & (data.hour >= cut), np.ones(20000, bool)]).astype(np.uint8)
    both = oracle.count(np.concatenate([data.lat, nlat]), np.concatenate([data.lon, nlon]), alive, ZMIN, ZMAX)
    v = s.view_counts(rects)
    _check((v.zoom, v.row, v.col, v.count), _expect(both, rects))
    v = s.view_counts(rects, (BASE + 30, BASE + 31))
    _check((v.zoom, v.row, v.col, v.count), _expect(oracle.count(nlat, nlon, None, ZMIN, ZMAX), rects))
    s.close()


def test_undated_batch(gpu, data):
    """(8) an undated batch is in the alltime view and in no window view."""
    s = data.stream(users=False)
    ulat, ulon = synth.generate("hotspots", 5000, seed=77)
    s.add(ulat, ulon)
    every = oracle.count(np.concatenate([data.lat, ulat]), np.concatenate([data.lon, ulon]),
                         np.concatenate([data.keep, np.ones(len(ulat), np.uint8)]), ZMIN, ZMAX)
    und = oracle.count(ulat, ulon, None, ZMIN, ZMAX)
    rects = [_around(und, 12, 16), _around(every, 17, 100), (4, 0, 16, 0, 16)]
    want = _expect(every, rects)
    dated = _expect(data.ref(), rects)
    assert want[3].sum() > dated[3].sum() > 0
    v = s.view_counts(rects)
    _check((v.zoom, v.row, v.col, v.count), want)
    v = s.view_counts(rects, (BASE - 5, BASE + 1000))
    _check((v.zoom, v.row, v.col, v.count), dated)
    s.close()


def test_out_of_square_points(gpu, data):
    """(9) kept points with |lat| > 85.06 and lon >= 180 (side records beside
    the table): view() returns those in the caller's unclipped rectangle and
    none outside it; hm_stream_view itself never returns them."""
    s = data.stream()
    lat, lon = synth.generate("hotspots", 3000, seed=91)
    lat, lon = lat.copy(), lon.copy()
    lat[:40] = np.where(np.arange(40) % 2, 1.0, -1.0) * np.linspace(85.06, 89.9, 40)
    lon[20:60] = np.tile([180.0, 200.0, 540.0, 181.5], 10)
    hx = BASE + 9
    s.add(lat, lon, None, np.full(3000, hx, np.uint32), user_id=["u2"] * 3000)
    assert len(s._x)

    def ref(lo, hi, extra=True):
        m = (data.keep == 1) & (data.hour >= lo) & (data.hour < hi) & extra
        return oracle.count(np.concatenate([data.lat, lat]), np.concatenate([data.lon, lon]),
                            np.concatenate([m, np.full(3000, lo <= hx < hi)]).astype(np.uint8), ZMIN, ZMAX)

    z, side = 5, 32
    cover = [(z, -3 * side, 4 * side, -side, 5 * side), (18, -(1 << 20), 1 << 20, 1 << 18, 1 << 21)]
    inside = [(z, 0, side, 0, side), (18, 0, 1 << 18, 0, 1 << 18)]
    for hours, r in ((None, ref(BASE, BASE + 18)), ((hx, hx + 1), ref(hx, hx + 1))):
        want = _expect(r, cover)
        out = (want[1] < 0) | (want[1] >= (1 << want[0])) | (want[2] >= (1 << want[0]))
        assert out.sum() > 20 and (want[0][out] == z).any() and (want[0][out] == 18).any()
        v = s.view_counts(cover, hours)
        _check((v.zoom, v.row, v.col, v.count), want)
        # the device query: the in-square part only
        n, keys, counts, _ = s.view_device(cover, hours)
        assert n == int((~out).sum())
        # rectangles that stop at the square's edge hold none of them
        v = s.view_counts(inside, hours)
        assert not ((v.row < 0) | (v.row >= (1 << v.zoom)) | (v.col >= (1 << v.zoom))).any()
        _check((v.zoom, v.row, v.col, v.count), _expect(r, inside))
    # another hour's window holds none; per group they are u2's
    v = s.view_counts(cover, (hx + 1, hx + 4))
    _check((v.zoom, v.row, v.col, v.count), _expect(ref(hx + 1, hx + 4), cover))
    assert not (v.row < 0).any()
    g, vz, vr, vc, vn = s.view(cover, (hx, hx + 1), "each")
    out = (vr < 0) | (vr >= (1 << vz)) | (vc >= (1 << vz))
    assert out.any() and (g[out] == s.labels.index("u2")).all()
    g, vz, vr, vc, vn = s.view(cover, (hx, hx + 1), s.labels.index("u1"))
    assert vz.size and not ((vr < 0) | (vr >= (1 << vz)) | (vc >= (1 << vz))).any()
    s.close()


# ------------------------------------------------------ other streams

def test_zmin_6_pyramid_offsets(gpu, data):
    """(10) zooms 6-12: the cell ids start at the zoom-6 offset."""
    lat, lon, keep, hour, _ = data.batches[0]
    lat2, lon2, keep2, hour2, _ = data.batches[1]
    s = StreamingHeatmap(6, 12, base_hour=BASE)
    s.add(lat, lon, keep, hour)
    s.add(lat2, lon2, keep2, hour2)
    la, lo_, kp = np.concatenate([lat, lat2]), np.concatenate([lon, lon2]), np.concatenate([keep, keep2])
    hr = np.concatenate([hour, hour2]).astype(np.int64)
    ref = oracle.count(la, lo_, kp, 6, 12)
    for rects in ([(6, 0, 64, 0, 64)], [(12, 0, 1 << 12, 0, 1 << 12)], [_around(ref, 12, 20), _around(ref, 6, 2)],
                  [(z, 0, 1 << z, 0, 1 << z) for z in range(6, 13)]):
        v = s.view_counts(rects)
        _check((v.zoom, v.row, v.col, v.count), _expect(ref, rects))
    w = oracle.count(la, lo_, kp & ((hr >= BASE + 2) & (hr < BASE + 4)), 6, 12)
    rects = [_around(w, 12, 20), (6, 0, 64, 0, 64)]
    v = s.view_counts(rects, (BASE + 2, BASE + 4))
    _check((v.zoom, v.row, v.col, v.count), _expect(w, rects))
    for zbad in (5, 13, 0):
        assert _raw_view(s, [(zbad, 0, 1, 0, 1)])[0] == _lib.HM_E_ARG
        with pytest.raises(ValueError):
            s.view([(zbad, 0, 1, 0, 1)])
    s.close()


def test_tiny_stream_single_partial_chunk(gpu):
    """(11) 200 points, zooms 0-6: the log is one partial chunk of one block."""
    lat, lon = synth.generate("hotspots", 200, seed=13)
    rng = np.random.default_rng(13)
    keep = (rng.random(200) > 0.1).astype(np.uint8)
    hour = (BASE + rng.integers(0, 4, 200)).astype(np.int64)
    s = StreamingHeatmap(0, 6, base_hour=BASE)
    s.add(lat, lon, keep, hour.astype(np.uint32))
    assert 0 < s.cells()[0] < 2048
    ref = oracle.count(lat, lon, keep, 0, 6)
    for rects in ([(6, 0, 64, 0, 64)], [(0, 0, 1, 0, 1)], [_around(ref, 6, 3), _around(ref, 3, 1)]):
        v = s.view_counts(rects)
        _check((v.zoom, v.row, v.col, v.count), _expect(ref, rects))
    w = oracle.count(lat, lon, keep & ((hour >= BASE + 1) & (hour < BASE + 3)), 0, 6)
    rects = [_around(w, 6, 5), (2, 0, 4, 0, 4)]
    v = s.view_counts(rects, (BASE + 1, BASE + 3))
    _check((v.zoom, v.row, v.col, v.count), _expect(w, rects))
    e = StreamingHeatmap(0, 6, base_hour=BASE)          # an empty log
    assert e.view_device([(6, 0, 64, 0, 64)])[0] == 0
    e.close()
    s.close()


# ---------------------------------------------------------------- tiles

def _tile_of(row_id):
    return tuple(int(v) for v in row_id.rsplit("|", 1)[1].split("_"))


def test_tile_rows_match_window_rows(gpu):
    """(12) tile_rows == the entries of window_rows / rows('alltime') whose
    tile is asked for, which are the reference's rows (the mixed-user data of
    tests/test_gpu_stream_window.py::test_window_rows_match_reference)."""
    mz, d = 9, 5
    users_all = ["all", "u1", "u2", "xhidden", "rt-7", "rt-9", "u3"]
    rng = np.random.default_rng(5)
    bs = []
    for b in range(4):
        n = 1500
        lat, lon = synth.generate("hotspots", n, seed=21, start=b * n)
        keep = (rng.random(n) > 0.15).astype(np.uint8)
        hour = (BASE + 2 * b + rng.integers(0, 4, n)).astype(np.uint32)
        users = [users_all[i] for i in rng.integers(0, len(users_all), n)]
        bs.append((lat, lon, keep, hour, users))
    s = StreamingHeatmap(0, mz + d, base_hour=BASE - 100)
    for lat, lon, keep, hour, users in bs:
        s.add(lat, lon, keep, hour, user_id=users)
    lat = np.concatenate([b[0] for b in bs])
    lon = np.concatenate([b[1] for b in bs])
    keep = np.concatenate([b[2] for b in bs])
    hour = np.concatenate([b[3] for b in bs]).astype(np.int64)
    users = sum((b[4] for b in bs), [])

    def reference(m, label):
        src = np.where(keep[m].astype(bool), "mobile", "background")
        rows = oracle.build_heatmap_rows(lat[m], lon[m], src, [u for u, t in zip(users, m) if t], mz, d)
        return {k.replace("|alltime|", "|%s|" % label, 1): v for k, v in rows.items()}

    lo, hi = BASE + 3, BASE + 6
    full = s.window_rows(lo, hi, "w")
    have = sorted({_tile_of(k) for k in full})
    # 40 tiles, several of every tile zoom the rows have, and one without data
    tiles = [t for tz in range(1, mz + 1) for t in [x for x in have if x[0] == tz][:4]]
    tiles = (tiles + [t for t in have if t not in tiles])[:40]
    assert len(tiles) == 40 and len({t[0] for t in tiles}) >= 8
    blank = (mz, 0, 0)
    assert blank not in have
    tiles.append(blank)
    subset = {k: v for k, v in full.items() if _tile_of(k) in set(tiles)}
    assert subset and len(subset) < len(full)
    got = s.tile_rows(tiles, (lo, hi), "w", max_zoom_level=mz, delta=d)
    assert got == subset
    want = reference((hour >= lo) & (hour < hi), "w")
    assert subset == {k: v for k, v in want.items() if _tile_of(k) in set(tiles)}
    # one user's rows, the literal 'all' rows, an unknown label
    u1 = {k: v for k, v in subset.items() if k.startswith("u1|")}
    assert u1 and s.tile_rows(tiles, (lo, hi), "w", user="u1", max_zoom_level=mz, delta=d) == u1
    al = {k: v for k, v in subset.items() if k.startswith("all|")}
    assert al and s.tile_rows(tiles, (lo, hi), "w", user="all", max_zoom_level=mz, delta=d) == al
    rt = {k: v for k, v in subset.items() if k.startswith("route|")}
    assert rt and s.tile_rows(tiles, (lo, hi), "w", user="route", max_zoom_level=mz, delta=d) == rt
    assert s.tile_rows(tiles, (lo, hi), "w", user="nobody", max_zoom_level=mz, delta=d) == {}
    t = s.tile_table(tiles, (lo, hi), "last3h", max_zoom_level=mz, delta=d)
    assert sorted(t.column("id").to_pylist()) == sorted(k.replace("|w|", "|last3h|", 1) for k in subset)
    # alltime
    every = s.rows("alltime", max_zoom_level=mz, delta=d)
    sub_all = {k: v for k, v in every.items() if _tile_of(k) in set(tiles)}
    assert sub_all and s.tile_rows(tiles, max_zoom_level=mz, delta=d) == sub_all
    assert sub_all == {k: v for k, v in reference(np.ones(len(lat), bool), "alltime").items()
                       if _tile_of(k) in set(tiles)}
    assert s.tile_rows([blank], (lo, hi), "w", max_zoom_level=mz, delta=d) == {}
    assert s.tile_rows(tiles, (BASE + 50, BASE + 60), "w", max_zoom_level=mz, delta=d) == {}
    assert tile_rects([(1, 1, 0)], d) == [(1 + d, 32, 64, 0, 32)]
    for bad in ((mz, 1 << mz, 0), (3, 0, -1), (0, 0, 0), (mz + 1, 0, 0)):
        with pytest.raises(ValueError):
            s.tile_rows([bad], (lo, hi), "w", max_zoom_level=mz, delta=d)
    with pytest.raises(ValueError):
        s.tile_rows(tiles, (lo, hi), "a|b", max_zoom_level=mz, delta=d)
    with pytest.raises(ValueError):
        s.tile_rows(tiles, (lo, hi), None, max_zoom_level=mz, delta=d)
    s.close()


def test_tile_rows_with_points_outside_the_chain_windows(gpu):
    """tile_rows when a side record lies outside the chain windows (|lon| >
    11520: the reference's re-projection chain moves such points between
    tiles): still exactly the subset of window_rows, which are the reference's."""
    from heatmap_amd import heatmap as hm

    mz, d = 9, 5
    n = 1500
    rng = np.random.default_rng(12)
    lat, lon = synth.generate("hotspots", n, seed=21)
    lat, lon = lat.copy(), lon.copy()
    lat[:3], lon[:3] = [10.0, 40.0, -30.0], [12000.0, -11800.0, 11900.0]
    users = [["all", "u1", "u2", "xhidden", "rt-7"][i] for i in rng.integers(0, 5, n)]
    hour = (BASE + rng.integers(0, 3, n)).astype(np.uint32)
    hour[:3] = BASE + 1
    s = StreamingHeatmap(0, mz + d, base_hour=BASE)
    s.add(lat, lon, None, hour, user_id=users)
    det = s._x[s._x[:, 2] == mz + d]
    assert len(det) and not hm._in_chain_window(det[:, 3], det[:, 4], mz + d, d).all()
    lo, hi = BASE + 1, BASE + 3
    full = s.window_rows(lo, hi, "w")
    m = (hour >= lo) & (hour < hi)
    want = oracle.build_heatmap_rows(lat[m], lon[m], np.full(int(m.sum()), "mobile"),
                                     [u for u, t in zip(users, m) if t], mz, d)
    assert full == {k.replace("|alltime|", "|w|", 1): v for k, v in want.items()}
    tiles = sorted({_tile_of(k) for k in full if 0 <= _tile_of(k)[1] < (1 << _tile_of(k)[0])
                    and 0 <= _tile_of(k)[2] < (1 << _tile_of(k)[0])})[::3]
    assert len(tiles) > 32
    subset = {k: v for k, v in full.items() if _tile_of(k) in set(tiles)}
    assert subset and s.tile_rows(tiles, (lo, hi), "w", max_zoom_level=mz, delta=d) == subset
    u1 = {k: v for k, v in subset.items() if k.startswith("u1|")}
    assert u1 and s.tile_rows(tiles, (lo, hi), "w", user="u1", max_zoom_level=mz, delta=d) == u1
    every = s.rows("alltime", max_zoom_level=mz, delta=d)
    assert s.tile_rows(tiles, max_zoom_level=mz, delta=d) == {k: v for k, v in every.items()
                                                               if _tile_of(k) in set(tiles)}
    s.close()
