"""Distinct visitors per cell and k-anonymous tiles on the resident streaming
heatmap (hm_stream_visitors; StreamingHeatmap.visitors / visitors_device /
top_visited / tile_visitors, tile_raster and tile_images with min_users) vs
the oracle.

The model: one oracle.count per group over that group's selected points gives
the group's cell set; a cell's visitors are the sets that hold it, its points
the sum of the groups' counts there (checked against one oracle.count over all
selected points).  Results are compared exactly, as sets of (zoom, row, col,
points, visitors) records, since the order is unspecified.  A second,
independent model is the stream's own per-group view reduced with numpy.

Data: 4 batches x 6000 'hotspots' points over the hours BASE .. BASE + 11,
consecutive batches overlapping in hours (repeated keys in the log, a group in
several buckets), 10% dropped by keep, 48 group ids drawn with a skew: low
zooms see up to 48 visitors per cell, zoom 18 mostly 1 - 3."""
import ctypes

import numpy as np
import pytest

import raster_model as rm
from oracle import oracle
from heatmap_amd import _lib, device, raster, synth
from heatmap_amd.stream import NOGROUP, StreamingHeatmap

pytestmark = pytest.mark.gpu
BASE = 480000
ZMIN, ZMAX = 0, 18
NG = 48
SENT = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A
ALL = (BASE, BASE + 12)


def _in_rects(z, r, c, rects):
    m = np.zeros(z.size, dtype=bool)
    for rz, rlo, rhi, clo, chi in rects:
        m |= (z == rz) & (r >= rlo) & (r < rhi) & (c >= clo) & (c < chi)
    return m


def _whole(z):
    return [(z, 0, 1 << z, 0, 1 << z)]


def _rec(z, r, c, p, v):
    """(zoom, row, col, points, visitors) records in a canonical order"""
    a = np.stack([np.asarray(x).astype(np.int64).reshape(-1) for x in (z, r, c, p, v)], axis=1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))] if len(a) else a


def _label(g):
    """the user id the second stream files group id g under: two 'x...' ids (no
    group), two 'rt-...' ids (one group, 'route'), plain ids otherwise"""
    return {5: "xa", 11: "xb", 7: "rt-a", 13: "rt-b"}.get(int(g), "u%d" % g)


def _effective(g):
    """the group a user id ends up in: all 'x...' ids together, 'rt-...' together"""
    return {5: -1, 11: -1, 13: 7}.get(int(g), int(g))


class Data:
    def __init__(self, nb=4, n=6000, seed=23):
        self.batches = []
        for b in range(nb):
            lat, lon = synth.generate("hotspots", n, seed=seed, start=b * n)
            rng = np.random.default_rng(seed * 100 + b)
            hour = (BASE + 2 * b + rng.integers(0, 6, n)).astype(np.uint32)   # 0-5, 2-7, 4-9, 6-11
            keep = (rng.random(n) > 0.1).astype(np.uint8)
            group = np.floor(NG * rng.random(n) ** 3).astype(np.uint32)
            self.batches.append((lat, lon, keep, hour, group))
        self.lat, self.lon, self.keep = (np.concatenate([b[j] for b in self.batches]) for j in range(3))
        self.hour = np.concatenate([b[3] for b in self.batches]).astype(np.int64)
        self.group = np.concatenate([b[4] for b in self.batches]).astype(np.int64)
        self.eff = np.array([_effective(g) for g in self.group], dtype=np.int64)
        self._memo = {}

    def stream(self, how="group", **kw):
        s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, **kw)
        for lat, lon, keep, hour, group in self.batches:
            if how == "group":
                s.add(lat, lon, keep, hour, group=group)
            elif how == "user":
                s.add(lat, lon, keep, hour, user_id=[_label(g) for g in group])
            else:
                s.add(lat, lon, keep, hour)
        return s

    def model(self, lo=ALL[0], hi=ALL[1], groups=None, drop=None, tag="group"):
        """every cell's (zoom, row, col, points, visitors) over keep & (lo <=
        hour < hi), with `groups` as each point's group (default: the ids fed)
        and the points of group `drop` left out; computed once"""
        key = (lo, hi, tag, drop)
        if key not in self._memo:
            g = self.group if groups is None else groups
            sel = (self.keep == 1) & (self.hour >= lo) & (self.hour < hi)
            if drop is not None:
                sel &= g != drop
            self._memo[key] = _model(self.lat, self.lon, sel, g)
        return self._memo[key]


def _model(lat, lon, sel, g):
    parts = []
    for gid in np.unique(g[sel]):
        m = sel & (g == gid)
        ref = oracle.count(lat[m], lon[m], None, ZMIN, ZMAX)
        assert ref["status"] == 0
        parts.append(np.stack([np.asarray(ref[k]).astype(np.int64) for k in ("zoom", "row", "col", "count")], axis=1))
    if not parts:
        return np.zeros((0, 5), dtype=np.int64)
    a = np.concatenate(parts)
    u, inv = np.unique(a[:, :3], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    pts = np.zeros(len(u), dtype=np.int64)
    np.add.at(pts, inv, a[:, 3])
    vis = np.bincount(inv, minlength=len(u))
    out = _rec(u[:, 0], u[:, 1], u[:, 2], pts, vis)
    # the points are one count over all selected points
    ref = oracle.count(lat[sel], lon[sel], None, ZMIN, ZMAX)
    assert np.array_equal(out[:, :4], _rec(ref["zoom"], ref["row"], ref["col"], ref["count"], ref["count"])[:, :4])
    return out


def _pick(model, rects, m=1):
    """(the model's records inside the rectangles with >= m visitors, cells withheld, points withheld)"""
    a = model[_in_rects(model[:, 0], model[:, 1], model[:, 2], rects)]
    low = a[:, 4] < m
    return a[~low], int(low.sum()), int(a[low, 3].sum())


def _device(s, rects, hours=None, m=1):
    """visitors_device on the host: (records, withheld cells, withheld points)"""
    n, keys, pts, vis, wc, wp = s.visitors_device(rects, hours, m)
    z, r, c = device.decode_keys(keys[:n].cpu().numpy().view(np.uint64))
    return _rec(z, r, c, pts[:n].cpu().numpy(), vis[:n].cpu().numpy().view(np.uint32)), wc, wp


def _check(s, model, rects, hours=None, m=1):
    got, wc, wp = _device(s, rects, hours, m)
    want, mc, mp = _pick(model, rects, m)
    assert np.array_equal(got, want), (rects, hours, m, len(got), len(want))
    assert (wc, wp) == (mc, mp), (rects, hours, m)
    return got


def _heaviest(model, z):
    a = model[model[:, 0] == z]
    i = int(np.argmax(a[:, 3]))
    return int(a[i, 1]), int(a[i, 2])


def _around(model, z, half):
    r, c = _heaviest(model, z)
    return (z, r - half, r + half, c - half, c + half)


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def main(gpu, data):
    """the stream fed with explicit group ids; the tests that use it leave it as it is"""
    s = data.stream()
    yield s
    s.close()


def _rect_sets(model):
    return {"zoom0": _whole(0), "zoom1": _whole(1), "zoom6": _whole(6),
            "hot18": [_around(model, 18, 40)],
            "overlap": [_around(model, 12, 8), _around(model, 12, 12)],     # a cell in two rectangles: once
            "two zooms": [_around(model, 13, 16), _around(model, 18, 300)],
            "partly outside": [(14, -100, 1 << 13, -5, 1 << 14)]}


# ------------------------------------------------------------ the numbers

def test_threshold_one_is_the_merged_view(main, data):
    """min_visitors = 1: keys and points are exactly the merged view's, the
    visitors the model's and, independently, the per-group view's rows per
    cell; nothing is withheld"""
    model = data.model()
    assert model[model[:, 0] == 0][0, 4] == NG           # zoom 0: one cell, every group
    assert np.median(model[model[:, 0] == 18][:, 4]) <= 3
    for name, rects in _rect_sets(model).items():
        got = _check(main, model, rects, ALL, 1)
        assert len(got), name
        _, z, r, c, n = main.view(rects, ALL, "merged")
        assert np.array_equal(got[:, :4], _rec(z, r, c, n, n)[:, :4]), name
        g, z, r, c, n = main.view(rects, ALL, "each")
        u, cnt = np.unique(np.stack([z, r, c], axis=1).astype(np.int64), axis=0, return_counts=True)
        assert np.array_equal(got[:, [0, 1, 2, 4]], _rec(u[:, 0], u[:, 1], u[:, 2], cnt, cnt)[:, [0, 1, 2, 4]]), name


def test_thresholds(main, data):
    """2, the selection's median, its maximum and the maximum + 1 (nothing
    emitted, everything withheld); emitted + withheld are the totals of
    threshold 1 in every case"""
    model = data.model()
    for name, rects in _rect_sets(model).items():
        every, _, _ = _pick(model, rects)
        vmax = int(every[:, 4].max())
        for m in sorted({2, int(np.median(every[:, 4])), vmax, vmax + 1}):
            got, wc, wp = _device(main, rects, ALL, m)
            want, mc, mp = _pick(model, rects, m)
            assert np.array_equal(got, want), (name, m)
            assert (wc, wp) == (mc, mp), (name, m)
            assert len(got) + wc == len(every) and int(got[:, 3].sum()) + wp == int(every[:, 3].sum())
        got, wc, wp = _device(main, rects, ALL, vmax + 1)
        assert len(got) == 0 and (wc, wp) == (len(every), int(every[:, 3].sum())), name
        assert len(_device(main, rects, ALL, vmax)[0]) >= 1


def test_more_survivors_than_a_block_chunk(main, data):
    """whole zoom 14: more emitted cells than one 256 x 8 chunk of the sweep,
    from a number of (group, cell) records that is no multiple of 64 or 256"""
    model = data.model()
    nd = main.view_device(_whole(14), ALL, "each")[0]
    assert nd % 64 and nd % 256
    assert len(_check(main, model, _whole(14), ALL, 1)) > 256 * 8
    assert len(_check(main, model, _whole(14), ALL, 2)) > 0


def test_hours(main, data):
    """a window that cuts the hours (a group whose only records of a cell lie
    outside it does not count), windows outside the stream's hours"""
    full = data.model()
    rects = [_whole(6)[0], _around(full, 18, 300), _whole(0)[0]]
    for lo, hi in ((BASE + 3, BASE + 5), (BASE + 8, BASE + 40), (BASE - 9, BASE + 2)):
        cut = data.model(max(lo, BASE), min(hi, BASE + 12))
        a, b = _pick(cut, rects)[0], _pick(full, rects)[0]
        assert len(a) < len(b) or (a[:, 4] < b[:, 4]).any()       # the window does change visitors
        for m in (1, 2, 5):
            _check(main, cut, rects, (lo, hi), m)
    for lo, hi in ((BASE + 100, BASE + 200), (BASE - 50, BASE)):
        n, _, _, _, wc, wp = main.visitors_device(rects, (lo, hi), 1)
        assert (n, wc, wp) == (0, 0, 0)
    with pytest.raises(ValueError):
        main.visitors(rects, (BASE + 5, BASE + 5))


def test_alltime_counts_undated_points(gpu, data):
    """undated points are in alltime and in no window; their group visits too"""
    s = data.stream()
    lat, lon = synth.generate("hotspots", 2000, seed=77)
    g = np.full(2000, NG + 3, np.uint32)                 # a group only the undated points have
    s.add(lat, lon, None, None, group=g)
    rects = [_whole(5)[0], _whole(0)[0], _around(data.model(), 17, 200)]
    for m in (1, 3):
        _check(s, data.model(), rects, ALL, m)
    al = _model(np.concatenate([data.lat, lat]), np.concatenate([data.lon, lon]),
                np.concatenate([data.keep == 1, np.ones(2000, bool)]), np.concatenate([data.group, g.astype(np.int64)]))
    assert al[al[:, 0] == 0][0, 4] == NG + 1
    for m in (1, 3, NG + 1):
        _check(s, al, rects, None, m)
    s.close()


def test_user_id_stream(gpu, data):
    """fed with user ids: the 'x...' ids together add exactly one visitor where
    present, 'rt-a' and 'rt-b' are one group"""
    s = data.stream("user")
    model = data.model(groups=data.eff, tag="user")
    plain = data.model()
    assert model[model[:, 0] == 0][0, 4] == NG - 2       # xa + xb -> one, rt-a + rt-b -> one
    assert (model[:, 4] <= plain[:, 4]).all() and (model[:, 4] < plain[:, 4]).any()
    for rects in ([_whole(0)[0], _whole(3)[0]], _whole(9), [_around(model, 18, 300)]):
        for m in (1, 2, 4):
            _check(s, model, rects, ALL, m)
    # the no-group records alone: one visitor wherever they are
    only_x = (data.keep == 1) & (data.eff == -1)
    xs = _model(data.lat, data.lon, only_x, data.eff)
    assert len(xs) and (xs[:, 4] == 1).all()
    s.close()


def test_no_ids_and_empty(gpu, data):
    s = data.stream("none")
    model = data.model(groups=np.zeros_like(data.group), tag="none")
    assert (model[:, 4] == 1).all()
    for rects in (_whole(0), _whole(10), [_around(model, 18, 300)]):
        _check(s, model, rects, ALL, 1)
        got, wc, wp = _device(s, rects, ALL, 2)
        every = _pick(model, rects)[0]
        assert len(got) == 0 and (wc, wp) == (len(every), int(every[:, 3].sum()))
    s.close()
    e = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    for hours in (None, ALL):
        assert e.visitors_device(_whole(3), hours, 1)[::4] == (0, 0) and e.visitors_device(_whole(3), hours, 1)[5] == 0
        assert [len(a) for a in e.visitors(_whole(3), hours)] == [0] * 5
    assert e.top_visited(5, _whole(3)) == []
    e.close()


def test_forget_and_compaction(gpu, data):
    """compacting the log changes nothing; after forget(groups=[g]) visitors
    fall by exactly one in g's cells and nowhere else"""
    s = data.stream()
    model = data.model()
    rects = [_whole(7)[0], _around(model, 18, 300), _whole(1)[0]]
    before = _check(s, model, rects, ALL, 1)
    s.cells()                                            # compacts the log
    assert np.array_equal(_check(s, model, rects, ALL, 1), before)
    _check(s, model, rects, ALL, 3)
    g = 2
    s.forget(groups=[g])
    less = data.model(drop=g)
    after = _check(s, less, rects, ALL, 1)
    for m in (2, 4):
        _check(s, less, rects, ALL, m)
    own = _pick(_model(data.lat, data.lon, (data.keep == 1) & (data.group == g), data.group), rects)[0]
    was = {tuple(q[:3]): int(q[4]) for q in before.tolist()}
    now = {tuple(q[:3]): int(q[4]) for q in after.tolist()}
    gs = {tuple(q[:3]) for q in own.tolist()}
    assert gs and all(was[k] - now.get(k, 0) == (1 if k in gs else 0) for k in was)
    s.close()


def test_wide_counts_are_not_packed(gpu):
    """one cell with 2^40 points from each of two groups: points 2^41, visitors 2"""
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    key = np.array([(9 << 58) | (100 << 29) | 200] * 2, dtype=np.uint64)
    s.import_cells(key, np.array([1 << 40] * 2, dtype=np.uint64), np.array([3, 900000], np.uint32),
                   np.array([BASE + 1, BASE + 2], np.uint32))
    z, r, c, p, v = s.visitors(_whole(9))
    assert (z.tolist(), r.tolist(), c.tolist(), p.tolist(), v.tolist()) == ([9], [100], [200], [1 << 41], [2])
    n, _, _, _, wc, wp = s.visitors_device(_whole(9), None, 3)
    assert (n, wc, wp) == (0, 1, 1 << 41)
    s.close()


def test_out_of_square_side_records(gpu, data):
    """visitors() joins the side cells that lie in the rectangles as given,
    with their own visitors and the same threshold"""
    s = data.stream()
    n = 600
    lat, lon = synth.generate("hotspots", n, seed=91)
    lat, lon = lat.copy(), lon.copy()
    lat[:200] = 88.5
    lon[:200] = np.where(np.arange(200) % 4 == 0, 200.0, 10.0)
    g = (np.arange(n) % 5).astype(np.uint32)             # five groups in the heavy side cells
    s.add(lat, lon, None, np.full(n, BASE + 4, np.uint32), group=g)
    assert len(s._x)
    al = _model(np.concatenate([data.lat, lat]), np.concatenate([data.lon, lon]),
                np.concatenate([data.keep == 1, np.ones(n, bool)]), np.concatenate([data.group, g.astype(np.int64)]))
    rects = [(10, -(1 << 12), 1 << 10, -(1 << 10), 1 << 13), (4, -40, 40, -40, 40)]
    outside = lambda a: (a[:, 1] < 0) | (a[:, 2] >= (1 << a[:, 0]))   # noqa: E731
    for m in (1, 3, 5, 6):
        want = _pick(al, rects, m)[0]
        got = _rec(*s.visitors(rects, ALL, m))
        assert np.array_equal(got, want), m
        assert outside(want).any() == (m <= 5)
        dev = _device(s, rects, ALL, m)[0]               # the device part: the cells inside the square only
        assert np.array_equal(dev, want[~outside(want)])
    top = s.top_visited(4096, rects, ALL, 3)
    want = _pick(al, rects, 3)[0]
    want = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0], -want[:, 4]))]
    assert top == [((q[0], q[1], q[2]), q[4], q[3]) for q in want[:4096].tolist()]
    assert any(r < 0 for (_, r, _), _, _ in top)
    s.close()


# ------------------------------------------------------------ the C contract

def _raw(s, rects, lo, hi, m, cap, alloc=None, with_vis=True, n_ptr=True, wh=True):
    """hm_stream_visitors with sentinel-filled arrays of `alloc` entries:
    (status, n, keys, points, visitors, withheld) -- n and withheld keep their
    sentinels when the call leaves them alone"""
    torch = s._torch
    alloc = cap if alloc is None else alloc
    dev = "cuda:%d" % s.device_index
    keys = torch.full((alloc,), SENT, dtype=torch.int64, device=dev)
    pts = torch.full((alloc,), SENT, dtype=torch.int64, device=dev)
    vis = torch.full((alloc,), SENT32, dtype=torch.int32, device=dev)
    ra = (ctypes.c_int64 * max(1, 5 * len(rects)))(*[v for r in rects for v in r])
    n = ctypes.c_int64(-7)
    w = (ctypes.c_int64 * 2)(-7, -7)
    s.ctx.bind_stream()
    st = s.ctx.L.hm_stream_visitors(s.ptr, lo, hi, ra, len(rects), m, device._ptr(keys), device._ptr(pts),
                                    device._ptr(vis) if with_vis else None, cap, ctypes.byref(n) if n_ptr else None,
                                    w if wh else None)
    torch.cuda.synchronize()
    return st, n.value, keys.cpu().numpy(), pts.cpu().numpy(), vis.cpu().numpy().view(np.uint32), (w[0], w[1])


def _raw_rec(keys, pts, vis, n):
    z, r, c = device.decode_keys(keys[:n].view(np.uint64))
    return _rec(z, r, c, pts[:n], vis[:n])


def test_capacity_contract(main, data):
    model = data.model()
    rects = [_whole(8)[0], _around(model, 18, 100)]
    for m in (1, 3):
        want, mc, mp = _pick(model, rects, m)
        need = len(want)
        assert need > 64
        # sizing: no arrays at all
        st, n, _, _, _, w = _raw(main, rects, *ALL, m, 0, 0)
        assert (st, n, w) == (_lib.HM_E_CAPACITY, need, (mc, mp))
        # exact, with and without the visitors array
        st, n, keys, pts, vis, w = _raw(main, rects, *ALL, m, need, need + 3)
        assert (st, n, w) == (_lib.HM_OK, need, (mc, mp))
        assert np.array_equal(_raw_rec(keys, pts, vis, n), want)
        assert (keys[need:] == SENT).all() and (pts[need:] == SENT).all() and (vis[need:] == SENT32).all()
        st, n, keys, pts, vis, w = _raw(main, rects, *ALL, m, need, need, with_vis=False, wh=False)
        assert (st, n) == (_lib.HM_OK, need) and (vis == SENT32).all() and w == (-7, -7)
        assert np.array_equal(_raw_rec(keys, pts, np.ones(need), n)[:, :4], want[:, :4])
        # one short: the size, and nothing at or beyond capacity
        st, n, keys, pts, vis, w = _raw(main, rects, *ALL, m, need - 1, need + 3)
        assert (st, n, w) == (_lib.HM_E_CAPACITY, need, (mc, mp))
        assert (keys[need - 1:] == SENT).all() and (pts[need - 1:] == SENT).all() and (vis[need - 1:] == SENT32).all()
        got = _raw_rec(keys, pts, vis, need - 1)         # what was written is a part of the answer
        assert len({tuple(q) for q in got.tolist()} - {tuple(q) for q in want.tolist()}) == 0
        assert len(np.unique(got[:, :3], axis=0)) == need - 1


def test_no_bucket_left_for_the_labels(gpu):
    """a 1024-slot bucket table holding 600 groups: their 600 labels do not
    fit, HM_E_CAPACITY as a per-group view, and the stream is as it was"""
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=4096, max_buckets=1)
    ng = 600
    keys = ((np.uint64(9) << np.uint64(58)) | (np.arange(ng, dtype=np.uint64) % np.uint64(50) << np.uint64(29))
            | np.uint64(7))
    s.import_cells(keys, np.arange(1, ng + 1).astype(np.uint64), np.arange(ng, dtype=np.uint32),
                   np.full(ng, BASE + 1, np.uint32))
    cells = s.cells()
    merged = _rec(*s.view(_whole(9), None, "merged")[1:], np.zeros(50))
    assert len(merged) == 50
    st, n, keys_o, _, _, w = _raw(s, _whole(9), -1, -1, 1, 100)
    assert (st, n, w) == (_lib.HM_E_CAPACITY, 0, (0, 0)) and (keys_o == SENT).all()
    with pytest.raises(RuntimeError, match="capacity"):
        s.view(_whole(9), None, "each")
    with pytest.raises(RuntimeError, match="capacity"):
        s.visitors(_whole(9))
    assert s.cells() == cells
    assert np.array_equal(_rec(*s.view(_whole(9), None, "merged")[1:], np.zeros(50)), merged)
    s.close()


def test_refused_arguments(main):
    ok = _whole(8)
    bad = [(ok, *ALL, 0), (ok, *ALL, -3), ([], *ALL, 1), (ok * 33, *ALL, 1), ([(19, 0, 4, 0, 4)], *ALL, 1),
           ([(-1, 0, 4, 0, 4)], *ALL, 1), (ok, BASE + 5, BASE + 5, 1), (ok, BASE + 5, BASE + 4, 1),
           ([(8, 4, 4, 0, 4)], *ALL, 1), ([(8, 0, 4, 9, 3)], *ALL, 1)]
    for rects, lo, hi, m in bad:
        st, n, keys, pts, vis, w = _raw(main, rects, lo, hi, m, 64)
        assert st == _lib.HM_E_ARG, (rects[:1], lo, hi, m)
        assert n == -7 and w == (-7, -7)
        assert (keys == SENT).all() and (pts == SENT).all() and (vis == SENT32).all()
    st, _, keys, pts, vis, w = _raw(main, ok, *ALL, 1, 64, n_ptr=False)
    assert st == _lib.HM_E_ARG and w == (-7, -7) and (keys == SENT).all()
    # arrays missing with room asked for, a negative capacity, no stream
    L = main.ctx.L
    n = ctypes.c_int64(-7)
    ra = (ctypes.c_int64 * 5)(*ok[0])
    one = main._torch.full((8,), SENT, dtype=main._torch.int64, device="cuda:%d" % main.device_index)
    assert L.hm_stream_visitors(main.ptr, *ALL, ra, 1, 1, None, device._ptr(one), None, 8, ctypes.byref(n),
                                None) == _lib.HM_E_ARG
    assert L.hm_stream_visitors(main.ptr, *ALL, ra, 1, 1, device._ptr(one), None, None, 8, ctypes.byref(n),
                                None) == _lib.HM_E_ARG
    assert L.hm_stream_visitors(main.ptr, *ALL, ra, 1, 1, device._ptr(one), device._ptr(one), None, -1,
                                ctypes.byref(n), None) == _lib.HM_E_ARG
    assert L.hm_stream_visitors(None, *ALL, ra, 1, 1, device._ptr(one), device._ptr(one), None, 8, ctypes.byref(n),
                                None) == _lib.HM_E_ARG
    assert n.value == -7 and (one.cpu().numpy() == SENT).all()
    # the Python layer refuses the same before any call
    for m in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            main.visitors_device(ok, ALL, m)
    with pytest.raises(ValueError):
        main.visitors_device(ok * 33, ALL, 1)


def test_outside_the_square_is_empty(main):
    rects = [(9, -8, 0, 0, 4), (9, 0, 4, 1 << 9, 1 << 10)]
    st, n, keys, _, _, w = _raw(main, rects, *ALL, 1, 16)
    assert (st, n, w) == (_lib.HM_OK, 0, (0, 0)) and (keys == SENT).all()
    st, n, keys, _, _, w = _raw(main, _whole(4), BASE + 100, BASE + 200, 1, 16)
    assert (st, n, w) == (_lib.HM_OK, 0, (0, 0)) and (keys == SENT).all()


# ------------------------------------------------------------ rankings

def test_top_visited(main, data):
    """k below, at and above the number of cells; ties in visitors cut by key"""
    model = data.model()
    for rects, m in ((_whole(5), 1), ([_around(model, 18, 200)], 1), ([_whole(3)[0], _around(model, 16, 64)], 4),
                     (_whole(11), 2)):
        want = _pick(model, rects, m)[0]
        want = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0], -want[:, 4]))]
        ncell = len(want)
        assert 2 <= ncell
        for k in sorted({1, min(10, ncell - 1), min(ncell, 4096), min(ncell + 5, 4096)}):
            got = main.top_visited(k, rects, ALL, m)
            assert got == [((q[0], q[1], q[2]), q[4], q[3]) for q in want[:k].tolist()], (rects, m, k)
        if ncell > 10:
            assert want[9, 4] == want[10, 4]             # the cut at k = 10 falls among equal visitors
    assert main.top_visited(3, _whole(5), ALL, NG + 1) == []
    with pytest.raises(ValueError):
        main.top_visited(0, _whole(5))


# ------------------------------------------------------------ tiles

def _tiles_around(model, tz, b, count):
    """`count` tiles of zoom tz in a row, starting at the one under the heaviest cell"""
    r, c = _heaviest(model, tz + b)
    tr, tc = r >> b, min(c >> b, (1 << tz) - count)
    return [(tz, tr, tc + j) for j in range(count)]


def test_tile_rasters(main, data):
    """tile_raster(min_users) and tile_visitors against the raster model's
    scatter of the model's thresholded cells: two adjacent tiles (their halos
    share cells), and 33 tiles (two queries, nothing added twice)"""
    model = data.model()
    b, h = 3, 2
    for tiles in (_tiles_around(model, 9, b, 2), _tiles_around(model, 12, b, 33),
                  [(0, 0, 0), (1, 1, 0)] + _tiles_around(model, 15, b, 2)):
        plain = main.tile_raster(tiles, ALL, None, b, h)
        assert main._torch.equal(main.tile_raster(tiles, ALL, None, b, h, min_users=None), plain)
        assert main._torch.equal(main.tile_raster(tiles, ALL, None, b, h, min_users=1), plain)
        for m in (1, 2, 5):
            cells = model[model[:, 4] >= m]
            want = rm.densify_arrays(cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 3], tiles, b, h)
            got = main.tile_raster(tiles, ALL, None, b, h, min_users=m).cpu().numpy()
            assert np.array_equal(got, want), (len(tiles), m)
            wantv = rm.densify_arrays(cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 4], tiles, b, h)
            gotv = main.tile_visitors(tiles, ALL, b, h, min_users=m).cpu().numpy()
            assert np.array_equal(gotv, wantv), (len(tiles), m)
            if m == 2:
                assert want.sum() and (want != plain.cpu().numpy()).any()
    # a window, and alltime
    tiles = _tiles_around(model, 10, b, 2)
    cut = data.model(BASE + 3, BASE + 5)
    cells = cut[cut[:, 4] >= 2]
    want = rm.densify_arrays(cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 3], tiles, b, h)
    assert np.array_equal(main.tile_raster(tiles, (BASE + 3, BASE + 5), None, b, h, min_users=2).cpu().numpy(), want)
    cells = model[model[:, 4] >= 2]
    want = rm.densify_arrays(cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 3], tiles, b, h)
    assert np.array_equal(main.tile_raster(tiles, None, None, b, h, min_users=2).cpu().numpy(), want)


def test_tile_images_and_refusals(main, data):
    model = data.model()
    tiles = _tiles_around(model, 11, 4, 2)
    for m in (None, 3):
        img = main.tile_images(tiles, ALL, None, 4, radius=2, min_users=m)
        grid = main.tile_raster(tiles, ALL, None, 4, halo=2, min_users=m)
        assert main._torch.equal(img, raster.render(grid, 4, 2, 2)[0])
    assert not main._torch.equal(main.tile_images(tiles, ALL, None, 4, radius=2, min_users=3),
                                 main.tile_images(tiles, ALL, None, 4, radius=2))
    for kw in ({"min_users": 2, "user": "u1"}, {"min_users": 0}, {"min_users": 2.5}):
        with pytest.raises(ValueError):
            main.tile_raster(tiles, ALL, bins_log2=4, **kw)
        with pytest.raises(ValueError):
            main.tile_images(tiles, ALL, bins_log2=4, **kw)
    with pytest.raises(ValueError):
        main.tile_visitors(tiles, ALL, 4, 0, min_users=0)
    with pytest.raises(ValueError):
        main.tile_visitors([(17, 0, 0)], ALL, 4)
