"""Sliding hour windows and retention of the resident streaming heatmap
(hm_stream_window, hm_stream_expire) vs the oracle: a window over the hours
[lo, hi) equals one oracle count over the kept points of those hours, and after
expire(cut) the stream equals one fed only the points of hours >= cut (and the
undated ones), with the bucket slots of the expired hours and of every rollup
label free again.

The main stream's log holds well over 256 * HMS_RL_PPT = 8192 cells, so the
filter and relabel kernels run several blocks and a ragged last chunk; the tiny
stream is the single partial chunk."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, synth
from heatmap_amd.device import Counts
from heatmap_amd.stream import ALLGROUPS, ALLTIME, NOGROUP, StreamingHeatmap

pytestmark = pytest.mark.gpu
BASE = 480000  # epoch hour (2024-10-04)
ZMIN, ZMAX = 0, 18
USERS = ["u1", "u2", "u3", "xhidden", "xother"]


def _same(got, ref):
    got = got.sorted()
    assert ref["status"] == 0
    assert np.array_equal(got.zoom, ref["zoom"])
    assert np.array_equal(got.row, ref["row"])
    assert np.array_equal(got.col, ref["col"])
    assert np.array_equal(got.count, ref["count"])


def _equal(a, b):
    a, b = a.sorted(), b.sorted()
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


class Data:
    """6 batches x 20 000 'hotspots' points; a batch's hours overlap the next
    one's (BASE + 3b .. BASE + 3b + 2 ... as tests/test_gpu_stream.py's
    _batches, so hours BASE .. BASE + 17), 10% dropped by keep, three user
    groups and two 'x...' ids (no group)."""

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

    def ref(self, lo, hi, extra=None):
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


def _undated(n=5000, seed=77):
    lat, lon = synth.generate("hotspots", n, seed=seed)
    return lat, lon


# ------------------------------------------------------------------ windows

def test_window_one_hour_and_mid_batch(gpu, data):
    """(1) a one-hour window == that hour's counts; (2) a window that cuts
    through the middle of two batches' hours."""
    s = data.stream()
    assert s.cells()[0] > 8192 * 4
    h = BASE + 4
    w = s.window_counts(h, h + 1)
    _same(w, data.ref(h, h + 1))
    _equal(w, s.counts(h))
    _equal(s.counts(window=(h, h + 1)), w)
    _same(s.window_counts(BASE + 4, BASE + 8), data.ref(BASE + 4, BASE + 8))
    # the bounds: lo is in the window, hi is not
    _same(s.window_counts(BASE + 5, BASE + 6), data.ref(BASE + 5, BASE + 6))
    s.close()


def test_window_clamped_empty_and_bad_bounds(gpu, data):
    """(3) bounds below the base hour and far above the data are clamped: every
    hour, which is the alltime counts while nothing is undated; (4) a window
    without data is empty; (5) hi <= lo is an argument error."""
    s = data.stream(users=False)
    every = s.window_counts(BASE - 1000, BASE + (1 << 40))
    _same(every, data.ref(BASE, BASE + 18))
    _equal(every, s.counts(ALLTIME))
    for lo, hi in ((BASE + 100, BASE + 200), (BASE - 50, BASE - 10), (BASE - 50, BASE),
                   (BASE + (1 << 28), BASE + (1 << 29)), (BASE + 18, BASE + 19)):
        n, _, _, _ = s.window_device(lo, hi)
        assert n == 0, (lo, hi)
        assert s.window_counts(lo, hi).count.size == 0
    for lo, hi in ((BASE + 5, BASE + 5), (BASE + 6, BASE + 2)):
        with pytest.raises(ValueError):
            s.window(lo, hi)
        n = ctypes.c_int64(0)
        assert s.ctx.L.hm_stream_window(s.ptr, lo, hi, 1, None, None, None, 0, ctypes.byref(n)) == _lib.HM_E_ARG
    # too small a buffer: HM_E_CAPACITY and the cells needed
    n = ctypes.c_int64(0)
    rc = s.ctx.L.hm_stream_window(s.ptr, BASE, BASE + 18, 1, None, None, None, 0, ctypes.byref(n))
    assert rc == _lib.HM_E_CAPACITY and n.value == every.count.size
    s.close()


def test_window_undated_batch(gpu, data):
    """(6) an undated batch is in no window and in alltime."""
    s = data.stream(users=False)
    ulat, ulon = _undated()
    s.add(ulat, ulon)
    _same(s.window_counts(BASE - 5, BASE + 1000), data.ref(BASE, BASE + 18))
    _same(s.window_counts(BASE + 4, BASE + 8), data.ref(BASE + 4, BASE + 8))
    _same(s.counts(ALLTIME), oracle.count(np.concatenate([data.lat, ulat]), np.concatenate([data.lon, ulon]),
                                          np.concatenate([data.keep, np.ones(len(ulat), np.uint8)]), ZMIN, ZMAX))
    s.close()


def test_window_per_group(gpu, data):
    """(7) merge_groups=False: every group's cells == the oracle count with
    that group's mask, the 'x...' users under NOGROUP."""
    s = data.stream()
    lo, hi = BASE + 4, BASE + 11
    g, z, r, c, cnt = s.window(lo, hi, merge_groups=False)
    assert sorted(np.unique(g).tolist()) == sorted([s.labels.index(u) for u in ("u1", "u2", "u3")] + [NOGROUP])
    for u in ("u1", "u2", "u3"):
        m = g == s.labels.index(u)
        _same(Counts(z[m], r[m], c[m], cnt[m], 0, []), data.ref(lo, hi, data.users == u))
    m = g == NOGROUP
    _same(Counts(z[m], r[m], c[m], cnt[m], 0, []), data.ref(lo, hi, np.char.startswith(data.users, "x")))
    g, z, r, c, cnt = s.window(lo, hi, merge_groups=True)
    assert (g == ALLGROUPS).all()
    _same(Counts(z, r, c, cnt, 0, []), data.ref(lo, hi))
    s.close()


def test_window_same_hour_twice(gpu, data):
    """(8) the same hours added twice before the query (a log with repeated
    keys): the counts are summed."""
    s = data.stream(users=False)
    lat, lon, keep, hour, _ = data.batches[1]
    s.add(lat, lon, keep, hour)
    lo, hi = BASE + 3, BASE + 6          # batch 1's hours
    ref = data.ref(lo, hi)
    again = oracle.count(np.concatenate([data.lat, lat]), np.concatenate([data.lon, lon]),
                         np.concatenate([data.keep * ((data.hour >= lo) & (data.hour < hi)), keep]), ZMIN, ZMAX)
    assert again["count"].sum() > ref["count"].sum()
    _same(s.window_counts(lo, hi), again)
    s.close()


def test_window_and_expire_out_of_square_points(gpu, data):
    """(9) kept points with |lat| > 85.06 and lon >= 180 (cells outside the
    square, kept beside the table): in the window that holds their hour and in
    no other, gone after an expire past that hour."""
    s = data.stream()
    lat, lon = synth.generate("hotspots", 3000, seed=91)
    lat, lon = lat.copy(), lon.copy()
    lat[:40] = np.where(np.arange(40) % 2, 1.0, -1.0) * np.linspace(85.06, 89.9, 40)
    lon[20:60] = np.tile([180.0, 200.0, 540.0, 181.5], 10)
    hx = BASE + 9
    s.add(lat, lon, None, np.full(3000, hx, np.uint32), user_id=["u2"] * 3000)

    def ref(lo, hi):
        m = (data.keep == 1) & (data.hour >= lo) & (data.hour < hi)
        inw = lo <= hx < hi
        return oracle.count(np.concatenate([data.lat, lat]), np.concatenate([data.lon, lon]),
                            np.concatenate([m, np.full(3000, inw)]).astype(np.uint8), ZMIN, ZMAX)

    w = s.window_counts(hx, hx + 1)
    assert (w.row < 0).any() and (w.col >= (1 << w.zoom)).any()
    _same(w, ref(hx, hx + 1))
    _same(s.window_counts(hx - 3, hx + 2), ref(hx - 3, hx + 2))
    for lo, hi in ((hx + 1, hx + 4), (hx - 4, hx)):
        o = s.window_counts(lo, hi)
        assert not (o.row < 0).any() and not (o.col >= (1 << o.zoom)).any()
        _same(o, ref(lo, hi))
    g, z, r, c, cnt = s.window(hx, hx + 1, merge_groups=False)
    out = (r < 0) | (c >= (1 << z))
    assert out.any() and (g[out] == s.labels.index("u2")).all()
    nx = len(s._x)
    before = s.cells()[0]
    dropped, _ = s.expire(hx + 1)
    assert dropped == before - s.cells()[0] + nx        # the side records count as cells
    a = s.counts(ALLTIME)
    assert not (a.row < 0).any() and not (a.col >= (1 << a.zoom)).any()
    _same(a, data.ref(hx + 1, BASE + 18))
    s.close()


def test_window_rows_match_reference(gpu):
    """(10) window_rows(lo, hi, 'w') == build_heatmaps over the window's
    points with the timespan label 'w' (compared as the year/month/day rows of
    tests/test_gpu_stream.py are)."""
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

    def want(lo, hi, label):
        m = (hour >= lo) & (hour < hi)
        src = np.where(keep[m].astype(bool), "mobile", "background")
        rows = oracle.build_heatmap_rows(lat[m], lon[m], src, [u for u, t in zip(users, m) if t], mz, d)
        return {k.replace("|alltime|", "|%s|" % label, 1): v for k, v in rows.items()}

    for lo, hi in ((BASE + 3, BASE + 6), (BASE, BASE + 10)):
        got = s.window_rows(lo, hi, "w")
        assert got and got == want(lo, hi, "w"), (lo, hi)
    t = s.window_table(BASE + 3, BASE + 6, "last3h")
    assert sorted(t.column("id").to_pylist()) == sorted(want(BASE + 3, BASE + 6, "last3h"))
    assert s.window_rows(BASE + 50, BASE + 60, "w") == {}
    with pytest.raises(ValueError):
        s.window_rows(BASE, BASE + 3, "a|b")
    s.close()


def test_tiny_stream_single_partial_chunk(gpu):
    """200 points, zooms 0-6: the log is one partial chunk of one block."""
    lat, lon = synth.generate("hotspots", 200, seed=13)
    rng = np.random.default_rng(13)
    keep = (rng.random(200) > 0.1).astype(np.uint8)
    hour = (BASE + rng.integers(0, 4, 200)).astype(np.int64)
    s = StreamingHeatmap(0, 6, base_hour=BASE)
    s.add(lat, lon, keep, hour.astype(np.uint32))
    assert 0 < s.cells()[0] < 8192
    m = keep & ((hour >= BASE + 1) & (hour < BASE + 3))
    _same(s.window_counts(BASE + 1, BASE + 3), oracle.count(lat, lon, m.astype(np.uint8), 0, 6))
    before = s.cells()[0]
    dropped, freed = s.expire(BASE + 2)
    assert dropped == before - s.cells()[0] and dropped > 0
    assert s.buckets() == len(np.unique(hour[(keep == 1) & (hour >= BASE + 2)]))
    _same(s.counts(ALLTIME), oracle.count(lat, lon, keep & (hour >= BASE + 2), 0, 6))
    _same(s.window_counts(BASE, BASE + 3), oracle.count(lat, lon, keep & (hour == BASE + 2), 0, 6))
    s.close()


# ---------------------------------------------------------------- retention

def _group_of(users):
    """the row group of each user id: 'x...' ids have none"""
    return np.where(np.char.startswith(users, "x"), "", users)


def test_expire_mid_data(gpu, data):
    """(11) expire(cut) with the cut inside a batch's hours and an undated
    batch in the stream; (12) then a batch of a new hour and a batch of an
    expired hour (its bucket is created again)."""
    s = data.stream()
    ulat, ulon = _undated()
    uusers = np.array(["u1", "xhidden"])[np.arange(len(ulat)) % 2]
    s.add(ulat, ulon, user_id=uusers.tolist())
    cut = BASE + 8
    s.rollup("day", merge_groups=False)         # label buckets: reclaimed by the expire
    s.window(BASE, BASE + 3)
    buckets_before = s.buckets()
    before = s.cells()[0]
    dropped, freed = s.expire(cut)
    # exact: the surviving (group, hour) pairs, the undated ones included; no label is left
    kept = (data.keep == 1) & (data.hour >= cut)
    pairs = {(g, h) for g, h in zip(_group_of(data.users[kept]).tolist(), data.hour[kept].tolist())}
    pairs |= {(g, -1) for g in _group_of(uusers).tolist()}
    assert s.buckets() == len(pairs)
    assert freed == buckets_before - len(pairs) and freed > 0
    after = s.cells()[0]
    assert dropped == before - after and dropped > 0
    lat = np.concatenate([data.lat, ulat])
    lon = np.concatenate([data.lon, ulon])
    alive = np.concatenate([kept, np.ones(len(ulat), bool)]).astype(np.uint8)
    _same(s.counts(ALLTIME), oracle.count(lat, lon, alive, ZMIN, ZMAX))
    hourly = s.hourly()
    assert sorted(hourly) == sorted(np.unique(data.hour[kept]).tolist()) and min(hourly) >= cut
    for h in (cut, BASE + 17):
        _same(hourly[h], data.ref(h, h + 1))
    # cells: one per (bucket, cell) -- every (group, hour)'s, plus the undated buckets'
    per_bucket = len(s.rollup("hour", merge_groups=False)[0])
    und = sum(len(oracle.count(ulat, ulon, (_group_of(uusers) == g).astype(np.uint8), ZMIN, ZMAX)["count"])
              for g in ("u1", ""))
    assert after == per_bucket + und
    assert s.cells()[0] == after
    # (12) a new hour and an expired hour after the expire
    nlat, nlon = synth.generate("hotspots", 20000, seed=7, start=6 * 20000)
    s.add(nlat, nlon, None, np.full(20000, BASE + 30, np.uint32), user_id=["u2"] * 20000)
    old = BASE + 2
    olat, olon = synth.generate("hotspots", 20000, seed=7, start=7 * 20000)
    s.add(olat, olon, None, np.full(20000, old, np.uint32), user_id=["u3"] * 20000)
    lat, lon = np.concatenate([lat, nlat, olat]), np.concatenate([lon, nlon, olon])
    alive = np.concatenate([alive, np.ones(40000, np.uint8)])
    hour = np.concatenate([data.hour, np.full(len(ulat), -1), np.full(20000, BASE + 30), np.full(20000, old)])
    _same(s.counts(ALLTIME), oracle.count(lat, lon, alive, ZMIN, ZMAX))
    _same(s.counts(old), oracle.count(olat, olon, None, ZMIN, ZMAX))
    for lo, hi in ((BASE, BASE + 10), (BASE + 16, BASE + 31)):
        _same(s.window_counts(lo, hi), oracle.count(lat, lon, alive & ((hour >= lo) & (hour < hi)), ZMIN, ZMAX))
    s.close()


def test_expire_nothing_and_everything(gpu, data):
    """(13) a cut with nothing below it returns (0, 0) and changes nothing;
    (14) a cut past every hour leaves the undated cells only, or nothing, and a
    later add works."""
    s = data.stream(users=False, base=BASE - 10)
    s.window(BASE, BASE + 5)
    nb, nc = s.buckets(), s.cells()[0]
    for cut in (BASE, BASE - 5, BASE - 10, BASE - 1000):
        assert s.expire(cut) == (0, 0)
        assert (s.buckets(), s.cells()[0]) == (nb, nc)
    _same(s.counts(ALLTIME), data.ref(BASE, BASE + 18))
    assert s.ctx.L.hm_stream_expire(s.ptr, BASE, None, None) == _lib.HM_OK      # the outputs are optional
    dropped, freed = s.expire(BASE + 1000)
    assert dropped == nc and s.cells()[0] == 0 and s.buckets() == 0
    assert s.counts(ALLTIME).count.size == 0 and s.hourly() == {}
    assert s.expire(BASE + 2000) == (0, 0)
    lat, lon, keep, hour, _ = data.batches[2]
    s.add(lat, lon, keep, hour)
    _same(s.counts(ALLTIME), oracle.count(lat, lon, keep, ZMIN, ZMAX))
    s.close()
    # with an undated batch: it alone survives
    s = data.stream(users=False)
    ulat, ulon = _undated()
    s.add(ulat, ulon)
    und = oracle.count(ulat, ulon, None, ZMIN, ZMAX)
    s.expire(BASE + (1 << 30))
    assert s.cells()[0] == len(und["count"]) and s.buckets() == 1
    _same(s.counts(ALLTIME), und)
    assert s.hourly() == {}
    lat, lon, keep, hour, _ = data.batches[0]
    s.add(lat, lon, keep, hour)
    _same(s.window_counts(BASE, BASE + 3), oracle.count(lat, lon, keep, ZMIN, ZMAX))
    s.close()


def test_expire_non_compact_and_many_buckets(gpu, data):
    """(15) expire on a log with repeated keys, and after one batch of 70
    groups in one hour (more than HMS_MAX_PARTS buckets: the grouped fold)."""
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    lat, lon, keep, hour, _ = data.batches[0]           # hours BASE .. BASE + 2
    rng = np.random.default_rng(15)
    gid = rng.integers(0, 3, len(lat)).astype(np.uint32)
    s.add(lat, lon, keep, hour, group=gid)
    s.add(lat, lon, keep, hour, group=gid)              # every key twice: not compact
    glat, glon = synth.generate("hotspots", 20000, seed=15)
    g70 = rng.integers(0, 70, 20000).astype(np.uint32)
    s.add(glat, glon, None, np.full(20000, BASE + 2, np.uint32), group=g70)
    cut = BASE + 1
    s.expire(cut)
    k0 = keep & (hour >= cut)
    alat, alon = np.concatenate([lat, lat, glat]), np.concatenate([lon, lon, glon])
    alive = np.concatenate([k0, k0, np.ones(20000, np.uint8)])
    ag = np.concatenate([gid, gid, g70])
    ah = np.concatenate([hour, hour, np.full(20000, BASE + 2)]).astype(np.int64)
    assert s.buckets() == len({(g, h) for g, h in zip(ag[alive == 1].tolist(), ah[alive == 1].tolist())})
    _same(s.counts(ALLTIME), oracle.count(alat, alon, alive, ZMIN, ZMAX))
    _same(s.window_counts(BASE + 2, BASE + 3), oracle.count(alat, alon, alive & (ah == BASE + 2), ZMIN, ZMAX))
    g, z, r, c, cnt = s.window(BASE, BASE + 3, merge_groups=False)
    for u in (0, 2, 69):
        m = g == u
        _same(Counts(z[m], r[m], c[m], cnt[m], 0, []), oracle.count(alat, alon, alive & (ag == u), ZMIN, ZMAX))
    # a batch after it lands in the re-keyed log
    s.add(lat, lon, keep, hour, group=gid)
    alat, alon = np.concatenate([alat, lat]), np.concatenate([alon, lon])
    alive = np.concatenate([alive, keep])
    _same(s.counts(ALLTIME), oracle.count(alat, alon, alive, ZMIN, ZMAX))
    s.close()


def test_expire_reclaims_bucket_slots(gpu):
    """(16) more one-hour batches than the bucket table has slots (max_buckets
    = 1, the smallest hm_stream_create takes: 1024 slots), with expire(newest -
    8) after each: no HM_E_CAPACITY, and never more buckets than the 9 retained
    hours plus the labels interned since the last expire (one: the merged
    window's).  The same batches without expire run out of buckets."""
    nhours, n = 1040, 2000
    pool = 16
    lat, lon = synth.generate("hotspots", pool * n, seed=16)
    part = lambda h: slice((h % pool) * n, (h % pool + 1) * n)   # noqa: E731
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, max_buckets=1)
    cap = None
    for h in range(nhours):
        s.add(lat[part(h)], lon[part(h)], None, np.full(n, BASE + h, np.uint32))
        s.expire(BASE + h - 8)
        assert s.buckets() <= 9
        if h % 64 == 63 or h == nhours - 1:
            nw, _, _, _ = s.window_device(BASE + h - 8, BASE + h + 1)
            assert nw > 0 and s.buckets() <= 9 + 1
            cap = cap or s.cells()[1]
            assert s.cells()[1] == cap                   # the log stopped growing
    last = np.concatenate([np.arange(n) + (h % pool) * n for h in range(nhours - 9, nhours)])
    _same(s.window_counts(BASE, BASE + nhours), oracle.count(lat[last], lon[last], None, ZMIN, ZMAX))
    _same(s.counts(ALLTIME), oracle.count(lat[last], lon[last], None, ZMIN, ZMAX))
    s.close()
    # the control: the same stream without retention runs out of bucket slots
    c = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, max_buckets=1)
    with pytest.raises(RuntimeError, match="capacity"):
        for h in range(nhours):
            c.add(lat[part(h)], lon[part(h)], None, np.full(n, BASE + h, np.uint32))
    assert 1000 <= c.buckets() <= 1024
    c.close()
