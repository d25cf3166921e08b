"""Export, import and merge of the resident streaming heatmap (hm_stream_export,
hm_stream_import; StreamingHeatmap.snapshot / save / load / restore /
merge_from) vs the oracle and vs the stream the state came from.

The streams hold well over 256 * 8 = 2048 cells, so the import kernel runs
several blocks and a ragged last chunk; the kernel-edge cases import synthetic
cells of known sums at the wave edge (64) and the block-chunk edge (2048)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, synth
from heatmap_amd.stream import ALLTIME, NOGROUP, UNDATED_HOUR, StreamingHeatmap

pytestmark = pytest.mark.gpu
BASE = 480000  # epoch hour (2024-10-04)
ZMIN, ZMAX = 0, 18
USERS = ["u1", "u2", "u3", "xhidden", "xother"]


def _rec(*cols):
    """records of the columns, sorted"""
    a = np.stack([np.asarray(c).astype(np.int64) for c in cols], axis=1)
    return a[np.lexsort(a.T[::-1])]


def _same(got, ref):
    got = got.sorted()
    assert ref["status"] == 0
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k]), k


class Data:
    """6 batches x 20 000 'hotspots' points; a batch's hours overlap the next
    one's (BASE + 3b .. BASE + 3b + 2), 10% dropped by keep, three user groups
    and two 'x...' ids (no group)."""

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
        # an undated batch and a few kept points outside the square (hour BASE + 9)
        self.ulat, self.ulon = synth.generate("hotspots", 5000, seed=77)
        self.uusers = [USERS[i] for i in np.arange(5000) % 4]
        xlat, xlon = synth.generate("hotspots", 60, seed=91)
        self.xlat, self.xlon = xlat.copy(), xlon.copy()
        self.xlat[:20] = np.where(np.arange(20) % 2, 1.0, -1.0) * np.linspace(85.06, 89.9, 20)
        self.xlon[10:40] = np.tile([180.0, 200.0, 540.0], 10)
        self._memo = {}

    def feed(self, s, which=range(6), users=True):
        for b in which:
            lat, lon, keep, hour, us = self.batches[b]
            s.add(lat, lon, keep, hour, user_id=us if users else None)
        return s

    def stream(self, which=range(6), users=True, base=BASE, **kw):
        return self.feed(StreamingHeatmap(ZMIN, ZMAX, base_hour=base, **kw), which, users)

    def full(self):
        """the six batches, the undated batch and the out-of-square points"""
        s = self.stream()
        s.add(self.ulat, self.ulon, user_id=self.uusers)
        s.add(self.xlat, self.xlon, None, np.full(60, BASE + 9, np.uint32), user_id=["u2"] * 60)
        assert len(s._x)
        return s

    def ref(self, lo, hi, batches=range(6)):
        """oracle.count over keep & (lo <= hour < hi) of the batches, computed once"""
        key = (lo, hi, tuple(batches))
        if key not in self._memo:
            inb = np.isin(np.arange(len(self.lat)) // 20000, list(batches))
            m = (self.keep == 1) & (self.hour >= lo) & (self.hour < hi) & inb
            self._memo[key] = oracle.count(self.lat, self.lon, m.astype(np.uint8), ZMIN, ZMAX)
        return self._memo[key]


@pytest.fixture(scope="module")
def data():
    return Data()


def _state(s):
    """everything a query can see of a stream, in comparable form"""
    a = s.counts(ALLTIME).sorted()
    return {"alltime": _rec(a.zoom, a.row, a.col, a.count),
            "hourly": _rec(*s.rollup("hour", merge_groups=False)),
            "window": _rec(*s.window(BASE + 4, BASE + 11)),
            "view": _rec(*s.view([(6, 0, 64, 0, 64), (12, 1000, 3000, 500, 3500)], (BASE + 2, BASE + 15), "each")),
            "cells": s.cells()[0], "labels": list(s.labels)}


def _assert_state(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert (np.array_equal(got[k], v) if isinstance(v, np.ndarray) else got[k] == v), k


# -------------------------------------------------------- snapshot round trip

def test_round_trip_restore_and_file(gpu, data, tmp_path):
    """(1) restore(snapshot()) and load(save()) answer every query as the
    source does, and the source's alltime counts are the oracle's."""
    a = data.full()
    want = _state(a)
    assert len(want["view"]) and len(want["window"])
    lat = np.concatenate([data.lat, data.ulat, data.xlat])
    lon = np.concatenate([data.lon, data.ulon, data.xlon])
    keep = np.concatenate([data.keep, np.ones(5060, np.uint8)])
    _same(a.counts(ALLTIME), oracle.count(lat, lon, keep, ZMIN, ZMAX))
    rows = a.rows("day")
    assert rows
    snap = a.snapshot()
    assert snap["labels"].tolist() == a.labels and (snap["hours"] == _lib.HM_STREAM_UNDATED).any()
    b = StreamingHeatmap.from_snapshot(snap)
    path = tmp_path / "stream.npz"
    a.save(path)
    with np.load(path, allow_pickle=False) as f:
        assert int(f["version"]) == 1 and len(f["keys"]) == len(snap["keys"])
    c = StreamingHeatmap.load(path, initial_cells=4096)
    for s in (b, c):
        assert (s.zmin, s.zmax, s.base_hour) == (ZMIN, ZMAX, BASE)
        _assert_state(_state(s), want)
        assert s.rows("day") == rows
        assert np.array_equal(_rec(*s.export()), _rec(*a.export()))
    _assert_state(_state(a), want)               # the source is as it was
    # into an existing stream: other zooms are refused, the same zooms join
    d = StreamingHeatmap(ZMIN, ZMAX - 1, base_hour=BASE)
    with pytest.raises(ValueError, match="zooms"):
        d.restore(snap)
    with pytest.raises(ValueError, match="zooms"):
        StreamingHeatmap.load(path, zmax=ZMAX - 1)
    with pytest.raises(ValueError, match="version"):
        d.restore(dict(snap, version=99))
    assert d.cells()[0] == 0
    for s in (a, b, c, d):
        s.close()


def test_export_content(gpu, data):
    """(2) the dated records are the hourly per-group rollup, the undated ones
    carry HM_STREAM_UNDATED (-1 in export()) and are the undated batch's
    cells, and the counts sum to 19 zooms x the kept points."""
    s = data.stream()
    s.add(data.ulat, data.ulon)                    # undated, no group
    g, h, z, r, c, cnt = s.export()
    assert h.dtype == np.int64 and g.dtype == np.uint32
    dated = h != UNDATED_HOUR
    assert np.array_equal(_rec(g[dated], h[dated], z[dated], r[dated], c[dated], cnt[dated]),
                          _rec(*s.rollup("hour", merge_groups=False)))
    und = oracle.count(data.ulat, data.ulon, None, ZMIN, ZMAX)
    assert (g[~dated] == NOGROUP).all()
    assert np.array_equal(_rec(z[~dated], r[~dated], c[~dated], cnt[~dated]),
                          _rec(und["zoom"], und["row"], und["col"], und["count"]))
    assert int(cnt.sum()) == (int(data.keep.sum()) + 5000) * (ZMAX - ZMIN + 1)
    assert len(cnt) == s.cells()[0]
    # the C level: the undated marker, optional outputs, capacity
    n, keys, counts, groups, hours = s.export_device()
    hw = hours[:n].cpu().numpy().view(np.uint32)
    assert n == len(cnt) and int((hw == _lib.HM_STREAM_UNDATED).sum()) == len(und["count"])
    assert hw[hw != _lib.HM_STREAM_UNDATED].min() == BASE and hw[hw != _lib.HM_STREAM_UNDATED].max() == BASE + 17
    k2, c2 = gpu.empty_like(keys), gpu.empty_like(counts)
    m = ctypes.c_int64(0)
    L = s.ctx.L
    assert L.hm_stream_export(s.ptr, k2.data_ptr(), c2.data_ptr(), None, None, n, ctypes.byref(m)) == _lib.HM_OK
    assert m.value == n and np.array_equal(_rec(k2[:n].cpu().numpy(), c2[:n].cpu().numpy()),
                                           _rec(keys[:n].cpu().numpy(), counts[:n].cpu().numpy()))
    for cap in (0, n - 1):
        m = ctypes.c_int64(0)
        rc = L.hm_stream_export(s.ptr, k2.data_ptr(), c2.data_ptr(), None, None, cap, ctypes.byref(m))
        assert rc == _lib.HM_E_CAPACITY and m.value == n
    assert L.hm_stream_export(s.ptr, None, None, None, None, 4, ctypes.byref(m)) == _lib.HM_E_ARG
    s.close()
    e = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    m = ctypes.c_int64(7)
    assert e.ctx.L.hm_stream_export(e.ptr, None, None, None, None, 0, ctypes.byref(m)) == _lib.HM_OK and m.value == 0
    assert e.export_device()[0] == 0 and all(len(v) == 0 for v in e.export())
    assert e.ctx.L.hm_stream_import(e.ptr, None, None, None, None, 0, 0) == _lib.HM_OK
    e.close()


def test_restore_then_keep_streaming(gpu, data):
    """(3) a stream restored after batch 3 and the original, both fed batches
    4-6 and expired: equal windows, cells and buckets, equal to the oracle over
    the surviving hours; and a restored stream fed one-hour batches of new
    hours holds exactly the sum of its parts."""
    a = data.stream(range(3))
    b = StreamingHeatmap.from_snapshot(a.snapshot())
    n0 = b.cells()[0]
    assert n0 == a.cells()[0] > 2048
    for s in (a, b):
        data.feed(s, range(3, 6))
        s.expire(BASE + 7)
    assert a.cells()[0] == b.cells()[0]
    assert a.buckets() == b.buckets() == len({(u if u[0] != "x" else "", h) for u, h, k in
                                              zip(data.users.tolist(), data.hour.tolist(), data.keep.tolist())
                                              if k and h >= BASE + 7})
    for merge in (True, False):
        assert np.array_equal(_rec(*a.window(BASE + 7, BASE + 18, merge)), _rec(*b.window(BASE + 7, BASE + 18, merge)))
    _same(b.window_counts(BASE + 7, BASE + 18), data.ref(BASE + 7, BASE + 18))
    _same(b.counts(ALLTIME), data.ref(BASE + 7, BASE + 18))
    assert a.cells()[0] == b.cells()[0]
    a.close()
    b.close()
    # new one-hour batches after a restore: cells() is the sum of the parts
    src = data.stream(range(3), users=False)
    r = StreamingHeatmap.from_snapshot(src.snapshot(), initial_cells=1 << 16)
    total = r.cells()[0]
    assert total == src.cells()[0]
    for j in range(3):
        lat, lon = synth.generate("hotspots", 3000, seed=31, start=j * 3000)
        r.add(lat, lon, None, np.full(3000, BASE + 100 + j, np.uint32))
        total += len(oracle.count(lat, lon, None, ZMIN, ZMAX)["count"])
        assert r.cells()[0] == total
    src.close()
    r.close()


def _by_label(s, g, *cols):
    """records with the group id replaced by its label's rank among `names`"""
    names = sorted(set(USERS) | {"all"})
    code = np.array([names.index(s.labels[i]) if i != NOGROUP else -1 for i in g.tolist()], dtype=np.int64)
    return _rec(code, *cols)


def test_merge_from(gpu, data):
    """(4) two shards with different label ids and base hours merged == one
    stream fed everything; the source is unchanged; hours that do not fit are
    refused before anything changes."""
    # three points that fix S2's label order (u3 before u2 before u1), one outside the square
    tlat, tlon = np.array([10.0, 86.5, -20.0]), np.array([20.0, 30.0, 200.0])
    thour = np.full(3, BASE + 4, np.uint32)
    s1 = data.stream((0, 2, 4))
    s2 = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE - 50)
    s2.add(tlat[:2], tlon[:2], None, thour[:2], user_id=["u3", "u3"])
    s2.add(tlat[2:], tlon[2:], None, thour[2:], user_id=["u2"])
    data.feed(s2, (1, 3, 5))
    one = data.stream()
    one.add(tlat, tlon, None, thour, user_id=["u3", "u3", "u2"])
    assert s1.labels != s2.labels and sorted(s1.labels) == sorted(s2.labels) and len(s2._x)
    before2 = (_rec(*s2.export()), list(s2.labels), s2.cells()[0])
    s1.merge_from(s2)
    assert s1.rows("alltime") == one.rows("alltime")
    lo, hi = BASE + 2, BASE + 13
    g, z, r, c, cnt = s1.window(lo, hi, merge_groups=False)
    og, oz, orow, oc, ocnt = one.window(lo, hi, merge_groups=False)
    assert np.array_equal(_by_label(s1, g, z, r, c, cnt), _by_label(one, og, oz, orow, oc, ocnt))
    a, b = s1.counts(ALLTIME).sorted(), one.counts(ALLTIME).sorted()
    assert np.array_equal(_rec(a.zoom, a.row, a.col, a.count), _rec(b.zoom, b.row, b.col, b.count))
    assert s1.cells()[0] == one.cells()[0]
    assert np.array_equal(_rec(*s2.export()), before2[0]) and s2.labels == before2[1] and s2.cells()[0] == before2[2]
    # an hour below s1's base: refused, nothing changes (not even the labels)
    s3 = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE - 100)
    lat, lon, keep, hour, _ = data.batches[0]
    s3.add(lat[:500], lon[:500], None, np.full(500, BASE - 5, np.uint32), user_id=["newcomer"] * 500)
    before1 = (_rec(*s1.export()), list(s1.labels))
    with pytest.raises(ValueError, match="hours"):
        s1.merge_from(s3)
    assert np.array_equal(_rec(*s1.export()), before1[0]) and s1.labels == before1[1]
    z17 = StreamingHeatmap(ZMIN, ZMAX - 1, base_hour=BASE)
    with pytest.raises(ValueError, match="zooms"):
        s1.merge_from(z17)
    for s in (s1, s2, s3, one, z17):
        s.close()


def test_repeated_cells_add_up(gpu, data):
    """(5) the same export imported twice: every count doubles and the
    distinct cells stay; cells of an hour that a later add also brings sum
    with it; a snapshot restored into a stream that holds its hours sums too."""
    src = data.stream(range(2))
    n, keys, counts, groups, hours = src.export_device()
    want = _rec(*src.export())
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    for _ in range(2):
        s.import_cells(keys[:n], counts[:n], groups[:n], hours[:n], labels=src.labels)
    assert s.cells()[0] == n
    want2 = want.copy()
    want2[:, 5] *= 2
    assert np.array_equal(_rec(*s.export()), want2)
    s.close()
    # import, then an add of the same hours
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    s.import_cells(keys[:n], counts[:n], groups[:n], hours[:n], labels=src.labels, distinct=True)
    assert s.cells()[0] == n
    data.feed(s, [1])
    both = oracle.count(np.concatenate([data.lat[:40000], data.batches[1][0]]),
                        np.concatenate([data.lon[:40000], data.batches[1][1]]),
                        np.concatenate([data.keep[:40000], data.batches[1][2]]), ZMIN, ZMAX)
    _same(s.counts(ALLTIME), both)
    s.close()
    # a distinct import into buckets that hold cells already is not compact
    t = data.stream(range(2))
    t.restore(src.snapshot())
    assert t.cells()[0] == n and t.labels == src.labels
    assert np.array_equal(_rec(*t.export()), want2)
    t.close()
    src.close()


# ---------------------------------------------------------------- kernel edges

def _cells(n, pattern, zmin=0):
    """n synthetic cells (keys, counts, groups or None, hours or None) and
    their sums per (group, hour, zoom, row, col), sorted.  Keys repeat (cell i
    and cell i + m share one), so some sums have two terms."""
    i = np.arange(n, dtype=np.int64)
    j = i % max(1, n - n // 4)
    z = 18 - (j % 3)
    r = (j * 2654435761) % (1 << z)
    c = (j * 40503) % (1 << z)
    z[j == 0], r[j == 0], c[j == 0] = 18, (1 << 18) - 1, (1 << 18) - 1     # the square's last cell
    z[j == 1], r[j == 1], c[j == 1] = zmin, 0, 0                            # the first cell of the lowest zoom
    keys = ((z.astype(np.uint64) << np.uint64(58)) | (r.astype(np.uint64) << np.uint64(29)) | c.astype(np.uint64))
    counts = (i % 5 + 1).astype(np.uint64)
    counts[0] = 1 << 40
    if pattern == "one":          # one bucket
        groups, hours = None, np.full(n, BASE + 3, np.uint32)
    elif pattern == "own":        # every cell its own (group, hour): every lane probes alone
        groups, hours = i.astype(np.uint32), (BASE + i % 40).astype(np.uint32)
    elif pattern == "runs":       # runs of 100 cells alternating between two buckets
        groups, hours = None, (BASE + (i // 100) % 2).astype(np.uint32)
    elif pattern == "undated":    # neither array
        groups, hours = None, None
    else:                         # three groups, two hours in runs
        groups, hours = (i % 3).astype(np.uint32), (BASE + (i // 100) % 2).astype(np.uint32)
    g = np.full(n, NOGROUP, np.int64) if groups is None else groups.astype(np.int64)
    h = np.full(n, UNDATED_HOUR, np.int64) if hours is None else hours.astype(np.int64)
    u, inv = np.unique(np.stack([g, h, z, r, c], axis=1), axis=0, return_inverse=True)
    tot = np.zeros(len(u), dtype=np.int64)
    np.add.at(tot, inv.reshape(-1), counts.astype(np.int64))
    return keys, counts, groups, hours, _rec(*u.T, tot)


@pytest.mark.parametrize("pattern", ["one", "own", "runs"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_import_kernel_edges(gpu, n, pattern):
    """(6) sizes at the wave edge and the block-chunk edge of the 256 x 8
    layout, for each bucket pattern: the export is the input summed per key."""
    keys, counts, groups, hours, want = _cells(n, pattern)
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=4096, max_buckets=4096)
    s.import_cells(keys, counts, groups, hours)
    assert np.array_equal(_rec(*s.export()), want)
    assert s.cells()[0] == len(want)
    assert s.buckets() == len(np.unique(want[:, :2], axis=0))
    s.close()


def test_import_grows_the_log_and_takes_device_tensors(gpu):
    """(6) 50 000 cells into a log of 1024: it has to grow; no groups and no
    hours at all; CUDA tensors as input."""
    keys, counts, groups, hours, want = _cells(50000, "runs")
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1024)
    assert s.cells()[1] == 1024
    s.import_cells(keys, counts, groups, hours)
    assert s.cells()[1] >= 50000
    assert np.array_equal(_rec(*s.export()), want)
    s.close()
    keys, counts, groups, hours, want = _cells(3000, "undated")
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1024)
    s.import_cells(gpu.from_numpy(keys.view(np.int64)).cuda(), gpu.from_numpy(counts.view(np.int64)).cuda())
    assert np.array_equal(_rec(*s.export()), want)
    assert s.buckets() == 1
    # int64 hours with UNDATED_HOUR, explicit group ids: as export() returns them
    g, h, z, r, c, cnt = s.export()
    k = (z.astype(np.uint64) << np.uint64(58)) | (r.astype(np.uint64) << np.uint64(29)) | c.astype(np.uint64)
    t = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    t.import_cells(k, cnt, g, h, distinct=True)
    assert np.array_equal(_rec(*t.export()), want) and t._explicit_max == -1
    t.import_cells(k[:10], cnt[:10], np.full(10, 41, np.uint32), h[:10])
    assert t._explicit_max == 41 and t.buckets() == 2
    with pytest.raises(ValueError, match="same length"):
        t.import_cells(k, cnt[:5])
    with pytest.raises(ValueError, match="one entry per cell"):
        t.import_cells(k, cnt, g[:5])
    with pytest.raises(ValueError, match="cell 3: hour"):
        t.import_cells(k[:10], cnt[:10], None, np.array([BASE] * 3 + [1 << 33] + [BASE] * 6, dtype=np.int64))
    with pytest.raises(ValueError, match="cell 2: group id 5 "):
        t.import_cells(k[:4], cnt[:4], np.array([0, 1, 5, 1], np.uint32), h[:4], labels=["all", "u1"])
    assert t.labels == ["all"]
    s.close()
    t.close()


def _key(z, r, c):
    return np.uint64((z << 58) | (r << 29) | c)


BAD = {"zoom_below_zmin": ("key", _key(1, 0, 0)), "zoom_above_zmax": ("key", _key(19, 0, 0)),
       "row_2^z": ("key", _key(5, 32, 0)), "col_2^z": ("key", _key(5, 0, 32)), "count_0": ("count", 0),
       "group_allgroups": ("group", 0xFFFFFFFF), "hour_below_base": ("hour", BASE - 1),
       "hour_past_range": ("hour", BASE + (1 << 28))}


@pytest.mark.parametrize("kind", list(BAD))
def test_import_invalid_cell(gpu, kind):
    """(7) one invalid cell at index 1337 and a later one at 2500, valid cells
    around both: ValueError naming 1337 (HM_E_ARG and hm_last_error at the C
    level), nothing appended; a valid import and an add still work."""
    zmin = 2
    keys, counts, groups, hours, want = _cells(3000, "groups", zmin=zmin)
    s = StreamingHeatmap(zmin, ZMAX, base_hour=BASE, initial_cells=4096, max_buckets=4096)
    s.import_cells(keys[:500], counts[:500], groups[:500], hours[:500])
    before = _rec(*s.export())
    arrays = {"key": keys.copy(), "count": counts.copy(), "group": groups.copy(), "hour": hours.copy()}
    what, value = BAD[kind]
    arrays[what][1337] = value
    later = "key" if what == "count" else "count"
    arrays[later][2500] = _key(19, 0, 0) if later == "key" else 0
    with pytest.raises(ValueError, match="cell 1337 "):
        s.import_cells(arrays["key"], arrays["count"], arrays["group"], arrays["hour"])
    dev = [gpu.from_numpy(arrays[k].view(np.int64 if arrays[k].itemsize == 8 else np.int32)).cuda()
           for k in ("key", "count", "group", "hour")]
    rc = s.ctx.L.hm_stream_import(s.ptr, *(t.data_ptr() for t in dev), 3000, 0)
    assert rc == _lib.HM_E_ARG and s.ctx.last_error() == (1337, _lib.HM_E_ARG)
    assert np.array_equal(_rec(*s.export()), before)
    # the later cell alone is reported when the first is mended
    arrays[what][1337] = {"key": keys, "count": counts, "group": groups, "hour": hours}[what][1337]
    with pytest.raises(ValueError, match="cell 2500 "):
        s.import_cells(arrays["key"], arrays["count"], arrays["group"], arrays["hour"])
    assert np.array_equal(_rec(*s.export()), before)
    total = int(before[:, 5].sum())
    s.import_cells(keys, counts, groups, hours)
    total += int(counts.astype(np.int64).sum())
    assert int(s.export()[5].sum()) == total
    lat, lon = synth.generate("hotspots", 2000, seed=3)
    s.add(lat, lon, None, np.full(2000, BASE + 1, np.uint32))
    assert int(s.export()[5].sum()) == total + 2000 * (ZMAX - zmin + 1)
    assert int(s.counts(ALLTIME).count.sum()) == total + 2000 * (ZMAX - zmin + 1)
    s.close()


def test_import_bucket_table_full(gpu):
    """(7) a 1024-slot bucket table (hm_stream_create's smallest, which
    max_buckets = 1 gives: max_buckets = 1024 is rounded up to 2048 slots) and
    2000 distinct hours: HM_E_CAPACITY, and the counts are unchanged."""
    keys, counts, groups, hours, _ = _cells(2000, "one")
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=4096, max_buckets=1)
    s.import_cells(keys[:300], counts[:300], None, hours[:300])
    before = _rec(*s.export())
    with pytest.raises(RuntimeError, match="capacity"):
        s.import_cells(keys, counts, None, (BASE + np.arange(2000)).astype(np.uint32))
    assert s.buckets() <= 1024
    assert np.array_equal(_rec(*s.export()), before)
    assert s.cells()[0] == len(before)
    s.close()
