"""Forgetting and selective export of the resident streaming heatmap
(hm_stream_forget, hm_stream_export_select; StreamingHeatmap.forget and the
users / groups / hours arguments of export, snapshot and merge_from).

The model is the stream's own export() taken before the call and filtered in
numpy; where stated the C oracle over the raw points is used instead.  The
main stream is test_gpu_stream_snapshot.py's recipe (six 20 000-point batches,
an undated batch, out-of-square points): its log is many 8192-cell chunks with
a ragged last one.  The kernel-edge cases import synthetic distinct cells, so
a cell's place in the log, its group and the chunk it falls in are known."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, device, synth
from heatmap_amd.stream import ALLTIME, NOGROUP, UNDATED_HOUR, StreamingHeatmap

pytestmark = pytest.mark.gpu
BASE = 480000  # epoch hour (2024-10-04)
ZMIN, ZMAX = 0, 18
USERS = ["u1", "u2", "u3", "xhidden", "xother"]
MID = (BASE + 4, BASE + 11)
U32P = ctypes.POINTER(ctypes.c_uint32)


def _rec(*cols):
    """records of the columns, sorted"""
    a = np.stack([np.asarray(c).astype(np.int64) for c in cols], axis=1)
    return a[np.lexsort(a.T[::-1])]


def _summed(*cols):
    """sorted records with the last column summed over equal leading ones"""
    a = _rec(*cols)
    if not len(a):
        return a
    u, inv = np.unique(a[:, :-1], axis=0, return_inverse=True)
    tot = np.zeros(len(u), dtype=np.int64)
    np.add.at(tot, inv.reshape(-1), a[:, -1])
    return np.concatenate([u, tot[:, None]], axis=1)


def _same(got, ref):
    got = got.sorted()
    assert ref["status"] == 0
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k]), k


def _selected(cols, ids=None, hours=None):
    """mask of export() columns (group, hour, ...) inside a selection"""
    g, h = np.asarray(cols[0]).astype(np.int64), np.asarray(cols[1]).astype(np.int64)
    m = np.ones(len(g), dtype=bool)
    if ids is not None:
        m &= np.isin(g, np.array(list(ids), dtype=np.int64))
    if hours is not None:
        m &= (h != UNDATED_HOUR) & (h >= hours[0]) & (h < hours[1])
    return m


def _only(cols, m):
    return tuple(np.asarray(c)[m] for c in cols)


class Data:
    """test_gpu_stream_snapshot.py's recipe: 6 batches x 20 000 'hotspots'
    points; a batch's hours overlap the next one's (BASE + 3b .. BASE + 3b +
    2), 10% dropped by keep, three user groups and two 'x...' ids (no group);
    an undated batch; 60 points of u2 at BASE + 9 of which 40 lie outside the
    square."""

    def __init__(self, nb=6, n=20000, seed=7):
        self.batches = []
        for b in range(nb):
            lat, lon = synth.generate("hotspots", n, seed=seed, start=b * n)
            rng = np.random.default_rng(seed * 100 + b)
            hour = (BASE + 3 * b + rng.integers(0, 3, n)).astype(np.uint32)
            keep = (rng.random(n) > 0.1).astype(np.uint8)
            users = [USERS[i] for i in rng.integers(0, len(USERS), n)]
            self.batches.append((lat, lon, keep, hour, users))
        self.ulat, self.ulon = synth.generate("hotspots", 5000, seed=77)
        self.uusers = [USERS[i] for i in np.arange(5000) % 4]
        xlat, xlon = synth.generate("hotspots", 60, seed=91)
        self.xlat, self.xlon = xlat.copy(), xlon.copy()
        self.xlat[:20] = np.where(np.arange(20) % 2, 1.0, -1.0) * np.linspace(85.06, 89.9, 20)
        self.xlon[10:40] = np.tile([180.0, 200.0, 540.0], 10)
        # every point of full(): hour -1 for the undated ones
        self.lat = np.concatenate([b[0] for b in self.batches] + [self.ulat, self.xlat])
        self.lon = np.concatenate([b[1] for b in self.batches] + [self.ulon, self.xlon])
        self.keep = np.concatenate([b[2] for b in self.batches] + [np.ones(5060, np.uint8)])
        self.hour = np.concatenate([b[3].astype(np.int64) for b in self.batches] +
                                   [np.full(5000, UNDATED_HOUR, np.int64), np.full(60, BASE + 9, np.int64)])
        self.users = np.array(sum((b[4] for b in self.batches), []) + self.uusers + ["u2"] * 60)
        self.batch = np.concatenate([np.arange(nb * n) // n, np.full(5060, nb)])
        self._memo = {}

    def feed(self, s, which=range(6)):
        for b in which:
            lat, lon, keep, hour, us = self.batches[b]
            s.add(lat, lon, keep, hour, user_id=us)
        return s

    def full(self, **kw):
        """the six batches, the undated batch and the out-of-square points"""
        s = self.feed(StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, **kw))
        s.add(self.ulat, self.ulon, user_id=self.uusers)
        s.add(self.xlat, self.xlon, None, np.full(60, BASE + 9, np.uint32), user_id=["u2"] * 60)
        assert len(s._x)
        return s

    def ref(self, name, m):
        """oracle.count over keep & m, computed once per name"""
        if name not in self._memo:
            self._memo[name] = oracle.count(self.lat, self.lon, ((self.keep == 1) & m).astype(np.uint8), ZMIN, ZMAX)
        return self._memo[name]

    def in_hours(self, hours):
        return (self.hour != UNDATED_HOUR) & (self.hour >= hours[0]) & (self.hour < hours[1])


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def forgot_u2(gpu, data):
    """(the full stream after forget(users=['u2']), its export() before, the call's answer)"""
    s = data.full()
    before = s.export()
    ret = s.forget(users=["u2"])
    yield s, before, ret
    s.close()


RECTS = [(6, 0, 64, 0, 64), (12, 1000, 3000, 500, 3500)]


def _in_rects(cols):
    z, r, c = (np.asarray(v).astype(np.int64) for v in cols[2:5])
    m = np.zeros(len(z), dtype=bool)
    for rz, rlo, rhi, clo, chi in RECTS:
        m |= (z == rz) & (r >= rlo) & (r < rhi) & (c >= clo) & (c < chi)
    return m


# ------------------------------------------------------------ the main stream

def test_one_user(forgot_u2, data):
    """(1) forget(users=['u2']): the export, the alltime counts, the answer, and a per-group rollup, a window and a
    view hold what the model holds and no cell of u2"""
    s, before, (dropped, freed) = forgot_u2
    u2 = s._index["u2"]
    gone = _selected(before, [u2])                       # (`before` holds the side records too, as the answer does)
    assert gone.any() and not gone.all()
    want = _only(before, ~gone)
    assert np.array_equal(_rec(*s.export()), _rec(*want))
    assert dropped == int(gone.sum())
    assert freed == len(np.unique(_rec(before[0][gone], before[1][gone]), axis=0))   # u2's (group, hour) buckets
    assert "u2" in s.labels and not len(s._x)            # the label stays; the side records were all u2's
    _same(s.counts(ALLTIME), data.ref("not u2", data.users != "u2"))
    g, h = want[0], want[1]
    dated = h != UNDATED_HOUR
    hourly = s.rollup("hour", merge_groups=False)
    assert not (hourly[0] == u2).any()
    assert np.array_equal(_rec(*hourly), _rec(*_only(want, dated)))
    m = _selected(want, None, MID)
    win = s.window(*MID, merge_groups=False)
    assert len(win[0]) and not (win[0] == u2).any()
    assert np.array_equal(_rec(*win), _summed(g[m], *(c[m] for c in want[2:])))
    m = _selected(want, None, (BASE + 2, BASE + 15)) & _in_rects(want)
    view = s.view(RECTS, (BASE + 2, BASE + 15), "each")
    assert len(view[0]) and not (view[0] == u2).any()
    assert np.array_equal(_rec(*view), _summed(g[m], *(c[m] for c in want[2:])))


def test_rasters_after_forgetting_a_user(forgot_u2):
    """(15) a tile that held u2's points: its raster is the model (the export before, without u2) densified"""
    s, before, _ = forgot_u2
    g, h, z, r, c, cnt = (np.asarray(v).astype(np.int64) for v in before)
    u2, b = s._index["u2"], 5
    lim = 1 << 12
    inside = (z == 12) & (r >= 0) & (r < lim) & (c >= 0) & (c < lim)     # side records are never drawn
    mine = np.flatnonzero(inside & (g == u2))
    j = mine[np.argmax(cnt[mine])]
    tile = (12 - b, int(r[j]) >> b, int(c[j]) >> b)

    def dense(m):
        grid = np.zeros((1 << b, 1 << b), dtype=np.int64)
        m = m & inside & ((r >> b) == tile[1]) & ((c >> b) == tile[2])
        np.add.at(grid, (r[m] - (tile[1] << b), c[m] - (tile[2] << b)), cnt[m])
        return grid

    want = dense(g != u2)
    assert (dense(np.ones(len(g), bool)) != want).any()                  # u2 was drawn there
    assert np.array_equal(s.tile_raster([tile], None, None, bins_log2=b)[0].cpu().numpy(), want)
    assert not s.tile_raster([tile], None, "u2", bins_log2=b).any()


def test_middle_hours(gpu, data):
    """(2) hours MID of every group: the window over them is empty, the undated cells stay, alltime = the oracle
    over the complement"""
    s = data.full()
    try:
        before = s.export()
        gone = _selected(before, None, MID)
        assert s.forget(hours=MID)[0] == int(gone.sum()) > 0
        assert len(s.window(*MID)[0]) == 0
        got = s.export()
        assert np.array_equal(_rec(*got), _rec(*_only(before, ~gone)))
        und = before[1] == UNDATED_HOUR
        assert und.any() and np.array_equal(_rec(*_only(got, got[1] == UNDATED_HOUR)), _rec(*_only(before, und)))
        _same(s.counts(ALLTIME), data.ref("not MID", ~data.in_hours(MID)))
    finally:
        s.close()


def test_users_and_hours(gpu, data):
    """(3) only u1's and u3's cells of MID go"""
    s = data.full()
    try:
        before = s.export()
        gone = _selected(before, [s._index["u1"], s._index["u3"]], MID)
        assert s.forget(users=["u3", "u1", "u3"], hours=MID)[0] == int(gone.sum()) > 0
        assert np.array_equal(_rec(*s.export()), _rec(*_only(before, ~gone)))
        _same(s.counts(ALLTIME), data.ref("not u1 u3 of MID", ~(np.isin(data.users, ["u1", "u3"]) & data.in_hours(MID))))
    finally:
        s.close()


def test_against_expire(gpu, data):
    """(4) with label buckets interned: forget(hours=(BASE, cut)) is expire(cut), answer included"""
    a, b = data.full(), data.full()
    try:
        assert a.rows("day") == b.rows("day")
        cut = BASE + 7
        ra, rb = a.expire(cut), b.forget(hours=(BASE, cut))
        assert ra == rb and ra[0] > 0 and ra[1] > 0
        assert np.array_equal(_rec(*a.export()), _rec(*b.export()))
        assert a.buckets() == b.buckets() and a.cells() == b.cells()
    finally:
        a.close()
        b.close()


def test_nothing_selected(gpu, data):
    """(5) an unknown id, a range beyond the data: (0, 0), and the stream as it was, rollup labels included"""
    s = data.full()
    try:
        assert s.rows("day")
        before, cells, buckets = s.export(), s.cells(), s.buckets()
        for kw in ({"groups": [12345]}, {"users": ["nobody"]}, {"hours": (BASE + 100, BASE + 200)},
                   {"hours": (BASE - 50, BASE - 10)}, {"groups": [12345, 777], "hours": (BASE, BASE + 18)},
                   {"users": ["u1"], "hours": (BASE + 18, BASE + 19)}):
            assert s.forget(**kw) == (0, 0), kw
            assert (s.cells(), s.buckets()) == (cells, buckets), kw
        assert "nobody" not in s.labels
        assert np.array_equal(_rec(*s.export()), _rec(*before))
        for kw in ({"groups": [12345]}, {"users": ["nobody"]}, {"hours": (BASE + 100, BASE + 200)}):
            assert all(len(c) == 0 for c in s.export(**kw)), kw
    finally:
        s.close()


def test_everything(gpu, data):
    """(6) the C call with NULL groups and the alltime pair empties the stream; the batches again = the oracle"""
    s = data.full()
    try:
        cells = s.cells()[0]
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert s.ctx.L.hm_stream_forget(s.ptr, None, 0, -1, -1, ctypes.byref(a), ctypes.byref(b)) == _lib.HM_OK
        assert a.value == cells and b.value > 0
        assert s.cells()[0] == 0 and s.buckets() == 0
        s._x = s._x[:0]                                  # (the C call knows nothing of the wrapper's side records)
        data.feed(s)
        _same(s.counts(ALLTIME), data.ref("the six batches", data.batch < 6))
    finally:
        s.close()


def test_nogroup(gpu, data):
    """(7) NOGROUP: only the cells of the 'x...' users go"""
    s = data.full()
    try:
        before = s.export()
        gone = _selected(before, [NOGROUP])
        assert s.forget(groups=[NOGROUP])[0] == int(gone.sum()) > 0
        assert np.array_equal(_rec(*s.export()), _rec(*_only(before, ~gone)))
        _same(s.counts(ALLTIME), data.ref("not x", np.array([u[:1] != "x" for u in data.users])))
    finally:
        s.close()


# ---------------------------------------------------------------- kernel edges

EZ = 9     # the synthetic cells' zoom: 512 x 512 of them


def _cells(n, start=0):
    """n distinct cells of zoom EZ in hm_count's layout, counts i + 1"""
    i = np.arange(start, start + n, dtype=np.uint64)
    return (np.uint64(EZ) << np.uint64(58)) | ((i >> np.uint64(9)) << np.uint64(29)) | (i & np.uint64(511)), i + np.uint64(1)


PATTERNS = {
    "alternate": lambda i: i % 2,
    "by wave": lambda i: (i // 64) % 2,
    "first chunk": lambda i: (i >= 8192).astype(np.int64),
    "last cell": lambda i: (i == len(i) - 1).astype(np.int64),
    "first cell": lambda i: (i == 0).astype(np.int64),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_kernel_edges(gpu, pattern):
    """(8) wave, block-chunk and 8192-cell chunk edges, under each layout of the two groups in the log; forgetting
    either group: export() = the model, and forget and export_select of one selection are complements"""
    for n in (1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 5):
        keys, counts = _cells(n)
        groups = (PATTERNS[pattern](np.arange(n)) + 1).astype(np.uint32)          # 1 or 2
        for target in (2, 1):
            s = StreamingHeatmap(EZ - 1, EZ, base_hour=BASE, initial_cells=1024, max_buckets=1)
            try:
                s.import_cells(keys, counts, groups, np.full(n, BASE + 1, np.uint32), distinct=True)
                before = s.export()
                assert len(before[0]) == n
                gone = _selected(before, [target])
                picked = s.export(groups=[target])
                assert np.array_equal(_rec(*picked), _rec(*_only(before, gone))), (n, target)
                assert s.forget(groups=[target]) == (int(gone.sum()), int(gone.any())), (n, target)
                after = s.export()
                assert np.array_equal(_rec(*after), _rec(*_only(before, ~gone))), (n, target)
                both = tuple(np.concatenate([x, y]) for x, y in zip(picked, after))
                assert np.array_equal(_rec(*both), _rec(*before)), (n, target)
                assert s.cells()[0] == n - int(gone.sum())
            finally:
                s.close()


def test_many_groups(gpu):
    """(9) 2000 groups x 3 hours; sets of 1, 2, 64, 65 and 1000 ids, unsorted, with repeats and with ids that do
    not exist, one after the other on one stream"""
    ng, n = 2000, 6000
    keys, counts = _cells(n)
    i = np.arange(n)
    s = StreamingHeatmap(EZ - 1, EZ, base_hour=BASE, initial_cells=8192)
    try:
        s.import_cells(keys, counts, (i % ng).astype(np.uint32), (BASE + i // ng).astype(np.uint32), distinct=True)
        rng = np.random.default_rng(9)
        order = rng.permutation(ng)
        at = 0
        for size, hours in ((1, None), (2, None), (64, (BASE + 1, BASE + 3)), (65, None), (1000, (BASE, BASE + 1))):
            ids = order[at:at + size]
            at += size
            given = np.concatenate([ids, ids[: size // 2 + 1], [ng + 5, 4000000000, ng + 77]])
            given = given[rng.permutation(len(given))]
            before = s.export()
            gone = _selected(before, ids, hours)
            assert gone.sum() == size * (3 if hours is None else hours[1] - hours[0])
            assert np.array_equal(_rec(*s.export(groups=given, hours=hours)), _rec(*_only(before, gone)))
            assert s.forget(groups=given, hours=hours) == (int(gone.sum()), int(gone.sum()))
            assert np.array_equal(_rec(*s.export()), _rec(*_only(before, ~gone)))
    finally:
        s.close()


def test_forget_reclaims_bucket_slots(gpu):
    """(10) more groups than the bucket table has slots (max_buckets = 1024: 2048 slots), 64 new ones a round with
    the previous round's forgotten: no HM_E_CAPACITY.  The same imports without forget run out of slots."""
    rounds, per = 36, 64
    assert rounds * per > 2048

    def load(s, k):
        keys, counts = _cells(per, k * per)
        s.import_cells(keys, counts, (k * per + np.arange(per)).astype(np.uint32), np.full(per, BASE + k % 5, np.uint32),
                       distinct=True)

    s = StreamingHeatmap(EZ - 1, EZ, base_hour=BASE, initial_cells=1024, max_buckets=1024)
    try:
        for k in range(rounds):
            load(s, k)
            if k:
                assert s.forget(groups=(k - 1) * per + np.arange(per)) == (per, per)
            assert s.buckets() == per
        g, h, z, r, c, cnt = s.export()
        assert np.array_equal(np.sort(g), (rounds - 1) * per + np.arange(per))
        assert np.array_equal(np.sort(cnt), (rounds - 1) * per + np.arange(per) + 1)
    finally:
        s.close()
    c = StreamingHeatmap(EZ - 1, EZ, base_hour=BASE, initial_cells=1024, max_buckets=1024)
    try:
        with pytest.raises(RuntimeError, match="capacity"):
            for k in range(rounds):
                load(c, k)
        assert 2000 <= c.buckets() <= 2048
    finally:
        c.close()


def test_state_around_the_call(gpu, data):
    """(11) a log with repeated keys; a forget right after a rollup; then a batch into a forgotten (group, hour) and
    one into a new hour: the counts are the oracle's over what should be there"""
    lat, lon, keep, hour, us = data.batches[0]
    us = np.array(us)
    lat1, lon1, keep1, _, us1 = data.batches[1]
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    try:
        s.add(lat, lon, keep, hour, user_id=list(us))
        s.add(lat, lon, keep, hour, user_id=list(us))            # the same buckets: the log's keys repeat
        dropped, _ = s.forget(users=["u2"])
        assert dropped > 0
        twice = oracle.count(np.tile(lat, 2), np.tile(lon, 2), np.tile(keep & (us != "u2"), 2).astype(np.uint8), ZMIN,
                             ZMAX)
        _same(s.counts(ALLTIME), twice)
        assert not (s.export()[0] == s._index["u2"]).any()
        assert s.rollup("day")[0].size                           # label buckets
        assert s.forget(users=["u1"], hours=(BASE, BASE + 2))[0] > 0
        s.add(lat, lon, keep, hour, user_id=list(us))            # u1, u2 and their hours come back
        late = np.full(len(lat1), BASE + 40, np.uint32)
        s.add(lat1, lon1, keep1, late, user_id=us1)              # a new hour
        left = keep & (us != "u2") & ~((us == "u1") & (hour < BASE + 2))
        la = np.concatenate([lat, lat, lat, lat1])
        lo = np.concatenate([lon, lon, lon, lon1])
        kp = np.concatenate([left, left, keep, keep1]).astype(np.uint8)
        hr = np.concatenate([hour, hour, hour, late]).astype(np.int64)
        _same(s.counts(ALLTIME), oracle.count(la, lo, kp, ZMIN, ZMAX))
        early = (kp == 1) & (hr < BASE + 2)
        _same(s.window_counts(BASE, BASE + 2), oracle.count(la, lo, early.astype(np.uint8), ZMIN, ZMAX))
        _same(s.window_counts(BASE + 40, BASE + 41), oracle.count(lat1, lon1, keep1, ZMIN, ZMAX))
    finally:
        s.close()


def test_export_select_by_ctypes(gpu, data):
    """(12) the sizing call, capacity n - 1 with a guard behind it, NULL groups_out / hours_out, the records"""
    torch = gpu
    s = data.full()
    try:
        L = s.ctx.L
        n0, k0, c0, g0, h0 = s.export_device()
        full = (g0[:n0].cpu().numpy().view(np.uint32), h0[:n0].cpu().numpy().view(np.uint32).astype(np.int64),
                k0[:n0].cpu().numpy().view(np.uint64) >> np.uint64(32), k0[:n0].cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF),
                c0[:n0].cpu().numpy())
        ids = (ctypes.c_uint32 * 3)(s._index["u3"], s._index["u1"], s._index["u3"])
        m = np.isin(full[0], [s._index["u1"], s._index["u3"]]) & (full[1] >= MID[0]) & (full[1] < MID[1])
        want, n = _rec(*_only(full, m)), int(m.sum())
        assert 0 < n < n0
        got = ctypes.c_int64(-1)
        assert L.hm_stream_export_select(s.ptr, ids, 3, *MID, None, None, None, None, 0,
                                         ctypes.byref(got)) == _lib.HM_E_CAPACITY
        assert got.value == n
        out = [torch.full((n + 64,), -7, dtype=torch.int64 if j < 2 else torch.int32, device="cuda") for j in range(4)]
        got = ctypes.c_int64(-1)
        assert L.hm_stream_export_select(s.ptr, ids, 3, *MID, *(device._ptr(t) for t in out), n - 1,
                                         ctypes.byref(got)) == _lib.HM_E_CAPACITY
        assert got.value == n
        assert all(bool((t[n - 1:] == -7).all()) for t in out)               # nothing at or behind the capacity
        out = [torch.full((n + 64,), -7, dtype=torch.int64, device="cuda") for j in range(2)]
        assert L.hm_stream_export_select(s.ptr, ids, 3, *MID, device._ptr(out[0]), device._ptr(out[1]), None, None, n,
                                         ctypes.byref(got)) == _lib.HM_OK
        assert got.value == n and all(bool((t[n:] == -7).all()) for t in out)
        k = out[0][:n].cpu().numpy().view(np.uint64)
        assert np.array_equal(_rec(k >> np.uint64(32), k & np.uint64(0xFFFFFFFF), out[1][:n].cpu().numpy()),
                              _rec(*(want[:, j] for j in (2, 3, 4))))
        out = [torch.full((n + 64,), -7, dtype=torch.int64 if j < 2 else torch.int32, device="cuda") for j in range(4)]
        assert L.hm_stream_export_select(s.ptr, ids, 3, *MID, *(device._ptr(t) for t in out), n + 64,
                                         ctypes.byref(got)) == _lib.HM_OK
        assert got.value == n and all(bool((t[n:] == -7).all()) for t in out)
        k = out[0][:n].cpu().numpy().view(np.uint64)
        assert np.array_equal(_rec(out[2][:n].cpu().numpy().view(np.uint32), out[3][:n].cpu().numpy().view(np.uint32),
                                   k >> np.uint64(32), k & np.uint64(0xFFFFFFFF), out[1][:n].cpu().numpy()), want)
        # every group, all time: the undated marker, and the whole export
        assert L.hm_stream_export_select(s.ptr, None, 0, -1, -1, None, None, None, None, 0,
                                         ctypes.byref(got)) == _lib.HM_E_CAPACITY
        assert got.value == n0 and (full[1] == _lib.HM_STREAM_UNDATED).any()
        # an empty selection is HM_OK with 0
        none = (ctypes.c_uint32 * 1)(31337)
        assert L.hm_stream_export_select(s.ptr, none, 1, -1, -1, None, None, None, None, 0,
                                         ctypes.byref(got)) == _lib.HM_OK
        assert got.value == 0
        assert s.cells()[0] == n0                                            # the log is as it was
    finally:
        s.close()


def _by_label(s):
    g, h, z, r, c, cnt = s.export()
    names = {lab: j for j, lab in enumerate(sorted(set(USERS) | {"all", "route"}))}
    lab = np.array([len(names) if v == NOGROUP else names[s.labels[v]] for v in g.tolist()], dtype=np.int64)
    return lab, h, z, r, c, cnt


def test_move_users(gpu, data):
    """(13) b.merge_from(a, users=U); a.forget(users=U): together the two streams hold what they held before"""
    a = data.full()
    b = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE - 24)
    try:
        lat, lon, _, hour, _ = data.batches[4]
        b.add(lat[:10], lon[:10], None, hour[:10], user_id=["u3"] * 10)      # u3 first: other label ids than a's
        data.feed(b, [3, 0])                                                 # hours that overlap a's
        assert a.labels != b.labels and set(a.labels) == set(b.labels)
        before = _summed(*(np.concatenate([x, y]) for x, y in zip(_by_label(a), _by_label(b))))
        moved = ["u1", "u3"]
        b.merge_from(a, users=moved)
        a.forget(users=moved)
        ga = a.export()[0]
        assert not np.isin(ga, [a._index[u] for u in moved]).any() and (ga == a._index["u2"]).any()
        after = _summed(*(np.concatenate([x, y]) for x, y in zip(_by_label(a), _by_label(b))))
        assert np.array_equal(after, before)
        # a selective snapshot keeps the full label list and restores as any other
        snap = a.snapshot(users=["u2"], hours=MID)
        assert snap["labels"].tolist() == a.labels and len(snap["keys"])
        c = StreamingHeatmap.from_snapshot(snap)
        want = a.export(users=["u2"], hours=MID)
        assert len(want[0]) and np.array_equal(_rec(*c.export()), _rec(*want))
        c.close()
    finally:
        a.close()
        b.close()


def test_errors(gpu, data):
    """(14) every HM_E_ARG of the selection leaves the stream and the outputs alone; the wrapper's ValueErrors"""
    s = data.feed(StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE), [0])
    try:
        L = s.ctx.L
        before, state = s.export(), (s.cells(), s.buckets())
        one, bad = (ctypes.c_uint32 * 2)(1, 2), (ctypes.c_uint32 * 3)(1, 0xFFFFFFFF, 2)
        a, b, n = ctypes.c_int64(77), ctypes.c_int64(78), ctypes.c_int64(79)
        for groups, ng, lo, hi in ((bad, 3, -1, -1), (None, 3, -1, -1), (None, -1, BASE, BASE + 5), (one, 0, -1, -1),
                                   (one, -2, -1, -1), (one, _lib.HM_SELECT_MAX_GROUPS + 1, -1, -1),
                                   (one, 2, BASE + 5, BASE + 5), (one, 2, BASE + 9, BASE + 5), (None, 0, -1, -2)):
            assert L.hm_stream_forget(s.ptr, groups, ng, lo, hi, ctypes.byref(a), ctypes.byref(b)) == _lib.HM_E_ARG
            assert L.hm_stream_export_select(s.ptr, groups, ng, lo, hi, None, None, None, None, 0,
                                             ctypes.byref(n)) == _lib.HM_E_ARG
        assert L.hm_stream_export_select(s.ptr, one, 2, -1, -1, None, None, None, None, -1, ctypes.byref(n)) == _lib.HM_E_ARG
        assert L.hm_stream_export_select(s.ptr, one, 2, -1, -1, None, None, None, None, 5, ctypes.byref(n)) == _lib.HM_E_ARG
        assert L.hm_stream_export_select(s.ptr, one, 2, -1, -1, None, None, None, None, 0, None) == _lib.HM_E_ARG
        assert (a.value, b.value, n.value) == (77, 78, 79)
        for kw in ({}, {"users": ["xhidden"]}, {"users": ["u1", "rt-5"]}, {"hours": (BASE + 5, BASE + 5)},
                   {"hours": (BASE + 5, BASE)}, {"groups": [0xFFFFFFFF]}, {"groups": [-3]}, {"hours": 5}):
            with pytest.raises(ValueError):
                s.forget(**kw)
        for kw in ({"users": ["xhidden"]}, {"hours": (BASE + 5, BASE + 5)}, {"groups": [1 << 32]}):
            with pytest.raises(ValueError):
                s.export(**kw)
            with pytest.raises(ValueError):
                s.snapshot(**kw)
        assert (s.cells(), s.buckets()) == state
        assert np.array_equal(_rec(*s.export()), _rec(*before))
        # a NULL answer pointer is fine
        assert L.hm_stream_forget(s.ptr, one, 2, BASE, BASE + 1, None, None) == _lib.HM_OK
    finally:
        s.close()
