"""GPU: the error contract of include/heatmap_amd.h -- "per-point errors set
the status of the first failing point (input order) and hm_last_error()
reports its index", and every point is projected and can fail whether kept or
not -- for every entry point that takes points: hm_project, hm_count (pipeline
and general fallback), hm_count_grouped (dense and compacted key lists),
hm_count_grouped_packed and hm_stream_add (its three fold paths, after a
one-bucket and after a several-bucket batch).

The reference is oracle.count's (status, err_index) on the same arrays (for
hm_project the first non-zero status of oracle.project); the exception must be
the reference's as well.  After every failing call an error-free call on the
same context must give the oracle's counts and clear hm_last_error; a failed
stream batch must leave the resident counts as they were.

The second half approaches this path's own limit, HM_E_RANGE for a cell whose
zoom-0 tile lies outside rows [-16, 16) or columns [-2^47, 2^47)
(csrc/hm_genkey.h), from both sides, against oracle.count_tiles / oracle.count.
"""
import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, device, synth
from heatmap_amd.stream import StreamingHeatmap

pytestmark = pytest.mark.gpu

N = 20_000
T1 = 8192                   # points per level-1 tile (HM_T1), as tests/test_gpu_l1_whole_tiles.py
POSITIONS = [0, 63, 64, 2047, 2048, 4095, 4096, N - 1]
NAN, DOMAIN, INF, RANGE = _lib.HM_E_NAN, _lib.HM_E_DOMAIN, _lib.HM_E_INF, _lib.HM_E_RANGE
# (lat or None, lon or None) written into a copy of the cloud; what the oracle was seen to answer
KINDS = {"lat_nan": (np.nan, None), "lat_95": (95.0, None), "lat_-90": (-90.0, None), "lat_inf": (np.inf, None),
         "lon_nan": (None, np.nan), "lon_inf": (None, np.inf), "lon_1e300": (None, 1e300),
         "lat_95_lon_inf": (95.0, np.inf)}
SEEN = {"lat_nan": NAN, "lat_95": DOMAIN, "lat_-90": DOMAIN, "lat_inf": DOMAIN, "lon_nan": NAN, "lon_inf": INF,
        "lon_1e300": RANGE, "lat_95_lon_inf": DOMAIN}
SBASE = 480_000             # base hour of the streams


def _ctx():
    return device.context(0)


def _catch(fn):
    """((kind, index), exception, result) of one wrapper call."""
    try:
        res = fn()
    except (ValueError, OverflowError, NotImplementedError) as e:
        idx, kind = _ctx().last_error()
        return (kind, idx), e, None
    return (0, -1), None, res


def _expect(lat, lon, keep, zmin, zmax):
    ref = oracle.count(lat, lon, keep, zmin, zmax)
    return ((ref["status"], ref["err_index"]) if ref["status"] else (0, -1)), ref


def _check_exception(e, kind, idx):
    if kind == NAN:
        assert type(e) is ValueError and "NaN" in str(e), repr(e)
    elif kind == DOMAIN:
        assert type(e) is ValueError and "domain" in str(e), repr(e)
    elif kind == INF:
        assert type(e) is OverflowError, repr(e)
    else:
        assert kind == RANGE and type(e) is _lib.DevicePathUnsupported and "(point %d)" % idx in str(e), repr(e)


def _same_counts(got, ref):
    got = got.sorted()
    assert ref["status"] == 0
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k]), k


def _mask(n):
    return (np.arange(n) % 9 != 4).astype(np.uint8)


def _groups(n):
    return ((np.arange(n) % 5) * 7919).astype(np.uint32)


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _decode_packed(res):
    keys, gc = res
    k = keys.cpu().numpy().view(np.uint64)
    gcn = gc.cpu().numpy().view(np.uint64)
    z, r, c = device.decode_keys(k)
    return device.GroupedCounts((gcn >> np.uint64(32)).astype(np.uint32), z, r, c,
                                (gcn & np.uint64(0xFFFFFFFF)).astype(np.int64))


def _same_grouped(got, lat, lon, g, keep, zmin, zmax, key=None):
    """got (GroupedCounts) == the oracle per group id."""
    got = got.sorted()
    kb = np.ones(lat.size, bool) if keep is None else keep.astype(bool)

    def refs():
        out = {k: [] for k in ("group", "zoom", "row", "col", "count")}
        for gid in np.unique(g[kb]):
            ref = oracle.count(lat, lon, (kb & (g == gid)).astype(np.uint8), zmin, zmax)
            assert ref["status"] == 0
            out["group"].append(np.full(ref["zoom"].size, gid, np.uint32))
            for k in ("zoom", "row", "col", "count"):
                out[k].append(ref[k])
        return {k: np.concatenate(v) for k, v in out.items()}

    exp = _cached(key, refs) if key else refs()
    for k in exp:
        assert np.array_equal(getattr(got, k), exp[k]), k


class Entry:
    """One entry point: run() the wrapper, verify() an error-free result against
    the oracle, recover() = an error-free call on the same context after a
    failure (the twin: the clean cloud under the same kind of keep mask)."""
    n = N
    zooms = (0, 14)
    seed = 5
    keeps = ("none", "mask")     # keep arguments the entry takes
    positions = POSITIONS

    def __init__(self, name):
        self.name = name

    def cloud(self):
        lat, lon = _cached(("cloud", self.n, self.seed), lambda: synth.uniform(self.n, seed=self.seed))
        return lat.copy(), lon.copy()

    def keep(self, kind):
        return None if kind == "none" else _mask(self.n)

    def prepare(self):
        return None

    def finish(self, st):
        pass

    def verify(self, st, res, lat, lon, keep, key=None):
        ref = _cached(key, lambda: oracle.count(lat, lon, keep, *self.zooms)) if key else \
            oracle.count(lat, lon, keep, *self.zooms)
        _same_counts(res, ref)

    def recover(self, st, keepkind):
        lat, lon = self.cloud()
        keep = self.keep(keepkind)
        got, e, res = _catch(lambda: self.run(st, lat, lon, keep))
        assert got == (0, -1) and _ctx().last_error() == (-1, 0)
        self.verify(st, res, lat, lon, keep, key=("twin", self.name, keepkind))
        return res


class Project(Entry):
    zooms = (14, 14)
    keeps = ("none",)            # hm_project has no keep mask

    def run(self, st, lat, lon, keep):
        p = device.project(lat, lon, 14)
        assert _ctx().last_error() == (p.first_error_index, p.first_error_kind)
        if p.first_error_kind:
            # the failing point's own status, and the first one in the array
            bad = np.flatnonzero((p.status != 0) & (p.status != _lib.HM_BIGCOL))
            assert bad[0] == p.first_error_index and p.status[bad[0]] == p.first_error_kind
            device.project(lat, lon, 14, raise_errors=True)
            raise AssertionError("raise_errors=True did not raise")
        assert p.first_error_index == -1
        return p

    def verify(self, st, res, lat, lon, keep, key=None):
        r, c, s, _ = oracle.project(lat, lon, 14)
        big = s == RANGE     # beyond int64: the oracle's E_RANGE is hm_project's HM_BIGCOL, not an error
        assert np.array_equal(res.status[~big], s[~big]) and np.all(res.status[big] == _lib.HM_BIGCOL)
        ok = s == 0
        assert np.array_equal(res.row[ok], r[ok]) and np.array_equal(res.col[ok], c[ok])


class CountPipeline(Entry):
    positions = POSITIONS + [T1, 2 * T1 - 1]     # first and last index of the second level-1 tile

    def run(self, st, lat, lon, keep):
        return device.count(lat, lon, keep, *self.zooms)

    def recover(self, st, keepkind):
        res = Entry.recover(self, st, keepkind)
        assert int(res.stage_us[7]) > 0, "the call left the pipeline"
        return res


class CountFallback(Entry):
    """The (1_000_000, 0, 21) uniform recipe of test_sparse_fallback_vs_oracle.
    Its 11M cells stay in device memory and are compared there, sorted, with
    the oracle's (cached per twin), so every recovery is a full comparison."""
    n = 1_000_000
    zooms = (0, 21)
    seed = 11
    positions = POSITIONS[:-1] + [n - 1]

    def cloud(self):
        lat, lon = Entry.cloud(self)
        lat[::1000] = 88.5
        lon[1::1000] = 200.0
        return lat, lon

    def run(self, st, lat, lon, keep):
        m, buf = device.count_device(lat, lon, keep, *self.zooms)
        return m, buf, _ctx().last_stats()[1]

    def verify(self, st, res, lat, lon, keep, key=None):
        import torch

        m, buf, stage_us = res
        assert int(stage_us[7]) == 0, "the call took the pipeline, not the general path"

        def ref():
            r = oracle.count(lat, lon, keep, *self.zooms)
            assert r["status"] == 0
            z, row, col = r["zoom"].astype(np.int64), r["row"], r["col"]
            lim = np.int64(1) << z
            inside = (row >= 0) & (row < lim) & (col >= 0) & (col < lim)
            keys = (z[inside] << 58) | (row[inside] << 29) | col[inside]      # HM_KEY; the oracle's order
            assert np.all(np.diff(keys) > 0)
            outside = np.stack([z, row, col, r["count"]], axis=1)[~inside]
            return torch.from_numpy(keys).cuda(), torch.from_numpy(r["count"][inside]).cuda(), outside

        rkeys, rcounts, routside = _cached(key, ref) if key else ref()
        keys, order = torch.sort(buf.keys[:m])
        assert torch.equal(keys, rkeys) and torch.equal(buf.counts[:m][order], rcounts)
        x = buf.xcells[:4 * buf.nx].cpu().numpy().reshape(-1, 4)
        assert np.array_equal(x[np.lexsort((x[:, 2], x[:, 1], x[:, 0]))], routside)


class Grouped(Entry):
    zooms = (0, 10)

    def __init__(self, name, dense):
        Entry.__init__(self, name)
        self.keeps = ("none",) if dense else ("mask",)

    def run(self, st, lat, lon, keep):
        return device.count_grouped(lat, lon, _groups(lat.size), keep, *self.zooms)

    def verify(self, st, res, lat, lon, keep, key=None):
        _same_grouped(res, lat, lon, _groups(lat.size), keep, *self.zooms, key=key)


class Packed(Entry):
    zooms = (0, 10)

    def run(self, st, lat, lon, keep):
        return device.count_grouped_packed_device(lat, lon, _groups(lat.size), keep, *self.zooms)

    def verify(self, st, res, lat, lon, keep, key=None):
        if res is None:      # HM_E_EXOTIC: some kept point lies outside the square
            r, c, s, _ = oracle.project(lat, lon, self.zooms[1])
            kb = np.ones(lat.size, bool) if keep is None else keep.astype(bool)
            lim = 1 << self.zooms[1]
            assert np.any(kb & ((r < 0) | (r >= lim) | (c < 0) | (c >= lim)))
            return
        _same_grouped(_decode_packed(res), lat, lon, _groups(lat.size), keep, *self.zooms, key=key)


class Stream(Entry):
    """hm_stream_add: form '1h' (one bucket: the speculative hm_count), '3h'
    (a few buckets: gathered runs) or 'many' (161 (group, hour) buckets, more
    than HMS_MAX_PARTS = 64: the grouped general path), as the stream's first
    batch ('fresh'), after a one-bucket batch ('after1') or after a
    three-bucket batch ('after3': the next batch is not counted speculatively)."""
    zooms = (0, 12)

    def __init__(self, name, form, state):
        Entry.__init__(self, name)
        self.form, self.state = form, state

    def columns(self, n):
        i = np.arange(n)
        if self.form == "1h":
            return np.full(n, SBASE + 3, np.uint32), None
        if self.form == "3h":
            return (SBASE + i % 3).astype(np.uint32), None
        return (SBASE + i % 7).astype(np.uint32), (i % 23).astype(np.uint32)

    def prepare(self):
        st = {"s": StreamingHeatmap(*self.zooms, base_hour=SBASE), "lat": [], "lon": [], "keep": []}
        if self.state != "fresh":
            lat, lon = synth.generate("hotspots", 3000, seed=8)
            hour = np.full(3000, SBASE + 40, np.uint32)
            if self.state == "after3":
                hour += (np.arange(3000) % 3).astype(np.uint32)
            st["s"].add(lat, lon, None, hour)
            self._took(st, lat, lon, None)
        st["before"] = st["s"].counts().sorted()
        return st

    @staticmethod
    def _took(st, lat, lon, keep):
        st["lat"].append(lat)
        st["lon"].append(lon)
        st["keep"].append(np.ones(lat.size, np.uint8) if keep is None else keep)

    def finish(self, st):
        st["s"].close()

    def run(self, st, lat, lon, keep):
        hour, group = self.columns(lat.size)
        st["s"].add(lat, lon, keep, hour, group=group)
        self._took(st, lat, lon, keep)
        return st["s"]

    def recover(self, st, keepkind):
        after = st["s"].counts().sorted()         # the failed batch changed no counts
        for k in ("zoom", "row", "col", "count"):
            assert np.array_equal(getattr(st["before"], k), getattr(after, k)), k
        return Entry.recover(self, st, keepkind)

    def verify(self, st, res, lat, lon, keep, key=None):
        args = (np.concatenate(st["lat"]), np.concatenate(st["lon"]), np.concatenate(st["keep"]))
        key = key + (self.state,) if key else None
        ref = _cached(key, lambda: oracle.count(*args, *self.zooms)) if key else oracle.count(*args, *self.zooms)
        _same_counts(res.counts(), ref)


ENTRIES = [Project("project"), CountPipeline("count"), CountFallback("count_fallback"),
           Grouped("grouped_dense", True), Grouped("grouped_keep", False), Packed("packed")] + \
          [Stream("stream_%s_%s" % (f, s), f, s) for f in ("1h", "3h", "many") for s in ("fresh", "after1", "after3")]
entries = pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])


def _case(entry, lat, lon, keep, keepkind, must_fail=None):
    """One call of the entry point against the oracle's (status, err_index),
    then the recovery call (or, for a call that must not fail, its counts)."""
    if isinstance(entry, Project):
        s = oracle.project(lat, lon, 14)[2]
        bad = np.flatnonzero((s != 0) & (s != RANGE))
        want = (int(s[bad[0]]), int(bad[0])) if bad.size else (0, -1)
    else:
        want, _ = _expect(lat, lon, keep, *entry.zooms)
    if must_fail is not None:
        assert (want[0] != 0) == must_fail, want
    st = entry.prepare()
    try:
        got, e, res = _catch(lambda: entry.run(st, lat, lon, keep))
        assert got == want, "%s: (kind, index) %r, the oracle has %r" % (entry.name, got, want)
        if want[0]:
            _check_exception(e, *want)
            entry.recover(st, keepkind)
        else:
            entry.verify(st, res, lat, lon, keep)
    finally:
        entry.finish(st)
    return want


def _poke(lat, lon, i, kind):
    a, b = KINDS[kind]
    if a is not None:
        lat[i] = a
    if b is not None:
        lon[i] = b


@entries
def test_error_kinds(gpu, entry):
    """Each kind of failing value at one index: the oracle's kind and index,
    the reference's exception; lat = 90.0 is valid and must not fail."""
    for kind in KINDS:
        for keepkind in entry.keeps[:1]:
            lat, lon = entry.cloud()
            _poke(lat, lon, 5000, kind)
            want = _case(entry, lat, lon, entry.keep(keepkind), keepkind)
            if isinstance(entry, Project) and kind == "lon_1e300":
                assert want == (0, -1)       # HM_BIGCOL: hm_project returns such columns
            else:
                assert want == (SEEN[kind], 5000), (kind, want)
    lat, lon = entry.cloud()
    lat[5000] = 90.0
    _case(entry, lat, lon, entry.keep(entry.keeps[0]), entry.keeps[0], must_fail=False)


@entries
def test_error_positions(gpu, entry):
    """One failing point at the wave edge, at the block steps of the key and
    list kernels (256 x 8, 256 x 16), at the ends of the input and (pipeline)
    of a level-1 tile; a latitude NaN and a longitude infinity take different
    branches of the projection."""
    for j, pos in enumerate(entry.positions):
        for kind in ("lat_nan", "lon_inf"):
            keepkind = entry.keeps[j % len(entry.keeps)]
            lat, lon = entry.cloud()
            _poke(lat, lon, pos, kind)
            assert _case(entry, lat, lon, entry.keep(keepkind), keepkind) == (SEEN[kind], pos)


@entries
def test_error_first_of_several(gpu, entry):
    for keepkind in entry.keeps:
        lat, lon = entry.cloud()
        lat[entry.n - 1] = np.nan
        lon[5000] = np.inf
        lat[12_345] = 95.0
        assert _case(entry, lat, lon, entry.keep(keepkind), keepkind) == (INF, 5000)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if "mask" in e.keeps],
                         ids=[e.name for e in ENTRIES if "mask" in e.keeps])
def test_error_unkept_point_still_fails(gpu, entry):
    for pos, kind in ((5000, "lat_nan"), (300, "lon_inf"), (entry.n - 1, "lat_95")):
        lat, lon = entry.cloud()
        _poke(lat, lon, pos, kind)
        keep = entry.keep("mask")
        keep[pos] = 0
        assert _case(entry, lat, lon, keep, "mask") == (SEEN[kind], pos)
    # and with nothing kept at all
    lat, lon = entry.cloud()
    lat[777] = np.nan
    assert _case(entry, lat, lon, np.zeros(entry.n, np.uint8), "mask") == (NAN, 777)


@pytest.mark.parametrize("dense", [True, False])
def test_grouped_unsettled_list_overflow(gpu, dense):
    """100_000 points, every latitude in +-[85.06, 89.9]: more than 2^16 points
    are left to the exact chain, so k_project_keys_slow sweeps the whole input
    instead of walking its list; the first failing point is still the one
    reported, and the error-free twin equals the oracle per group."""
    n = 100_000
    rng = np.random.default_rng(6)
    _, lon = synth.uniform(n, seed=6)
    lat = rng.choice([-1.0, 1.0], n) * rng.uniform(85.06, 89.9, n)
    g = ((np.arange(n) % 3) * 11).astype(np.uint32)
    keep = None if dense else _mask(n)
    got = device.count_grouped(lat, lon, g, keep, 4, 12)
    _same_grouped(got, lat, lon, g, keep, 4, 12)
    bad_lat, bad_lon = lat.copy(), lon.copy()
    bad_lat[99_000] = np.nan
    bad_lon[70_000] = np.inf
    want, _ = _expect(bad_lat, bad_lon, keep, 4, 12)
    assert want == (INF, 70_000)
    got, e, _ = _catch(lambda: device.count_grouped(bad_lat, bad_lon, g, keep, 4, 12))
    assert got == want
    _check_exception(e, *want)
    again = device.count_grouped(lat, lon, g, keep, 4, 12)
    assert _ctx().last_error() == (-1, 0)
    _same_grouped(again, lat, lon, g, keep, 4, 12)


def test_count_redo_list_overflow(gpu):
    """The recipe of test_count_redo_overflow_fallback (3M points, 40% polar:
    more deferred points than the redo list's 2^20) with one NaN late in the
    input: the fused exact fallback reports it at its index."""
    n = 3_000_000
    lat, lon = synth.uniform(n, seed=9)
    polar = (np.arange(n) % 5) < 2
    lat = np.where(polar, 86.0 + (lat % 3.0), lat)
    keep = (~polar).astype(np.uint8)
    lat[n - 12_345] = np.nan
    want, _ = _expect(lat, lon, keep, 0, 16)
    assert want == (NAN, n - 12_345)
    got, e, _ = _catch(lambda: device.count(lat, lon, keep, 0, 16))
    assert got == want
    _check_exception(e, *want)
    CountPipeline("count").recover(None, "mask")


@pytest.mark.parametrize("tiles", [False, True])
def test_chunked_count_reports_the_input_index(gpu, tiles):
    """device.count over forced chunks (one hm_count call each): the failing
    point keeps its index in the whole input for every kind of error, in
    hm_last_error as in the message, and a later call has its own index."""
    chunk = 7000
    if tiles:
        rows, cols = _tile_cloud(4, N)
        rows[2 * chunk + 11] = 16 << 4                   # beyond the key's rows, third chunk
        rows[2 * chunk + 500] = -(16 << 4) - 1
        got, e, _ = _catch(lambda: device.count(rows, cols, None, 0, 4, tiles=True, chunk=chunk))
        assert got == (RANGE, 2 * chunk + 11)
        _check_exception(e, RANGE, 2 * chunk + 11)
        return
    for kind, pos in (("lat_nan", 2 * chunk), ("lon_inf", 2 * chunk - 1), ("lat_95", chunk + 17),
                      ("lon_1e300", 2 * chunk + 1), ("lat_nan", 5)):
        lat, lon = synth.uniform(N, seed=5)
        lat, lon = lat.copy(), lon.copy()
        _poke(lat, lon, pos, kind)
        lat[N - 2] = np.nan                              # a later failure in the last chunk
        for keep in (None, _mask(N)):
            want, _ = _expect(lat, lon, keep, 0, 14)
            assert want == (SEEN[kind], pos)
            got, e, _ = _catch(lambda: device.count(lat, lon, keep, 0, 14, chunk=chunk))
            assert got == want, (kind, pos, got)
            _check_exception(e, *want)
    # a failing call afterwards reports its own index, not a rebased one: first a direct library
    # call that fails at the failed chunk's own (index, kind), then the wrappers
    import ctypes

    import torch

    lat, lon = synth.uniform(N, seed=5)
    lat = lat.copy()
    lat[2 * chunk + 5] = np.nan
    assert _catch(lambda: device.count(lat, lon, None, 0, 14, chunk=chunk))[0] == (NAN, 2 * chunk + 5)
    ctx = _ctx()
    la = torch.zeros(64, dtype=torch.float64, device="cuda")
    la[5] = float("nan")
    lo = torch.zeros(64, dtype=torch.float64, device="cuda")
    row = torch.empty(64, dtype=torch.int64, device="cuda")
    col = torch.empty(64, dtype=torch.int64, device="cuda")
    status = torch.empty(64, dtype=torch.uint8, device="cuda")
    rc = ctx.L.hm_project(ctx.ptr, *(ctypes.c_void_p(t.data_ptr()) for t in (la, lo)), 64, 14,
                          *(ctypes.c_void_p(t.data_ptr()) for t in (row, col, status)))
    assert rc == NAN and ctx.last_error() == (5, NAN)
    lat, lon = synth.uniform(chunk, seed=5)
    lat = lat.copy()
    lat[5] = np.nan
    assert _catch(lambda: device.count(lat, lon, None, 0, 14))[0] == (NAN, 5)
    assert _catch(lambda: device.count_grouped(lat, lon, _groups(chunk), None, 0, 10))[0] == (NAN, 5)
    lat, lon = synth.uniform(N, seed=5)
    _same_counts(device.count(lat, lon, None, 0, 14, chunk=chunk), oracle.count(lat, lon, None, 0, 14))
    assert _ctx().last_error() == (-1, 0)


# ------------------------------------------------------------- hm_stream_add's hours

def _stream_add_error(s, *args, **kw):
    return _catch(lambda: s.add(*args, **kw))[:2]


@pytest.mark.parametrize("nhours", [1, 3])
def test_stream_bad_hours(gpu, nhours):
    """A kept point dated before the base hour, or 2^28 hours or more after
    it, is HM_E_RANGE at its index; unkept it is not, and base + 2^28 - 1 is
    the last hour accepted."""
    n = 2000
    lat, lon = synth.generate("hotspots", n, seed=3)
    hour = (SBASE + np.arange(n) % nhours).astype(np.uint32)
    for bad in (SBASE - 1, SBASE + (1 << 28)):
        s = StreamingHeatmap(0, 12, base_hour=SBASE)
        try:
            h = hour.copy()
            h[900] = bad
            got, e = _stream_add_error(s, lat, lon, None, h)
            assert got == (RANGE, 900), (bad, got)
            _check_exception(e, RANGE, 900)
            assert s.counts().count.size == 0
            keep = np.ones(n, np.uint8)
            keep[900] = 0
            s.add(lat, lon, keep, h)         # the same point unkept does not fail
            assert _ctx().last_error() == (-1, 0)
            _same_counts(s.counts(), oracle.count(lat, lon, keep, 0, 12))
        finally:
            s.close()
    s = StreamingHeatmap(0, 12, base_hour=SBASE)
    try:
        h = hour.copy()
        h[900] = SBASE + (1 << 28) - 1
        s.add(lat, lon, None, h)
        _same_counts(s.counts(), oracle.count(lat, lon, None, 0, 12))
        _same_counts(s.counts(SBASE + (1 << 28) - 1), oracle.count(lat[900:901], lon[900:901], None, 0, 12))
    finally:
        s.close()


@pytest.mark.parametrize("state", ["fresh", "after3"])
@pytest.mark.parametrize("nhours", [1, 3])
def test_stream_bad_hour_and_projection_error(gpu, nhours, state):
    """The first failing point in input order wins whichever check finds it: a
    NaN at index 100 before a bad hour at index 900 is the NaN; the other way
    round it is the hour."""
    n = 2000
    lat, lon = synth.generate("hotspots", n, seed=3)
    hour = (SBASE + np.arange(n) % nhours).astype(np.uint32)
    for nan_at, hour_at, want in ((100, 900, (NAN, 100)), (900, 100, (RANGE, 100))):
        s = StreamingHeatmap(0, 12, base_hour=SBASE)
        try:
            if state == "after3":
                s.add(lat, lon, None, (SBASE + 50 + np.arange(n) % 3).astype(np.uint32))
            before = s.counts().sorted()
            la, h = lat.copy(), hour.copy()
            la[nan_at] = np.nan
            h[hour_at] = SBASE - 1
            got, e = _stream_add_error(s, la, lon, None, h)
            assert got == want, (nan_at, hour_at, got)
            _check_exception(e, *want)
            after = s.counts().sorted()
            assert np.array_equal(before.count, after.count) and np.array_equal(before.col, after.col)
        finally:
            s.close()


# ------------------------------------------------------------------ key-range limits

I64 = np.iinfo(np.int64)


def _same_tiles(got, ref):
    got = got.sorted()
    o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k][o]), k


def _same_grouped_tiles(got, rows, cols, g, keep, zmin, zmax):
    got = got.sorted()
    kb = np.ones(rows.size, bool) if keep is None else keep.astype(bool)
    exp = {k: [] for k in ("group", "zoom", "row", "col", "count")}
    for gid in np.unique(g[kb]):
        ref = oracle.count_tiles(rows, cols, zmin, zmax, (kb & (g == gid)).astype(np.uint8))
        o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
        exp["group"].append(np.full(o.size, gid, np.uint32))
        for k in ("zoom", "row", "col", "count"):
            exp[k].append(ref[k][o])
    for k in exp:
        assert np.array_equal(getattr(got, k), np.concatenate(exp[k])), k


def _tile_cloud(Z, n=300):
    rng = np.random.default_rng(Z)
    return rng.integers(0, 1 << Z, n), rng.integers(0, 1 << Z, n)


TILE_CALLS = {
    "count_tiles": lambda rows, cols, g, keep, Z: device.count(rows, cols, keep, 0, Z, tiles=True),
    "grouped_tiles": lambda rows, cols, g, keep, Z: device.count_grouped(rows, cols, g, keep, 0, Z, tiles=True),
}


def _verify_tiles(call, res, rows, cols, g, keep, Z):
    if call == "count_tiles":
        _same_tiles(res, oracle.count_tiles(rows, cols, 0, Z, keep))
    else:
        _same_grouped_tiles(res, rows, cols, g, keep, 0, Z)


@pytest.mark.parametrize("call", list(TILE_CALLS))
@pytest.mark.parametrize("Z", [0, 4, 15])
def test_tile_key_range(gpu, call, Z):
    """Tile input at the edge of the key's super-tile fields: the last rows
    and columns inside count like the oracle's at every zoom (negative ones
    through the arithmetic shift); one step further in any of the four
    directions is HM_E_RANGE at that point when kept, nothing when unkept."""
    rmax, rmin = (16 << Z) - 1, -(16 << Z)
    cmax, cmin = ((1 << 47) << Z) - 1, -((1 << 47) << Z)
    rows, cols = _tile_cloud(Z)
    g = _groups(rows.size)
    fn = TILE_CALLS[call]
    inside = {10: (rmax, 0), 100: (rmin, (1 << Z) - 1), 200: (0, cmax), 299: ((1 << Z) - 1, cmin), 150: (rmin, cmin),
              151: (rmax, cmax)}
    for i, (r, c) in inside.items():
        rows[i], cols[i] = r, c
    for keep in (None, _mask(rows.size)):
        _verify_tiles(call, fn(rows, cols, g, keep, Z), rows, cols, g, keep, Z)
    for i, (r, c) in {63: (rmax + 1, 0), 64: (rmin - 1, 5), 255: (0, cmax + 1), 256: (3, cmin - 1)}.items():
        r2, c2 = rows.copy(), cols.copy()
        r2[i], c2[i] = r, c
        got, e, _ = _catch(lambda: fn(r2, c2, g, None, Z))
        assert got == (RANGE, i), (i, r, c, got)
        _check_exception(e, RANGE, i)
        keep = np.ones(rows.size, np.uint8)
        keep[i] = 0
        res = fn(r2, c2, g, keep, Z)             # unkept: not an error
        assert _ctx().last_error() == (-1, 0)
        _verify_tiles(call, res, r2, c2, g, keep, Z)


@pytest.mark.parametrize("call", list(TILE_CALLS))
def test_tile_key_range_zoom21(gpu, call):
    """At zoom 21 col >> 21 always fits the 48-bit column field: the int64
    extremes count, with the last rows inside."""
    Z = 21
    rows, cols = _tile_cloud(Z)
    g = _groups(rows.size)
    for i, (r, c) in {0: ((16 << Z) - 1, I64.max), 64: (-(16 << Z), I64.min), 299: (5, I64.max),
                      128: (-(16 << Z), 7)}.items():
        rows[i], cols[i] = r, c
    for zmin in (0, 21):
        for keep in (None, _mask(rows.size)):
            if call == "count_tiles":
                _same_tiles(device.count(rows, cols, keep, zmin, Z, tiles=True),
                            oracle.count_tiles(rows, cols, zmin, Z, keep))
            else:
                _same_grouped_tiles(device.count_grouped(rows, cols, g, keep, zmin, Z, tiles=True), rows, cols, g,
                                    keep, zmin, Z)
    r2 = rows.copy()
    r2[200] = 16 << Z
    got, e, _ = _catch(lambda: TILE_CALLS[call](r2, cols, g, None, Z))
    assert got == (RANGE, 200)
    _check_exception(e, RANGE, 200)


def _edge_longitudes(zmax, sign):
    """(last longitude inside, first outside) the column field on one side:
    zoom-0 column 2^47 - 1 | 2^47, or -2^47 | -2^47 - 1, found by projecting the
    doubles around the edge with the oracle at zoom zmax."""
    edge = (360.0 * 2.0 ** 47 - 180.0) if sign > 0 else (-360.0 * 2.0 ** 47 - 180.0)
    xs = [edge]
    for _ in range(64):
        xs.insert(0, np.nextafter(xs[0], -np.inf))
        xs.append(np.nextafter(xs[-1], np.inf))
    xs = np.asarray(xs)
    r, c, s, _ = oracle.project(np.zeros(xs.size), xs, zmax)
    assert not s.any()
    sc = c >> zmax
    if sign > 0:
        inside, outside = xs[sc == (1 << 47) - 1][-1], xs[sc == (1 << 47)][0]
    else:
        inside, outside = xs[sc == -(1 << 47)][0], xs[sc == -(1 << 47) - 1][-1]
    return float(inside), float(outside)


LATLON_CALLS = {
    "count": lambda lat, lon, keep, zmax: device.count(lat, lon, keep, 0, zmax),
    "grouped": lambda lat, lon, keep, zmax: device.count_grouped(lat, lon, _groups(lat.size), keep, 0, zmax),
}


def _verify_latlon(call, res, lat, lon, keep, zmax):
    if call == "count":
        _same_counts(res, oracle.count(lat, lon, keep, 0, zmax))
    else:
        _same_grouped(res, lat, lon, _groups(lat.size), keep, 0, zmax)


@pytest.mark.parametrize("call", list(LATLON_CALLS))
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("zmax", [0, 10])
def test_latlon_key_range(gpu, call, zmax, sign):
    """A longitude in the last zoom-0 column of the key's column field counts
    like the oracle's; the next column is HM_E_RANGE at the point's index when
    kept and nothing when unkept."""
    inside, outside = _edge_longitudes(zmax, sign)
    fn = LATLON_CALLS[call]
    lat, lon = synth.uniform(N, seed=5)
    lat, lon = lat.copy(), lon.copy()
    lon[4097] = inside
    for keep in (None, _mask(N)):
        assert keep is None or keep[4097]
        _verify_latlon(call, fn(lat, lon, keep, zmax), lat, lon, keep, zmax)
    lon[4097] = outside
    assert _expect(lat, lon, None, 0, zmax)[0] == (0, -1)      # the reference bins it
    got, e, _ = _catch(lambda: fn(lat, lon, None, zmax))
    assert got == (RANGE, 4097), got
    _check_exception(e, RANGE, 4097)
    keep = np.ones(N, np.uint8)
    keep[4097] = 0
    res = fn(lat, lon, keep, zmax)
    assert _ctx().last_error() == (-1, 0)
    _verify_latlon(call, res, lat, lon, keep, zmax)


def _mixed_stream(form):
    def call(lat, lon, keep, zmax):
        hour, group = Stream("mixed", form, "fresh").columns(lat.size)
        s = StreamingHeatmap(0, zmax, base_hour=SBASE)
        try:
            s.add(lat, lon, keep, hour, group=group)
        finally:
            s.close()
    return call


MIXED_CALLS = dict(LATLON_CALLS, packed=lambda lat, lon, keep, zmax: device.count_grouped_packed_device(
    lat, lon, _groups(lat.size), keep, 0, zmax), stream_1h=_mixed_stream("1h"), stream_3h=_mixed_stream("3h"),
    stream_many=_mixed_stream("many"))


@pytest.mark.parametrize("call", list(MIXED_CALLS))
def test_key_range_and_nan_mixed(gpu, call):
    """A point beyond the key's column field at index 100 and a NaN at index
    5000.  The header ranks reference errors among themselves only: a count
    made by hm_count's level pipeline (hm_stream_add's for up to 64 buckets
    too) meets projection errors before it builds a key; the key kernels of
    hm_count_grouped*, and of hm_stream_add beyond 64 buckets, take one
    minimum over both.  Either point, with its own kind and exception, is
    within the contract."""
    _, outside = _edge_longitudes(10, 1)
    lat, lon = synth.uniform(N, seed=5)
    lat, lon = lat.copy(), lon.copy()
    lon[100] = outside
    lat[5000] = np.nan
    got, e, _ = _catch(lambda: MIXED_CALLS[call](lat, lon, None, 10))
    assert got in ((RANGE, 100), (NAN, 5000)), got
    _check_exception(e, *got)
    print("mixed RANGE@100 / NaN@5000, %s reports %r" % (call, got))
