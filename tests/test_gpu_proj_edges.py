"""GPU: every kernel that projects lat/lon, fed the projection's own edges
(tests/proj_edges.py), cell for cell against oracle.count.

Five kernels carry a copy of the accept-or-defer decision that bit-exact
tiles depend on: k_l1_fast (hm_project_l1), k_project_partition and
k_project_keys_fast (hm_project_fast), k_project / k_redo / k_collect_exotic /
k_project_keys_slow (hm_project_point or the
exact chain).  test_proj_edges_host.py shows that the statements, compiled for
the host, agree with the oracle on the catalogue; here the device executes
them, and the plumbing around them -- redo list, tile re-feed, exotic list,
fused re-run, sweep -- carries the points they defer.

Bulk points are synth.generate("hotspots"); every count case runs without a
keep mask and with i % 7 != 3.  Every comparison is exact.  Where a call goes
through level 1 of the pipeline, hm_last_stats' slow points must EQUAL the
number of points the host-compiled statements defer -- hm_project_l1 on the
whole 8192-point tiles, hm_project_fast on the partial last one: the device
then made the same decision as the host build on every point (a difference on
one point shows; halve the input to find it)."""
import functools

import numpy as np
import pytest

import proj_edges as pe
from oracle import oracle
from heatmap_amd import device, synth
from heatmap_amd.device import Counts
from heatmap_amd.stream import ALLTIME, StreamingHeatmap

GPU = pytest.mark.gpu

T1 = 8192                 # points per level-1 tile (HM_T1)
REDO_CAP_MIN = 1 << 20    # hm_count's redo and exotic lists hold max(2^20, n / 256) points
LIST_CAP_MIN = 1 << 16    # the grouped paths' deferred list holds max(2^16, n / 256)
STREAM_MAX_PARTS = 64     # HMS_MAX_PARTS: batches of more buckets take the grouped general path
SCAN_LIMIT = 4096 * 4096  # HM_SCAN_LIMIT: dense children per level of the pipeline
BASE = 480000             # epoch hour of the stream cases
KEEPS = [False, True]


def _mask(n, keep):
    return (np.arange(n) % 7 != 3).astype(np.uint8) if keep else None


def _same(got, ref):
    assert ref["status"] == 0
    got = got.sorted()
    assert got.zoom.size == ref["zoom"].size
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k]), k


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _bulk(n, seed):
    return _frozen(*synth.generate("hotspots", n, seed=seed))


def _catalogue(Z, m, start=0):
    """m points of count_set(Z) from `start`, wrapping: the named edges first"""
    lat, lon = pe.count_set(Z)
    i = (start + np.arange(m)) % lat.size
    return lat[i], lon[i]


def _placed(n, seed, Z, where, start=0):
    """n bulk points with catalogue points at the input indices `where`"""
    lat, lon = (a.copy() for a in _bulk(n, seed))
    where = np.asarray(where)
    lat[where], lon[where] = _catalogue(Z, where.size, start)
    return _frozen(lat, lon)


def _deferred(host_math, lat, lon, Z):
    """points the host-compiled statements defer: hm_project_l1 on the whole
    tiles, hm_project_fast on the partial last one"""
    full = lat.size // T1 * T1
    a = pe.host_model(host_math, "l1", lat[:full], lon[:full], Z)[2]
    b = pe.host_model(host_math, "fast", lat[full:], lon[full:], Z)[2]
    return int((~a).sum()) + int((~b).sum())


@functools.lru_cache(maxsize=None)
def _ref(case, args, keep, zmin, zmax):
    lat, lon = case(*args)
    ref = oracle.count(lat, lon, _mask(lat.size, keep), zmin, zmax)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _level1_case(host_math, case, args, Z, keep, chunk=None):
    """one hm_count through level 1: cells, slow points, no re-run"""
    lat, lon = case(*args)
    kp = _mask(lat.size, keep)
    got = device.count(lat, lon, kp, 0, Z) if chunk is None else device.count(lat, lon, kp, 0, Z, chunk=chunk)
    _same(got, _ref(case, args, keep, 0, Z))
    if chunk is None:
        assert int(got.stage_us[7]) != 0, "the call took the general path, not the pipeline"
        assert got.slow_points == _deferred(host_math, lat, lon, Z)
        assert int(got.stage_us[5]) == 0, "a level-1 re-run"
    return got


# --------------------------------------------------------------------------
# projection: k_project against the reference's own results
# --------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("zi", range(6))
def test_project_edges(gpu, zi):
    """device.project on project_set against tests/golden/projection_edges.npz:
    status (row error first), and the tile wherever the reference returns one.
    A column beyond int64 (golden status 8: lon 1e15 at zoom 30) comes back as
    HM_BIGCOL with the row and the column as an integer-valued double, the
    reference's own Python int (oracle._col_of is tile.py:21 literally)."""
    from heatmap_amd import _lib

    g = np.load(pe.GOLDEN)
    z = int(g["zoom"][zi])
    exp, row, col = pe.golden_expect(g, zi)
    big = exp == 8
    exp = np.where(big, _lib.HM_BIGCOL, exp).astype(np.uint8)
    got = device.project(g["lat"], g["lon"], z)
    assert np.array_equal(got.status, exp)
    ok = exp == 0
    assert np.array_equal(got.row[ok], row[ok]) and np.array_equal(got.col[ok], col[ok])
    assert big.any() == (z == 30)
    for i in np.flatnonzero(big).tolist():
        assert got.row[i] == row[i]
        assert int(got.col[i:i + 1].view(np.float64)[0]) == oracle._col_of(float(g["lon"][i]), z)
    bad = np.flatnonzero((exp != 0) & ~big)
    assert bad.size and (got.first_error_index, got.first_error_kind) == (int(bad[0]), int(exp[bad[0]]))


# --------------------------------------------------------------------------
# whole tiles: k_l1_fast, k_redo, the deferred points' tile re-feed
# --------------------------------------------------------------------------

WHOLE_Z = [3, 18, 21]
WHOLE_N = 3 * T1
WHOLE_KINDS = ["scattered", "only", "one"]


@functools.lru_cache(maxsize=None)
def _whole_case(kind, Z):
    if kind == "scattered":   # half the input, the named edges among them, at seeded places
        where = np.sort(np.random.default_rng(Z).permutation(WHOLE_N)[:WHOLE_N // 2])
        return _placed(WHOLE_N, 40 + Z, Z, where)
    if kind == "only":        # the middle tile is catalogue points only, the latitudes first: whole waves defer
        return _placed(WHOLE_N, 41 + Z, Z, T1 + np.arange(T1))
    assert kind == "one"      # one catalogue point (null island) in the call
    lat, lon = (a.copy() for a in _bulk(WHOLE_N, 42 + Z))
    lat[T1 + 4321] = lon[T1 + 4321] = 0.0
    return _frozen(lat, lon)


@functools.lru_cache(maxsize=None)
def _lane_case(j, Z):
    """catalogue points at every input index that is j mod 16, a different
    1536 of them for every j (the 16 cases hold 24576 catalogue points)"""
    return _placed(WHOLE_N, 43 + Z, Z, np.arange(j, WHOLE_N, 16), start=j * (WHOLE_N // 16))


def test_whole_tile_inputs(host_math):
    for Z in WHOLE_Z:
        cl, co = pe.count_set(Z)
        named = int(pe.count_mask(Z)[:pe.n_named()].sum())
        assert named <= WHOLE_N // 2
        lat, lon = _whole_case("scattered", Z)
        assert set(zip(cl[:named].tolist(), co[:named].tolist())) <= set(zip(lat.tolist(), lon.tolist())), \
            "every named edge is in the scattered case"
        lat, lon = _whole_case("only", Z)
        ok = pe.host_model(host_math, "l1", lat[T1:2 * T1], lon[T1:2 * T1], Z)[2]
        # input index i of a tile: thread (i mod 1024) / 2, its point 2 (i / 1024) + (i & 1)
        w = ok.reshape(8, 8, 64, 2)   # [i / 1024, wave, lane, i & 1]
        assert (~w).all(axis=2).sum() >= 32, "waves whose 64 lanes all defer a point"
        assert w.any(), "and points the kernel accepts in the same tile"
        lat, lon = _whole_case("one", Z)
        assert _deferred(host_math, lat, lon, Z) >= 1
        seen = set()
        for j in range(16):
            lat, lon = _lane_case(j, Z)
            seen |= set(zip(lat[j::16].tolist(), lon[j::16].tolist()))
        assert len(seen) > 20000


@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("Z", WHOLE_Z)
@pytest.mark.parametrize("kind", WHOLE_KINDS)
def test_whole_tiles(gpu, host_math, kind, Z, keep):
    _level1_case(host_math, _whole_case, (kind, Z), Z, keep)


@GPU
@pytest.mark.parametrize("Z", WHOLE_Z)
@pytest.mark.parametrize("j", range(16))
def test_whole_tiles_thread_positions(gpu, host_math, j, Z):
    """catalogue points at input index j mod 16, for each j: every one of a
    thread's 16 points (it reads the pairs 2 (512 q + tid), + 1) in turn"""
    for keep in KEEPS:
        _level1_case(host_math, _lane_case, (j, Z), Z, keep)


@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("Z", WHOLE_Z)
def test_chunked(gpu, host_math, Z, keep):
    """chunk = T1 + 1: every chunk a whole tile and a one-point partial one,
    the chunks' cells (and the cells outside the square) merged"""
    _level1_case(host_math, _whole_case, ("scattered", Z), Z, keep, chunk=T1 + 1)


# --------------------------------------------------------------------------
# the partial last tile: k_project_partition, mode 0
# --------------------------------------------------------------------------

PARTIAL_N = [T1 + 777, 777, T1 - 1]


@functools.lru_cache(maxsize=None)
def _partial_case(n, Z):
    """catalogue points in the tail: 600 of the last 777 points, the first
    named latitudes (n = 777) and the first named longitudes (n = T1 + 777);
    n = T1 - 1 is one partial tile of catalogue points only, random pairs"""
    if n == T1 - 1:
        return _placed(n, 50 + Z, Z, np.arange(n), start=pe.n_named() + T1)
    where = n - 777 + np.sort(np.random.default_rng(n + Z).permutation(777)[:600])
    first_lon = int(pe.count_mask(Z)[:pe.latitudes().size].sum())
    return _placed(n, 50 + Z, Z, where, start=first_lon if n > T1 else 0)


@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("Z", WHOLE_Z)
@pytest.mark.parametrize("n", PARTIAL_N)
def test_partial_tile(gpu, host_math, n, Z, keep):
    lat, lon = _partial_case(n, Z)
    full = n // T1 * T1
    assert int((~pe.host_model(host_math, "fast", lat[full:], lon[full:], Z)[2]).sum()) >= 100
    _level1_case(host_math, _partial_case, (n, Z), Z, keep)


# --------------------------------------------------------------------------
# more deferred points than the redo list holds: the fused exact chain
# (k_project_partition mode 2), and the exotic list's rebuild
# --------------------------------------------------------------------------

OVER_Z = 18
OVER_N = REDO_CAP_MIN + 2 * T1
OVER_KINDS = ["equator", "polar"]


@functools.lru_cache(maxsize=None)
def _overflow_case(kind):
    """2^20 + 1 points that every fast path defers, the rest count_set and bulk,
    shuffled.  equator: (0.0, lon), (lat, 0.0) and (0.0, 0.0) in turn, all
    inside the square.  polar: the catalogue's latitudes past the square's edge,
    all outside it -- more kept points than the exotic list holds as well (no
    keep mask), so k_collect_exotic rebuilds it."""
    m = REDO_CAP_MIN + 1
    rest = OVER_N - m
    blat, blon = _bulk(OVER_N, 60)
    lat, lon = blat.copy(), blon.copy()
    i = np.arange(m)
    if kind == "equator":
        lat[:m] = np.where(i % 3 == 1, blat[:m], 0.0)
        lon[:m] = np.where(i % 3 == 0, blon[:m], 0.0)
    else:
        cl = pe.count_set(OVER_Z)[0]
        far = cl[(np.abs(cl) > 85.0512) & (np.abs(cl) <= 90.0)]
        assert far.size > 3000
        lat[:m] = far[i % far.size]
    half = rest // 2
    lat[m:m + half], lon[m:m + half] = _catalogue(OVER_Z, half)
    o = np.random.default_rng(61).permutation(OVER_N)
    return _frozen(lat[o], lon[o])


@pytest.mark.parametrize("kind", OVER_KINDS)
def test_overflow_inputs(host_math, kind):
    lat, lon = _overflow_case(kind)
    assert lat.size == OVER_N and OVER_N % T1 == 0 and max(REDO_CAP_MIN, OVER_N // 256) == REDO_CAP_MIN
    assert _deferred(host_math, lat, lon, OVER_Z) > REDO_CAP_MIN
    r, c, st, _ = oracle.project(lat, lon, OVER_Z)
    assert (st == 0).all()
    out = (r < 0) | (r >= (1 << OVER_Z)) | (c < 0) | (c >= (1 << OVER_Z))
    if kind == "polar":
        assert out.sum() > REDO_CAP_MIN and out[_mask(OVER_N, True) == 1].sum() <= REDO_CAP_MIN
    else:
        assert 0 < out.sum() < 2 * T1
        assert ((lat == 0.0) & (lon == 0.0)).sum() > 300000


@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("kind", OVER_KINDS)
def test_redo_overflow(gpu, host_math, kind, keep):
    """k_l1_fast defers more points than the redo list holds (hm_project_l1's
    count, checked on the CPU by test_overflow_inputs); level 1 runs again as
    k_project_partition with the exact chain fused, whose decisions are
    hm_project_fast's on every tile: the slow points are the points THAT run
    resolved.  (Before this module the first run's deferred points were added
    to them: 2,108,114 slow points for the 1,054,057 deferred of the polar
    case without a keep mask.)"""
    lat, lon = _overflow_case(kind)
    got = device.count(lat, lon, _mask(OVER_N, keep), 0, OVER_Z)
    assert got.slow_points > REDO_CAP_MIN
    assert got.slow_points == int((~pe.host_model(host_math, "fast", lat, lon, OVER_Z)[2]).sum())
    assert int(got.stage_us[7]) != 0   # (the equator case's one hot region also overflows: slot 5 is 1 there)
    _same(got, _ref(_overflow_case, (kind,), keep, 0, OVER_Z))


# --------------------------------------------------------------------------
# the general path of hm_count: k_project_keys_fast / k_project_keys_slow
# --------------------------------------------------------------------------

GEN_Z = 21
GEN_CLOUD = 330000


@functools.lru_cache(maxsize=None)
def _general_case():
    """count_set mixed into a uniform cloud whose kept points occupy more
    zoom-11 tiles than the pipeline's last level (zooms 5, 11, 14 at zmax 21)
    has dense children for: parents x 4^3 > HM_SCAN_LIMIT = 2^24, more than
    262144 tiles.  The call then takes count_fallback."""
    ula, ulo = synth.generate("uniform", GEN_CLOUD, seed=62)
    cl, co = pe.count_set(GEN_Z)
    lat, lon = np.concatenate([ula, cl]), np.concatenate([ulo, co])
    o = np.random.default_rng(63).permutation(lat.size)
    return _frozen(lat[o], lon[o])


def test_general_inputs():
    lat, lon = _general_case()
    r, c, st, _ = oracle.project(lat, lon, 11)
    for keep in KEEPS:
        kb = np.ones(lat.size, bool) if not keep else _mask(lat.size, True).astype(bool)
        insq = kb & (r >= 0) & (r < 2048) & (c >= 0) & (c < 2048)
        parents = np.unique(r[insq] * 2048 + c[insq]).size
        print("kept zoom-11 tiles:", parents)
        assert parents << 6 > SCAN_LIMIT, keep
    assert lat.size < 400000


@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("zmin", [0, GEN_Z])
def test_general_path(gpu, zmin, keep):
    lat, lon = _general_case()
    got = device.count(lat, lon, _mask(lat.size, keep), zmin, GEN_Z)
    assert int(got.stage_us[7]) == 0, "the call took the pipeline, not the general path"
    _same(got, _ref(_general_case, (), keep, zmin, GEN_Z))


# --------------------------------------------------------------------------
# grouped counts: k_project_keys_fast, k_project_keys_slow (list and sweep)
# --------------------------------------------------------------------------

GROUPS = 3


def _grouped_same(got, lat, lon, kp, gid, zmin, Z):
    got = got.sorted()
    assert set(np.unique(got.group).tolist()) <= set(range(GROUPS))
    for g in range(GROUPS):
        sel = (gid == g).astype(np.uint8) if kp is None else (kp & (gid == g)).astype(np.uint8)
        ref = oracle.count(lat, lon, sel, zmin, Z)
        assert ref["status"] == 0
        m = got.group == g
        assert int(m.sum()) == ref["zoom"].size, g
        for k in ("zoom", "row", "col", "count"):
            assert np.array_equal(getattr(got, k)[m], ref[k]), (g, k)


@functools.lru_cache(maxsize=None)
def _grouped_case(kind, Z):
    """listed: count_set and bulk, about 40,000 points.  sweep: 80,000 points
    of which 70,000 lie on the equator -- more deferred points than the 2^16
    list holds, so k_project_keys_slow sweeps the input."""
    cl, co = pe.count_set(Z)
    if kind == "listed":
        n = 40000
        bl, bo = _bulk(n - cl.size, 70 + Z)
        lat, lon = np.concatenate([cl, bl]), np.concatenate([co, bo])
    else:
        n = 80000
        bl, bo = _bulk(70000, 71 + Z)
        lat = np.concatenate([np.zeros(70000), cl[:10000]])
        lon = np.concatenate([bo, co[:10000]])
    o = np.random.default_rng(72 + Z).permutation(n)
    gid = (np.random.default_rng(73 + Z).integers(0, GROUPS, n)).astype(np.uint32)
    return _frozen(lat[o], lon[o], gid)


def test_grouped_inputs(host_math):
    for Z in (18, 21):
        lat, lon, gid = _grouped_case("listed", Z)
        slow = int((~pe.host_model(host_math, "fast", lat, lon, Z)[2]).sum())
        assert 38000 <= lat.size <= 42000 and 1000 < slow <= LIST_CAP_MIN
    lat, lon, gid = _grouped_case("sweep", 18)
    assert lat.size == 80000 and max(LIST_CAP_MIN, 80000 // 256) == LIST_CAP_MIN
    assert int((~pe.host_model(host_math, "fast", lat, lon, 18)[2]).sum()) > LIST_CAP_MIN


@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("kind,Z", [("listed", 18), ("listed", 21), ("sweep", 18)])
def test_grouped(gpu, kind, Z, keep):
    lat, lon, gid = _grouped_case(kind, Z)
    kp = _mask(lat.size, keep)
    zmin = Z - 4
    _grouped_same(device.count_grouped(lat, lon, gid, kp, zmin, Z), lat, lon, kp, gid, zmin, Z)
    assert device.context(0).last_error() == (-1, 0)


@functools.lru_cache(maxsize=None)
def _packed_case(Z):
    """the points of the listed case inside the square, and one outside it"""
    lat, lon, gid = _grouped_case("listed", Z)
    r, c, st, _ = oracle.project(lat, lon, Z)
    insq = (r >= 0) & (r < (1 << Z)) & (c >= 0) & (c < (1 << Z))
    lat, lon, gid = lat[insq], lon[insq], gid[insq]
    e = lat.size // 2
    pair = pe.square_edge_pairs()[Z, "north"]
    assert lat[e] != pair[1]
    lat = lat.copy()
    lat[e] = pair[1]                      # row -1: one double past the square's edge
    return _frozen(lat, lon, gid) + (e,)


@GPU
@pytest.mark.parametrize("Z", [18, 21])
def test_grouped_packed(gpu, Z):
    """Packed records hold tiles of the square only: None (HM_E_EXOTIC) when a
    kept point is outside it -- here by one ulp of latitude -- and the records
    when that point is not kept."""
    lat, lon, gid, e = _packed_case(Z)
    assert oracle.project(lat[e:e + 1], lon[e:e + 1], Z)[0][0] == -1
    zmin = Z - 4
    assert device.count_grouped_packed_device(lat, lon, gid, None, zmin, Z) is None
    kp = np.ones(lat.size, np.uint8)
    assert device.count_grouped_packed_device(lat, lon, gid, kp, zmin, Z) is None
    kp[e] = 0
    res = device.count_grouped_packed_device(lat, lon, gid, kp, zmin, Z)
    assert res is not None
    k = res[0].cpu().numpy().view(np.uint64)
    gc = res[1].cpu().numpy().view(np.uint64)
    z, r, c = device.decode_keys(k)
    got = device.GroupedCounts((gc >> np.uint64(32)).astype(np.uint32), z, r, c,
                               (gc & np.uint64(0xFFFFFFFF)).astype(np.int64))
    _grouped_same(got, lat, lon, kp, gid, zmin, Z)


# --------------------------------------------------------------------------
# the stream: one add of count_set, per-bucket pipeline and grouped path
# --------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("nhours", [3, 35])
def test_stream(gpu, nhours, keep):
    """One StreamingHeatmap.add of count_set with 2 groups: 6 buckets (the
    per-bucket pipeline) and 70 (> HMS_MAX_PARTS: the grouped path).  The
    batch holds kept points outside the square, so the add splits: those are
    counted per (group, hour) by hm_count_grouped, the rest inserted."""
    Z = 18
    lat, lon = pe.count_set(Z)
    n = lat.size
    assert 2 * nhours > STREAM_MAX_PARTS or nhours == 3
    rng = np.random.default_rng(80 + nhours)
    hour = (BASE + rng.integers(0, nhours, n)).astype(np.uint32)
    gid = rng.integers(0, 2, n).astype(np.uint32)
    kp = _mask(n, keep)
    kb = np.ones(n, np.uint8) if kp is None else kp
    s = StreamingHeatmap(0, Z, base_hour=BASE)
    s.add(lat, lon, kp, hour, group=gid)
    _same(s.counts(ALLTIME), oracle.count(lat, lon, kp, 0, Z))
    hourly = s.hourly()
    assert sorted(hourly) == sorted(np.unique(hour[kb == 1]).tolist())
    for h in sorted(hourly)[:3] + sorted(hourly)[-1:]:
        sel = kb & (hour == h).astype(np.uint8)
        _same(hourly[h], oracle.count(lat, lon, sel, 0, Z))
        _same(s.counts(h), oracle.count(lat, lon, sel, 0, Z))
    g, p, z, r, c, cnt = s.rollup("alltime", merge_groups=False)
    for u in (0, 1):
        m = g == u
        _same(Counts(z[m], r[m], c[m], cnt[m], 0, []), oracle.count(lat, lon, kb & (gid == u).astype(np.uint8), 0, Z))
    s.close()
