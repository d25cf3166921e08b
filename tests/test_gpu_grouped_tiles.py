"""GPU: hm_count_grouped_tiles and hm_count_grouped_packed_tiles -- grouped
counts from zoom-zmax tile coordinates -- and hm_count_tiles on the general
fallback, against the oracle.

All three list the kept tiles with k_tiles_list (csrc/hm_general.hip): a block
step of 4096 tiles reserves its room in the (row, col, group, index) list with
one atomic after a block scan of the keep flags.  The reference is, per group
id, oracle.count_tiles(rows, cols, zmin, zmax, keep & (group == id)); every
field of the sorted records is compared, as test_gpu_general.py does for
lat/lon input."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, device, synth

pytestmark = pytest.mark.gpu

STEP = 4096                       # tiles per block step of k_tiles_list
SIZES = [1, 255, 4095, 4096, 4097, 100_000]
ZOOMS = [(0, 0), (0, 14), (6, 21), (21, 21)]
GROUPS = ["one", "sparse7", "thousand", "wide"]
KEEPS = ["none", "most", "nothing", "last_step"]
FIELDS = ("group", "zoom", "row", "col", "count")


def _exotic_cloud(n, seed, frac=0.05):
    """A hotspot cloud with a share of polar latitudes and longitudes at or
    beyond +-180 (the cloud of test_gpu_general.py)."""
    rng = np.random.default_rng(seed)
    lat, lon = synth.generate("hotspots", n, seed=seed)
    lat, lon = lat.copy(), lon.copy()
    m = rng.random(n) < frac
    k = int(m.sum())
    lat[m] = rng.choice([-1.0, 1.0], k) * rng.uniform(85.06, 89.9, k)
    lon[m] = rng.choice([180.0, 200.0, -200.0, 540.0, -180.0, 179.99999999999997], k)
    return lat, lon


def _tiles(n, Z, exotic, seed):
    """Zoom-Z tiles of a hotspot cloud (in the square); exotic: 5% of them
    with negative rows, rows >= 2^Z, negative columns and columns up to
    +-2^40, as test_exotic_tiles."""
    lat, lon = synth.generate("hotspots", n, seed=seed)
    rows, cols, st, _ = oracle.project(lat, lon, Z)
    assert not st.any()
    if exotic:
        rng = np.random.default_rng(seed)
        m = rng.random(n) < 0.05
        m[n // 2] = True
        k = int(m.sum())
        rows[m] = rng.integers(-(8 << Z), 8 << Z, k)
        cols[m] = rng.integers(-(1 << 40), 1 << 40, k)
    return rows, cols


def _group_ids(kind, n, zmax, seed):
    rng = np.random.default_rng(seed + 1)
    if kind == "one":
        return np.full(n, 3, np.uint32)
    if kind == "sparse7":
        return rng.integers(0, 7, n).astype(np.uint32) * 7919
    if kind == "thousand":
        return rng.integers(0, 1000, n).astype(np.uint32)
    return rng.integers(0, 5_000_000, n).astype(np.uint32)      # past 2^22: 128-bit keys at zoom 21


def _keep(kind, n, seed):
    if kind == "none":
        return None
    if kind == "most":
        return (np.random.default_rng(seed + 2).random(n) < 0.8).astype(np.uint8)
    if kind == "nothing":
        return np.zeros(n, np.uint8)
    k = np.zeros(n, np.uint8)
    k[(n - 1) // STEP * STEP:] = 1                               # only the last block step holds kept tiles
    return k


def _reference(rows, cols, g, keep, zmin, zmax):
    """(expected records, None): the oracle per group id.  With more than 200
    ids (the 1000-id cases of 100_000 tiles keep the oracle for each id; one
    call costs 2 ms whatever its size) the expected records are a plain numpy
    count of every (group, zoom, row >> k, col >> k), and the second value
    lists 40 ids that _check pins to the oracle one by one, beside the
    oracle's count of all ids together."""
    kb = np.ones(rows.size, bool) if keep is None else keep.astype(bool)
    ids = np.unique(g[kb])
    exp = {k: [] for k in FIELDS}
    if ids.size <= 200 or (rows.size >= SIZES[-1] and ids.size <= 2000):
        for gid in ids:
            ref = oracle.count_tiles(rows, cols, zmin, zmax, (kb & (g == gid)).astype(np.uint8))
            o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
            exp["group"].append(np.full(o.size, gid, np.uint32))
            for k in FIELDS[1:]:
                exp[k].append(ref[k][o])
        return {k: np.concatenate(v) if v else np.zeros(0, np.int64) for k, v in exp.items()}, None
    r, c, gg = rows[kb], cols[kb], g[kb]
    for z in range(zmin, zmax + 1):
        rec = np.stack([gg.astype(np.int64), r >> (zmax - z), c >> (zmax - z)], axis=1)
        u, cnt = np.unique(rec, axis=0, return_counts=True)
        exp["group"].append(u[:, 0].astype(np.uint32))
        exp["zoom"].append(np.full(len(u), z, np.int32))
        exp["row"].append(u[:, 1])
        exp["col"].append(u[:, 2])
        exp["count"].append(cnt.astype(np.int64))
    exp = {k: np.concatenate(v) for k, v in exp.items()}
    o = np.lexsort((exp["col"], exp["row"], exp["zoom"], exp["group"]))
    return {k: v[o] for k, v in exp.items()}, ids[:: max(1, ids.size // 40)]


def _check(got, rows, cols, g, keep, zmin, zmax):
    got = got.sorted()
    exp, sample = _reference(rows, cols, g, keep, zmin, zmax)
    for k in FIELDS:
        assert np.array_equal(getattr(got, k), exp[k]), k
    if sample is not None:
        kb = np.ones(rows.size, bool) if keep is None else keep.astype(bool)
        for gid in sample:
            ref = oracle.count_tiles(rows, cols, zmin, zmax, (kb & (g == gid)).astype(np.uint8))
            o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
            m = got.group == gid
            for k in FIELDS[1:]:
                assert np.array_equal(getattr(got, k)[m], ref[k][o]), (gid, k)
        # every group together: the ungrouped oracle count
        ref = oracle.count_tiles(rows, cols, zmin, zmax, keep)
        o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
        rec = np.stack([got.zoom.astype(np.int64), got.row, got.col], axis=1)
        u, inv = np.unique(rec, axis=0, return_inverse=True)
        tot = np.zeros(len(u), np.int64)
        np.add.at(tot, inv.reshape(-1), got.count)
        assert np.array_equal(u[:, 0], ref["zoom"][o]) and np.array_equal(u[:, 1], ref["row"][o])
        assert np.array_equal(u[:, 2], ref["col"][o]) and np.array_equal(tot, ref["count"][o])


def _grid():
    """The sizes up to the block step + 1 with every zoom range, the group
    kind, keep mask and tile kind rotating; 100_000 tiles with each group
    kind; then group kind, keep mask and tile kind crossed at the block step
    + 1."""
    out = []
    i = 0
    for n in SIZES[:-1]:
        for zmin, zmax in ZOOMS:
            grp = GROUPS[i % 4] if zmax == 21 or GROUPS[i % 4] != "wide" else "thousand"
            out.append((n, zmin, zmax, grp, KEEPS[(i + i // 4) % 4], bool((i + i // 8) % 2)))
            i += 1
    big = SIZES[-1]              # several block steps per block, every group kind, mostly kept
    out += [(big, 0, 0, "one", "most", False), (big, 0, 14, "sparse7", "most", True),
            (big, 6, 21, "thousand", "none", True), (big, 21, 21, "wide", "none", True),
            (big, 16, 21, "wide", "most", True), (big, 0, 14, "thousand", "last_step", False)]
    for grp in GROUPS:
        for kp in KEEPS:
            for exotic in (False, True):
                out.append((STEP + 1, 6 if grp == "wide" else 0, 21 if grp == "wide" else 14, grp, kp, exotic))
    return out


@pytest.mark.parametrize("n,zmin,zmax,groups,keep,exotic", _grid())
def test_grouped_tiles_vs_oracle(gpu, n, zmin, zmax, groups, keep, exotic):
    seed = n % 1000 + zmax
    rows, cols = _tiles(n, zmax, exotic, seed)
    g = _group_ids(groups, n, zmax, seed)
    kp = _keep(keep, n, seed)
    got = device.count_grouped(rows, cols, g, kp, zmin, zmax, tiles=True)
    assert device.context(0).last_error() == (-1, 0)
    if keep == "nothing":
        assert got.count.size == 0
    _check(got, rows, cols, g, kp, zmin, zmax)


def _raw_grouped_tiles(rows, cols, keep, group, zmin, zmax, capacity):
    """hm_count_grouped_tiles as the C caller sees it: (status, n_out, records)."""
    import torch

    ctx = device.context(0)
    r = device._dev(rows, torch.int64, 0)
    c = device._dev(cols, torch.int64, 0)
    k = None if keep is None else device._dev(keep, torch.uint8, 0)
    g = None if group is None else device._dev(np.asarray(group, np.uint32).view(np.int32), torch.int32, 0)
    cells = torch.empty(5 * max(capacity, 1), dtype=torch.int64, device=r.device)
    nout = ctypes.c_int64(-1)
    rc = ctx.L.hm_count_grouped_tiles(ctx.ptr, device._ptr(r), device._ptr(c), device._ptr(k), device._ptr(g),
                                      rows.size, zmin, zmax, device._ptr(cells), capacity, ctypes.byref(nout))
    x = cells[:5 * min(max(nout.value, 0), capacity)].cpu().numpy().reshape(-1, 5)
    return rc, nout.value, x


@pytest.mark.parametrize("keep", ["none", "most"])
def test_grouped_tiles_null_group(gpu, keep):
    """group = NULL is one group 0, and its records are hm_count_tiles' cells."""
    n, zmin, zmax = 5000, 0, 16
    rows, cols = _tiles(n, zmax, True, seed=3)
    kp = _keep(keep, n, 3)
    rc, m, x = _raw_grouped_tiles(rows, cols, kp, None, zmin, zmax, 4 * n * (zmax + 1))
    assert rc == _lib.HM_OK and m == len(x)
    assert not x[:, 0].any()
    got = device.GroupedCounts(x[:, 0].astype(np.uint32), x[:, 1].astype(np.int32), x[:, 2], x[:, 3], x[:, 4]).sorted()
    ref = device.count(rows, cols, kp, zmin, zmax, tiles=True).sorted()
    for k in FIELDS[1:]:
        assert np.array_equal(getattr(got, k), getattr(ref, k)), k
    _check(got, rows, cols, np.zeros(n, np.uint32), kp, zmin, zmax)


def test_grouped_tiles_capacity(gpu):
    """capacity 0: HM_E_CAPACITY with *n_out = the records of the full call;
    that capacity exactly: HM_OK and the same records."""
    n, zmin, zmax = 5000, 2, 15
    rows, cols = _tiles(n, zmax, True, seed=4)
    g = _group_ids("sparse7", n, zmax, 4)
    full = device.count_grouped(rows, cols, g, None, zmin, zmax, tiles=True).sorted()
    rc, m, _ = _raw_grouped_tiles(rows, cols, None, g, zmin, zmax, 0)
    assert rc == _lib.HM_E_CAPACITY and m == full.count.size
    rc, m2, x = _raw_grouped_tiles(rows, cols, None, g, zmin, zmax, m)
    assert rc == _lib.HM_OK and m2 == m and len(x) == m
    got = device.GroupedCounts(x[:, 0].astype(np.uint32), x[:, 1].astype(np.int32), x[:, 2], x[:, 3], x[:, 4]).sorted()
    for k in FIELDS:
        assert np.array_equal(getattr(got, k), getattr(full, k)), k
    rc, m3, _ = _raw_grouped_tiles(rows, cols, None, g, zmin, zmax, m - 1)
    assert rc == _lib.HM_E_CAPACITY and m3 == m


@pytest.mark.parametrize("zmin,zmax", [(0, 14), (6, 21)])
def test_grouped_tiles_equal_grouped_points(gpu, zmin, zmax):
    """count_grouped of points == count_grouped of their projected tiles."""
    lat, lon = _exotic_cloud(120_000, seed=zmax)
    rng = np.random.default_rng(zmax)
    g = rng.integers(0, 50, lat.size).astype(np.uint32) * 7919
    keep = (rng.random(lat.size) < 0.8).astype(np.uint8)
    p = device.project(lat, lon, zmax)
    assert not p.status.any()
    a = device.count_grouped(lat, lon, g, keep, zmin, zmax).sorted()
    b = device.count_grouped(p.row, p.col, g, keep, zmin, zmax, tiles=True).sorted()
    assert (b.row < 0).any() and b.count.sum() == int(keep.sum()) * (zmax - zmin + 1)
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def _decode_packed(keys, gc):
    k = keys.cpu().numpy().view(np.uint64)
    gcn = gc.cpu().numpy().view(np.uint64)
    z, r, c = device.decode_keys(k)
    return device.GroupedCounts((gcn >> np.uint64(32)).astype(np.uint32), z, r, c,
                                (gcn & np.uint64(0xFFFFFFFF)).astype(np.int64))


@pytest.mark.parametrize("zmin,zmax", ZOOMS)
@pytest.mark.parametrize("n", SIZES)
def test_grouped_packed_tiles_vs_oracle(gpu, n, zmin, zmax):
    """hm_count_grouped_packed_tiles on in-square tiles: the oracle's records
    per group, those of one zoom contiguous, zoom zmax first.  One kept tile
    outside the square -- row -1, row 2^Z, column -1 or column 2^Z -- is
    HM_E_EXOTIC (None); the same tile unkept is accepted."""
    i = SIZES.index(n) + ZOOMS.index((zmin, zmax))
    seed = n % 1000 + zmax + 7
    rows, cols = _tiles(n, zmax, False, seed)
    groups = GROUPS[i % 4] if zmax == 21 or GROUPS[i % 4] != "wide" else "sparse7"
    if n == SIZES[-1] and groups == "thousand":
        groups = "sparse7"       # 1000 oracle calls over 100_000 tiles, twice, take 4 s
    g = _group_ids(groups, n, zmax, seed)
    kp = _keep(KEEPS[(i // 2) % 4] if n > 1 else "none", n, seed)
    res = device.count_grouped_packed_device(rows, cols, g, kp, zmin, zmax, tiles=True)
    assert res is not None
    got = _decode_packed(*res)
    if got.count.size:
        assert np.all(np.diff(got.zoom) <= 0) and got.zoom[0] == zmax and got.zoom[-1] == zmin
    _check(got, rows, cols, g, kp, zmin, zmax)
    at = n // 2
    for r, c in ((-1, 0), (1 << zmax, 0), (0, -1), (0, 1 << zmax)):
        r2, c2 = rows.copy(), cols.copy()
        r2[at], c2[at] = r, c
        keep2 = np.ones(n, np.uint8) if kp is None else kp.copy()
        keep2[at] = 1
        assert device.count_grouped_packed_device(r2, c2, g, keep2, zmin, zmax, tiles=True) is None, (r, c)
        keep2[at] = 0
        res = device.count_grouped_packed_device(r2, c2, g, keep2, zmin, zmax, tiles=True)
        assert res is not None, (r, c)
    _check(_decode_packed(*res), r2, c2, g, keep2, zmin, zmax)


FALLBACK_N = 320_000


def test_count_tiles_general_fallback(gpu):
    """hm_count_tiles of a sparse zoom-21 tile set takes the general path
    (count_fallback: k_tiles_list with the keep mask, no group array).
    Measured on an MI355X: this recipe stays on the pipeline up to 316_113
    tiles and takes the general path from 317_089 on (the level plan's dense
    child space passes its limit); 320_000 is the next round size."""
    n = FALLBACK_N
    rng = np.random.default_rng(21)
    rows = rng.integers(0, 1 << 21, n)
    cols = rng.integers(0, 1 << 21, n)
    rows[::1000] = -5
    cols[1::1000] = (1 << 21) + 9
    keep = (np.arange(n) % 7 != 3).astype(np.uint8)
    got = device.count(rows, cols, keep, 0, 21, tiles=True)
    assert int(got.stage_us[7]) == 0, "the call took the pipeline, not the general path"
    got = got.sorted()
    ref = oracle.count_tiles(rows, cols, 0, 21, keep)
    o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
    for k in FIELDS[1:]:
        assert np.array_equal(getattr(got, k), ref[k][o]), k
