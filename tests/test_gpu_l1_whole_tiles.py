"""Level 1 over whole lat/lon tiles (k_l1_fast).

The kernel takes every whole 8192-point tile of a lat/lon call (tile input
and the partial last tile go through k_project_partition).  Its blocks read
the regions of their slots from a per-call table (rebuilt for an overflow
re-run) and copy their staged keys out in three batches of LDS reads; none
of that may change a count.  Every case is compared cell for cell with
oracle.count, without a keep mask and with one (two instantiations).
"""
import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import device, synth

pytestmark = pytest.mark.gpu

T1 = 8192   # points per level-1 tile (HM_T1)


def _same(got, ref):
    got = got.sorted()
    assert got.zoom.size == ref["zoom"].size
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k]), k


def _mask(n, keep):
    return (np.arange(n) % 7 != 3).astype(np.uint8) if keep else None


def _centre(rows, cols, Z):
    """lat/lon of the centres of zoom-Z tiles: far from the guard band."""
    y = np.pi - 2.0 * np.pi * (rows + 0.5) / float(1 << Z)
    return np.degrees(np.arctan(np.sinh(y))), (cols + 0.5) / float(1 << Z) * 360.0 - 180.0


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("n,zmax", [(T1, 18), (3 * T1, 18), (3 * T1 + 1, 18), (T1, 3)])
def test_whole_tile_sizes(gpu, n, zmax, keep):
    """Whole tiles, whole tiles plus a partial one, and a level of fewer than
    1024 cold digits (zmax 3: 64 of them, the other slots are dead)."""
    lat, lon = synth.generate("hotspots", n, seed=3)
    kp = _mask(n, keep)
    _same(device.count(lat, lon, kp, 0, zmax), oracle.count(lat, lon, kp, 0, zmax))


@pytest.mark.parametrize("keep", [False, True])
def test_merged_wave(gpu, keep):
    """One tile, every kept point the same point: all 64 lanes of a wave share
    a slot, so each count is merged and each rank comes from the lane mask."""
    lat = np.full(T1, 37.7749)
    lon = np.full(T1, -122.4194)
    kp = _mask(T1, keep)
    _same(device.count(lat, lon, kp, 0, 18), oracle.count(lat, lon, kp, 0, 18))


@pytest.mark.parametrize("keep", [False, True])
def test_empty_tile(gpu, keep):
    """The middle tile of three stages nothing (total = 0): the keep mask drops
    it, or, without a mask, all its points are polar and deferred."""
    n = 3 * T1
    lat, lon = synth.generate("hotspots", n, seed=4)
    kp = None
    if keep:
        kp = np.ones(n, np.uint8)
        kp[T1:2 * T1] = 0
    else:
        lat[T1:2 * T1] = 85.06 + (np.arange(T1) % 389) * 0.01
    got = device.count(lat, lon, kp, 0, 18)
    if not keep:
        assert got.slow_points >= T1
    _same(got, oracle.count(lat, lon, kp, 0, 18))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("zmax", [13, 18, 21])
def test_hot_sharded_dead(gpu, zmax, keep):
    """Hot tiles, a sharded cold digit and dead slots in one call: 1M hotspot
    points plus 2^18 points spread over one zoom-5 tile in the south Pacific
    (no hotspot there; more than the 16 tiles' worth that shards a digit).
    At zmax 18 and 21 the hot tiles are zoom-11 ones and that spread stays
    cold, a sharded cold digit; at zmax 13 they are zoom-6 tiles, so it lands
    in hot tiles instead.  zmax 21 stores 32-bit hot keys."""
    lat, lon = synth.generate("hotspots", 1_000_000, seed=31)
    rng = np.random.default_rng(5)
    m = 1 << 18
    # zoom-5 tile (row 20, col 5): lon in [-123.75, -112.5), lat in about (-48.9, -40.9)
    lat = np.concatenate([lat, rng.uniform(-48.0, -42.0, m)])
    lon = np.concatenate([lon, rng.uniform(-123.0, -113.0, m)])
    perm = rng.permutation(lat.size)
    lat, lon = lat[perm], lon[perm]
    kp = _mask(lat.size, keep)
    with device.tuned(HM_HOT_MIN_KEYS=0):
        got = device.count(lat, lon, kp, 0, zmax)
    assert got.stage_us[6] > 0, "no hot tiles"
    _same(got, oracle.count(lat, lon, kp, 0, zmax))


@pytest.mark.parametrize("keep", [False, True])
def test_overflow_rerun_latlon(gpu, keep):
    """tests/test_gpu_hot.py's under-sampled hot tile, as lat/lon points at
    their tiles' centres: tile B's region overflows in k_l1_fast and the
    level is re-run with exact sizes, from a slot table rebuilt for them."""
    Z = 18
    n = 1 << 22
    idx = np.arange(n)
    rows = np.full(n, 5000, np.int64)
    cols = np.full(n, 9000, np.int64)
    sampled = idx % 16 == 0
    b = sampled & ((idx // 16) % 1500 == 0)
    b |= (~sampled) & (idx % 3 != 0)
    rows[b] = 200064 + (idx[b] % 60)
    cols[b] = 100000 + (idx[b] % 89)
    lat, lon = _centre(rows, cols, Z)
    kp = _mask(n, keep)
    with device.tuned(HM_HOT_MIN_KEYS=0):
        got = device.count(lat, lon, kp, 0, Z)
    assert int(got.stage_us[5]) >= 1, "no level-1 re-run: the region did not overflow"
    assert got.slow_points == 0
    _same(got, oracle.count(lat, lon, kp, 0, Z))


@pytest.mark.parametrize("keep", [False, True])
def test_deferred_points(gpu, keep):
    """Longitudes exactly on zoom-18 column boundaries and latitudes in
    (85.06, 89), mixed into two tiles: these points go to k_redo and, the
    polar ones, to cells outside the square."""
    Z = 18
    n = 2 * T1
    lat, lon = synth.generate("hotspots", n, seed=6)
    i = np.arange(n)
    edge = i % 5 == 1
    lon[edge] = (i[edge] * 37 % (1 << Z)) / float(1 << Z) * 360.0 - 180.0
    polar = i % 9 == 2
    lat[polar] = 85.06 + (i[polar] % 391) * 0.01
    kp = _mask(n, keep)
    got = device.count(lat, lon, kp, 0, Z)
    assert got.slow_points >= int((edge | polar).sum()) // 2
    _same(got, oracle.count(lat, lon, kp, 0, Z))
