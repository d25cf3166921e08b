"""Final aggregation at every work-item size, and every run-shard count.

Two parameters of the count pipeline depend on the size of the call and never
take their production values at parity sizes:

  keys per final-aggregation work item (hm_api.cpp CountCall::plan: HM_TA = 262144,
  halved down to HM_TA_MIN = 16384 until the call holds HM_TA_ITEMS = 128
  items' worth of points): 16384 below 4,194,304 points, 262144 from
  33,554,432.  It sets the items per bucket (k_level1_buckets, the run scan),
  each item's [a, b) and runs [r0, r1) (k_items), where hm_stream_runs clips
  a run at an item edge, and whether a bucket takes k_aggregate's single-item
  pyramid or the slot add plus k_aggregate_merged.  Forced here with
  device.tuned(HM_TA_MIN=T, HM_TA_ITEMS=2**30), which gives T for any n, and
  read back from hm_last_stats slot 8 in every case.

  run-counter shards per level-2+ child (HM_RUN_SHARD_BITS: 4 by default, 0
  with hot tiles or the spread plan, lowered while children << bits > 2^25).

Tile input (hm_count_tiles), so bucket sizes are exact; a bucket is one
128 x 128 block of zoom-Z tiles filled by test_gpu_buckets._bucket_tiles'
patterns.  Expected counts: oracle.count_tiles (oracle.count for the lat/lon
case), compared cell for cell after sorting.  Each input's reference is
computed once and shared by the cases that run it.
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import device, synth
from test_gpu_buckets import _bucket_tiles
from test_gpu_l1_whole_tiles import _centre

pytestmark = pytest.mark.gpu

TA = 262144          # HM_TA
TA_MIN = 16384       # default HM_TA_MIN
TA_ITEMS = 128       # default HM_TA_ITEMS
TN = 8192            # HM_TN: keys per partition work item; also HM_T1, points per level-1 tile
NO_SPREAD = 1e30     # HM_SPREAD_MIN_KEYS: never the 3-zoom levels
PATS = ("spread", "same", "corner")


def _same(got, ref):
    got = got.sorted()
    assert got.zoom.size == ref["zoom"].size
    for k in ("zoom", "row", "col", "count"):
        assert np.array_equal(getattr(got, k), ref[k]), k


def _count(rows, cols, zmin, Z, T=None, keep=None, tiles=True, **knobs):
    """One count under the knobs, the item size forced to T (None: the
    default selection); the item size is asserted from slot 8."""
    if T is not None:
        knobs.update(HM_TA_MIN=T, HM_TA_ITEMS=2 ** 30)
    with device.tuned(**knobs):
        got = device.count(rows, cols, keep, zmin, Z, tiles=tiles)
    if T is not None:
        assert int(got.stage_us[8]) == T
    return got


def _local(rng, size, pattern):
    """size tiles of one bucket in the pattern, as (row, col) inside the bucket."""
    r, c = _bucket_tiles(rng, 18, [size], [pattern])
    return r & 127, c & 127


def _buckets(rng, specs, blocks):
    """The buckets specs[i] = (size, pattern) at bucket coordinates blocks[i],
    bucket after bucket."""
    rows, cols = [], []
    for (s, p), (br, bc) in zip(specs, blocks):
        r, c = _local(rng, s, p)
        rows.append(br * 128 + r)
        cols.append(bc * 128 + c)
    return np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)


def _outside(rows, cols, blocks):
    """Mask of the tiles that lie in none of the buckets."""
    side = 1 << 40
    used = np.array([br * side + bc for br, bc in blocks], np.int64)
    return ~np.isin((rows >> 7) * side + (cols >> 7), used)


def _bucket_counts(ref, z, blocks):
    """The reference's counts of the zoom-z cells `blocks` (0 if absent)."""
    m = ref["zoom"] == z
    d = dict(zip(zip(ref["row"][m].tolist(), ref["col"][m].tolist()), ref["count"][m].tolist()))
    return [d.get((int(br), int(bc)), 0) for br, bc in blocks]


# ---------------------------------------------------------------------------
# 1. item edges at every item size, two-level plan (Z = 18)
# ---------------------------------------------------------------------------

P5 = (11, 20)   # the zoom-5 tile (8192 x 8192 zoom-18 tiles, 64 x 64 buckets) that holds every bucket


def _edge_sizes(T):
    if T == TA:   # the point budget
        return [T - 1, T, T + 1, 2 * T + 1, 3 * T + 7]
    return [512, 513, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 7]


@functools.lru_cache(maxsize=2)
def _edges(T, zmin):
    """Buckets of the edge sizes in ONE zoom-5 parent, so that their runs at
    the last level start wherever a parent work item (8192 keys) meets them,
    over a background in the same parent (about 50 keys per other bucket: the
    small path) and a thin one over the world.  Every pattern at every size
    up to T = 32768, one pattern per size above (the point budget).  Returned
    contiguous: background, then bucket after bucket."""
    rng = np.random.default_rng(T)
    sizes = _edge_sizes(T)
    if T <= 32768:
        specs = [(s, p) for s in sizes for p in PATS]
    else:
        specs = [(s, PATS[i % 3]) for i, s in enumerate(sizes)]
    ids = rng.choice(64 * 64, len(specs), replace=False)
    blocks = [(P5[0] * 64 + int(k) // 64, P5[1] * 64 + int(k) % 64) for k in ids]
    rows, cols = _buckets(rng, specs, blocks)
    wr, wc = rng.integers(0, 1 << 18, 5000), rng.integers(0, 1 << 18, 5000)
    pr, pc = P5[0] * 8192 + rng.integers(0, 8192, 200_000), P5[1] * 8192 + rng.integers(0, 8192, 200_000)
    br, bc = np.concatenate([wr, pr]), np.concatenate([wc, pc])
    ok = _outside(br, bc, blocks)
    rows = np.concatenate([br[ok], rows]).astype(np.int64)
    cols = np.concatenate([bc[ok], cols]).astype(np.int64)
    ref = oracle.count_tiles(rows, cols, zmin, 18)
    if zmin <= 11:
        assert _bucket_counts(ref, 11, blocks) == [s for s, _ in specs]
    return rows, cols, rng.permutation(rows.size), ref


EDGE_CASES = [(T, layout, hot, 0) for T in (1024, 16384, 32768, 65536, 131072, TA)
              for layout in ("scattered", "contiguous") for hot in (0, 1)]
EDGE_CASES.insert(12, (32768, "scattered", 0, 14))   # (next to the other T = 32768 cases)


@pytest.mark.parametrize("T,layout,hot,zmin", EDGE_CASES)
def test_item_edges_two_levels(gpu, T, layout, hot, zmin):
    """Buckets of 512, 513 (HM_SP_MAX, the edge into the dense path), T-1, T,
    T+1, 2T-1, 2T, 2T+1 and 3T+7 keys at item size T.  Scattered: one
    permutation of all points (each parent work item holds a piece of every
    bucket: many runs per bucket, short ones for the smaller buckets).
    Contiguous: each bucket's points adjacent in the input, so its runs are
    whole parent work items but for the first and last, which start and end
    where the neighbouring bucket does (the sizes are odd: not a multiple of
    the 8 keys of a 16-B vector), and an item edge falls inside a long run.
    hot 0: every bucket goes through level 2's runs; hot 1: the defaults,
    under which the buckets of >= 65536 keys are hot tiles.  zmin 14 ends the
    output inside the final pyramid."""
    rows, cols, perm, ref = _edges(T, zmin)
    if layout == "scattered":
        rows, cols = rows[perm], cols[perm]
    got = _count(rows, cols, zmin, 18, T, HM_HOT=hot, HM_SPREAD_MIN_KEYS=NO_SPREAD)
    assert int(got.stage_us[7]) == 2
    if not hot:
        assert int(got.stage_us[6]) == 0
    _same(got, ref)


# ---------------------------------------------------------------------------
# 2. level 1 as the last level (Z = 12): items over a sharded digit's regions
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _one_level():
    """Z = 12: the level-1 digits (zoom-5 tiles) are the final buckets.  One
    digit of 600,001 points and one of 262144 = 16 x 16384 = 1 x 262144 (an
    exact multiple of both item sizes), both above HM_L1_SHARD_TILES * HM_T1 =
    131072 and so written as 8 regions (runs), plus small digits."""
    rng = np.random.default_rng(12)
    specs = [(600_001, "spread"), (TA, "spread"), (1, "same"), (513, "spread"), (5000, "corner"), (TA_MIN, "same")]
    ids = rng.choice(32 * 32, len(specs), replace=False)
    blocks = [(int(k) // 32, int(k) % 32) for k in ids]
    rows, cols = _buckets(rng, specs, blocks)
    perm = rng.permutation(rows.size)
    rows, cols = rows[perm], cols[perm]
    ref = oracle.count_tiles(rows, cols, 0, 12)
    assert _bucket_counts(ref, 5, blocks) == [s for s, _ in specs]
    return rows, cols, ref


@pytest.mark.parametrize("T", [TA_MIN, TA])
def test_item_edges_one_level(gpu, T):
    """hm_stream_runs' path for at most HM_L1_SHARDS long runs: at T = 262144
    an item spans several of a digit's 8 regions (75,000 and 32768 keys
    each), at 16384 most items lie inside one and the others cross from one
    region into the next."""
    rows, cols, ref = _one_level()
    got = _count(rows, cols, 0, 12, T)
    assert int(got.stage_us[7]) == 1
    _same(got, ref)


# ---------------------------------------------------------------------------
# 3. multi-item buckets with lg < 7 (zmax <= 6: one bucket of side 2^zmax)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _low_zoom(Z, n):
    rng = np.random.default_rng(100 + Z)
    rows = rng.integers(0, 1 << Z, n).astype(np.int64)
    cols = rng.integers(0, 1 << Z, n).astype(np.int64)
    return rows, cols


@pytest.mark.parametrize("Z,n,T", [(0, 40_000, None), (3, 70_001, None), (6, 100_000, None), (6, 100_000, 1024)])
@pytest.mark.parametrize("top_only", [False, True])
def test_low_zoom_multi_item_bucket(gpu, Z, n, T, top_only):
    """One bucket of 3 to 7 items (98 at T = 1024) with a 2^Z x 2^Z histogram:
    k_aggregate's squeeze-then-add arm and k_aggregate_merged's
    hm_bucket_pyramid arm.  zmin 0, and zmin = Z (the top level alone)."""
    rows, cols = _low_zoom(Z, n)
    zmin = Z if top_only else 0
    got = _count(rows, cols, zmin, Z, T)
    assert int(got.stage_us[8]) == (T or TA_MIN)
    assert n > int(got.stage_us[8]), "one item"
    assert int(got.stage_us[7]) == 1
    _same(got, oracle.count_tiles(rows, cols, zmin, Z))


# ---------------------------------------------------------------------------
# 4. three-level plan (Z = 21), and lat/lon input
# ---------------------------------------------------------------------------

P11 = (1234, 777)   # the zoom-11 tile (8 x 8 zoom-14 buckets) that holds the Z = 21 buckets


@functools.lru_cache(maxsize=1)
def _three_levels(T):
    rng = np.random.default_rng(21 + T)
    specs = [(T - 1, "spread"), (T, "same"), (T + 1, "corner"), (2 * T + 1, "spread")]
    ids = rng.choice(64, len(specs), replace=False)
    blocks = [(P11[0] * 8 + int(k) // 8, P11[1] * 8 + int(k) % 8) for k in ids]
    rows, cols = _buckets(rng, specs, blocks)
    wr, wc = rng.integers(0, 1 << 21, 20_000), rng.integers(0, 1 << 21, 20_000)
    pr, pc = P11[0] * 1024 + rng.integers(0, 1024, 30_000), P11[1] * 1024 + rng.integers(0, 1024, 30_000)
    br, bc = np.concatenate([wr, pr]), np.concatenate([wc, pc])
    ok = _outside(br, bc, blocks)
    rows = np.concatenate([br[ok], rows]).astype(np.int64)
    cols = np.concatenate([bc[ok], cols]).astype(np.int64)
    perm = rng.permutation(rows.size)
    rows, cols = rows[perm], cols[perm]
    ref = oracle.count_tiles(rows, cols, 0, 21)
    assert _bucket_counts(ref, 14, blocks) == [s for s, _ in specs]
    return rows, cols, ref


@pytest.mark.parametrize("T,contig,hot", [(TA_MIN, 1, 0), (TA_MIN, 0, 0), (131072, 1, 0), (131072, 0, 0),
                                          (131072, 1, 1)])
def test_item_edges_three_levels(gpu, T, contig, hot):
    """Z = 21 (z5 -> z11 -> z14): zoom-14 buckets of T-1, T, T+1 and 2T+1
    keys in one zoom-11 tile, read at the last level from one run per bucket
    (HM_CONTIG 1, the child-contiguous middle level) or from the middle
    level's runs (0); hot 1: the defaults, under which the zoom-11 tile is a
    mid-level hot tile."""
    rows, cols, ref = _three_levels(T)
    got = _count(rows, cols, 0, 21, T, HM_CONTIG=contig, HM_HOT=hot, HM_SPREAD_MIN_KEYS=NO_SPREAD)
    assert int(got.stage_us[7]) == 3
    if not hot:
        assert int(got.stage_us[6]) == 0
    _same(got, ref)


def test_item_edges_latlon(gpu):
    """Z = 18 from lat/lon at item size 65536: the keys k_l1_fast (whole
    8192-point tiles) and k_redo (one point in 16 lies exactly on the west
    edge of its column: deferred and resolved exactly) write.  Kept points
    are tile centres of buckets of T-1, T, T+1 and 2T+1 points plus a
    background; the mask drops 100,000 more points, some of them inside the
    buckets."""
    T = 65536
    rng = np.random.default_rng(4)
    specs = [(T - 1, "spread"), (T, "corner"), (T + 1, "spread"), (2 * T + 1, "spread")]
    ids = rng.choice(64 * 64, len(specs), replace=False)
    blocks = [(P5[0] * 64 + int(k) // 64, P5[1] * 64 + int(k) % 64) for k in ids]
    rows, cols = _buckets(rng, specs, blocks)
    br, bc = rng.integers(0, 1 << 18, 100_000), rng.integers(0, 1 << 18, 100_000)
    ok = _outside(br, bc, blocks)
    dr = np.concatenate([rng.integers(0, 1 << 18, 50_000), rows[:50_000]])
    dc = np.concatenate([rng.integers(0, 1 << 18, 50_000), cols[:50_000]])
    keep = np.concatenate([np.ones(rows.size + int(ok.sum()), np.uint8), np.zeros(dr.size, np.uint8)])
    rows = np.concatenate([rows, br[ok], dr])
    cols = np.concatenate([cols, bc[ok], dc])
    lat, lon = _centre(rows, cols, 18)
    edge = np.arange(rows.size) % 16 == 3
    lon[edge] = cols[edge] / float(1 << 18) * 360.0 - 180.0
    perm = rng.permutation(rows.size)
    lat, lon, keep = lat[perm], lon[perm], keep[perm]
    ref = oracle.count(lat, lon, keep, 0, 18)
    assert _bucket_counts(ref, 11, blocks) == [s for s, _ in specs]
    got = _count(lat, lon, 0, 18, T, keep=keep, tiles=False, HM_HOT=0, HM_SPREAD_MIN_KEYS=NO_SPREAD)
    assert int(got.stage_us[7]) == 2
    assert got.slow_points >= int(edge.sum()) // 2
    _same(got, ref)


# ---------------------------------------------------------------------------
# 5. hot tiles as multi-item buckets
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _hot(T):
    rng = np.random.default_rng(5 + T)
    specs = [(2 * T + 1, "spread"), (T, "corner")]
    blocks = [(700, 1300), (1801, 95)]
    rows, cols = _buckets(rng, specs, blocks)
    br, bc = rng.integers(0, 1 << 18, 500_000), rng.integers(0, 1 << 18, 500_000)
    ok = _outside(br, bc, blocks)
    rows = np.concatenate([rows, br[ok]]).astype(np.int64)
    cols = np.concatenate([cols, bc[ok]]).astype(np.int64)
    perm = rng.permutation(rows.size)
    rows, cols = rows[perm], cols[perm]
    ref = oracle.count_tiles(rows, cols, 0, 18)
    assert _bucket_counts(ref, 11, blocks) == [s for s, _ in specs]
    return rows, cols, ref


@pytest.mark.parametrize("T,spread_cold", [(TA_MIN, False), (TA_MIN, True), (65536, False), (65536, True)])
def test_hot_tiles_multi_item(gpu, T, spread_cold):
    """Two hot zoom-11 tiles (HM_HOT_MIN_KEYS = 0) over 500,000 uniform
    points: 2T+1 keys (three items, the last of one key) and T keys (one full
    item), read from the level-1 regions level 1 gave them.  spread_cold: the
    three-level hot arrangement of test_gpu_hot.test_hot_with_spread_plan."""
    rows, cols, ref = _hot(T)
    knobs = {"HM_HOT_MIN_KEYS": 0}
    if spread_cold:
        knobs["HM_SPREAD_MIN_COLD"] = 0
    got = _count(rows, cols, 0, 18, T, **knobs)
    assert int(got.stage_us[6]) == 2
    assert int(got.stage_us[7]) == (3 if spread_cold else 2)
    _same(got, ref)


# ---------------------------------------------------------------------------
# 6. items that span more than one 256-run staging chunk
# ---------------------------------------------------------------------------

NPARENT_ITEMS = 306
BUCKET_A = (P5[0] * 64 + 9, P5[1] * 64 + 50)    # 16 keys per parent work item
BUCKET_B = (P5[0] * 64 + 41, P5[1] * 64 + 3)    # 82 keys per parent work item


@functools.lru_cache(maxsize=1)
def _many_runs():
    rng = np.random.default_rng(6)
    n = NPARENT_ITEMS * TN
    rows = P5[0] * 8192 + rng.integers(0, 8192, n)
    cols = P5[1] * 8192 + rng.integers(0, 8192, n)
    i = np.arange(n)
    for (br, bc), sel in ((BUCKET_A, i % 512 == 0), (BUCKET_B, i % 100 == 50)):
        m = int(sel.sum())
        rows[sel] = br * 128 + rng.integers(0, 128, m)
        cols[sel] = bc * 128 + rng.integers(0, 128, m)
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    ref = oracle.count_tiles(rows, cols, 0, 18)
    na, nb = _bucket_counts(ref, 11, [BUCKET_A, BUCKET_B])
    assert 512 < na <= 32768 and 512 < nb <= 32768, "one dense item each at item size 32768"
    return rows, cols, ref


@pytest.mark.parametrize("shard_bits", [0, -1])
def test_item_of_many_runs(gpu, shard_bits):
    """More runs in one item than hm_stream_runs stages at a time (256 in
    k_aggregate).  All 306 x 8192 points lie in one zoom-5 parent.  Level 1
    writes each 8192-point input tile as one contiguous piece of one of the
    digit's regions, every region a multiple of 8192 keys, so the parent's
    306 work items of HM_TN = 8192 keys are those input tiles, and level 2
    writes one run per (work item, bucket present in it).  Bucket A holds
    every 512th input point, 16 per input tile (plus the ~2 of the uniform
    rest that fall into it): 306 runs, all shorter than HM_LONG_RUN = 32, so
    every key goes through the pieces path.  Bucket B holds every 100th, 81
    or 82 per tile: 306 runs of >= 32 keys, the bodies path with heads and
    tails.  Each is one dense item at item size 32768 (about 5,500 and 25,600
    keys), and k_items gives a single-item bucket r0 = rbase (the last run
    starting at or before a = keybase is the first) and r1 = rbase + nruns
    (every run starts before b = keybase + nkeys): r1 - r0 = 306 > 256.  The
    count comes from this reading of the code, not from a measurement.
    HM_HOT = 0 so that HM_RUN_SHARD_BITS alone decides the shard count: 0
    (one counter per child) and the default."""
    rows, cols, ref = _many_runs()
    got = _count(rows, cols, 0, 18, 32768, HM_HOT=0, HM_RUN_SHARD_BITS=shard_bits, HM_SPREAD_MIN_KEYS=NO_SPREAD)
    assert int(got.stage_us[6]) == 0
    assert int(got.stage_us[7]) == 2
    _same(got, ref)


# ---------------------------------------------------------------------------
# 7. every run-shard count
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _hotspot_tiles():
    lat, lon = synth.generate("hotspots", 1_000_000, seed=7)
    rows, cols, st, _ = oracle.project(lat, lon, 18)
    assert not st.any()
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    return rows, cols, oracle.count_tiles(rows, cols, 0, 18)


@functools.lru_cache(maxsize=1)
def _uniform_tiles():
    rng = np.random.default_rng(77)
    rows = rng.integers(0, 1 << 18, 1_500_000).astype(np.int64)
    cols = rng.integers(0, 1 << 18, 1_500_000).astype(np.int64)
    return rows, cols, oracle.count_tiles(rows, cols, 0, 18)


@pytest.mark.parametrize("shard_bits", [0, 1, 2, 3, 4, 5])
def test_run_shards(gpu, shard_bits):
    """1, 2, 4, 8, 16 and 32 run counters per level-2 child on a hotspot
    cloud (the largest cities' zoom-5 parents hold 17 work items and more, so
    a shard of 32 gets more than one run), hot tiles off."""
    rows, cols, ref = _hotspot_tiles()
    got = _count(rows, cols, 0, 18, HM_HOT=0, HM_RUN_SHARD_BITS=shard_bits)
    assert int(got.stage_us[6]) == 0
    assert int(got.stage_us[7]) == 2
    assert int(got.stage_us[8]) == TA_MIN
    _same(got, ref)


@pytest.mark.parametrize("shard_bits", [4, 5])
def test_run_shards_with_hot_tiles(gpu, shard_bits):
    """Sharded counters next to hot tiles (the default with them is 0)."""
    rows, cols, ref = _hotspot_tiles()
    got = _count(rows, cols, 0, 18, HM_HOT_MIN_KEYS=0, HM_RUN_SHARD_BITS=shard_bits)
    assert int(got.stage_us[6]) > 0, "no hot tiles"
    _same(got, ref)


@pytest.mark.parametrize("shard_bits", [2, 4])
def test_run_shards_spread_plan(gpu, shard_bits):
    """Sharded counters under the spread plan (the default with it is 0)."""
    rows, cols, ref = _uniform_tiles()
    got = _count(rows, cols, 0, 18, HM_SPREAD_MIN_KEYS=1, HM_RUN_SHARD_BITS=shard_bits)
    assert int(got.stage_us[7]) == 3
    _same(got, ref)


def test_run_shards_range(gpu):
    with pytest.raises(ValueError):
        with device.tuned(HM_RUN_SHARD_BITS=6):
            pass
    ctx = device.context(0)
    assert ctx.tune("HM_RUN_SHARD_BITS", -1) == -1   # still the default


# ---------------------------------------------------------------------------
# 8. the default selection, and the knobs' validation
# ---------------------------------------------------------------------------

def _default_item(n):
    ta = TA
    while ta > TA_MIN and n < ta * TA_ITEMS:
        ta >>= 1
    return ta


@functools.lru_cache(maxsize=1)
def _uniform_z14():
    rng = np.random.default_rng(8)
    n = TA_MIN * 2 * TA_ITEMS
    return rng.integers(0, 1 << 14, n).astype(np.int64), rng.integers(0, 1 << 14, n).astype(np.int64)


@pytest.mark.parametrize("n,item", [(4_194_303, 16384), (4_194_304, 32768)])
def test_default_item_size(gpu, n, item):
    """No knob set: the item is 16384 keys below 32768 x 128 points, 32768
    from there (zooms 10-14: the oracle's time)."""
    assert _default_item(n) == item
    rows, cols = _uniform_z14()
    rows, cols = rows[:n], cols[:n]
    got = device.count(rows, cols, None, 10, 14, tiles=True)
    assert int(got.stage_us[8]) == item
    _same(got, oracle.count_tiles(rows, cols, 10, 14))


def test_item_size_formula():
    """The selection restated; the larger steps are asserted from slot 8 where
    a test already runs the size: 2^22 and 48M points in tests/test_gpu_hot.py,
    48M in test_gpu_plan.py, 6e8 and 1e9 in test_gpu_fullsize.py."""
    assert [_default_item(n) for n in (0, 1 << 22, 10_000_000, 1 << 24, 1 << 25, 48_000_000, 10 ** 9)] == \
        [16384, 32768, 65536, 131072, 262144, 262144, 262144]


def test_item_knobs_validation(gpu):
    ctx = device.context(0)
    for bad in (3000, 24576, 512, 2 * TA, 0, -1024):
        with pytest.raises(ValueError):
            ctx.tune("HM_TA_MIN", bad)
    for bad in (0, -1, 0.5):
        with pytest.raises(ValueError):
            ctx.tune("HM_TA_ITEMS", bad)
    # a rejected value changes nothing; an accepted one returns the previous
    assert ctx.tune("HM_TA_MIN", 1024) == TA_MIN
    assert ctx.tune("HM_TA_MIN", TA) == 1024
    assert ctx.tune("HM_TA_MIN", TA_MIN) == TA
    assert ctx.tune("HM_TA_ITEMS", 1) == TA_ITEMS
    assert ctx.tune("HM_TA_ITEMS", TA_ITEMS) == 1
    with device.tuned(HM_TA_MIN=65536, HM_TA_ITEMS=2 ** 30):
        pass
    assert ctx.tune("HM_TA_MIN", TA_MIN) == TA_MIN
    assert ctx.tune("HM_TA_ITEMS", TA_ITEMS) == TA_ITEMS


def test_slot8_is_optional(gpu):
    """hm_last_stats writes slot 8 only for a caller that asks for more than 8
    slots, and nothing past it.  (Slot 8 after a call that took the general
    path: tests/test_gpu_general.py test_sparse_fallback_vs_oracle.)"""
    import ctypes

    rng = np.random.default_rng(9)
    rows = rng.integers(0, 1 << 12, 3000).astype(np.int64)
    got = device.count(rows, rows[::-1].copy(), None, 0, 12, tiles=True)
    assert int(got.stage_us[7]) == 1 and int(got.stage_us[8]) == TA_MIN
    ctx = device.context(0)
    us = (ctypes.c_double * 10)(*([-7.0] * 10))
    ctx.L.hm_last_stats(ctx.ptr, None, us, 8)
    assert us[8] == -7.0 and us[9] == -7.0 and us[7] == 1.0
    ctx.L.hm_last_stats(ctx.ptr, None, us, 10)
    assert us[8] == TA_MIN and us[9] == -7.0
