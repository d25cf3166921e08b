"""GPU: the general count path (csrc/hm_general.hip, gen_count in hm_api.cpp)
at run, tile, digit and key-width edges, against plain numpy.

test_gpu_general.py and test_gpu_grouped_tiles.py feed the path hotspot clouds
with random groups; where a key falls relative to a lane, a 64-item fragment, a
256-item round or a tile is then left to chance.  Here every input is a list of
explicit zoom-zmax tiles (int64 row, col), a uint32 group and no keep mask, so
the test controls each 128-bit key,
    sr + 16 (5) | sc + 2^47 (48) | group (32) | morton(ro, co) (2Z)
(hm_genkey.h; restated below with Python ints in _keys), its place in the
sorted list, and the bytes in which the keys differ (the radix passes
gen_count runs).  The unmarked tests check those properties of the inputs on
the CPU; the gpu tests compare every field of the sorted records with
np.unique counts of (group, row >> k, col >> k) per zoom -- int64 arithmetic
shifts, the reference's tile shift -- and, where a case has at most 8 groups,
each group with oracle.count_tiles.  Every comparison is exact.

The sizes rest on these tile sizes; a change of one of them means the sizes
here are to be revisited:
    HM_CS_TILE   4096  k_cascade items per tile        (hm_general.hip)
    HM_CS2_TILE  4096  k_cascade2 items per tile       (hm_general.hip)
    HmOs<uint64_t>::TILE 8192, HmOs<hm_u128>::TILE 4096  k_rx_onesweep keys per
                       tile, narrow and wide keys      (hm_general.hip)
A fragment is a wave's 64 consecutive items, a round the block's 256; the
cascade look-back reads 64 predecessor tiles at a time (hm_cs_lookback).

Record widths: 5 = hm_count_grouped_tiles (staged int64 records, single zoom
steps), 2 = hm_count_grouped_packed_tiles (packed records, fused two-zoom
steps), 4 = hm_count_tiles with every tile outside the square (staged), or in
split mode when the call takes the sparse fallback (hm_last_stats slot 7 is 0
then and only then)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import _lib, device

GPU = pytest.mark.gpu

CS_TILE = 4096            # HM_CS_TILE and HM_CS2_TILE
OS_TILE_NARROW = 8192     # HmOs<uint64_t>::TILE
OS_TILE_WIDE = 4096       # HmOs<hm_u128>::TILE
LOOKBACK = 64             # predecessor tiles per look-back round trip
MANY_TILES = (LOOKBACK + 1) * CS_TILE + 1
FIELDS = ("group", "zoom", "row", "col", "count")


# --------------------------------------------------------------------------
# the key of hm_genkey.h, with Python ints (object arrays)
# --------------------------------------------------------------------------

def _spread(x):
    """bit i of x (21 bits) to bit 2i"""
    x = x & 0x1FFFFF
    x = (x | (x << 16)) & 0x0000FFFF0000FFFF
    x = (x | (x << 8)) & 0x00FF00FF00FF00FF
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0F
    x = (x | (x << 2)) & 0x3333333333333333
    return (x | (x << 1)) & 0x5555555555555555


def _keys(rows, cols, g, Z):
    """The 128-bit keys as an object array of Python ints."""
    r = np.asarray(rows, np.int64).astype(object)
    c = np.asarray(cols, np.int64).astype(object)
    gg = np.asarray(g, np.uint32).astype(object)
    sr, sc = r >> Z, c >> Z
    assert all(-16 <= x < 16 for x in sr) and all(-(1 << 47) <= x < (1 << 47) for x in sc)
    mask = (1 << Z) - 1
    m = (_spread(r & mask) << 1) | _spread(c & mask)
    root = ((sr + 16) << 80) | ((sc + (1 << 47)) << 32) | gg
    return (root << (2 * Z)) | m


def _or_and(keys):
    o, a = 0, (1 << 128) - 1
    for k in keys:
        o |= k
        a &= k
    return o, a


def _varying_bytes(keys):
    """The radix passes of gen_count: bytes where the OR and AND of all keys
    differ."""
    o, a = _or_and(keys)
    return [b for b in range(16) if ((o ^ a) >> (8 * b)) & 0xFF]


def _is_wide(keys):
    o, a = _or_and(keys)
    return (o >> 64) != (a >> 64)


def _compact(m):
    """even bits of m (uint64 array) packed: the inverse of _spread"""
    m = m.astype(np.uint64) & np.uint64(0x5555555555555555)
    for s, k in ((1, 0x3333333333333333), (2, 0x0F0F0F0F0F0F0F0F), (4, 0x00FF00FF00FF00FF),
                 (8, 0x0000FFFF0000FFFF), (16, 0x00000000FFFFFFFF)):
        m = (m | (m >> np.uint64(s))) & np.uint64(k)
    return m.astype(np.int64)


def _cells_of_codes(codes):
    """(rows, cols) of Morton codes: row bits on the odd positions"""
    codes = np.asarray(codes, np.uint64)
    return _compact(codes >> np.uint64(1)), _compact(codes)


# --------------------------------------------------------------------------
# reference, calls, comparison
# --------------------------------------------------------------------------

def _reference(rows, cols, g, zmin, zmax):
    exp = {k: [] for k in FIELDS}
    gg = np.asarray(g, np.uint32).astype(np.int64)
    for z in range(zmin, zmax + 1):
        rec = np.stack([gg, rows >> (zmax - z), cols >> (zmax - z)], axis=1)
        u, cnt = np.unique(rec, axis=0, return_counts=True)
        exp["group"].append(u[:, 0].astype(np.uint32))
        exp["zoom"].append(np.full(len(u), z, np.int32))
        exp["row"].append(u[:, 1])
        exp["col"].append(u[:, 2])
        exp["count"].append(cnt.astype(np.int64))
    exp = {k: np.concatenate(v) for k, v in exp.items()}
    o = np.lexsort((exp["col"], exp["row"], exp["zoom"], exp["group"]))
    return _frozen({k: v[o] for k, v in exp.items()})


@functools.lru_cache(maxsize=None)
def _ref(case, args, zmin, zmax):
    """the reference of a cached case, computed once and shared"""
    rows, cols, g = case(*args)
    return _reference(rows, cols, g, zmin, zmax)


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def _from_zoom(exp, zmin):
    m = exp["zoom"] >= zmin
    return {k: v[m] for k, v in exp.items()}


def _decode_packed(keys, gc):
    return _decode_packed_host(keys.cpu().numpy(), gc.cpu().numpy())


def _decode_packed_host(keys, gc):
    k = np.ascontiguousarray(keys).view(np.uint64)
    gcn = np.ascontiguousarray(gc).view(np.uint64)
    z, r, c = device.decode_keys(k)
    return device.GroupedCounts((gcn >> np.uint64(32)).astype(np.uint32), z, r, c,
                                (gcn & np.uint64(0xFFFFFFFF)).astype(np.int64))


def _run(width, rows, cols, g, zmin, zmax, fallback=False):
    """The sorted records of one call; width 4 counts without groups."""
    if width == 5:
        got = device.count_grouped(rows, cols, g, None, zmin, zmax, tiles=True)
        assert device.context(0).last_error() == (-1, 0)
        return got.sorted()
    if width == 2:
        res = device.count_grouped_packed_device(rows, cols, g, None, zmin, zmax, tiles=True)
        assert res is not None
        got = _decode_packed(*res)
        assert np.all(np.diff(got.zoom) <= 0) and got.zoom[0] == zmax and got.zoom[-1] == zmin
        return got.sorted()
    assert width == 4
    got = device.count(rows, cols, None, zmin, zmax, tiles=True)
    assert (int(got.stage_us[7]) == 0) == fallback
    return device.GroupedCounts(np.zeros(got.count.size, np.uint32), got.zoom, got.row, got.col, got.count).sorted()


def _same(got, exp, fields=FIELDS):
    for k in fields:
        assert np.array_equal(getattr(got, k), exp[k]), k


def _pin_to_oracle(got, rows, cols, g, zmin, zmax):
    """each group id (at most 8) against oracle.count_tiles"""
    ids = np.unique(g)
    assert ids.size <= 8
    for gid in ids:
        ref = oracle.count_tiles(rows, cols, zmin, zmax, (g == gid).astype(np.uint8))
        o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
        m = got.group == gid
        for k in FIELDS[1:]:
            assert np.array_equal(getattr(got, k)[m], ref[k][o]), (gid, k)


def _pin_sum_to_oracle(got, rows, cols, zmin, zmax):
    """every group together: the ungrouped oracle count"""
    ref = oracle.count_tiles(rows, cols, zmin, zmax)
    o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
    rec = np.stack([got.zoom.astype(np.int64), got.row, got.col], axis=1)
    u, inv = np.unique(rec, axis=0, return_inverse=True)
    tot = np.zeros(len(u), np.int64)
    np.add.at(tot, inv.reshape(-1), got.count)
    assert np.array_equal(u[:, 0], ref["zoom"][o]) and np.array_equal(u[:, 1], ref["row"][o])
    assert np.array_equal(u[:, 2], ref["col"][o]) and np.array_equal(tot, ref["count"][o])


def _check(widths, rows, cols, g, zmin, zmax, exp):
    """Each width against the reference and, group by group, the oracle."""
    for w in widths:
        got = _run(w, rows, cols, g, zmin, zmax)
        if w == 4:   # no groups: every record in group 0
            _same(got, exp, FIELDS[1:])
            _pin_to_oracle(got, rows, cols, np.zeros(rows.size, np.uint32), zmin, zmax)
        else:
            _same(got, exp)
            _pin_to_oracle(got, rows, cols, g, zmin, zmax)


def _shuffled(seed, *arrays):
    o = np.random.default_rng(seed).permutation(arrays[0].size)
    return tuple(a[o] for a in arrays)


# --------------------------------------------------------------------------
# 1. no sort pass: every key the same
# --------------------------------------------------------------------------

NP0_SIZES = [2, CS_TILE + 1, OS_TILE_NARROW + 1, MANY_TILES]
NP0_Z = 14


@functools.lru_cache(maxsize=None)
def _np0_case(n, exotic):
    """n copies of one tile of one group, zooms 10..14 (in the square: five
    zooms are fused, fused, last for packed records)."""
    rows = np.full(n, -1 if exotic else 5461, np.int64)
    cols = np.full(n, 10922, np.int64)
    g = np.full(n, 9 if exotic else 0xDEADBEEF, np.uint32)
    return rows, cols, g


@pytest.mark.parametrize("exotic", [False, True])
def test_np0_inputs(exotic):
    for n in NP0_SIZES[:2]:
        rows, cols, g = _np0_case(n, exotic)
        exp = _ref(_np0_case, (n, exotic), NP0_Z - 4, NP0_Z)
        assert _varying_bytes(_keys(rows, cols, g, NP0_Z)) == []
        assert _varying_bytes(_keys(rows, cols, np.zeros(n, np.uint32), NP0_Z)) == []
        assert exp["count"].tolist() == [n] * 5 and exp["zoom"].tolist() == list(range(NP0_Z - 4, NP0_Z + 1))
        assert (exp["row"] < 0).all() == exotic
    assert (MANY_TILES + CS_TILE - 1) // CS_TILE == LOOKBACK + 2   # tile 65 looks back past 64 zero-head tiles


@GPU
@pytest.mark.parametrize("n", NP0_SIZES)
@pytest.mark.parametrize("exotic", [False, True])
def test_np0(gpu, n, exotic):
    """np == 0: buffer 0 goes straight into the cascade.  One record per zoom
    with count n; of the 66 cascade tiles of the largest size all but the first
    publish zero heads."""
    rows, cols, g = _np0_case(n, exotic)
    exp = _ref(_np0_case, (n, exotic), NP0_Z - 4, NP0_Z)
    _check((5, 4) if exotic else (5, 2), rows, cols, g, NP0_Z - 4, NP0_Z, exp)


# --------------------------------------------------------------------------
# 2. one pass on one chosen byte: two distinct keys
# --------------------------------------------------------------------------

# name: (Z, (row, col, group) a, (row, col, group) b, the byte, exotic)
ONE_BYTE = {
    "col_bit0": (14, (100, 200, 5), (100, 201, 5), 0, False),                      # key bit 0
    "morton_byte1": (14, (100, 200, 5), (100, 200 ^ 32, 5), 1, False),             # col bit 5: key bit 10
    "group_low_half": (14, (100, 200, 5), (100, 200, 5 | 1 << 10), 4, False),      # key bit 28 + 10
    "group_high_half": (21, (100, 200, 0), (100, 200, 1 << 22), 8, False),         # key bit 42 + 22 = 64
    "sc": (14, (100, 200 + (32 << 14), 5), (100, 200 + (48 << 14), 5), 8, True),   # sc bit 4: key bit 60 + 4
    "sr": (21, (100 + (2 << 21), 200, 5), (100 + (3 << 21), 200, 5), 15, True),    # sr bit 0: key bit 122
}
SPLITS = ["one_a", "one_b", "half"]


@functools.lru_cache(maxsize=None)
def _one_byte_case(name, split):
    Z, a, b, byte, exotic = ONE_BYTE[name]
    n = (OS_TILE_WIDE if byte >= 8 else OS_TILE_NARROW) + 1
    if split == "one_a":
        sel = np.ones(n, bool)
        sel[n // 3] = False
    elif split == "one_b":
        sel = np.zeros(n, bool)
        sel[2 * n // 3] = True
    else:
        sel = np.arange(n) % 2 == 1                # interleaved in input order
    rows = np.where(sel, b[0], a[0]).astype(np.int64)
    cols = np.where(sel, b[1], a[1]).astype(np.int64)
    g = np.where(sel, b[2], a[2]).astype(np.uint32)
    return rows, cols, g


@pytest.mark.parametrize("name", list(ONE_BYTE))
def test_one_byte_inputs(name):
    Z, a, b, byte, exotic = ONE_BYTE[name]
    for split in SPLITS:
        rows, cols, g = _one_byte_case(name, split)
        keys = _keys(rows, cols, g, Z)
        assert len(set(keys.tolist())) == 2
        assert _varying_bytes(keys) == [byte]
        assert _is_wide(keys) == (byte >= 8)
        assert rows.size == (OS_TILE_WIDE if byte >= 8 else OS_TILE_NARROW) + 1
        nb = int((keys == max(keys)).sum())
        assert nb == {"one_a": rows.size - 1, "one_b": 1, "half": rows.size // 2}[split]
        insq = (rows >= 0) & (rows < (1 << Z)) & (cols >= 0) & (cols < (1 << Z))
        assert insq.all() != exotic and insq.any() != exotic
        if exotic:   # width 4 sorts the same byte: the keys without the group
            assert _varying_bytes(_keys(rows, cols, np.zeros(rows.size, np.uint32), Z)) == [byte]
    if name == "group_high_half":   # equal low halves
        assert len(set((keys & ((1 << 64) - 1)).tolist())) == 1


@GPU
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", list(ONE_BYTE))
def test_one_byte(gpu, name, split):
    """A single radix pass on the byte named; for group_high_half, sc and sr a
    byte of the high half only (k >> sh with sh >= 64)."""
    Z, a, b, byte, exotic = ONE_BYTE[name]
    rows, cols, g = _one_byte_case(name, split)
    exp = _ref(_one_byte_case, (name, split), Z - 3, Z)
    _check((5, 4) if exotic else (5, 2), rows, cols, g, Z - 3, Z, exp)


# --------------------------------------------------------------------------
# 3. all 16 passes
# --------------------------------------------------------------------------

ALL16_SIZES = [OS_TILE_WIDE + 1, 3 * OS_TILE_WIDE + 1]
ALL16_Z = 21


ALL16_FLIP = [8 * b for b in range(15)] + [122]      # one key bit of every byte (byte 15: sr bit 0)


def _flip_key_bit(rows, cols, g, t, Z):
    """the tiles and groups whose keys are the given ones with bit t flipped"""
    rows, cols, g = rows.copy(), cols.copy(), g.copy()
    if t < 2 * Z:                                     # Morton: columns on the even bits
        (rows if t % 2 else cols)[:] ^= np.int64(1) << np.int64(t // 2)
    elif t < 2 * Z + 32:
        g ^= np.uint32(1 << (t - 2 * Z))
    elif t < 2 * Z + 80:                              # sc = col >> Z
        cols ^= np.int64(1) << np.int64(Z + t - 2 * Z - 32)
    else:                                             # sr = row >> Z
        rows ^= np.int64(1) << np.int64(Z + t - 2 * Z - 80)
    return rows, cols, g


@functools.lru_cache(maxsize=None)
def _all16_case(n):
    """Z = 21: rows with sr -16..15, columns over the whole int64 range (sc
    -2^42..2^42 - 1: both signs, every bit of the field varies), groups over
    the whole u32 range.  The last quarter repeats the first, and between
    them in input order come copies of the first with one key bit flipped,
    one sixteenth of it for each byte: a pass left out leaves such a copy
    between the two equal keys."""
    rng = np.random.default_rng(n)
    rows = rng.integers(-(16 << ALL16_Z), 16 << ALL16_Z, n)
    cols = rng.integers(-(1 << 63), (1 << 63) - 1, n, endpoint=True)
    cols[2::5] = rng.integers(-(1 << 30), 1 << 30, cols[2::5].size)
    g = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rows[:2] = [-(16 << ALL16_Z), (16 << ALL16_Z) - 1]
    cols[:2] = [-(1 << 63), (1 << 63) - 1]
    g[:2] = [0, 0xFFFFFFFF]
    q = n // 4
    per = q // 16
    for b, t in enumerate(ALL16_FLIP):
        src, dst = slice(b * per, (b + 1) * per), slice(q + b * per, q + (b + 1) * per)
        rows[dst], cols[dst], g[dst] = _flip_key_bit(rows[src], cols[src], g[src], t, ALL16_Z)
    rows[n - q:], cols[n - q:], g[n - q:] = rows[:q], cols[:q], g[:q]
    return rows, cols, g


@functools.lru_cache(maxsize=None)
def _all16_exotic_case(n):
    """the same tiles without the few inside the square, and no groups"""
    rows, cols, g = _all16_case(n)
    out = ~((rows >= 0) & (rows < (1 << ALL16_Z)) & (cols >= 0) & (cols < (1 << ALL16_Z)))
    rows, cols = rows[out], cols[out]
    return rows, cols, np.zeros(rows.size, np.uint32)


@pytest.mark.parametrize("n", ALL16_SIZES)
def test_all16_inputs(n):
    rows, cols, g = _all16_case(n)
    exp = _ref(_all16_case, (n,), 16, ALL16_Z)
    keys = _keys(rows, cols, g, ALL16_Z)
    assert _varying_bytes(keys) == list(range(16))
    assert (exp["count"] == 2).any() and rows.size == n
    q = n // 4
    per = q // 16
    assert per >= 64 and (keys[n - q:] == keys[:q]).all()
    for b, t in enumerate(ALL16_FLIP):   # equal but for one bit of byte b, and between the equal keys in input order
        assert t // 8 == b
        assert ((keys[q + b * per:q + (b + 1) * per] ^ keys[b * per:(b + 1) * per]) == 1 << t).all(), b
    rows, cols, g = _all16_exotic_case(n)
    assert n - 8 <= rows.size <= n
    # group bits 42..73: bytes 6, 7 and 8 hold nothing else
    assert _varying_bytes(_keys(rows, cols, g, ALL16_Z)) == [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 15]


@GPU
@pytest.mark.parametrize("n", ALL16_SIZES)
def test_all16(gpu, n):
    """HM_OS_MAXP = 16 passes (width 5); the same tiles without groups are 13
    passes with bytes 6..8 skipped between bytes of both halves (width 4)."""
    rows, cols, g = _all16_case(n)
    exp = _ref(_all16_case, (n,), 16, ALL16_Z)
    got = _run(5, rows, cols, g, 16, ALL16_Z)
    _same(got, exp)
    _pin_sum_to_oracle(got, rows, cols, 16, ALL16_Z)
    rows, cols, g = _all16_exotic_case(n)
    _check((4,), rows, cols, g, 16, ALL16_Z, _ref(_all16_exotic_case, (n,), 16, ALL16_Z))


# --------------------------------------------------------------------------
# 4. a run against the cascade's lanes, fragments, rounds and tiles
# --------------------------------------------------------------------------

PH_P = [0, 1, 63, 64, 255, 256, CS_TILE - 1, CS_TILE]
PH_H = [CS_TILE - 1, CS_TILE, CS_TILE + 1, 3 * CS_TILE]
PH_Q = [0, 1, CS_TILE + 1]
PH_GROUPS = {1: (14, (3,)), 3: (21, (5, 1 << 22, 0xFFFFFFF0))}   # groups: (Z, ids); three ids at Z = 21: wide keys
PH_BASE = 5 << 16                                                 # first Morton code: whole families above it


def _phase_grid():
    """every (p, h) with one q, rotating, and every p once more with another
    h and q: 40 of the 96 combinations"""
    out = []
    for ip, p in enumerate(PH_P):
        for ih, h in enumerate(PH_H):
            out.append((p, h, PH_Q[(ip + ih) % 3]))
    for ip, p in enumerate(PH_P):
        ih = (ip + 1) % 4
        out.append((p, PH_H[ih], PH_Q[(ip + ih + 1) % 3]))
    assert len(set(out)) == 40
    return out


@functools.lru_cache(maxsize=None)
def _phase_case(p, h, q, groups):
    """Per group, in sorted order: p distinct cells, one cell h times, q
    distinct cells (consecutive Morton codes); input order shuffled."""
    Z, ids = PH_GROUPS[groups]
    codes = np.concatenate([PH_BASE + np.arange(p), np.full(h, PH_BASE + p), PH_BASE + p + 1 + np.arange(q)])
    r1, c1 = _cells_of_codes(codes)
    rows, cols = np.tile(r1, len(ids)), np.tile(c1, len(ids))
    g = np.repeat(np.array(ids, np.uint32), codes.size)
    return _shuffled(p + h + q, rows, cols, g)


@pytest.mark.parametrize("groups", [1, 3])
def test_phase_inputs(groups):
    Z, ids = PH_GROUPS[groups]
    grid = _phase_grid()
    assert {x[0] for x in grid} == set(PH_P) and {x[1] for x in grid} == set(PH_H) and {x[2] for x in grid} == set(PH_Q)
    for p, h, q in grid:
        rows, cols, g = _phase_case(p, h, q, groups)
        cells, cnt = np.unique(np.stack([g.astype(np.int64), rows, cols], axis=1), axis=0, return_counts=True)
        keys = _keys(cells[:, 1], cells[:, 2], cells[:, 0].astype(np.uint32), Z)
        o = np.argsort(keys, kind="stable")
        assert cnt[o].tolist() == ([1] * p + [h] + [1] * q) * groups, (p, h, q)
        assert cells[o, 0].tolist() == sorted(cells[:, 0].tolist())
        assert _is_wide(keys) == (groups == 3)


@GPU
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("p,h,q", _phase_grid())
def test_run_phases(gpu, p, h, q, groups):
    """The run's head at item p and its tail at item p + h - 1 of the sorted
    keys: on and either side of lane, fragment, round and tile boundaries, runs
    of a whole tile and more (tiles that publish no head), through single
    (width 5) and fused (width 2) steps."""
    Z, ids = PH_GROUPS[groups]
    rows, cols, g = _phase_case(p, h, q, groups)
    exp = _ref(_phase_case, (p, h, q, groups), Z - 3, Z)
    _check((5, 2), rows, cols, g, Z - 3, Z, exp)


# --------------------------------------------------------------------------
# 5. fused-step alignment: four-child families at every offset
# --------------------------------------------------------------------------

FU_S = [0, 1, 2, 3, 61, 62, 63]
FU_BLOCK = 1 << 19        # first Morton code of the block: rows [512, 576) x cols [0, 128)
FU_CELLS = 8192
FU_K = [1, 2, 3, 4, 5, 6]
FU_GRID = [("full", s, w) for s in FU_S for w in (False, True)] + [("holes", s, w) for s in (1, 2) for w in (False, True)]


def _fused_cells(kind, s, wide):
    """The distinct cells in key order, (codes, groups): s lone cells (codes
    j << 12: their ancestors stay distinct, and before the block's, for six
    levels), the block of 8192 consecutive codes -- whole four-child families
    six levels up -- and, for wide keys, one cell of a last group.  holes:
    every second family loses one child, every third two (every sixth, both:
    one child is left)."""
    i = np.arange(FU_CELLS)
    f, child = i >> 2, i & 3
    keep = np.ones(FU_CELLS, bool)
    if kind == "holes":
        keep &= ~((f % 2 == 1) & (child == f % 4))
        keep &= ~((f % 3 == 2) & ((child == (f + 1) % 4) | (child == (f + 2) % 4)))
    block = FU_BLOCK + i[keep]
    codes = np.concatenate([np.arange(s) << 12, block] + ([[0]] if wide else []))
    if wide:   # groups at and above 1 << 22: the high halves differ at zoom 21
        g = np.concatenate([np.full(s, 1 << 22), np.full(block.size, 1 << 23), [0xFFFFFFFF]])
    else:
        g = np.full(codes.size, 3)
    return codes.astype(np.uint64), g.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _fused_case(kind, s, wide):
    """Cell i of the key order holds 1 + (i mod 5) points, so the ENDs are not
    the indices; input order shuffled.  The reference holds six
    zooms."""
    Z = 21 if wide else 14
    codes, g = _fused_cells(kind, s, wide)
    mult = 1 + np.arange(codes.size) % 5
    r1, c1 = _cells_of_codes(codes)
    return _shuffled(s + 11, np.repeat(r1, mult), np.repeat(c1, mult), np.repeat(g, mult))


def _runs(keys, shift):
    """(start, length) of the runs of equal keys >> shift in a sorted list"""
    fam = np.array([k >> shift for k in keys], dtype=object)
    head = np.concatenate([[True], fam[1:] != fam[:-1]])
    start = np.flatnonzero(head)
    return start, np.diff(np.append(start, len(keys)))


def _straddled(start, length, at):
    """the run that holds items at - 1 and at: (its length, items before at), or None"""
    j = np.searchsorted(start, at, side="right") - 1
    if start[j] < at < start[j] + length[j]:
        return int(length[j]), int(at - start[j])
    return None


@pytest.mark.parametrize("kind,s,wide", FU_GRID)
def test_fused_inputs(kind, s, wide):
    """What k_cascade2 sees at its fused levels (input levels Z and Z - 2; the
    level below each is folded by the last cell of a run of at most 4)."""
    Z = 21 if wide else 14
    codes, g = _fused_cells(kind, s, wide)
    r1, c1 = _cells_of_codes(codes)
    keys0 = _keys(r1, c1, g, Z)
    assert keys0.tolist() == sorted(set(keys0.tolist()))     # in key order, distinct
    assert _is_wide(keys0) == wide
    exp = _ref(_fused_case, (kind, s, wide), Z, Z)
    assert np.array_equal(exp["count"][exp["zoom"] == Z], (1 + np.arange(codes.size) % 5)[np.lexsort((c1, r1, g))])
    for lvl in (0, 2):                                       # input level Z - lvl
        keys = sorted({k >> (2 * lvl) for k in keys0.tolist()})
        start, length = _runs(keys, 2)
        assert length.max() == 4
        lone = length[:s]
        assert (lone == 1).all()                             # the lone cells stay lone
        blk = slice(s, len(start) - (1 if wide else 0))
        if kind == "full" or lvl == 2:
            assert (length[blk] == 4).all() and (start[blk] % 4 == s % 4).all()
            for at in [64 * j for j in range(1, len(keys) // 64 + 1)]:
                if at <= s or at >= s + (FU_CELLS >> (2 * lvl)):
                    continue
                hit = _straddled(start, length, at)
                assert hit == (None if s % 4 == 0 else (4, 4 - s % 4)), (lvl, at)
            if lvl == 0:
                assert len(keys) > CS_TILE
        else:
            # runs of 1, 2, 3 and 4 cells; 2-, 3- and 4-cell runs at every
            # offset mod 4, and split every way by fragment and round edges
            for ln in (2, 3, 4):
                assert set((start[length == ln] % 4).tolist()) == {0, 1, 2, 3}, ln
            assert set(length.tolist()) == {1, 2, 3, 4}
            for edge in (64, 256):
                hits = {_straddled(start, length, at) for at in range(edge, len(keys), edge)}
                want = {(ln, b) for ln in (2, 3, 4) for b in range(1, ln)}
                assert want <= hits, (edge, want - hits)
            assert _straddled(start, length, CS_TILE) is not None
            # heads 1, 2 and 3 items before a fragment: the run's END lies 2, 3
            # and 4 items back in the previous fragment
            back = {(64 - int(st) % 64) for st, ln in zip(start, length) if st % 64 > 60 and st % 64 + ln > 64}
            assert back == {1, 2, 3}


@GPU
@pytest.mark.parametrize("K", FU_K)
@pytest.mark.parametrize("kind,s,wide", FU_GRID)
def test_fused_alignment(gpu, kind, s, wide, K):
    """K zooms: packed records run single, fused, fused, ..., single?, last
    (two = kz >= 1 && kz + 2 <= K); width 5 runs the same input through single
    steps."""
    Z = 21 if wide else 14
    rows, cols, g = _fused_case(kind, s, wide)
    exp = _ref(_fused_case, (kind, s, wide), Z - 5, Z)
    zmin = Z - K + 1
    _check((2, 5), rows, cols, g, zmin, Z, _from_zoom(exp, zmin))


TW_A = [56, 57, 58, 59, 60]
TW_GROUPS = (7, 7 | 1 << 22)      # equal low 22 bits: the same cell's two keys differ in the high half only
TW_Z = 21


def _twin_cells(a):
    """One four-child family in two groups whose keys differ above bit 64
    only, next to each other in key order: a lone cells and the family in the
    first group, the family and 64 more whole families in the second.  The
    second family's head is item a + 4 = 60..64: its run ends on lanes 63, 0,
    1, 2 and 3 of the next fragment, and the cells before it that a 64-bit
    comparison takes for its own lie 1..4 items back."""
    codes = np.concatenate([np.arange(a) << 12, FU_BLOCK + np.arange(4), FU_BLOCK + np.arange(4 + 256)])
    g = np.concatenate([np.full(a + 4, TW_GROUPS[0]), np.full(4 + 256, TW_GROUPS[1])])
    return codes.astype(np.uint64), g.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _twin_case(a):
    codes, g = _twin_cells(a)
    mult = 1 + np.arange(codes.size) % 5
    r1, c1 = _cells_of_codes(codes)
    return _shuffled(a, np.repeat(r1, mult), np.repeat(c1, mult), np.repeat(g, mult))


@pytest.mark.parametrize("a", TW_A)
def test_twin_inputs(a):
    codes, g = _twin_cells(a)
    keys = _keys(*_cells_of_codes(codes), g, TW_Z).tolist()
    assert keys == sorted(set(keys)) and _is_wide(keys)
    lo = (1 << 64) - 1
    for j in range(4):   # the same cells: equal low halves, other high halves
        assert keys[a + j] & lo == keys[a + 4 + j] & lo and keys[a + j] >> 64 != keys[a + 4 + j] >> 64
    start, length = _runs(keys, 2)
    assert (length[a:] == 4).all() and start[a + 1] == a + 4 and (length[:a] == 1).all()


@GPU
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("a", TW_A)
def test_twin_families(gpu, a, K):
    """Neighbouring runs that a comparison or a shuffle of the low half alone
    would join, at a fragment edge of a fused step."""
    rows, cols, g = _twin_case(a)
    zmin = TW_Z - K + 1
    _check((2, 5), rows, cols, g, zmin, TW_Z, _from_zoom(_ref(_twin_case, (a,), TW_Z - 3, TW_Z), zmin))


# --------------------------------------------------------------------------
# 6. the narrow sort tile
# --------------------------------------------------------------------------

NT_SIZES = [OS_TILE_NARROW - 1, OS_TILE_NARROW, OS_TILE_NARROW + 1, 2 * OS_TILE_NARROW + 1, MANY_TILES]
NT_Z = 14


@functools.lru_cache(maxsize=None)
def _narrow_case(n):
    """n distinct random tiles inside the square, one group"""
    rng = np.random.default_rng(n)
    codes = np.unique(rng.integers(0, 1 << (2 * NT_Z), n + n // 4 + 16))
    codes = rng.permutation(codes)[:n]
    rows, cols = codes >> NT_Z, codes & ((1 << NT_Z) - 1)
    g = np.full(n, 77, np.uint32)
    return rows, cols, g


@pytest.mark.parametrize("n", NT_SIZES[:-1])
def test_narrow_tile_inputs(n):
    rows, cols, g = _narrow_case(n)
    exp = _ref(_narrow_case, (n,), NT_Z - 2, NT_Z)
    keys = _keys(rows, cols, g, NT_Z)
    assert rows.size == n and len(set(keys.tolist())) == n and not _is_wide(keys)
    assert int((exp["zoom"] == NT_Z).sum()) == n and len(_varying_bytes(keys)) == 4


@GPU
@pytest.mark.parametrize("n", NT_SIZES)
def test_narrow_sort_tile(gpu, n):
    """Narrow keys either side of HmOs<uint64_t>::TILE = 8192, and 66 cascade
    tiles that all publish heads (the look-back adds 64 aggregates, then
    more)."""
    rows, cols, g = _narrow_case(n)
    exp = _ref(_narrow_case, (n,), NT_Z - 2, NT_Z)
    assert np.unique(rows * (1 << NT_Z) + cols).size == n
    _check((5, 2), rows, cols, g, NT_Z - 2, NT_Z, exp)


# --------------------------------------------------------------------------
# 7. capacity cuts, with a sentinel behind the capacity
# --------------------------------------------------------------------------

PATTERN = 0x5A5A5A5A5A5A5A5A
PAD = 4096
CAP_Z, CAP_ZMIN = 14, 11        # K = 4: packed records cut a fused step


@functools.lru_cache(maxsize=None)
def _capacity_case(width):
    n = 5000
    rng = np.random.default_rng(width)
    rows = 8000 + rng.integers(0, 64, n)
    cols = rng.integers(0, 128, n)
    if width == 4:
        rows = -1 - rng.integers(0, 64, n)
    g = (rng.integers(0, 3, n) * 1000).astype(np.uint32) if width != 4 else np.zeros(n, np.uint32)
    return rows, cols, g


def _raw_call(width, rows, cols, g, zmin, zmax, capacity):
    """The C call with outputs PAD entries longer than the capacity and filled
    with PATTERN: (status, n_out, [whole output arrays])."""
    import torch

    ctx = device.context(0)
    r = device._dev(rows, torch.int64, 0)
    c = device._dev(cols, torch.int64, 0)
    gg = device._dev(np.asarray(g, np.uint32).view(np.int32), torch.int32, 0)
    alloc = capacity + PAD
    nout = ctypes.c_int64(-1)
    if width == 5:
        outs = [torch.full((5 * alloc,), PATTERN, dtype=torch.int64, device=r.device)]
        rc = ctx.L.hm_count_grouped_tiles(ctx.ptr, device._ptr(r), device._ptr(c), None, device._ptr(gg), rows.size,
                                          zmin, zmax, device._ptr(outs[0]), capacity, ctypes.byref(nout))
    elif width == 2:
        outs = [torch.full((alloc,), PATTERN, dtype=torch.int64, device=r.device) for _ in range(2)]
        rc = ctx.L.hm_count_grouped_packed_tiles(ctx.ptr, device._ptr(r), device._ptr(c), None, device._ptr(gg),
                                                 rows.size, zmin, zmax, device._ptr(outs[0]), device._ptr(outs[1]),
                                                 capacity, ctypes.byref(nout))
    else:
        outs = [torch.full((4 * alloc,), PATTERN, dtype=torch.int64, device=r.device)]
        keys = torch.full((1024,), PATTERN, dtype=torch.int64, device=r.device)
        counts = torch.full((1024,), PATTERN, dtype=torch.int64, device=r.device)
        nk = ctypes.c_int64(-1)
        rc = ctx.L.hm_count_tiles(ctx.ptr, device._ptr(r), device._ptr(c), None, rows.size, zmin, zmax,
                                  device._ptr(keys), device._ptr(counts), 1024, ctypes.byref(nk),
                                  device._ptr(outs[0]), capacity, ctypes.byref(nout))
        assert nk.value == 0 and int(ctx.last_stats()[1][7]) != 0          # no cell in the square; not the fallback
        assert bool((keys == PATTERN).all()) and bool((counts == PATTERN).all())
    return rc, nout.value, [o.cpu().numpy().reshape(alloc, -1) for o in outs]


@GPU
@pytest.mark.parametrize("width", [5, 2, 4])
def test_capacity_cut(gpu, width):
    """HM_E_CAPACITY with *n_out the full total, the records below the capacity
    those of the full call slot for slot, and no word written behind it: one
    record short, one record into zoom zmax - 1's records, and capacity 1."""
    rows, cols, g = _capacity_case(width)
    rc, total, full = _raw_call(width, rows, cols, g, CAP_ZMIN, CAP_Z, rows.size * 4)
    assert rc == _lib.HM_OK and 0 < total <= rows.size * 4
    for a in full:
        assert (a[total:] == PATTERN).all()
    a = full[0]
    if width == 2:
        got = _decode_packed_host(full[0][:total, 0], full[1][:total, 0])
    elif width == 5:
        got = device.GroupedCounts(a[:total, 0].astype(np.uint32), a[:total, 1].astype(np.int32), a[:total, 2],
                                   a[:total, 3], a[:total, 4])
    else:
        got = device.GroupedCounts(np.zeros(total, np.uint32), a[:total, 0].astype(np.int32), a[:total, 1],
                                   a[:total, 2], a[:total, 3])
    _same(got.sorted(), _reference(rows, cols, g, CAP_ZMIN, CAP_Z))
    zoom = got.zoom
    top = int((zoom == CAP_Z).sum())
    assert (zoom[:top] == CAP_Z).all() and zoom[top] == CAP_Z - 1   # zoom zmax's records first, then zmax - 1's
    for cap in (total - 1, top + 1, 1):
        rc, m, cut = _raw_call(width, rows, cols, g, CAP_ZMIN, CAP_Z, cap)
        assert rc == _lib.HM_E_CAPACITY and m == total, cap
        for x, f in zip(cut, full):
            assert np.array_equal(x[:cap], f[:cap]), cap
            assert (x[cap:] == PATTERN).all(), cap


# --------------------------------------------------------------------------
# 8. split mode: the square / exotic boundary on lane, fragment and tile edges
# --------------------------------------------------------------------------

SPLIT_E = [1, 63, 64, CS_TILE - 1, CS_TILE + 1]
SPLIT_Z = 21
SPLIT_HOT = 10_000


@functools.lru_cache(maxsize=None)
def _split_case(E):
    """test_count_tiles_general_fallback's 320_000 sparse zoom-21 tiles (past
    the measured threshold of the sparse fallback) with its keep mask, its
    columns past the square (sc = 1: last in key order) and, in place of its
    scattered negative rows, E distinct cells with sr = -1: the first E keys.
    One tile of the square comes 10_000 times."""
    n = 320_000
    rng = np.random.default_rng(21)
    rows = rng.integers(0, 1 << SPLIT_Z, n)
    cols = rng.integers(0, 1 << SPLIT_Z, n)
    cols[1::1000] = (1 << SPLIT_Z) + 9
    keep = (np.arange(n) % 7 != 3).astype(np.uint8)
    j = np.arange(E)
    rows = np.concatenate([rows, -1 - j // 64, np.full(SPLIT_HOT, 123_456)])
    cols = np.concatenate([cols, 1000 + j % 64, np.full(SPLIT_HOT, 654_321)])
    keep = np.concatenate([keep, np.ones(E + SPLIT_HOT, np.uint8)])
    return _shuffled(E, rows, cols, keep)


@functools.lru_cache(maxsize=None)
def _split_reference(E, zmin):
    rows, cols, keep = _split_case(E)
    ref = oracle.count_tiles(rows, cols, zmin, SPLIT_Z, keep)
    o = np.lexsort((ref["col"], ref["row"], ref["zoom"]))
    return _frozen({k: ref[k][o] for k in FIELDS[1:]})


@pytest.mark.parametrize("E", SPLIT_E)
def test_split_inputs(E):
    rows, cols, keep = _split_case(E)
    kb = keep.astype(bool)
    sr, sc = rows[kb] >> SPLIT_Z, cols[kb] >> SPLIT_Z
    assert int((sr == -1).sum()) == E and set(np.unique(sr).tolist()) == {-1, 0}
    assert set(np.unique(sc[sr == -1]).tolist()) == {0} and set(np.unique(sc).tolist()) == {0, 1}
    first = np.unique(np.stack([rows[kb][sr == -1], cols[kb][sr == -1]], axis=1), axis=0)
    assert len(first) == E                                       # distinct
    # the sr field leads the key: the E cells come first, the square next, sc = 1 last
    pick = np.concatenate([np.flatnonzero(sr == -1), np.flatnonzero((sr == 0) & (sc == 0))[:500],
                           np.flatnonzero(sc == 1)[:50]])
    keys = _keys(rows[kb][pick], cols[kb][pick], np.zeros(pick.size, np.uint32), SPLIT_Z)
    o = np.argsort(keys, kind="stable")
    assert (sr[pick][o][:E] == -1).all() and (sc[pick][o][-50:] == 1).all()
    assert rows.size <= 330_000 + CS_TILE + 1


@GPU
@pytest.mark.parametrize("zmin", [0, SPLIT_Z])
@pytest.mark.parametrize("E", SPLIT_E)
def test_split_boundary(gpu, E, zmin):
    """count_fallback: cells of the square leave as HM_KEYs, the others as
    records, from per-tile cursor reservations (k_cascade; zmin = 21:
    k_cascade_emit's per-block ones).  Both lists against the oracle."""
    rows, cols, keep = _split_case(E)
    m, buf = device.count_device(rows, cols, keep, zmin, SPLIT_Z, tiles=True)
    assert int(device.context(0).last_stats()[1][7]) == 0, "the call took the pipeline, not the general path"
    ref = _split_reference(E, zmin)
    z, r, c = device.decode_keys(buf.keys[:m].cpu().numpy().view(np.uint64))
    cnt = buf.counts[:m].cpu().numpy()
    x = buf.xcells[:4 * buf.nx].cpu().numpy().reshape(-1, 4)
    insq = (ref["row"] >= 0) & (ref["row"] < (1 << ref["zoom"])) & (ref["col"] >= 0) & (ref["col"] < (1 << ref["zoom"]))
    assert m == int(insq.sum()) and buf.nx == int((~insq).sum()) and buf.nx >= E
    o = np.lexsort((c, r, z))
    for k, v in zip(FIELDS[1:], (z, r, c, cnt)):
        assert np.array_equal(v[o], ref[k][insq]), k
    o = np.lexsort((x[:, 2], x[:, 1], x[:, 0]))
    for i, k in enumerate(FIELDS[1:]):
        assert np.array_equal(x[o, i], ref[k][~insq]), k
