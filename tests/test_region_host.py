"""heatmap_amd/region.py on the CPU: RegionSet's constructors against
brute-force models.

from_tile_polygons is checked against a per-cell loop over the bounding box
that applies the documented crossing rule to one cell at a time (no sorting, no
pairing): a cell (row, col) is inside iff an odd number of the row's crossings
x satisfy ceil(x - 0.5) <= col."""
import math

import numpy as np
import pytest

from heatmap_amd import tile
from heatmap_amd.region import MAX_REGIONS, RegionSet


def brute_cells(rings, zoom, box):
    """{(row, col)} of the region over box = (r0, r1, c0, c1), clipped to the square"""
    side = 1 << zoom
    out = set()
    edges = []
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        for i in range(len(ring)):
            edges.append((ring[i], ring[(i + 1) % len(ring)]))
    r0, r1, c0, c1 = box
    for r in range(max(r0, 0), min(r1, side)):
        yc = r + 0.5
        starts = []
        for (x0, y0), (x1, y1) in edges:
            if (y0 <= yc) != (y1 <= yc):
                x = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0)
                starts.append(math.ceil(x - 0.5))
        for c in range(max(c0, 0), min(c1, side)):
            if sum(1 for s in starts if s <= c) % 2:
                out.add((r, c))
    return out


def cells_of(rs, j):
    r, c = rs.cells(j)
    assert len(set(zip(r.tolist(), c.tolist()))) == len(r)   # no cell twice
    return set(zip(r.tolist(), c.tolist()))


def check_table(rs):
    """the invariants of the span table"""
    assert rs.row_ptr[0] == 0 and rs.row_ptr[-1] == rs.nspans and (np.diff(rs.row_ptr.astype(np.int64)) >= 0).all()
    assert 0 <= rs.row_lo and rs.row_lo + rs.nrows <= (1 << rs.zoom)
    assert (rs.col_lo < rs.col_hi).all() and (rs.col_hi <= (1 << rs.zoom)).all() and (rs.region < rs.nregions).all()
    for i in range(rs.nrows):
        a, b = int(rs.row_ptr[i]), int(rs.row_ptr[i + 1])
        key = list(zip(rs.col_lo[a:b].tolist(), rs.region[a:b].tolist()))
        assert key == sorted(key), i
        for g in set(rs.region[a:b].tolist()):
            m = rs.region[a:b] == g
            lo, hi = rs.col_lo[a:b][m].astype(np.int64), rs.col_hi[a:b][m].astype(np.int64)
            assert (lo[1:] > hi[:-1]).all(), (i, g)   # disjoint AND not touching: merged
    if rs.nrows:
        assert rs.row_ptr[1] > 0 and rs.row_ptr[-1] > rs.row_ptr[-2]   # the first and last rows hold spans


TRIANGLE = [np.array([[2.2, 1.1], [13.7, 4.4], [5.1, 12.9]])]
CONCAVE = [np.array([[1.0, 1.0], [14.0, 1.0], [14.0, 14.0], [8.0, 5.0], [1.0, 14.0]])]
HOLED = [np.array([[2.0, 2.0], [13.0, 2.0], [13.0, 13.0], [2.0, 13.0]]),
         np.array([[5.0, 5.0], [10.0, 5.0], [10.0, 10.0], [5.0, 10.0]])]
TWO_PARTS = [np.array([[1.3, 1.3], [4.6, 1.3], [4.6, 4.6], [1.3, 4.6]]),
             np.array([[9.2, 8.1], [14.9, 9.0], [11.0, 14.2]])]
OUTSIDE = [np.array([[-5.3, -4.2], [20.7, -3.1], [22.4, 19.9], [-2.5, 21.3]]),          # covers the square
           np.array([[3.0, 3.0], [6.0, 3.0], [6.0, 6.0], [3.0, 6.0]])]                  # with a hole
THIN = [np.array([[3.6, 2.0], [3.9, 2.0], [3.9, 9.0], [3.6, 9.0]])]                     # between centres: no span
ON_CENTRES = [np.array([[2.5, 2.5], [9.5, 2.5], [9.5, 7.5], [2.5, 7.5]])]               # the half-open rule


@pytest.mark.parametrize("name,rings", [("triangle", TRIANGLE), ("concave", CONCAVE), ("holed", HOLED),
                                        ("two_parts", TWO_PARTS), ("outside", OUTSIDE), ("thin", THIN),
                                        ("on_centres", ON_CENTRES)])
def test_tile_polygon_against_the_per_cell_rule(name, rings):
    rs = RegionSet.from_tile_polygons([rings], 4)
    check_table(rs)
    want = brute_cells(rings, 4, (-8, 24, -8, 24))
    assert cells_of(rs, 0) == want
    assert rs.area().tolist() == [len(want)]
    if name == "thin":
        assert rs.nspans == 0 and rs.nrows == 0 and rs.row_ptr.tolist() == [0]
    if name == "on_centres":
        # centres at x = 2.5 .. 8.5 are inside [2.5, 9.5), rows y = 2.5 .. 6.5 likewise
        assert want == {(r, c) for r in range(2, 7) for c in range(2, 9)}
    if name == "holed":
        assert (7, 7) not in want and (3, 3) in want
    if name == "outside":
        assert len(want) == 256 - 9


def test_overlapping_regions_keep_both():
    a = [np.array([[1.0, 1.0], [9.0, 1.0], [9.0, 9.0], [1.0, 9.0]])]
    b = [np.array([[5.0, 4.0], [14.0, 4.0], [14.0, 12.0], [5.0, 12.0]])]
    rs = RegionSet.from_tile_polygons([a, b, TRIANGLE], 4, names=["a", "b", "t"])
    check_table(rs)
    for j, rings in enumerate([a, b, TRIANGLE]):
        assert cells_of(rs, j) == brute_cells(rings, 4, (0, 16, 0, 16))
    assert cells_of(rs, 0) & cells_of(rs, 1) == {(r, c) for r in range(4, 9) for c in range(5, 9)}
    assert rs.names == ["a", "b", "t"]


def test_zoom_0_and_a_larger_zoom():
    whole = [np.array([[0.1, 0.1], [0.9, 0.1], [0.9, 0.9], [0.1, 0.9]])]
    rs = RegionSet.from_tile_polygons([whole], 0)
    assert cells_of(rs, 0) == {(0, 0)} and (rs.row_lo, rs.nrows) == (0, 1)
    miss = [np.array([[0.6, 0.6], [0.9, 0.6], [0.9, 0.9]])]
    assert RegionSet.from_tile_polygons([miss], 0).nspans == 0
    rng = np.random.default_rng(5)
    ring = [np.array([[300.0, 500.0]]) + 40 * np.stack([np.cos(t), np.sin(t)], axis=1) * rng.uniform(0.4, 1.0, (9, 1))
            for t in [np.sort(rng.uniform(0, 2 * np.pi, 9))]]
    rs = RegionSet.from_tile_polygons([ring], 10)
    check_table(rs)
    assert cells_of(rs, 0) == brute_cells(ring, 10, (450, 550, 250, 350))


def test_bad_vertices_and_limits():
    with pytest.raises(ValueError):
        RegionSet.from_tile_polygons([[np.array([[1.0, 1.0], [np.nan, 2.0], [3.0, 3.0]])]], 4)
    with pytest.raises(ValueError):
        RegionSet.from_tile_polygons([[np.array([[1.0, 1.0], [np.inf, 2.0], [3.0, 3.0]])]], 4)
    with pytest.raises(ValueError):
        RegionSet.from_tile_polygons([[np.array([[1.0, 1.0], [2.0, 2.0]])]], 4)
    with pytest.raises(ValueError):
        RegionSet.from_polygons([[np.array([[90.0, 0.0], [10.0, 5.0], [0.0, 0.0]])]], 4)
    with pytest.raises(ValueError):
        RegionSet.from_polygons([[np.array([[10.0, np.nan], [10.0, 5.0], [0.0, 0.0]])]], 4)
    with pytest.raises(ValueError, match="regions"):
        RegionSet.from_tile_polygons([TRIANGLE] * (MAX_REGIONS + 1), 4)
    with pytest.raises(ValueError, match="regions"):
        RegionSet.from_tile_polygons([], 4)
    with pytest.raises(ValueError, match="zoom"):
        RegionSet.from_tile_polygons([TRIANGLE], 22)
    with pytest.raises(ValueError, match="spans"):
        RegionSet.from_mask(11, 0, 0, (np.indices((1025, 2048)).sum(0) % 2).astype(bool))   # 2^20 + 1024 spans
    with pytest.raises(ValueError, match="one zoom"):
        RegionSet.from_rects([(4, 0, 1, 0, 1), (5, 0, 1, 0, 1)])


def test_lat_lon_polygon_of_cell_corners():
    """A polygon whose vertices are cell corners (tile.latitude_from_row /
    longitude_from_column) selects exactly the cells it encloses: their centres
    are half a cell from every edge."""
    z = 9
    corners = [(100, 200), (100, 260), (130, 260), (130, 230), (150, 230), (150, 200)]   # (row, col), an L
    ring = np.array([[tile.Tile.latitude_from_row(r, z), tile.Tile.longitude_from_column(c, z)] for r, c in corners])
    rs = RegionSet.from_polygons([[ring]], z)
    check_table(rs)
    want = {(r, c) for r in range(100, 130) for c in range(200, 260)} | \
           {(r, c) for r in range(130, 150) for c in range(200, 230)}
    assert cells_of(rs, 0) == want


def test_mask_round_trips():
    rng = np.random.default_rng(11)
    m = rng.random((13, 17)) < 0.45
    m[4] = False                                    # a covered row without a span
    rs = RegionSet.from_mask(6, 20, 30, m)
    check_table(rs)
    assert cells_of(rs, 0) == {(20 + r, 30 + c) for r, c in zip(*np.nonzero(m))}
    assert rs.row_ptr[5] == rs.row_ptr[4]
    mi = rng.integers(0, 5, (13, 17))
    rs = RegionSet.from_mask(6, 20, 30, mi)
    check_table(rs)
    assert rs.nregions == 4
    for v in range(1, 5):
        assert cells_of(rs, v - 1) == {(20 + r, 30 + c) for r, c in zip(*np.nonzero(mi == v))}
    m3 = rng.random((3, 13, 17)) < 0.5
    rs = RegionSet.from_mask(6, 20, 30, m3)
    check_table(rs)
    for j in range(3):
        assert cells_of(rs, j) == {(20 + r, 30 + c) for r, c in zip(*np.nonzero(m3[j]))}
    assert rs.area().tolist() == m3.sum(axis=(1, 2)).tolist()
    # clipped to the square on every side
    rs = RegionSet.from_mask(3, -2, -3, np.ones((14, 14), dtype=bool))
    assert cells_of(rs, 0) == {(r, c) for r in range(8) for c in range(8)}
    assert RegionSet.from_mask(3, 0, 0, np.zeros((4, 4), dtype=bool)).nspans == 0


def test_touching_and_overlapping_spans_of_one_region_merge():
    rs = RegionSet._from_spans(5, [3, 3, 3, 3, 3, 4], [2, 5, 7, 20, 9, 1], [5, 8, 9, 22, 12, 2], [0, 0, 0, 0, 1, 0], 2)
    check_table(rs)
    assert rs.col_lo.tolist() == [2, 9, 20, 1] and rs.col_hi.tolist() == [9, 12, 22, 2]
    assert rs.region.tolist() == [0, 1, 0, 0] and rs.row_ptr.tolist() == [0, 3, 4] and rs.row_lo == 3
    # abutting spans of DIFFERENT regions stay apart
    rs = RegionSet.from_rects([(5, 0, 2, 0, 4), (5, 0, 2, 4, 9), (5, 1, 3, 2, 6)])
    check_table(rs)
    assert rs.col_lo.tolist() == [0, 4, 0, 2, 4, 2] and rs.region.tolist() == [0, 1, 0, 2, 1, 2]
    assert rs.bounding_rect() == (5, 0, 3, 0, 9)


def test_rects_are_clipped():
    rs = RegionSet.from_rects([(3, -2, 3, -5, 2), (3, 6, 12, 6, 12), (3, 9, 12, 0, 4)])
    check_table(rs)
    assert cells_of(rs, 0) == {(r, c) for r in range(3) for c in range(2)}
    assert cells_of(rs, 1) == {(r, c) for r in (6, 7) for c in (6, 7)}
    assert cells_of(rs, 2) == set() and rs.nregions == 3
