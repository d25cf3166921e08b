"""CPU: the three host-compiled projections -- hm_project_point, hm_project_fast
and hm_project_l1 (k_l1_fast's own statements), all of csrc/hm_project.h --
against the oracle on the edge catalogue of proj_edges.py, the catalogue's
pin to the reference (tests/golden/projection_edges.npz), and the properties
of the catalogue that the GPU module (test_gpu_proj_edges.py) relies on.
Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

import proj_edges as pe
from proj_edges import host_model, host_point
from oracle import oracle

GOLDEN = pe.GOLDEN
_golden_expect = pe.golden_expect
POINT_ZOOMS = [0, 3, 5, 11, 14, 18, 21, 26, 30]
FAST_ZOOMS = [0, 3, 5, 11, 14, 18, 21]       # the count paths' zooms (the fast models hold int32 tiles)


@functools.lru_cache(maxsize=None)
def _oracle(z):
    lat, lon = pe.project_set()
    r, c, st, _ = oracle.project(lat, lon, z)
    for a in (r, c, st):
        a.setflags(write=False)
    return r, c, st


# --------------------------------------------------------------------------
# the catalogue itself
# --------------------------------------------------------------------------

def test_catalogue_is_deterministic_and_sized():
    lat, lon = pe.project_set()
    assert lat.size == lon.size == pe.n_named() + pe.N_PAIRS
    assert 7000 < pe.latitudes().size < 10000 and 2500 < pe.longitudes().size < 5000
    for f in (pe.latitudes, pe.longitudes, pe.project_set, pe.square_edge_pairs, pe.boundary_longitudes):
        f.cache_clear()
    lat2, lon2 = pe.project_set()
    assert np.array_equal(lat, lat2, equal_nan=True) and np.array_equal(lon, lon2, equal_nan=True)


@pytest.mark.parametrize("z", FAST_ZOOMS)
def test_count_set_drops_only_latitudes_past_the_pole(z):
    """A condition on the catalogue: at the count paths' zooms the only error
    status is DOMAIN, and exactly two families carry it: |lat| > 90, and the
    catalogue's latitudes within 1e-9 of the south pole, -90 included, where
    tan(x) + 1 / cos(x) cancels to zero or below and the reference's log raises
    (projection_edges.npz holds the reference's own errors there)."""
    lat, lon = pe.project_set()
    st = _oracle(z)[2]
    assert np.array_equal(st != 0, (np.abs(lat) > 90.0) | (lat < -89.99999999))
    assert (st[lat == -90.0] == oracle.E_DOMAIN).all() and (st[lat == 90.0] == 0).all() and (st[lat == -89.0] == 0).all()
    assert set(np.unique(st).tolist()) == {0, oracle.E_DOMAIN}
    cl, co = pe.count_set(z)
    assert cl.size == int((st == 0).sum()) and (np.abs(cl) <= 90.0).all() and cl.size > lat.size - 2000


@pytest.mark.parametrize("z", [3, 14, 18, 21])
def test_catalogue_classes(z):
    """Every class of the issue is present in count_set(z): a later edit of the
    catalogue cannot hollow it out."""
    lat, lon = pe.count_set(z)
    r, c, st, _ = oracle.project(lat, lon, z)
    assert (st == 0).all()
    n = 1 << z
    a = np.abs(lat)
    assert ((a > 85.05) & (a < 85.0511)).sum() >= 100, "between HM_LAT_SQ and the square's edge"
    assert (((a > 85.05) & (a < 85.0511)) & (r >= 0) & (r < n)).sum() >= 100
    assert ((a > 85.0511) & (a <= 85.06)).sum() >= 1000, "past the edge, inside HM_LAT_FAST"
    assert ((lat > 85.0512) & (lat <= 85.06) & (r < 0)).any() and ((lat < -85.0512) & (lat >= -85.06) & (r >= n)).any()
    pairs = pe.square_edge_pairs()
    for which, rows in (("north", (0, -1)), ("south", (n - 1, n)), ("equator", (n // 2, n // 2 - 1))):
        p = pairs[z, which]
        assert abs(np.nextafter(p[0], p[1]) - p[1]) == 0.0      # adjacent doubles
        for x, want in zip(p, rows):
            m = lat == x
            assert m.any() and (r[m] == want).all(), (which, x)
    assert (lat == 0.0).sum() >= 2 and (r[lat == 0.0] == n // 2).all(), "equator"
    assert ((lat == 0.0) & (lon == 0.0)).any(), "null island"
    assert (np.abs(lat) == 45.0).any() and (np.abs(lat) == 86.0).any() and (np.abs(lat) == 90.0).any()
    b = pe.boundary_longitudes()
    near = np.zeros(lon.size, bool)
    exact = np.isin(lon, b)
    for x in np.unique(b):
        near |= (pe.ulp_distance(lon, x) <= 8.0) & (lon != x)
    assert near.sum() >= 1000 and exact.sum() >= 100, "within 8 ulp of a column boundary, and on one"
    assert (lon == 180.0).any() and (lon == -180.0).any()
    assert (c[lon == -180.0] == 0).all() and (c[lon == 180.0] == n).all()
    assert (c < 0).sum() >= 10 and (c >= n).sum() >= 10, "columns outside the square, both sides"
    assert ((lon > -1.1e-14) & (lon < -0.9e-14)).any(), "lon + 180 rounds to 180"
    d = 90.0 - np.abs(lat)
    edges = 90.0 - pe.table_edges()
    assert np.isin(edges, d).all() and edges.size > 280, "every interval edge of the polynomial table"


def test_golden_holds_the_catalogue():
    """the fixture was made from this catalogue: the same points, bit for bit"""
    g = np.load(GOLDEN)
    lat, lon = pe.project_set()
    m = g["lat"].size
    assert m >= pe.n_named(), "the named edges are never thinned"
    assert np.array_equal(g["lat"].view(np.uint64), lat[:m].view(np.uint64))
    assert np.array_equal(g["lon"].view(np.uint64), lon[:m].view(np.uint64))
    assert g["zoom"].tolist() == [0, 3, 14, 18, 21, 30]
    for k in ("row", "col", "row_err", "col_err"):
        assert g[k].shape == (6, m), k


# --------------------------------------------------------------------------
# oracle and host build against the reference's own results
# --------------------------------------------------------------------------

def test_oracle_equals_golden():
    g = np.load(GOLDEN)
    for i, z in enumerate(g["zoom"].tolist()):
        exp, row, col = _golden_expect(g, i)
        r, c, st, _ = oracle.project(g["lat"], g["lon"], z)
        assert np.array_equal(st, exp), z
        ok = exp == 0
        assert np.array_equal(r[ok], row[ok]) and np.array_equal(c[ok], col[ok]), z
    assert (g["col_err"] == 8).any(), "a column beyond int64 (lon 1e15 at zoom 30)"


def test_host_build_equals_golden(host_math):
    g = np.load(GOLDEN)
    for i, z in enumerate(g["zoom"].tolist()):
        exp, row, col = _golden_expect(g, i)
        r, c, st, _ = host_point(host_math, g["lat"], g["lon"], z)
        assert np.array_equal(st, exp), z
        ok = exp == 0
        assert np.array_equal(r[ok], row[ok]) and np.array_equal(c[ok], col[ok]), z


# --------------------------------------------------------------------------
# the host-compiled statements against the oracle, whole catalogue
# --------------------------------------------------------------------------

@pytest.mark.parametrize("z", POINT_ZOOMS)
def test_project_point_equals_oracle(host_math, z):
    lat, lon = pe.project_set()
    er, ec, est = _oracle(z)
    r, c, st, _ = host_point(host_math, lat, lon, z)
    assert np.array_equal(st, est)
    ok = est == 0
    assert np.array_equal(r[ok], er[ok]) and np.array_equal(c[ok], ec[ok])


@pytest.mark.parametrize("which", ["fast", "l1"])
@pytest.mark.parametrize("z", FAST_ZOOMS)
def test_models_accept_only_the_oracles_tile(host_math, which, z):
    """Wherever hm_project_fast or hm_project_l1 says ok: oracle status 0, the
    oracle's tile, inside [0, 2^z)^2."""
    lat, lon = pe.project_set()
    er, ec, est = _oracle(z)
    r, c, ok = host_model(host_math, which, lat, lon, z)
    assert ok.sum() >= 1000, "the models accept part of the catalogue: the check is not empty"
    assert (est[ok] == 0).all()
    assert np.array_equal(r[ok], er[ok]) and np.array_equal(c[ok], ec[ok])
    assert (r[ok] >= 0).all() and (r[ok] < (1 << z)).all() and (c[ok] >= 0).all() and (c[ok] < (1 << z)).all()


@pytest.mark.parametrize("z", FAST_ZOOMS)
def test_models_decide_alike(host_math, z):
    """hm_project_l1 restates hm_project_fast with other arithmetic (one fma
    for the column, |lon| < 180 for the range): where both accept they give one
    tile.  Their decisions may differ only inside a column guard band (the two
    y differ by a rounding), never on the row: the deferred sets differ by
    under 1% of the catalogue, which is why the GPU module counts the whole
    tiles' deferred points with one model and the partial tile's with the
    other."""
    lat, lon = pe.project_set()
    rf, cf, okf = host_model(host_math, "fast", lat, lon, z)
    rl, cl, okl = host_model(host_math, "l1", lat, lon, z)
    both = okf & okl
    assert np.array_equal(rf[both], rl[both]) and np.array_equal(cf[both], cl[both])
    diff = okf != okl
    assert diff.sum() <= lat.size // 100
    # a differing decision is a column matter: the same latitude with the ordinary longitude decides alike
    la = np.unique(lat[diff])
    lo = np.full(la.size, pe.ORDINARY_LON)
    assert np.array_equal(host_model(host_math, "fast", la, lo, z)[2], host_model(host_math, "l1", la, lo, z)[2])


@pytest.mark.parametrize("which", ["fast", "l1"])
@pytest.mark.parametrize("z", [18, 21])
def test_models_defer_the_edges(host_math, which, z):
    """At the product's zooms the fast models defer every equator point, every
    point on the meridian or the date line, and every point past HM_LAT_SQ."""
    lat, lon = pe.project_set()
    _, _, ok = host_model(host_math, which, lat, lon, z)
    must = (lat == 0.0) | (lon == 0.0) | (np.abs(lon) == 180.0) | (np.abs(lat) > 85.05)
    assert must.sum() > 5000 and not ok[must].any()
    assert not ok[~np.isfinite(lat) | ~np.isfinite(lon)].any()
    # and accept the ordinary point
    o = (lat == pe.ORDINARY_LAT) & (lon == pe.ORDINARY_LON)
    assert host_model(host_math, which, [pe.ORDINARY_LAT], [pe.ORDINARY_LON], z)[2].all() and not o.any()
