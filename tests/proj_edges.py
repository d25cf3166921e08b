"""The projection's own edges as one deterministic catalogue of points
(imported by test_proj_edges_host.py, test_gpu_proj_edges.py and
tests/golden/make_golden.py; not a conftest).

Every value is a double written out below, a ulp neighbour of one
(np.nextafter), a seeded draw, or one of an adjacent pair found by bisecting
the oracle's row.  What the classes are for:

  latitudes   the equator (R = 2^(Z-1) exactly: always deferred), |lat| = 45
              (the Sterbenz remark of hm_project_l1), the band 85.05 < |lat| <=
              85.06 between HM_LAT_SQ and HM_LAT_FAST, the square's edge
              85.0511287798066 and the adjacent doubles where row 0 becomes -1
              and row 2^Z - 1 becomes 2^Z, |lat| = 86 (d = 4: the table index
              wraps), the pole, |lat| > 90, and every edge d = 2^e (1 + j/64)
              of the polynomial table's intervals;
  longitudes  the meridian, +-180 and beyond, values a few ulps from a column
              boundary k 360 / 2^Z - 180 (RN(lon + 180) is itself rounded
              there, and / 360 differs from * RN(1/360)), worst near -1e-14.

project_set() is everything, error statuses included; count_set(zoom) the
points the oracle projects without error at that zoom.
"""
import ctypes
import functools
import os

import numpy as np

from oracle import oracle

SEED = 20261020
ZOOMS = (3, 14, 18, 21)                 # bisection and column-boundary zooms
ORDINARY_LAT, ORDINARY_LON = 47.6062, -122.3321
LAT_EDGE = 85.0511287798066             # atan(sinh(pi)) in degrees, as tile.py's callers write it
N_PAIRS = 20000

LAT_BASE = [0.0, 5e-324, 1e-300, 1e-17, 1e-14, 2e-14, 5e-14, 1e-9,
            45.0, 85.05, 85.06, 86.0, 89.0, 90.0 - 1e-9, 90.0, LAT_EDGE]
LON_BASE = [0.0, 5e-324, 1e-300, 1e-20, 1e-14, 2.0 ** -50, 2.0 ** -46,
            45.0, 90.0, 179.9, 180.0, 540.0, 1e6, 1e15]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def with_ulps(values, k):
    """each value and its neighbours 1..k ulps either side"""
    v = np.asarray(values, np.float64)
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def both_signs(v):
    v = np.asarray(v, np.float64)
    return np.concatenate([v, -v])


def table_edges():
    """90 - d at the polynomial table's interval edges d = 2^e (1 + j/64)"""
    d = np.array([2.0 ** e * (1.0 + j / 64.0) for e in range(2, 7) for j in range(64)])
    return 90.0 - d[d <= 90.0]


def _row(lat, z):
    return int(oracle.project(np.array([lat]), np.array([ORDINARY_LON]), z)[0][0])


def bisect_row(lo, hi, z, pred):
    """The adjacent doubles (a, b), lo <= a < b <= hi, with pred(row(a)) false
    and pred(row(b)) true; pred is false at lo and true at hi."""
    assert not pred(_row(lo, z)) and pred(_row(hi, z))
    while True:
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            assert np.nextafter(lo, np.inf) == hi
            return lo, hi
        if pred(_row(mid, z)):
            hi = mid
        else:
            lo = mid


@functools.lru_cache(maxsize=None)
def square_edge_pairs():
    """{(zoom, which): (a, b)}: north, rows 0 | -1 in [85.0, 85.06]; south, rows
    2^Z - 1 | 2^Z in [-85.06, -85.0] (b the more southern); equator, rows
    2^(Z-1) | 2^(Z-1) - 1 in [-1e-6, 1e-6]."""
    out = {}
    for z in ZOOMS:
        out[z, "north"] = bisect_row(85.0, 85.06, z, lambda r: r < 0)
        b, a = bisect_row(-85.06, -85.0, z, lambda r, z=z: r < (1 << z))
        out[z, "south"] = (a, b)
        out[z, "equator"] = bisect_row(-1e-6, 1e-6, z, lambda r, z=z: r < (1 << (z - 1)))
    return out


@functools.lru_cache(maxsize=None)
def latitudes():
    rng = np.random.default_rng(SEED)
    parts = [both_signs(with_ulps(LAT_BASE, 4)),
             both_signs(with_ulps(table_edges(), 2)),
             both_signs(rng.uniform(85.05, 85.06, 2000)),
             both_signs(rng.uniform(85.0511, 85.0512, 500)),
             np.array([x for p in square_edge_pairs().values() for x in p])]
    return _frozen(np.concatenate(parts))


def column_boundaries(z, rng):
    ks = [0, 1, 1 << (z - 1), (1 << (z - 1)) + 1, (1 << z) - 1, 1 << z]
    ks += rng.integers(0, (1 << z) + 1, 40).tolist()
    return np.array([k * 360.0 / (1 << z) - 180.0 for k in ks])


@functools.lru_cache(maxsize=None)
def boundary_longitudes():
    """the exact boundaries k 360 / 2^Z - 180 of ZOOMS (no neighbours)"""
    rng = np.random.default_rng(SEED + 1)
    return _frozen(np.concatenate([column_boundaries(z, rng) for z in ZOOMS]))


@functools.lru_cache(maxsize=None)
def longitudes():
    return _frozen(np.concatenate([both_signs(with_ulps(LON_BASE, 8)), with_ulps(boundary_longitudes(), 8)]))


@functools.lru_cache(maxsize=None)
def project_set():
    """(lat, lon): every latitude with one ordinary longitude, every longitude
    with one ordinary latitude, then N_PAIRS seeded pairs of the two lists."""
    la, lo = latitudes(), longitudes()
    rng = np.random.default_rng(SEED + 2)
    i = rng.integers(0, la.size, N_PAIRS)
    j = rng.integers(0, lo.size, N_PAIRS)
    ca, co = np.array(CORNERS).T
    lat = np.concatenate([la, np.full(lo.size, ORDINARY_LAT), ca, la[i]])
    lon = np.concatenate([np.full(la.size, ORDINARY_LON), lo, co, lo[j]])
    return _frozen(lat, lon)


# both coordinates on an edge at once: null island with every sign of zero,
# the equator and the square's edge on the meridian and the date line
CORNERS = [(a, b) for a in (0.0, -0.0, LAT_EDGE, -LAT_EDGE, 85.05, -85.05, 45.0, -45.0)
           for b in (0.0, -0.0, 180.0, -180.0, -1e-14)]


def n_named():
    """project_set()[:n_named()] are the named edges, the rest the random pairs"""
    return latitudes().size + longitudes().size + len(CORNERS)


@functools.lru_cache(maxsize=None)
def count_mask(zoom):
    lat, lon = project_set()
    return _frozen(oracle.project(lat, lon, zoom)[2] == 0)


@functools.lru_cache(maxsize=None)
def count_set(zoom):
    """the points of project_set() with oracle status 0 at `zoom`"""
    lat, lon = project_set()
    m = count_mask(zoom)
    return _frozen(lat[m].copy(), lon[m].copy())


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_edges.npz")


def golden_expect(g, i):
    """(status, row, col) the reference gives at g["zoom"][i]: the row's error
    wins (tile.py:10-11); status 8 is a column beyond int64"""
    re_, ce = g["row_err"][i], g["col_err"][i]
    return np.where(re_ != 0, re_, ce).astype(np.uint8), g["row"][i], g["col"][i]


def ulp_distance(a, b):
    """|a - b| in units of the larger magnitude's ulp (float; inf for NaN)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# --------------------------------------------------------------------------
# the host build of csrc/hm_project.h (conftest's host_math fixture)
# --------------------------------------------------------------------------

def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def l1_lib(L):
    """the host build with hmh_project_l1's argument types set"""
    P = ctypes.POINTER
    L.hmh_project_l1.argtypes = [P(ctypes.c_double), P(ctypes.c_double), ctypes.c_int64, ctypes.c_int,
                                 P(ctypes.c_int32), P(ctypes.c_int32), P(ctypes.c_uint8)]
    L.hmh_project_l1.restype = ctypes.c_int64
    return L


def host_point(L, lat, lon, z):
    lat, lon = np.ascontiguousarray(lat, np.float64), np.ascontiguousarray(lon, np.float64)
    n = lat.size
    row, col = np.zeros(n, np.int64), np.zeros(n, np.int64)
    st, slow = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    L.hmh_project(_p(lat, ctypes.c_double), _p(lon, ctypes.c_double), n, z, _p(row, ctypes.c_int64),
                  _p(col, ctypes.c_int64), _p(st, ctypes.c_uint8), _p(slow, ctypes.c_uint8))
    return row, col, st, slow


def host_model(L, which, lat, lon, z):
    """(row, col, ok) of hmh_project_fast ("fast") or hmh_project_l1 ("l1")"""
    lat, lon = np.ascontiguousarray(lat, np.float64), np.ascontiguousarray(lon, np.float64)
    n = lat.size
    row, col, ok = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    fn = l1_lib(L).hmh_project_l1 if which == "l1" else L.hmh_project_fast
    m = fn(_p(lat, ctypes.c_double), _p(lon, ctypes.c_double), n, z, _p(row, ctypes.c_int32), _p(col, ctypes.c_int32),
           _p(ok, ctypes.c_uint8))
    assert m == int(ok.sum())
    return row.astype(np.int64), col.astype(np.int64), ok.astype(bool)
