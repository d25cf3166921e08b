"""The host side of the region queries (hm_stream_region_series / _view /
_visitors; StreamingHeatmap.region_*): csrc/hm_region.h on the CPU, built into
a shim with the host compiler -- the lookup the kernel compiles from the same
text, and the checker the entry points run before any upload -- then the
Python methods' argument validation, the header and the export list."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from heatmap_amd import _lib
from heatmap_amd import stream as S
from heatmap_amd.region import RegionSet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")
SHIM = """
#include <stdlib.h>
#include "hm_region.h"
int64_t rg_next(const uint32_t* rp, const uint32_t* lo, const uint32_t* hi, uint32_t row_rel, uint32_t col, int64_t from)
{
    return hms_region_next(rp, lo, hi, row_rel, col, from);
}
int rg_check(int zoom, int64_t row_lo, int64_t nrows, int64_t nspans, int64_t nregions, const uint32_t* rp,
             const uint32_t* lo, const uint32_t* hi, const uint32_t* rg, int zmin, int zmax, int64_t* index)
{
    uint32_t* scratch = malloc(2 * 4096 * sizeof(uint32_t));
    for (int i = 0; i < 2 * 4096; i++) scratch[i] = 0xA5A5A5A5u;   /* any contents */
    const int r = hms_region_check(zoom, row_lo, nrows, nspans, nregions, rp, lo, hi, rg, zmin, zmax, scratch, index);
    free(scratch);
    return r;
}
void rg_ids(int z, int64_t row_lo, int64_t nrows, uint64_t* out)
{
    HmsRegionIds r = hms_region_ids(z, row_lo, nrows);
    out[0] = r.id_lo;
    out[1] = r.span;
}
int rg_limits(int64_t* out)
{
    out[0] = HMS_REGION_MAX_REGIONS, out[1] = HMS_REGION_MAX_SPANS, out[2] = HMS_REGION_MAX_ROWS;
    return HMS_RG_OK;
}
"""
RULES = {"ok": 0, "zoom": 1, "limits": 2, "rows": 3, "row_ptr": 4, "cols": 5, "region": 6, "order": 7, "overlap": 8}
U32P = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_region")
    src, lib = d / "shim.c", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                    str(src), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    L.rg_next.argtypes = [U32P, U32P, U32P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int64]
    L.rg_next.restype = ctypes.c_int64
    L.rg_check.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 4 + [U32P] * 4 + [ctypes.c_int] * 2 + \
                          [ctypes.POINTER(ctypes.c_int64)]
    L.rg_ids.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64)]
    L.rg_limits.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    return L


def _p(a):
    return a.ctypes.data_as(U32P)


def check(shim, rs, zmin=0, zmax=21, **over):
    """(rule, index) of hms_region_check on the RegionSet's table, fields replaced by `over`"""
    f = dict(zoom=rs.zoom, row_lo=rs.row_lo, nrows=rs.nrows, nspans=rs.nspans, nregions=rs.nregions,
             row_ptr=rs.row_ptr, col_lo=rs.col_lo, col_hi=rs.col_hi, region=rs.region)
    f.update(over)
    arrays = [np.ascontiguousarray(f[k], dtype=np.uint32) for k in ("row_ptr", "col_lo", "col_hi", "region")]
    idx = ctypes.c_int64(-7)
    rule = shim.rg_check(f["zoom"], f["row_lo"], f["nrows"], f["nspans"], f["nregions"], *(_p(a) for a in arrays),
                         zmin, zmax, ctypes.byref(idx))
    return rule, idx.value


def covering(shim, rs, row, col):
    """the span indices hms_region_next walks for cell (row, col)"""
    out, j = [], 0
    while True:
        j = shim.rg_next(_p(rs.row_ptr), _p(rs.col_lo), _p(rs.col_hi), row - rs.row_lo, col, j)
        if j < 0:
            return out
        out.append(j)
        j += 1


def test_limits_match_the_public_header(shim):
    out = (ctypes.c_int64 * 3)()
    shim.rg_limits(out)
    assert list(out) == [_lib.HM_REGION_MAX_REGIONS, _lib.HM_REGION_MAX_SPANS, _lib.HM_REGION_MAX_ROWS]
    text = open(os.path.join(REPO, "include", "heatmap_amd.h")).read()
    for name, v in (("HM_REGION_MAX_REGIONS", "4096"), ("HM_REGION_MAX_SPANS", "(1 << 20)"),
                    ("HM_REGION_MAX_ROWS", "(1 << 20)"), ("HM_REGION_MAX_TOTALS", "(1 << 22)")):
        assert re.search(r"#define %s %s\b" % (name, re.escape(v)), text) or ("#define %s %s" % (name, v)) in text


def test_next_walks_exactly_the_covering_spans(shim):
    """Random overlapping masks, rows without spans and a 64-wide checkerboard
    (32 spans per row): every cell of the covered rows, against the masks."""
    rng = np.random.default_rng(3)
    m3 = rng.random((5, 12, 40)) < 0.4
    m3[:, 5] = False
    m3[2, 7] = True
    sets = [(RegionSet.from_mask(7, 9, 11, m3), m3, 9, 11)]
    cb = (np.indices((6, 64)).sum(0) % 2 == 0)[None]
    sets.append((RegionSet.from_mask(6, 0, 0, cb), cb, 0, 0))
    for rs, m, r0, c0 in sets:
        assert np.diff(rs.row_ptr.astype(np.int64)).max() >= 32 or m.shape[0] > 1
        side = 1 << rs.zoom
        for row in range(rs.row_lo, rs.row_lo + rs.nrows):
            for col in range(side):
                inside = 0 <= row - r0 < m.shape[1] and 0 <= col - c0 < m.shape[2]
                want = sorted(j for j in range(m.shape[0]) if inside and m[j, row - r0, col - c0])
                got = covering(shim, rs, row, col)
                assert sorted(rs.region[got].tolist()) == want, (row, col)
                assert all(rs.col_lo[j] <= col < rs.col_hi[j] for j in got)
                assert all(int(rs.row_ptr[row - rs.row_lo]) <= j < int(rs.row_ptr[row - rs.row_lo + 1]) for j in got)
    assert rs.row_ptr[1] - rs.row_ptr[0] == 32


def test_ids_are_the_rows_of_the_pyramid(shim):
    for z, row_lo, nrows in [(0, 0, 1), (5, 3, 7), (21, (1 << 21) - 4, 4), (10, 0, 1024)]:
        out = (ctypes.c_uint64 * 2)()
        shim.rg_ids(z, row_lo, nrows, out)
        assert out[0] == (4 ** z - 1) // 3 + (row_lo << z) and out[1] == nrows << z
        assert out[0] + out[1] <= (4 ** (z + 1) - 1) // 3


def _tables():
    rng = np.random.default_rng(8)
    yield RegionSet.from_mask(6, 3, 4, rng.random((4, 20, 30)) < 0.5)
    yield RegionSet.from_mask(6, 0, 0, rng.integers(0, 9, (64, 64)))
    yield RegionSet.from_rects([(4, 0, 16, 0, 16), (4, 2, 5, 3, 9), (4, 15, 16, 15, 16)])
    yield RegionSet.from_rects([(0, 0, 1, 0, 1)])
    yield RegionSet.from_mask(5, 0, 0, np.zeros((3, 3), dtype=bool))          # no span, no row
    yield RegionSet.from_tile_polygons([[np.array([[1.5, 2.5], [30.2, 8.0], [12.0, 29.0]])],
                                        [np.array([[10.0, 1.0], [20.0, 1.0], [15.0, 31.5]])]], 5)
    yield RegionSet.from_mask(10, 0, 0, (np.arange(1024)[:, None] // 16 * 64 + np.arange(1024)[None] // 16 + 1))


def test_check_accepts_what_region_py_builds(shim):
    n = 0
    for rs in _tables():
        assert check(shim, rs, 0, 21) == (0, 0), rs.nspans
        n = max(n, rs.nregions)
    assert n == _lib.HM_REGION_MAX_REGIONS


def test_check_rejects_one_table_per_rule(shim):
    rs = RegionSet.from_rects([(4, 2, 5, 0, 4), (4, 2, 5, 4, 9), (4, 3, 6, 2, 6)])
    # rows 2..5; row_ptr [0, 2, 5, 8, 9]; row 3's spans: (0,4,r0) (2,6,r2) (4,9,r1)
    assert rs.row_ptr.tolist() == [0, 2, 5, 8, 9] and rs.col_lo[2:5].tolist() == [0, 2, 4]
    assert check(shim, rs) == (RULES["ok"], 0)
    assert check(shim, rs, 5, 9)[0] == RULES["zoom"] and check(shim, rs, 0, 3)[0] == RULES["zoom"]
    assert check(shim, rs, nregions=2) == (RULES["region"], 3)
    assert check(shim, rs, nregions=0)[0] == RULES["limits"]
    assert check(shim, rs, nregions=4097)[0] == RULES["limits"]
    assert check(shim, rs, nspans=(1 << 20) + 1)[0] == RULES["limits"]
    assert check(shim, rs, nrows=(1 << 20) + 1)[0] == RULES["limits"]
    assert check(shim, rs, row_lo=-1)[0] == RULES["rows"]
    assert check(shim, rs, row_lo=13)[0] == RULES["rows"]            # 13 + 4 rows > 16
    assert check(shim, rs, row_lo=12)[0] == RULES["ok"]
    rp = rs.row_ptr.copy()
    rp[0] = 1
    assert check(shim, rs, row_ptr=rp) == (RULES["row_ptr"], 0)
    rp = rs.row_ptr.copy()
    rp[2] = 1                                                        # falls after row 0's 2
    assert check(shim, rs, row_ptr=rp) == (RULES["row_ptr"], 1)
    rp = rs.row_ptr.copy()
    rp[4] = 8                                                        # does not end at nspans
    assert check(shim, rs, row_ptr=rp) == (RULES["row_ptr"], 4)
    rp = rs.row_ptr.copy()
    rp[3] = 12                                                       # beyond nspans
    assert check(shim, rs, row_ptr=rp) == (RULES["row_ptr"], 2)
    hi = rs.col_hi.copy()
    hi[6] = 17                                                       # beyond 2^zoom
    assert check(shim, rs, col_hi=hi) == (RULES["cols"], 6)
    hi = rs.col_hi.copy()
    hi[1] = rs.col_lo[1]                                             # empty
    assert check(shim, rs, col_hi=hi) == (RULES["cols"], 1)
    lo = rs.col_lo.copy()
    lo[3], lo[4] = lo[4], lo[3]                                      # row 3 unsorted by col_lo
    assert check(shim, rs, col_lo=lo) == (RULES["order"], 4)
    two = RegionSet.from_rects([(4, 0, 1, 3, 5), (4, 0, 1, 3, 8)])
    assert check(shim, two, region=two.region[::-1].copy()) == (RULES["order"], 1)   # equal col_lo, regions fall
    rg = rs.region.copy()
    rg[4] = 0                                                        # (4, 9) now overlaps region 0's (0, 4)? no: touches
    assert check(shim, rs, region=rg) == (RULES["ok"], 0)
    rg[3] = 0                                                        # (2, 6) overlaps region 0's (0, 4)
    assert check(shim, rs, region=rg) == (RULES["overlap"], 3)
    # an overlap two spans back, behind a span of another region
    far = dict(zoom=4, row_lo=0, nrows=1, nspans=3, nregions=2, row_ptr=[0, 3], col_lo=[0, 1, 5], col_hi=[9, 2, 7],
               region=[0, 1, 0])
    assert check(shim, rs, **far) == (RULES["overlap"], 2)
    far["col_lo"], far["col_hi"] = [0, 1, 9], [9, 2, 12]
    assert check(shim, rs, **far) == (RULES["ok"], 0)


def test_python_arguments_without_a_device():
    rs = RegionSet.from_rects([(6, 0, 4, 0, 4), (6, 2, 9, 2, 9)])
    assert S._check_regions(rs, 0, 10) is rs
    for bad in (None, [(6, 0, 4, 0, 4)], "rs"):
        with pytest.raises(ValueError, match="RegionSet"):
            S._check_regions(bad, 0, 10)
    with pytest.raises(ValueError, match="zoom"):
        S._check_regions(rs, 7, 10)
    with pytest.raises(ValueError, match="zoom"):
        S._check_regions(rs, 0, 5)
    index = {"all": 0, "u1": 1, "route": 2}
    assert S._region_series_args(rs, (10, 22), 1, None, index) == (10, 22, 1, 12, _lib.HM_VIEW_MERGED)
    assert S._region_series_args(rs, (10, 22), 5, "route", index) == (10, 22, 5, 3, 2)
    assert S._region_series_args(rs, (10, 22), 12, "nobody", index) == (10, 22, 12, 1, None)
    with pytest.raises(ValueError, match="hour_lo < hour_hi"):
        S._region_series_args(rs, (10, 10), 1, None, index)
    with pytest.raises(ValueError, match="frame_hours"):
        S._region_series_args(rs, (10, 22), 0, None, index)
    with pytest.raises(ValueError, match="'all'"):
        S._region_series_args(rs, (10, 22), 1, "all", index)
    with pytest.raises(ValueError, match="group label"):
        S._region_series_args(rs, (10, 22), 1, 3, index)
    with pytest.raises(ValueError, match="totals"):
        S._region_series_args(rs, (0, _lib.HM_REGION_MAX_TOTALS // 2 + 1), 1, None, index)
    assert S._region_series_args(rs, (0, _lib.HM_REGION_MAX_TOTALS // 2), 1, None, index)[3] == 1 << 21
    st, keep = S._region_struct(rs)
    assert (st.zoom, st.row_lo, st.nrows, st.nspans, st.nregions) == (6, 0, 9, rs.nspans, 2)
    assert [st.col_lo[j] for j in range(rs.nspans)] == rs.col_lo.tolist()
    assert [st.row_ptr[j] for j in range(rs.nrows + 1)] == rs.row_ptr.tolist()


def test_header_and_exports_have_the_entry_points():
    text = open(os.path.join(REPO, "include", "heatmap_amd.h")).read()
    for fn in ("hm_stream_region_series", "hm_stream_region_view", "hm_stream_region_visitors"):
        assert re.search(r"\bint %s\(hm_stream\* s," % fn, text), fn
        assert fn in _lib.EXPORTS
    assert "typedef struct hm_regions" in text
    assert re.search(r"#define HM_ABI_VERSION 7\b", text)
    fields = [f[0] for f in _lib.hm_regions._fields_]
    assert fields == ["zoom", "row_lo", "nrows", "nspans", "nregions", "row_ptr", "col_lo", "col_hi", "region"]
