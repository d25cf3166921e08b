"""csrc/hm_stream_rect.h on the CPU: the id range and column window that
hm_stream_view and hm_stream_raster hand their filter kernels for a rectangle,
against a brute-force enumeration of the pyramid cell ids
(4^z - 1)/3 + (row << z) + col.  The header is plain C: a shim around it is
built here with the host compiler."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")
SHIM = """
#include "hm_stream_rect.h"
void rect_ids(int z, int64_t rlo, int64_t rhi, int64_t clo, int64_t chi, uint64_t* box, uint64_t* out)
{
    HmsRectIds r = hms_rect_ids(z, rlo, rhi, clo, chi, &box[0], &box[1]);
    out[0] = r.id_lo;
    out[1] = r.span;
    out[2] = r.col_lo;
    out[3] = r.col_w;
}
"""


@pytest.fixture(scope="module")
def rect_ids(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_rect")
    src, lib = d / "shim.c", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                    str(src), "-o", str(lib)], check=True)
    fn = ctypes.CDLL(str(lib)).rect_ids
    fn.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_uint64)] * 2
    fn.restype = None

    def call(z, rect, box):
        """(id_lo, span, col_lo, col_w) of the clipped rect; box = [lo, hi] is updated in place"""
        b, out = (ctypes.c_uint64 * 2)(*box), (ctypes.c_uint64 * 4)()
        fn(z, *rect, b, out)
        box[:] = [b[0], b[1]]
        return tuple(out)

    return call


def off(z):
    return (4 ** z - 1) // 3


def clip(z, rlo, rhi, clo, chi):
    """The rectangle clipped to [0, 2^z)^2 as the two entry points do, or None"""
    rlo, clo, rhi, chi = max(rlo, 0), max(clo, 0), min(rhi, 1 << z), min(chi, 1 << z)
    return (rlo, rhi, clo, chi) if rhi > rlo and chi > clo else None


def halo_rect(z, tr, tc, bins_log2, halo):
    """hm_stream_raster's haloed square of tile (z - bins_log2, tr, tc), before clipping"""
    w = (1 << bins_log2) + 2 * halo
    oy, ox = (tr << bins_log2) - halo, (tc << bins_log2) - halo
    return (oy, oy + w, ox, ox + w)


def selected(z, ids, got):
    """Of the ids (an array inside the helper's range), those its column window keeps"""
    id_lo, span, col_lo, col_w = got
    assert ((ids >= id_lo) & (ids < id_lo + span)).all()
    col = (ids - off(z)) & ((1 << z) - 1)
    return ids[(col >= col_lo) & (col < col_lo + col_w)]


def rects_of(z):
    """Unclipped rectangles of zoom z: inside, on each edge, covering, and pushed
    past the origin and the far edges by a halo"""
    s = 1 << z
    out = [(0, s, 0, s), (-3, s + 3, -3, s + 3), (0, 1, 0, s), (s - 1, s, 0, s), (0, s, 0, 1), (0, s, s - 1, s)]
    if z >= 2:
        out += [(1, s - 1, 1, s - 1), (1, 2, s // 2, s // 2 + 1), (s // 4, s // 2 + 1, 1, 3)]
        for b in (1, 2):
            t = (1 << (z - b)) - 1
            out += [halo_rect(z, 0, 0, b, 3), halo_rect(z, t, t, b, 3), halo_rect(z, 0, t, b, 1),
                    halo_rect(z, t, 0, b, 8)]
    return out


@pytest.mark.parametrize("z", [0, 1, 2, 5])
def test_every_id_of_the_range(rect_ids, z):
    """Small zooms, every rectangle: the ids of [id_lo, id_lo + span) whose
    column is in the window are exactly the rectangle's cells."""
    for rect in rects_of(z):
        c = clip(z, *rect)
        assert c is not None
        rlo, rhi, clo, chi = c
        got = rect_ids(z, c, [2 ** 64 - 1, 0])
        want = sorted(off(z) + (r << z) + q for r in range(rlo, rhi) for q in range(clo, chi))
        ids = np.arange(got[0], got[0] + got[1], dtype=np.int64)
        assert selected(z, ids, got).tolist() == want, (z, rect)
        # the range is whole rows: it starts and ends where rows do, inside zoom z
        assert got[0] == off(z) + (rlo << z) and got[0] + got[1] == off(z) + (rhi << z) <= off(z + 1)


def test_spot_rows_at_zoom_21(rect_ids):
    """Zoom 21 (2^21 cells a row, ids up to 2^43): the range's edges, and every
    id of its first, a middle and its last row."""
    z, s = 21, 1 << 21
    t = (1 << 13) - 1
    for rect in [(0, s, 0, s), (5, 9, 7, 11), (s - 2, s + 6, s - 3, s + 5), (-8, 2, -8, 3), (12345, 12350, 0, 1),
                 (0, 3, s - 1, s), halo_rect(z, 0, t, 8, 8), halo_rect(z, t, 0, 8, 8), halo_rect(z, 4000, 4001, 8, 2)]:
        rlo, rhi, clo, chi = c = clip(z, *rect)
        got = rect_ids(z, c, [2 ** 64 - 1, 0])
        assert got[0] == off(z) + (rlo << z) and got[1] == (rhi - rlo) << z and got[0] + got[1] <= off(z + 1)
        for r in {rlo, (rlo + rhi) // 2, rhi - 1}:
            ids = off(z) + (r << z) + np.arange(s, dtype=np.int64)
            want = off(z) + (r << z) + np.arange(clo, chi, dtype=np.int64)
            assert np.array_equal(selected(z, ids, got), want), (rect, r)


def test_box_over_several_rectangles(rect_ids):
    """The running box holds every rectangle's id range and no more: from the
    smallest first-row id to one past the largest last-row id, in any order."""
    rects = [(5, (3, 9, 30, 40)), (2, (0, 4, 0, 4)), (21, halo_rect(21, 0, 0, 8, 8)), (5, (-2, 1, -2, 1)),
             (1, (1, 2, 0, 1))]
    for order in (rects, rects[::-1], rects[2:] + rects[:2]):
        box, lo, hi = [2 ** 64 - 1, 0], [], []
        for z, rect in order:
            rlo, rhi, clo, chi = c = clip(z, *rect)
            rect_ids(z, c, box)
            lo.append(off(z) + (rlo << z))
            hi.append(off(z) + ((rhi - 1) << z) + (1 << z) - 1)
            assert box == [min(lo), max(hi) + 1]
    assert box == [off(1) + 2, off(21) + (264 << 21)]
