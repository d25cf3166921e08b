"""Rasters of the resident streaming heatmap (hm_stream_raster,
StreamingHeatmap.tile_raster / tile_images) vs the oracle: a raster equals one
oracle count over the selected points (hours, group) densified by the model
(tests/raster_model.py), and equals hm_cells_raster of the view of the same
rectangles.  The tiles sit on the oracle's heaviest cells and the expected
grids are asserted non-zero.

The streams are those of tests/test_gpu_stream_view.py: the main one holds well
over 4 x 8192 cells (several blocks and a ragged last chunk), the tiny one is
one partial chunk, the zooms 6-12 one has pyramid offsets that do not start at 0."""
import ctypes

import numpy as np
import pytest

import raster_model as model
from oracle import oracle
from heatmap_amd import _lib, device, raster, synth
from heatmap_amd.stream import StreamingHeatmap
from test_gpu_stream_view import BASE, ZMAX, ZMIN, Data, _heaviest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def main(gpu, data):
    """the main stream with user groups; the tests that use it leave it as it is"""
    s = data.stream()
    assert s.cells()[0] > 4 * 8192
    yield s
    s.close()


def _expect(ref, tiles, b, h):
    assert ref["status"] == 0
    return model.densify_arrays(ref["zoom"], ref["row"], ref["col"], ref["count"], tiles, b, h)


def _tiles_on(ref, b):
    """the tile of zoom 18 - b that holds the oracle's heaviest zoom-18 cell,
    two of its neighbours (the halos overlap), and the tile of zoom 13 - b on
    the heaviest zoom-13 cell: two zooms in one call"""
    r, c = _heaviest(ref, 18)
    tz = 18 - b
    tr, tc = r >> b, c >> b
    nr, nc = (tr + 1 if tr + 1 < (1 << tz) else tr - 1), (tc + 1 if tc + 1 < (1 << tz) else tc - 1)
    r13, c13 = _heaviest(ref, 13)
    return [(tz, tr, tc), (tz, tr, nc), (tz, nr, nc), (13 - b, r13 >> b, c13 >> b)]


def _halo_rects(tiles, b, h):
    w = (1 << b) + 2 * h
    return [(tz + b, (tr << b) - h, (tr << b) - h + w, (tc << b) - h, (tc << b) - h + w) for tz, tr, tc in tiles]


SELECTIONS = {
    "alltime": (None, None),
    "window": ((BASE + 4, BASE + 8), None),
    "one_hour": ((BASE + 5, BASE + 6), None),
    "one_group": (None, "u2"),
    "group_window": ((BASE + 4, BASE + 8), "u3"),
}


@pytest.mark.parametrize("sel", sorted(SELECTIONS))
@pytest.mark.parametrize("b,h", [(5, 2), (3, 8)])
def test_equals_the_oracle_and_the_view(main, data, sel, b, h):
    hours, user = SELECTIONS[sel]
    lo, hi = hours or (BASE, BASE + 18)
    ref = data.ref(lo, hi, None if user is None else data.users == user)
    tiles = _tiles_on(ref, b)
    want = _expect(ref, tiles, b, h)
    assert want[0].any() and want[3].any() and (want[0] != want[1]).any()
    got = main.tile_raster(tiles, hours, user, bins_log2=b, halo=h)
    assert str(got.dtype) == "torch.int64" and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    # the same grids from the view's cells of the same (haloed) rectangles
    n, keys, counts, _ = main.view_device(_halo_rects(tiles, b, h), hours,
                                          "merged" if user is None else main.labels.index(user))
    assert n > 0
    again = raster.raster_cells(keys[:n], counts[:n], tiles, b, h)
    assert np.array_equal(again.cpu().numpy(), want)


def test_late_batch_and_undated_cells(gpu, data):
    """a log that needs adding: a late batch of old hours (its keys repeat in
    the log, which is not compacted by the query) and undated cells, which
    count in alltime only"""
    s = data.stream()
    lat0, lon0, keep0, hour0, us0 = data.batches[0]
    lat1, lon1, keep1, _, us1 = data.batches[1]
    s.add(lat0, lon0, keep0, hour0, user_id=us0)          # the same points again, hours already in the log
    s.add(lat1, lon1, keep1, None, user_id=us1)           # undated
    try:
        dated = oracle.count(np.concatenate([data.lat, lat0]), np.concatenate([data.lon, lon0]),
                             np.concatenate([data.keep, keep0]), ZMIN, ZMAX)
        every = oracle.count(np.concatenate([data.lat, lat0, lat1]), np.concatenate([data.lon, lon0, lon1]),
                             np.concatenate([data.keep, keep0, keep1]), ZMIN, ZMAX)
        b, h = 5, 1
        tiles = _tiles_on(every, b)
        want_all, want_dated = _expect(every, tiles, b, h), _expect(dated, tiles, b, h)
        assert want_all[0].any() and (want_all != want_dated).any()
        assert (want_dated[0] > _expect(data.ref(), tiles, b, h)[0]).any()      # the late batch added to bins
        assert np.array_equal(s.tile_raster(tiles, None, None, b, h).cpu().numpy(), want_all)
        assert np.array_equal(s.tile_raster(tiles, (BASE, BASE + 18), None, b, h).cpu().numpy(), want_dated)
        # one group, with the late batch in it
        m = np.concatenate([data.users, np.array(us0)]) == "u1"
        ref = oracle.count(np.concatenate([data.lat, lat0]), np.concatenate([data.lon, lon0]),
                           (np.concatenate([data.keep, keep0]) & m).astype(np.uint8), ZMIN, ZMAX)
        assert np.array_equal(s.tile_raster(tiles, (BASE, BASE + 18), "u1", b, h).cpu().numpy(),
                              _expect(ref, tiles, b, h))
    finally:
        s.close()


def test_the_stream_is_left_as_it_is(main, data):
    before = (main.cells(), main.buckets())
    tiles = _tiles_on(data.ref(), 5)
    for hours, user in SELECTIONS.values():
        main.tile_raster(tiles, hours, user, 5, 2)
    main.tile_images(tiles[:1], (BASE + 2, BASE + 9), None, bins_log2=5, radius=1)
    gpu_sync()
    assert (main.cells(), main.buckets()) == before


def gpu_sync():
    import torch

    torch.cuda.synchronize()


def test_tiny_stream(gpu):
    """50 points: one partial chunk of one block; an empty stream: zero grids"""
    lat, lon = synth.generate("hotspots", 50, seed=3)
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE)
    try:
        tiles = [(0, 0, 0), (5, 3, 3)]
        assert not s.tile_raster(tiles, None, None, 4, 2).any()
        s.add(lat, lon, None, np.full(50, BASE + 1, np.uint32))
        ref = oracle.count(lat, lon, np.ones(50, np.uint8), ZMIN, ZMAX)
        for b in (0, 4, 8):
            r, c = _heaviest(ref, 10 + b)
            tiles = [(0, 0, 0), (10, r >> b, c >> b), (10, r >> b, c >> b)]
            want = _expect(ref, tiles, b, 2)
            assert want[0].any() and want[1].any() and np.array_equal(want[1], want[2])
            assert np.array_equal(s.tile_raster(tiles, None, None, b, 2).cpu().numpy(), want)
        # a window that holds nothing, and one outside the stream's hours
        assert not s.tile_raster(tiles, (BASE + 2, BASE + 3), None, 4, 2).any()
        assert not s.tile_raster(tiles, (BASE - 9, BASE - 1), None, 4, 2).any()
    finally:
        s.close()


def test_zooms_6_to_12_stream(gpu, data):
    """pyramid offsets that do not start at 0; bin zooms at both ends of the stream's range"""
    s = StreamingHeatmap(6, 12, base_hour=BASE)
    try:
        for lat, lon, keep, hour, _ in data.batches[:2]:
            s.add(lat, lon, keep, hour)
        n = 2 * len(data.batches[0][0])
        ref = oracle.count(data.lat[:n], data.lon[:n], data.keep[:n], 6, 12)
        for tz, b, h in ((7, 5, 2), (1, 5, 8), (4, 8, 1), (6, 0, 8), (12, 0, 3)):
            r, c = _heaviest(ref, tz + b)
            tiles = [(tz, r >> b, c >> b), (tz, 0, 0), (tz, (1 << tz) - 1, (1 << tz) - 1)]
            want = _expect(ref, tiles, b, h)
            assert want[0].any()
            assert np.array_equal(s.tile_raster(tiles, None, None, b, h).cpu().numpy(), want)
        for tiles, b in (([(0, 0, 0)], 5), ([(5, 0, 0)], 8), ([(13, 0, 0)], 0)):
            with pytest.raises(ValueError):
                s.tile_raster(tiles, None, None, b, 0)
    finally:
        s.close()


def test_user_selection(main, data):
    tiles = _tiles_on(data.ref(), 5)
    with pytest.raises(ValueError, match="tile_rows"):
        main.tile_raster(tiles, None, "all")
    for user in ("nobody", "xhidden"):                    # 'x...' ids make no group: no label either
        g = main.tile_raster(tiles, None, user, 5, 1)
        assert tuple(g.shape) == (4, 34, 34) and not g.any()


def test_seventy_tiles_split(main, data):
    ref = data.ref()
    r, c = _heaviest(ref, 16)
    b, h = 3, 1
    tr, tc = max((r >> b) - 3, 0), max((c >> b) - 5, 0)
    tiles = [(13, tr + i // 10, tc + i % 10) for i in range(70)]
    want = _expect(ref, tiles, b, h)
    assert want[:64].any() and want[64:].any()
    assert np.array_equal(main.tile_raster(tiles, None, None, b, h).cpu().numpy(), want)


@pytest.mark.parametrize("scale,vmax", [("log", None), ("linear", 40)])
def test_tile_images_end_to_end(main, data, scale, vmax):
    hours = (BASE + 2, BASE + 12)
    ref = data.ref(*hours)
    b, radius = 6, 2
    r, c = _heaviest(ref, 17)
    tiles = [(17 - b, r >> b, c >> b), (17 - b, r >> b, (c >> b) ^ 1)]
    grid = _expect(ref, tiles, b, radius)
    lev, _, rgba = model.render(grid, b, radius, radius, scale, vmax, raster.RAMPS["heat"])
    assert len(np.unique(lev)) > 3
    got = main.tile_images(tiles, hours, None, bins_log2=b, radius=radius, scale=scale, vmax=vmax)
    assert str(got.dtype) == "torch.uint8" and tuple(got.shape) == (2, 64, 64, 4)
    assert np.array_equal(got.cpu().numpy(), rgba)
    png = raster.png_bytes(got[0])
    assert png[:8] == b"\x89PNG\r\n\x1a\n"


def test_raw_errors_leave_the_grid_untouched(main, gpu):
    torch = gpu
    g = torch.full((2, 10, 10), 0x1234567, dtype=torch.int64, device="cuda")
    ref = g.clone()

    def call(lo=-1, hi=-1, group=_lib.HM_VIEW_MERGED, tiles=((5, 1, 1),), ntiles=1, b=3, h=1, s=main.ptr, grid=g):
        flat = [int(v) for t in tiles for v in t]
        ta = (ctypes.c_int64 * len(flat))(*flat)
        return main.ctx.L.hm_stream_raster(s, lo, hi, group, ta, ntiles, b, h, device._ptr(grid))

    for kw in (dict(group=_lib.HM_VIEW_EACH), dict(group=-3), dict(group=0xFFFFFFFF), dict(lo=BASE + 2, hi=BASE + 2),
               dict(lo=BASE + 3, hi=BASE + 2), dict(ntiles=0), dict(ntiles=65), dict(b=-1),
               dict(b=9), dict(h=-1), dict(h=9), dict(tiles=((-1, 0, 0),)), dict(tiles=((5, 32, 0),)),
               dict(tiles=((5, 0, -1),)), dict(tiles=((16, 0, 0),)), dict(tiles=((5, 1, 1), (5, 1, 32)), ntiles=2),
               dict(s=None), dict(grid=torch.zeros(0, dtype=torch.int64, device="cuda"))):
        assert call(**kw) == _lib.HM_E_ARG, kw
    torch.cuda.synchronize()
    assert torch.equal(g, ref)
    assert call(group=0xFFFFFFFE) == _lib.HM_OK           # the cells without a group
    assert call(lo=BASE - 50, hi=BASE - 40) == _lib.HM_OK
    torch.cuda.synchronize()
    assert not g[0].any() and torch.equal(g[1], ref[1])
