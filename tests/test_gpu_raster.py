"""hm_cells_raster and hm_raster_render against the model (tests/raster_model.py)
on explicit cells and grids, so every edge is placed and not left to a cloud:
bins, halos, clipped corners, overlaps, selection, counts, argument errors;
impulses at the halo's and the interior's edges and on both sides of every
edge of the blur kernel's 32 x 32 block tiling; seams, scales, the width limit
per radius and the LUT.  Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import raster_model as model
from heatmap_amd import _lib, device, raster

pytestmark = pytest.mark.gpu
BLOCK = 32   # csrc/hm_pipeline.h HM_BLUR_BLOCK: outputs per side of a blur block


def _keys(cells):
    return np.array([(z << 58) | (r << 29) | c for z, r, c, _ in cells], dtype=np.uint64)


def _counts(cells):
    return np.array([n for _, _, _, n in cells], dtype=np.uint64)


def _scatter(cells, tiles, b, h):
    g = raster.raster_cells(_keys(cells), _counts(cells), tiles, b, h)
    w = (1 << b) + 2 * h
    assert tuple(g.shape) == (len(tiles), w, w)
    return g.cpu().numpy()


def _same(got, want):
    assert np.array_equal(np.asarray(got).astype(object), np.asarray(want).astype(object))


def _tile_cells(tz, tr, tc, b, h, seed):
    """cells on and around every edge of tile (tz, tr, tc)'s haloed square, its
    corners and a few random bins, some outside the square of the zoom"""
    z, s = tz + b, 1 << b
    rng = np.random.default_rng(seed)
    edges_r = [(tr << b) + d for d in (-h - 1, -h, -1, 0, s - 1, s, s + h - 1, s + h)]
    edges_c = [(tc << b) + d for d in (-h - 1, -h, -1, 0, s - 1, s, s + h - 1, s + h)]
    cells = [(z, r, c, int(rng.integers(1, 1000))) for r in edges_r for c in edges_c]
    cells += [(z, (tr << b) + int(rng.integers(-h, s + h)), (tc << b) + int(rng.integers(-h, s + h)),
               int(rng.integers(1, 1000))) for _ in range(40)]
    return [c for c in cells if 0 <= c[1] < (1 << 29) and 0 <= c[2] < (1 << 29)]


# ---------------------------------------------------------------- scatter

@pytest.mark.parametrize("b", [0, 1, 5, 8])
@pytest.mark.parametrize("h", [0, 1, 8])
def test_scatter_bins_halo_and_corners(gpu, b, h):
    """every bins_log2 x halo (halo > S included), the tile at each corner of
    the square (the halo is clipped there) and one inside; keys whose row or
    column is outside [0, 2^z) are never drawn"""
    tz = 3
    last = (1 << tz) - 1
    tiles = [(tz, 0, 0), (tz, 0, last), (tz, last, 0), (tz, last, last), (tz, 2, 5)]
    cells = []
    for j, t in enumerate(tiles):
        cells += _tile_cells(*t, b, h, seed=100 * b + 10 * h + j)
    side = 1 << (tz + b)
    assert any(c[1] >= side or c[2] >= side for c in cells) or h == 0
    want = model.densify(cells, tiles, b, h)
    assert all(want[t].any() for t in range(len(tiles)))
    _same(_scatter(cells, tiles, b, h), want)


@pytest.mark.parametrize("zoom", [0, 3, 8])
def test_scatter_whole_world(gpu, zoom):
    """tz = 0 with bins_log2 = zoom: the whole square, the halo all outside it"""
    rng = np.random.default_rng(zoom)
    side = 1 << zoom
    cells = [(zoom, int(r), int(c), int(n)) for r, c, n in
             zip(rng.integers(0, side, 50), rng.integers(0, side, 50), rng.integers(1, 99, 50))]
    cells += [(zoom, 0, 0, 3), (zoom, side - 1, side - 1, 4), (zoom, 0, side - 1, 5), (zoom, side - 1, 0, 6)]
    for h in (0, 2):
        got = _scatter(cells, [(0, 0, 0)], zoom, h)
        _same(got, model.densify(cells, [(0, 0, 0)], zoom, h))
        assert got.sum() == sum(c[3] for c in cells)
        if h:
            assert not got[0, :h].any() and not got[0, -h:].any() and not got[0, :, :h].any() and not got[0, :, -h:].any()


def test_scatter_overlap_repeat_zooms_and_selection(gpu):
    """a cell at the shared corner of four listed neighbours lands in all four
    (halo 1); a repeated tile has its own equal grid; tiles of three zooms in
    one call; cells of unlisted zooms and just outside a halo are ignored"""
    b, h = 4, 1
    tiles = [(5, 10, 10), (5, 10, 11), (5, 11, 10), (5, 11, 11), (5, 10, 10), (3, 2, 2), (7, 40, 41)]
    cr, cc = 11 << b, 11 << b                      # first bin of tile (5, 11, 11)
    cells = [(9, cr - 1, cc - 1, 7), (9, cr, cc, 11), (9, cr - 1, cc, 13), (9, cr, cc - 1, 17),
             (9, cr - 2, cc - 2, 100),             # inside (10, 10) only
             (9, (10 << b) - 2, 10 << b, 1000),    # just outside (10, 10)'s halo: in no listed tile
             (9, 12 << b, (12 << b) + 1, 1000),    # just outside (11, 11)'s halo
             (8, cr >> 1, cc >> 1, 5000), (10, cr << 1, cc << 1, 5000), (21, 5, 5, 1),   # unlisted zooms
             (7, 2 << b, 2 << b, 21), (7, (3 << b) + 1, 2 << b, 1000), (7, (3 << b), (3 << b), 23),
             (11, 40 << b, 41 << b, 29), (11, (40 << b) - 1, (42 << b), 31), (11, (40 << b) - 2, 41 << b, 1000)]
    got = _scatter(cells, tiles, b, h)
    _same(got, model.densify(cells, tiles, b, h))
    assert [int(got[t].sum()) for t in range(7)] == [148, 48, 48, 48, 148, 44, 60]
    assert np.array_equal(got[0], got[4])


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 5000])
def test_scatter_counts_add(gpu, n):
    """n around the 2048-key chunk of a block; repeated keys add; counts above 2^32"""
    rng = np.random.default_rng(n)
    b, h, tiles = 3, 1, [(2, 1, 1), (2, 1, 2)]
    r = rng.integers(6, 20, n)
    c = rng.integers(6, 28, n)
    cnt = rng.integers(1, 1 << 40, n)
    cells = list(zip([5] * n, r.tolist(), c.tolist(), cnt.tolist()))
    want = model.densify(cells, tiles, b, h)
    if n >= 2047:
        assert len(set(cells)) > 50 and len({x[:3] for x in cells}) < n // 4   # keys repeat
        assert max(int(v) for v in want.reshape(-1)) > 1 << 32
    _same(_scatter(cells, tiles, b, h), want)


def _raw_cells(ctx, keys, counts, n, tiles, ntiles, b, h, grid, ctx_ptr=True):
    flat = [int(v) for t in tiles or [] for v in t] or [0]
    ta = (ctypes.c_int64 * len(flat))(*flat) if tiles is not None else None
    return ctx.L.hm_cells_raster(ctx.ptr if ctx_ptr else None, device._ptr(keys), device._ptr(counts), n, ta, ntiles, b, h,
                                 device._ptr(grid))


def test_scatter_limits_and_errors(gpu):
    """the call zeroes the grid itself; 64 tiles are fine; 65 tiles and every
    other HM_E_ARG case leave the buffer untouched"""
    torch = gpu
    ctx = device.context(0)
    b, h = 2, 1
    w = (1 << b) + 2 * h
    cells = [(6, 17, 18, 5), (6, 19, 20, 9)]        # the second one in the halos of four tiles
    keys = torch.from_numpy(_keys(cells).view(np.int64)).cuda()
    counts = torch.from_numpy(_counts(cells).view(np.int64)).cuda()
    tiles = [(4, t // 8, t % 8) for t in range(64)]

    def pattern(nt):
        return torch.full((nt, w, w), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")

    g = pattern(64)
    assert _raw_cells(ctx, keys, counts, 2, tiles, 64, b, h, g) == _lib.HM_OK
    want = model.densify(cells, tiles, b, h)
    _same(g.cpu().numpy(), want)
    assert int(g.sum()) > 0 and int((g == 0).sum()) > 64 * w * w - 20
    # n = 0: an all-zero grid
    g = pattern(1)
    assert _raw_cells(ctx, keys, counts, 0, tiles[:1], 1, b, h, g) == _lib.HM_OK and not g.any()
    # the python wrapper splits more than 64 tiles
    many = tiles + [(4, 4, 4)] * 6
    _same(raster.raster_cells(keys, counts, many, b, h).cpu().numpy(), model.densify(cells, many, b, h))
    g = pattern(65)
    ref = g.clone()
    bad = [
        dict(tiles=tiles + [(4, 0, 0)], ntiles=65), dict(ntiles=0), dict(ntiles=-1), dict(b=-1), dict(b=9), dict(h=-1),
        dict(h=9), dict(tiles=[(-1, 0, 0)]), dict(tiles=[(4, 16, 0)]), dict(tiles=[(4, 0, 16)]),
        dict(tiles=[(4, -1, 0)]), dict(tiles=[(4, 0, -1)]), dict(tiles=[(20, 0, 0)]), dict(tiles=[(22, 0, 0)], b=0),
        dict(tiles=[(4, 0, 0), (4, 0, 16)], ntiles=2), dict(tiles=None), dict(n=-1), dict(ctx_ptr=False),
    ]
    for kw in bad:
        a = dict(keys=keys, counts=counts, n=2, tiles=[(4, 0, 0)], ntiles=1, b=b, h=h, grid=g, ctx_ptr=True)
        a.update(kw)
        assert _raw_cells(ctx, **a) == _lib.HM_E_ARG, kw
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert _raw_cells(ctx, empty, counts, 2, [(4, 0, 0)], 1, b, h, g) == _lib.HM_E_ARG      # null keys
    assert _raw_cells(ctx, keys, empty, 2, [(4, 0, 0)], 1, b, h, g) == _lib.HM_E_ARG        # null counts
    assert _raw_cells(ctx, keys, counts, 2, [(4, 0, 0)], 1, b, h, empty) == _lib.HM_E_ARG   # null grid
    torch.cuda.synchronize()
    assert torch.equal(g, ref)


# ----------------------------------------------------------------- render

def _render(grid, b, h, r, scale="log", vmax=None, lut="gray"):
    """device (levels, vs, rgba) of a numpy grid"""
    import torch

    g = torch.from_numpy(np.asarray(grid).astype(np.int64)).cuda()
    rgba, vs, lev = raster.render(g, b, h, r, scale, vmax, lut, levels=True)
    return lev.cpu().numpy(), vs, rgba.cpu().numpy()


def _check_render(grid, b, h, r, scale="log", vmax=None):
    lev, vs, rgba = _render(grid, b, h, r, scale, vmax)
    mlev, mvs, mrgba = model.render(grid, b, h, r, scale, vmax, raster.RAMPS["gray"])
    assert vs == mvs
    assert np.array_equal(lev, mlev)
    assert np.array_equal(rgba, mrgba)
    return lev, vs


def _edge_positions(b, h):
    """haloed-grid coordinates of: the halo's outermost and innermost bins, the
    interior's first and last, and both sides of every edge of the blur
    kernel's block tiling (interior multiples of BLOCK)"""
    s = 1 << b
    p = {0, 2 * h + s - 1, h, h + s - 1} | ({h - 1, h + s} if h else set())
    for e in range(BLOCK, s, BLOCK):
        p |= {h + e - 1, h + e}
    return sorted(p)


@pytest.mark.parametrize("r", [0, 1, 2, 8])
@pytest.mark.parametrize("b", [5, 6])
def test_render_impulses(gpu, b, r):
    """one grid with an impulse of its own weight at every pair of edge
    positions (S = 32: one block; S = 64: 2 x 2 blocks), halo 8"""
    h = 8
    pos = _edge_positions(b, h)
    assert (h + 31 in pos and h + 32 in pos) if b == 6 else (h + 31 in pos)
    w = (1 << b) + 2 * h
    g = np.zeros((1, w, w), dtype=np.int64)
    for i, y in enumerate(pos):
        for j, x in enumerate(pos):
            g[0, y, x] = 1 + 37 * i + 5 * j
    for scale in ("log", "linear"):
        lev, _ = _check_render(g, b, h, r, scale)
        assert lev.any()


@pytest.mark.parametrize("b,h,r", [(0, 8, 8), (0, 0, 0), (1, 1, 1), (3, 8, 2), (8, 2, 2), (8, 0, 0), (7, 8, 8)])
def test_render_single_impulses_and_shapes(gpu, b, h, r):
    """a lone count 1 at the first interior bin and one in the halo's corner:
    every tile size from one bin to 8 x 8 blocks"""
    w = (1 << b) + 2 * h
    g = np.zeros((2, w, w), dtype=np.int64)
    g[0, h, h] = 1
    g[1, 0, 0] = 1
    g[1, w - 1, w - 1] = 3
    lev, vs = _check_render(g, b, h, r)
    assert lev[0, 0, 0] >= 1 and vs >= 1


def test_render_dense_random(gpu):
    rng = np.random.default_rng(5)
    b, h, r = 7, 4, 3
    w = (1 << b) + 2 * h
    g = rng.integers(0, 1 << 20, (3, w, w))
    g[rng.random(g.shape) < 0.5] = 0
    for scale in ("log", "linear"):
        _check_render(g, b, h, r, scale)
    _check_render(g, b, h, r, "log", vmax=1 << 18)


def test_render_seamless(gpu):
    """two adjacent tiles rendered in separate calls with a fixed vmax equal
    the model's render of the 2-tile mosaic, cut in two"""
    b, h, r = 5, 2, 2
    s = 1 << b
    rng = np.random.default_rng(9)
    tiles = [(4, 7, 3), (4, 7, 4)]
    r0, c0 = (7 << b) - h, (3 << b) - h
    cells = [(9, r0 + int(y), c0 + int(x), int(n)) for y, x, n in
             zip(rng.integers(0, s + 2 * h, 300), rng.integers(0, 2 * s + 2 * h, 300), rng.integers(1, 50, 300))]
    cells += [(9, r0 + h + 5, c0 + h + s - 1, 40), (9, r0 + h + 9, c0 + h + s, 45)]    # on both sides of the seam
    mosaic = np.zeros((1, s + 2 * h, 2 * s + 2 * h), dtype=np.int64)
    for _, y, x, n in cells:
        mosaic[0, y - r0, x - c0] += n
    vmax = 60
    B = model.blur(mosaic, b, h, r)
    want = np.array([[model.level(v, vmax << (4 * r), r, "log") for v in row] for row in B[0]], dtype=np.uint8)
    assert want[:, s - 3:s + 3].any()
    grids = raster.raster_cells(_keys(cells), _counts(cells), tiles, b, h)
    for t in range(2):
        rgba, vs, lev = raster.render(grids[t:t + 1], b, h, r, "log", vmax, "gray", levels=True)
        assert vs == vmax << (4 * r)
        assert np.array_equal(lev[0].cpu().numpy(), want[:, t * s:(t + 1) * s])


def test_render_scale(gpu):
    b, h = 4, 2
    w = (1 << b) + 2 * h
    g = np.zeros((2, w, w), dtype=np.int64)
    g[0, h + 3, h + 3] = 10
    g[1, h + 8, h + 8] = 40
    g[1, 0, 0] = 1 << 30                           # the halo's corner: beyond radius 1 of any interior bin
    # auto vmax: the interior maximum of B over every tile of the call; the halo's value does not enter
    for scale in ("linear", "log"):
        lev, vs = _check_render(g, b, h, 1, scale)
        assert vs == 40 * 4 and lev.max() == 255 and lev[1, 8, 8] == 255 and lev[0, 3, 3] < 255
    # ... unless the blur carries it inside (radius 2 reaches interior bin 0 from halo bin 0)
    lev, vs = _check_render(g, b, h, 2)
    assert vs == (1 << 30) and lev[1, 0, 0] == 255
    # a fixed vmax below the data saturates
    for scale in ("linear", "log"):
        lev, vs = _check_render(g, b, h, 0, scale, vmax=5)
        assert vs == 5 and lev[0, 3, 3] == 255 and lev[1, 8, 8] == 255
    # vs == 0: all zeros, every pixel lut[0]
    z = np.zeros((1, w, w), dtype=np.int64)
    for scale in ("linear", "log"):
        lev, vs, rgba = _render(z, b, h, 2, scale)
        assert vs == 0 and not lev.any() and not rgba.any()
    # the LOG denominator clamp: a lone count 1 at radius 4 has Q(vs) = 0
    b, h = 4, 4
    one = np.zeros((1, 24, 24), dtype=np.int64)
    one[0, 12, 12] = 1
    lev, vs = _check_render(one, b, h, 4, "log")
    assert vs == 70 * 70 and lev[0, 8, 8] == 255 and lev[0, 4, 4] == 1
    # ... in the halo's corner only its weakest tail (weight 1 of 2^16) reaches the interior: Q(vs) = 0
    one[...] = 0
    one[0, 0, 0] = 1
    assert model.Q(1, 4) == 0
    lev, vs = _check_render(one, b, h, 4, "log")
    assert vs == 1 and lev[0, 0, 0] == 1 and int(lev.sum()) == 1
    lev, vs = _check_render(one, b, h, 4, "linear")
    assert lev[0, 0, 0] == 255


@pytest.mark.parametrize("r", [0, 8])
def test_render_width(gpu, r):
    """max g = 2^(56 - 4R) - 1 passes and equals the model; 2^(56 - 4R) is
    HM_E_WIDE with the outputs untouched, wherever in the halo it sits"""
    torch = gpu
    b, h = 3, 8
    w = (1 << b) + 2 * h
    lim = 1 << (56 - 4 * r)
    g = np.zeros((2, w, w), dtype=np.int64)
    g[0, h + 2, h + 2] = lim - 1
    g[1, 0, w - 1] = lim - 1
    g[1, h + 4, h + 4] = 12345
    for scale in ("linear", "log"):
        lev, vs = _check_render(g, b, h, r, scale)
        assert lev[0].max() == 255
        _check_render(g, b, h, r, scale, vmax=lim - 1)
    ctx = device.context(0)
    lut = raster._lut("gray", torch, torch.device("cuda:0"))
    for y, x in ((h + 2, h + 2), (0, w - 1), (w - 1, 0)):
        g2 = g.copy()
        g2[1, y, x] = lim
        gt = torch.from_numpy(g2).cuda()
        with pytest.raises(OverflowError):
            raster.render(gt, b, h, r)
        rgba = torch.full((2, 8, 8, 4), 0xA5, dtype=torch.uint8, device="cuda")
        lev = torch.full((2, 8, 8), 0xA5, dtype=torch.uint8, device="cuda")
        used = ctypes.c_uint64(77)
        rc = ctx.L.hm_raster_render(ctx.ptr, device._ptr(gt), 2, b, h, r, _lib.HM_SCALE_LOG, 0, device._ptr(lut),
                                    device._ptr(rgba), device._ptr(lev), ctypes.byref(used))
        assert rc == _lib.HM_E_WIDE and used.value == 77
        assert (rgba == 0xA5).all() and (lev == 0xA5).all()


def test_render_errors(gpu):
    torch = gpu
    ctx = device.context(0)
    b, h = 3, 2
    gt = torch.zeros((1, 12, 12), dtype=torch.int64, device="cuda")
    lut = raster._lut("gray", torch, torch.device("cuda:0"))
    rgba = torch.full((1, 8, 8, 4), 0xA5, dtype=torch.uint8, device="cuda")
    lev = torch.full((1, 8, 8), 0xA5, dtype=torch.uint8, device="cuda")
    none = torch.zeros(0, dtype=torch.uint8, device="cuda")

    def call(ctxp=ctx.ptr, grid=gt, nt=1, b=b, h=h, r=1, scale=_lib.HM_SCALE_LOG, vmax=0, lut=lut, rgba=rgba):
        return ctx.L.hm_raster_render(ctxp, device._ptr(grid), nt, b, h, r, scale, vmax, device._ptr(lut),
                                      device._ptr(rgba), device._ptr(lev), None)

    assert call() == _lib.HM_OK and not rgba.any() and not lev.any()   # vmax_used may be NULL
    rgba.fill_(0xA5), lev.fill_(0xA5)
    for kw in (dict(ctxp=None), dict(grid=none), dict(lut=none), dict(rgba=none), dict(nt=0), dict(nt=65), dict(b=-1),
               dict(b=9), dict(h=-1), dict(h=9), dict(r=-1), dict(r=3), dict(scale=2), dict(scale=-1),
               dict(vmax=1 << 52), dict(r=0, vmax=1 << 56), dict(r=2, vmax=1 << 48)):
        assert call(**kw) == _lib.HM_E_ARG, kw
    assert call(vmax=(1 << 52) - 1) == _lib.HM_OK
    rgba.fill_(0xA5)
    assert call(r=3) == _lib.HM_E_ARG
    torch.cuda.synchronize()
    assert (rgba == 0xA5).all()


def test_colour_lut(gpu):
    """rgba == lut[levels] for a LUT of 256 distinct words, bytes R, G, B, A"""
    rng = np.random.default_rng(3)
    lut = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256, (np.arange(256) * 13 + 5) % 256],
                   axis=1).astype(np.uint8)
    assert len({tuple(x) for x in lut.tolist()}) == 256
    b, h = 6, 1
    g = (2.0 ** rng.uniform(0, 40, (2, 66, 66))).astype(np.int64)   # every magnitude, so every level
    g[rng.random(g.shape) < 0.9] = 0
    lev, vs, rgba = _render(g, b, h, 1, "log", None, lut)
    assert len(np.unique(lev)) > 100 and 0 in lev
    assert np.array_equal(rgba, lut[lev])
    mlev, mvs, mrgba = model.render(g, b, h, 1, "log", None, lut)
    assert vs == mvs and np.array_equal(lev, mlev) and np.array_equal(rgba, mrgba)
    for name in ("heat", "gray"):
        assert np.array_equal(_render(g, b, h, 1, "log", None, name)[2], raster.RAMPS[name][lev])
