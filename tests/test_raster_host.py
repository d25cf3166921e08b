"""CPU: the raster model's own sanity (tests/raster_model.py is what the GPU
tests compare with) and the Python layer of heatmap_amd/raster.py that needs no
device: the argument helpers, the colour ramps and the PNG writer."""
import struct
import zlib

import numpy as np
import pytest

import raster_model as model
from heatmap_amd import _lib, raster
from heatmap_amd.stream import _raster_args


# ------------------------------------------------------------------ model

@pytest.mark.parametrize("radius", [0, 1, 2, 8])
def test_impulse_blurs_to_the_outer_product_of_the_weights(radius):
    b, h = 5, 8
    g = np.zeros((1, 32 + 2 * h, 32 + 2 * h), dtype=np.int64)
    g[0, h + 16, h + 16] = 1
    B = model.blur(g, b, h, radius)
    w = model.weights(radius)
    assert sum(w) == 1 << (2 * radius)
    want = np.zeros((32, 32), dtype=object)
    want[...] = 0
    for i, wi in enumerate(w):
        for j, wj in enumerate(w):
            want[16 - radius + i, 16 - radius + j] = wi * wj
    assert (B[0] == want).all()
    assert sum(int(v) for v in B.reshape(-1)) == 1 << (4 * radius)


def test_blur_reads_the_halo():
    """a point in the halo's outermost bin reaches the interior at radius = halo only"""
    b, h = 3, 2
    g = np.zeros((1, 12, 12), dtype=np.int64)
    g[0, 0, 5] = 7
    assert int(model.blur(g, b, h, 2)[0, 0, 3]) == 7 * 1 * 6
    assert not model.blur(g, b, h, 1).any()


@pytest.mark.parametrize("radius", [0, 1, 4, 8])
def test_Q_is_monotone_and_exact_at_powers_of_two(radius):
    one = 1 << (4 * radius)
    for k in range(0, 57 - 4 * radius):       # B < 2^56, so v + 2^4R < 2^57
        assert model.Q(one * ((1 << k) - 1), radius) == 256 * k
    vals = sorted(set([0, 1, 2, 3, one - 1, one, one + 1] + [one * j // 7 for j in range(1, 400)] +
                      [(1 << e) + d for e in range(1, 56) for d in (-1, 0, 1)]))
    qs = [model.Q(v, radius) for v in vals]
    assert all(a <= b for a, b in zip(qs, qs[1:]))
    assert qs[0] == 0


def test_levels():
    assert model.level(0, 100, 0, "linear") == 0
    assert model.level(5, 0, 0, "linear") == 0
    assert model.level(1, 1000, 0, "linear") == 1            # a lone point never disappears
    assert model.level(1000, 1000, 0, "linear") == 255
    assert model.level(5000, 1000, 0, "linear") == 255
    assert model.level(500, 1000, 0, "linear") == 127
    assert model.level(1, 1, 4, "log") == 1                  # Q(1) = 0 at radius 4: the denominator clamp
    assert model.Q(1, 4) == 0
    assert model.level(3, 3, 0, "log") == 255
    assert model.level(1, 3, 0, "log") == 127


def test_densify_halo_overlap_and_clipping():
    tiles = [(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 0, 0)]
    cells = [(3, 3, 3, 5), (3, 4, 4, 2), (3, 0, 0, 1), (2, 1, 1, 9), (3, 3, 3, 1)]
    g = model.densify(cells, tiles, 2, 1)
    # the four tiles meet between bins 3 and 4: both cells are in every haloed square
    assert [int(g[t].sum()) for t in range(5)] == [9, 8, 8, 8, 9]
    assert g[0, 4, 4] == 6 and g[0, 5, 5] == 2 and g[3, 0, 0] == 6 and g[3, 1, 1] == 2 and g[0, 1, 1] == 1
    assert (g[0] == g[4]).all()
    a = model.densify_arrays(*zip(*cells), tiles, 2, 1)
    assert (a == g.astype(np.int64)).all()


def test_render_wide():
    g = np.zeros((1, 3, 3), dtype=object)
    g[...] = 0
    g[0, 0, 0] = (1 << 52) - 1
    model.render(g, 0, 1, 1)
    g[0, 0, 0] = 1 << 52
    with pytest.raises(model.Wide):
        model.render(g, 0, 1, 1)


# ----------------------------------------------------------- python layer

def test_check_tiles_errors():
    ok = raster.check_tiles([(3, 7, 0), [3, 0, 7]], 5, 8, 0, 21)
    assert ok == ([(3, 7, 0), (3, 0, 7)], 5, 8)
    for tiles, b, h in (([], 5, 0), ([(3, 8, 0)], 5, 0), ([(3, 0, 8)], 5, 0), ([(3, -1, 0)], 5, 0),
                        ([(-1, 0, 0)], 5, 0), ([(3, 0)], 5, 0), ([(3, 0, 0)], 9, 0), ([(3, 0, 0)], -1, 0),
                        ([(3, 0, 0)], 5, 9), ([(3, 0, 0)], 5, -1), ([(17, 0, 0)], 5, 0)):
        with pytest.raises(ValueError):
            raster.check_tiles(tiles, b, h, 0, 21)
    with pytest.raises(ValueError):
        raster.check_tiles([(0, 0, 0)], 5, 0, 6, 12)      # zoom 5 below the stream's zmin
    assert len(raster.check_tiles([(0, 0, 0)] * 70, 0, 0, 0, 21)[0]) == 70   # splitting is the caller's


def test_check_render_errors():
    assert raster.check_render(8, 2, 2, "log", None) == (8, 2, 2, _lib.HM_SCALE_LOG, 0)
    assert raster.check_render(0, 8, 0, "linear", (1 << 56) - 1)[3:] == (_lib.HM_SCALE_LINEAR, (1 << 56) - 1)
    for args in ((8, 2, 3, "log", None), (8, 2, -1, "log", None), (8, 2, 2, "sqrt", None), (8, 2, 2, "log", 0),
                 (8, 8, 8, "log", 1 << 24), (8, 0, 0, "log", 1 << 56), (9, 0, 0, "log", None), (8, 9, 0, "log", None)):
        with pytest.raises(ValueError):
            raster.check_render(*args)


def test_stream_raster_args():
    index = {"all": 0, "u1": 1, "route": 2}
    t, lo, hi, gw, b, h = _raster_args(0, 18, index, [(13, 5, 6)], None, None, 5, 2)
    assert (t, lo, hi, gw, b, h) == ([(13, 5, 6)], _lib.HM_STREAM_ALLTIME, _lib.HM_STREAM_ALLTIME,
                                     _lib.HM_VIEW_MERGED, 5, 2)
    assert _raster_args(0, 18, index, [(13, 5, 6)], (10, 20), "u1", 5, 0)[1:4] == (10, 20, 1)
    assert _raster_args(0, 18, index, [(13, 5, 6)], None, "nobody", 5, 0)[3] is None
    with pytest.raises(ValueError, match="tile_rows"):
        _raster_args(0, 18, index, [(13, 5, 6)], None, "all", 5, 0)
    for kw in (dict(hours=(20, 20)), dict(hours=(20, 10)), dict(user=3), dict(tiles=[(14, 0, 0)]),
               dict(tiles=[(13, 1 << 13, 0)]), dict(halo=9), dict(bins_log2=9)):
        a = dict(tiles=[(13, 5, 6)], hours=None, user=None, bins_log2=5, halo=0)
        a.update(kw)
        with pytest.raises(ValueError):
            _raster_args(0, 18, index, **a)
    with pytest.raises(ValueError):
        _raster_args(6, 12, index, [(0, 0, 0)], None, None, 5, 0)


def test_ramps():
    assert {"heat", "gray"} <= set(raster.RAMPS)
    for name, r in raster.RAMPS.items():
        assert r.shape == (256, 4) and r.dtype == np.uint8, name
        assert r[0].tolist() == [0, 0, 0, 0], name
        assert (r[1:, 3] > 0).all(), name                 # every drawn level is visible
    g = raster.RAMPS["gray"]
    assert (g[1:, 0] == np.arange(1, 256)).all() and (g[1:, 0] == g[1:, 1]).all() and (g[1:, 1] == g[1:, 2]).all()
    h = raster.RAMPS["heat"]
    assert h[1].tolist() == [0, 0, 255, 64] and h[255].tolist() == [255, 0, 0, 255]
    assert (np.diff(h[1:, 3].astype(int)) >= 0).all()


def _png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, p = [], 8
    while p < len(data):
        n, tag = struct.unpack(">I4s", data[p:p + 8])
        body = data[p + 8:p + 8 + n]
        (crc,) = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
        out.append((tag, body))
        p += 12 + n
    assert p == len(data)
    return out


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (16, 5)])
def test_png_round_trip(shape):
    hgt, wid = shape
    img = np.random.default_rng(hgt * 10 + wid).integers(0, 256, (hgt, wid, 4)).astype(np.uint8)
    chunks = _png_chunks(raster.png_bytes(img))
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (wid, hgt, 8, 6, 0, 0, 0)   # 8-bit RGBA, no interlace
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(hgt, 1 + 4 * wid)
    assert (raw[:, 0] == 0).all()                         # filter type 0 on every scanline
    assert (raw[:, 1:].reshape(hgt, wid, 4) == img).all()
    assert chunks[2][1] == b""


def test_png_rejects_other_shapes():
    for bad in (np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 4), np.int32), np.zeros((0, 2, 4), np.uint8)):
        with pytest.raises(ValueError):
            raster.png_bytes(bad)


def test_no_device_raises():
    import torch

    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.DeviceUnavailable):
        raster.raster_cells(np.zeros(0, np.uint64), np.zeros(0, np.uint64), [(0, 0, 0)], 0)
    with pytest.raises(_lib.DeviceUnavailable):
        raster.render(None, 0, 0, 0)
