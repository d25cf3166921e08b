"""Dense tile rasters and rendered RGBA tiles -- host side of hm_cells_raster
and hm_raster_render (include/heatmap_amd.h, "Rasters").

    grid = raster_cells(keys, counts, [(tz, tr, tc)], bins_log2=8, halo=2)
    rgba, vs = render(grid, 8, 2, radius=2)          # uint8 [T, 256, 256, 4]
    open("tile.png", "wb").write(png_bytes(rgba[0].cpu().numpy()))

A grid is an int64 CUDA tensor [T, W, W], W = 2^bins_log2 + 2 halo: the bins of
zoom tz + bins_log2 under tile (tz, tr, tc) with a halo of neighbour bins, so a
tile blurred alone is seamless with its neighbours.  StreamingHeatmap.tile_raster
fills the same grids straight from the resident log, tile_frames a stack of
them [F, T, W, W], one per frame of the hours; accumulate sums such frames
into trailing windows (hm_raster_accumulate) and apng_bytes packs rendered
frames into an animated PNG.  There is no CPU fallback: without a device these
calls raise DeviceUnavailable.
"""
from __future__ import annotations

import ctypes
import struct
import zlib

import numpy as np

from . import _lib
from . import device as _dv

SCALES = {"linear": _lib.HM_SCALE_LINEAR, "log": _lib.HM_SCALE_LOG}


def _ramp(stops) -> np.ndarray:
    """256 x RGBA uint8 from integer piecewise-linear stops [(level, r, g, b,
    a)] (levels ascending from 1 to 255); entry 0 is fully transparent."""
    out = np.zeros((256, 4), dtype=np.uint8)
    for (l0, *c0), (l1, *c1) in zip(stops, stops[1:]):
        for l in range(l0, l1 + 1):
            out[l] = [(a * (l1 - l) + b * (l - l0) + (l1 - l0) // 2) // (l1 - l0) for a, b in zip(c0, c1)]
    return out


RAMPS = {
    # transparent blue -> cyan -> green -> yellow -> red, alpha rising with the level
    "heat": _ramp([(1, 0, 0, 255, 64), (64, 0, 255, 255, 128), (128, 0, 255, 0, 176), (192, 255, 255, 0, 224),
                   (255, 255, 0, 0, 255)]),
    "gray": _ramp([(1, 1, 1, 1, 255), (255, 255, 255, 255, 255)]),
}


def check_tiles(tiles, bins_log2, halo, zlo: int, zhi: int):
    """Validated (tiles as int tuples, bins_log2, halo) of a raster call whose
    bin zooms tz + bins_log2 must lie in [zlo, zhi]; any number of tiles (the
    callers split them into calls of HM_RASTER_MAX_TILES).  Pure: no device."""
    b, h = int(bins_log2), int(halo)
    if not 0 <= b <= _lib.HM_RASTER_MAX_BINS_LOG2:
        raise ValueError("bins_log2 must be 0..%d (got %r)" % (_lib.HM_RASTER_MAX_BINS_LOG2, bins_log2))
    if not 0 <= h <= _lib.HM_RASTER_MAX_HALO:
        raise ValueError("halo must be 0..%d (got %r)" % (_lib.HM_RASTER_MAX_HALO, halo))
    tiles = [tuple(int(v) for v in t) for t in tiles]
    if not tiles or any(len(t) != 3 for t in tiles):
        raise ValueError("a raster takes at least one tile (tz, tr, tc)")
    for tz, tr, tc in tiles:
        if tz < 0 or not (0 <= tr < (1 << tz) and 0 <= tc < (1 << tz)):
            raise ValueError("tile %r is not inside the square of its zoom" % ((tz, tr, tc),))
        if not zlo <= tz + b <= zhi:
            raise ValueError("tile %r with bins_log2 %d needs zoom %d; zooms %d..%d are held"
                             % ((tz, tr, tc), b, tz + b, zlo, zhi))
    return tiles, b, h


def check_render(bins_log2, halo, radius, scale, vmax):
    """Validated (bins_log2, halo, radius, scale word, vmax word) of render.
    Pure: no device."""
    b, h, r = int(bins_log2), int(halo), int(radius)
    if not 0 <= b <= _lib.HM_RASTER_MAX_BINS_LOG2:
        raise ValueError("bins_log2 must be 0..%d (got %r)" % (_lib.HM_RASTER_MAX_BINS_LOG2, bins_log2))
    if not 0 <= h <= _lib.HM_RASTER_MAX_HALO:
        raise ValueError("halo must be 0..%d (got %r)" % (_lib.HM_RASTER_MAX_HALO, halo))
    if not 0 <= r <= h:
        raise ValueError("radius must be 0..halo (got radius %r, halo %d)" % (radius, h))
    if scale not in SCALES:
        raise ValueError("scale must be 'linear' or 'log' (got %r)" % (scale,))
    v = 0 if vmax is None else int(vmax)
    if vmax is not None and not 1 <= v < (1 << (56 - 4 * r)):
        raise ValueError("vmax must be 1..2^%d - 1 at radius %d (got %r)" % (56 - 4 * r, r, vmax))
    return b, h, r, SCALES[scale], v


def _tile_array(tiles):
    return (ctypes.c_int64 * (3 * len(tiles)))(*[v for t in tiles for v in t])


def raster_cells(keys, counts, tiles, bins_log2, halo=0, device=0):
    """int64 CUDA tensor [T, W, W]: the cells (hm_count's keys and counts:
    count / rollup / window / view output, numpy or CUDA tensors) added into
    the grids of tiles = [(tz, tr, tc)]; equal keys add (hm_cells_raster)."""
    dev_index = int(device)
    torch = _dv._torch()
    tiles, b, h = check_tiles(tiles, bins_log2, halo, 0, _lib.HM_COUNT_MAX_ZOOM)
    ctx = _dv.context(dev_index)
    k = _dv._dev(np.asarray(keys).view(np.int64) if isinstance(keys, np.ndarray) else keys, torch.int64, dev_index)
    c = _dv._dev(np.asarray(counts).view(np.int64) if isinstance(counts, np.ndarray) else counts, torch.int64,
                dev_index)
    if k.numel() != c.numel():
        raise ValueError("keys and counts must have one entry per cell")
    w = (1 << b) + 2 * h
    grid = torch.empty((len(tiles), w, w), dtype=torch.int64, device="cuda:%d" % dev_index)
    for j in range(0, len(tiles), _lib.HM_RASTER_MAX_TILES):
        part = tiles[j:j + _lib.HM_RASTER_MAX_TILES]
        rc = ctx.L.hm_cells_raster(ctx.ptr, _dv._ptr(k), _dv._ptr(c), k.numel(), _tile_array(part), len(part), b, h,
                                   _dv._ptr(grid[j:j + len(part)]))
        if rc != _lib.HM_OK:
            _lib.raise_for(rc)
    return grid


def _lut(ramp, torch, dev):
    if isinstance(ramp, str):
        if ramp not in RAMPS:
            raise ValueError("unknown ramp %r (have %s)" % (ramp, ", ".join(sorted(RAMPS))))
        ramp = RAMPS[ramp]
    a = np.ascontiguousarray(ramp, dtype=np.uint8)
    if a.shape != (256, 4):
        raise ValueError("a ramp is 256 RGBA entries (got shape %r)" % (a.shape,))
    return torch.from_numpy(a.view("<u4").reshape(256).view(np.int32)).to(dev)


def render(grid, bins_log2, halo, radius, scale="log", vmax=None, ramp="heat", levels=False):
    """(rgba uint8 CUDA tensor [T, S, S, 4], vmax_used): the grids blurred with
    the binomial kernel of `radius` (<= halo), scaled ('linear' or 'log')
    against vmax (a count; None: the largest blurred value of the call, which
    vmax_used then reports, in units of 2^-(4 radius)) and coloured through
    ramp (a RAMPS name or a [256, 4] uint8 table).  levels=True also returns
    the uint8 [T, S, S] levels.  Raises OverflowError when a bin is too wide
    for the radius (>= 2^(56 - 4 radius)).  More than HM_RASTER_MAX_TILES
    tiles take several calls and so need a fixed vmax."""
    torch = _dv._torch()
    b, h, r, sw, v = check_render(bins_log2, halo, radius, scale, vmax)
    s, w = 1 << b, (1 << b) + 2 * h
    if not isinstance(grid, torch.Tensor) or grid.dtype != torch.int64 or grid.device.type != "cuda":
        raise ValueError("grid must be an int64 CUDA tensor (raster_cells / tile_raster)")
    if grid.dim() != 3 or grid.shape[0] < 1 or tuple(grid.shape[1:]) != (w, w):
        raise ValueError("grid must be [T, %d, %d] for bins_log2 %d and halo %d (got %r)"
                         % (w, w, b, h, tuple(grid.shape)))
    nt = grid.shape[0]
    if nt > _lib.HM_RASTER_MAX_TILES and vmax is None:
        raise ValueError("more than %d tiles are rendered in several calls: give a fixed vmax"
                         % _lib.HM_RASTER_MAX_TILES)
    grid = grid.contiguous()
    ctx = _dv.context(grid.device.index)
    lut = _lut(ramp, torch, grid.device)
    rgba = torch.empty((nt, s, s, 4), dtype=torch.uint8, device=grid.device)
    lev = torch.empty((nt, s, s), dtype=torch.uint8, device=grid.device) if levels else None
    used = ctypes.c_uint64(0)
    for j in range(0, nt, _lib.HM_RASTER_MAX_TILES):
        m = min(_lib.HM_RASTER_MAX_TILES, nt - j)
        rc = ctx.L.hm_raster_render(ctx.ptr, _dv._ptr(grid[j:j + m]), m, b, h, r, sw, v, _dv._ptr(lut),
                                    _dv._ptr(rgba[j:j + m]), _dv._ptr(lev[j:j + m]) if levels else None,
                                    ctypes.byref(used))
        if rc == _lib.HM_E_WIDE:
            raise OverflowError("a bin of 2^%d or more cannot be blurred at radius %d" % (56 - 4 * r, r))
        if rc != _lib.HM_OK:
            _lib.raise_for(rc)
    return (rgba, used.value, lev) if levels else (rgba, used.value)


def accumulate(grid, window=0):
    """int64 CUDA tensor of grid's shape: trailing sums along its first axis,
    the frames of StreamingHeatmap.tile_frames -- out[f] = grid[max(0, f -
    window + 1) .. f] summed (modulo 2^64); window = 0 or >= the number of
    frames: the cumulative sum; window = 1: a copy (hm_raster_accumulate)."""
    torch = _dv._torch()
    k = int(window)
    if k < 0:
        raise ValueError("window must be 0 (cumulative) or a number of frames (got %r)" % (window,))
    if not isinstance(grid, torch.Tensor) or grid.dtype != torch.int64 or grid.device.type != "cuda":
        raise ValueError("grid must be an int64 CUDA tensor (tile_frames)")
    if grid.dim() < 1 or grid.numel() < 1:
        raise ValueError("grid must hold at least one frame of at least one element (got %r)" % (tuple(grid.shape),))
    grid = grid.contiguous()
    out = torch.empty_like(grid)
    ctx = _dv.context(grid.device.index)
    rc = ctx.L.hm_raster_accumulate(ctx.ptr, _dv._ptr(grid), grid.shape[0], grid.numel() // grid.shape[0], k,
                                    _dv._ptr(out))
    if rc != _lib.HM_OK:
        _lib.raise_for(rc)
    return out


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _png_scanlines(a: np.ndarray) -> bytes:
    """the deflated scanlines of one [H, W, 4] image: filter type 0, then the row's bytes"""
    hgt, wid = a.shape[:2]
    raw = np.concatenate([np.zeros((hgt, 1), np.uint8), np.ascontiguousarray(a).reshape(hgt, wid * 4)], axis=1)
    return zlib.compress(raw.tobytes(), 6)


def png_bytes(rgba) -> bytes:
    """An 8-bit RGBA PNG of one [H, W, 4] uint8 image (numpy array or tensor)."""
    a = rgba.cpu().numpy() if hasattr(rgba, "cpu") else np.asarray(rgba)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("png_bytes takes one uint8 [H, W, 4] image (got %s %r)" % (a.dtype, a.shape))
    hgt, wid = a.shape[:2]
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", wid, hgt, 8, 6, 0, 0, 0)) +
            _png_chunk(b"IDAT", _png_scanlines(a)) + _png_chunk(b"IEND", b""))


def apng_bytes(frames_rgba, delay_ms=100, loops=0) -> bytes:
    """An animated PNG of [F, H, W, 4] uint8 frames (numpy array or tensor:
    one tile of StreamingHeatmap.tile_frame_images), each shown delay_ms
    milliseconds, played `loops` times (0: for ever).  IHDR, acTL, then per
    frame an fcTL and the frame's data -- IDAT for the first, so a viewer
    without APNG shows that one, fdAT for the others -- under consecutive
    sequence numbers, IEND."""
    a = frames_rgba.cpu().numpy() if hasattr(frames_rgba, "cpu") else np.asarray(frames_rgba)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 4 or min(a.shape[:3]) < 1:
        raise ValueError("apng_bytes takes uint8 [F, H, W, 4] frames (got %s %r)" % (a.dtype, a.shape))
    delay, plays = int(delay_ms), int(loops)
    if not 0 <= delay <= 0xFFFF:
        raise ValueError("delay_ms must be 0..65535 (got %r)" % (delay_ms,))
    if not 0 <= plays <= 0x7FFFFFFF:
        raise ValueError("loops must be 0 (for ever) or a number of plays (got %r)" % (loops,))
    nf, hgt, wid = a.shape[:3]
    out = [b"\x89PNG\r\n\x1a\n", _png_chunk(b"IHDR", struct.pack(">IIBBBBB", wid, hgt, 8, 6, 0, 0, 0)),
           _png_chunk(b"acTL", struct.pack(">II", nf, plays))]
    seq = 0
    for f in range(nf):
        # the whole canvas at (0, 0), delay / 1000 s, dispose: none, blend: source
        out.append(_png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, wid, hgt, 0, 0, delay, 1000, 0, 0)))
        seq += 1
        if f == 0:
            out.append(_png_chunk(b"IDAT", _png_scanlines(a[f])))
        else:
            out.append(_png_chunk(b"fdAT", struct.pack(">I", seq) + _png_scanlines(a[f])))
            seq += 1
    out.append(_png_chunk(b"IEND", b""))
    return b"".join(out)
