"""The raster specification of include/heatmap_amd.h ("Rasters") restated with
Python ints and numpy object arrays: densify with halo, binomial blur, Q,
levels and LUT.  Slow and plain on purpose -- every value is an exact Python
int, nothing is vectorised in Q -- so it is the reference the device results
are compared with bit for bit."""
from math import comb

import numpy as np


def densify(cells, tiles, bins_log2, halo):
    """cells: iterable of (zoom, row, col, count); returns int64 [T, W, W].
    Element [t][y][x] sums the cells of zoom tz + b at row (tr << b) - H + y,
    column (tc << b) - H + x; cells outside [0, 2^z)^2 are never drawn."""
    b, h = bins_log2, halo
    w = (1 << b) + 2 * h
    grid = np.zeros((len(tiles), w, w), dtype=object)
    grid[...] = 0
    cells = [tuple(int(v) for v in c) for c in cells]
    for t, (tz, tr, tc) in enumerate(tiles):
        z, oy, ox = tz + b, (tr << b) - h, (tc << b) - h
        for cz, r, c, n in cells:
            if cz != z or not (0 <= r < (1 << z) and 0 <= c < (1 << z)):
                continue
            y, x = r - oy, c - ox
            if 0 <= y < w and 0 <= x < w:
                grid[t, y, x] += n
    return grid


def densify_arrays(zoom, row, col, count, tiles, bins_log2, halo):
    """densify for large cell sets (numpy int64 arithmetic; counts must sum
    below 2^63)."""
    b, h = bins_log2, halo
    w = (1 << b) + 2 * h
    zoom, row, col, count = (np.asarray(a).astype(np.int64) for a in (zoom, row, col, count))
    grid = np.zeros((len(tiles), w, w), dtype=np.int64)
    for t, (tz, tr, tc) in enumerate(tiles):
        z, oy, ox = tz + b, (tr << b) - h, (tc << b) - h
        y, x = row - oy, col - ox
        m = (zoom == z) & (row >= 0) & (row < (1 << z)) & (col >= 0) & (col < (1 << z))
        m &= (y >= 0) & (y < w) & (x >= 0) & (x < w)
        np.add.at(grid[t], (y[m], x[m]), count[m])
    return grid


def weights(radius):
    return [comb(2 * radius, k) for k in range(2 * radius + 1)]


def blur(grid, bins_log2, halo, radius):
    """B[t][y][x] = sum_i sum_j w[i] w[j] g[H + y - R + i][H + x - R + j], Python ints"""
    h, r = halo, radius
    assert 0 <= r <= h
    w = weights(r)
    g = np.asarray(grid).astype(object)
    # S x S for a tile's grid; a mosaic of adjacent tiles (S + 2H by k S + 2H) blurs the same way
    sy, sx = g.shape[1] - 2 * h, g.shape[2] - 2 * h
    assert sy % (1 << bins_log2) == 0 and sx % (1 << bins_log2) == 0
    out = np.zeros((g.shape[0], sy, sx), dtype=object)
    out[...] = 0
    for i, wi in enumerate(w):
        for j, wj in enumerate(w):
            out += (wi * wj) * g[:, h - r + i:h - r + i + sy, h - r + j:h - r + j + sx]
    return out


def q(u):
    u = int(u)
    assert u >= 1
    e = u.bit_length() - 1
    return 256 * e + (((u << (63 - e)) & ((1 << 64) - 1)) >> 55 & 255)


def Q(v, radius):
    return q(int(v) + (1 << (4 * radius))) - 256 * 4 * radius


def level(B, vs, radius, scale):
    B, vs = int(B), int(vs)
    if B == 0 or vs == 0:
        return 0
    if scale == "linear":
        return min(255, max(1, B * 255 // vs))
    return min(255, max(1, Q(B, radius) * 255 // max(1, Q(vs, radius))))


class Wide(Exception):
    pass


def render(grid, bins_log2, halo, radius, scale="log", vmax=None, lut=None):
    """(levels uint8 [T, S, S], vs, rgba uint8 [T, S, S, 4] or None); raises
    Wide when a bin of the haloed grids is >= 2^(56 - 4 radius)"""
    g = np.asarray(grid).astype(object)
    if max(int(v) for v in g.reshape(-1)) >= 1 << (56 - 4 * radius):
        raise Wide()
    B = blur(g, bins_log2, halo, radius)
    flat = [int(v) for v in B.reshape(-1)]
    vs = (int(vmax) << (4 * radius)) if vmax else max(flat)
    lev = np.array([level(v, vs, radius, scale) for v in flat], dtype=np.uint8).reshape(B.shape)
    rgba = None if lut is None else np.asarray(lut, dtype=np.uint8).reshape(256, 4)[lev]
    return lev, vs, rgba
