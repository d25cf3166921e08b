"""Region sets for the streaming heatmap's region queries (hm_stream_region_*;
StreamingHeatmap.region_totals / region_series / region_view /
region_visitors): places whose outline is not a rectangle -- a district, a
geofence, the polygons of a choropleth.  Host side, pure numpy, no device.

A RegionSet is up to MAX_REGIONS regions, each a set of cells of ONE zoom,
held as row spans in CSR form (csrc/hm_region.h is the same table in C):

    row_lo, nrows       the rows covered, [row_lo, row_lo + nrows)
    row_ptr[nrows + 1]  row i's spans are [row_ptr[i], row_ptr[i + 1])
    col_lo, col_hi, region   span j: the columns [col_lo[j], col_hi[j]) of
                        region[j]  (uint32 each)

Within a row the spans are sorted by (col_lo, region).  The spans of one region
in one row are disjoint: touching or overlapping ones are merged when the table
is built.  Spans of different regions may overlap, and a cell then belongs to
each of them.  Everything is clipped to [0, 2^zoom)^2; a covered row may have
no span.
"""
from __future__ import annotations

import numpy as np

MAX_REGIONS = 4096        # HM_REGION_MAX_REGIONS
MAX_SPANS = 1 << 20       # HM_REGION_MAX_SPANS
MAX_ROWS = 1 << 20        # HM_REGION_MAX_ROWS
MAX_ZOOM = 21             # HM_MAX_ZOOM


def _check_zoom(zoom) -> int:
    if isinstance(zoom, bool) or not isinstance(zoom, (int, np.integer)) or not 0 <= int(zoom) <= MAX_ZOOM:
        raise ValueError("zoom must be an integer 0..%d (got %r)" % (MAX_ZOOM, zoom))
    return int(zoom)


def _check_nregions(n: int) -> int:
    if not 1 <= n <= MAX_REGIONS:
        raise ValueError("a region set holds 1..%d regions (got %d)" % (MAX_REGIONS, n))
    return n


class RegionSet:
    """One zoom and a CSR span table (module docstring).  Build one with
    from_tile_polygons, from_polygons, from_mask or from_rects."""

    def __init__(self, zoom, row_lo, nrows, row_ptr, col_lo, col_hi, region, nregions, names=None):
        self.zoom = _check_zoom(zoom)
        self.row_lo, self.nrows = int(row_lo), int(nrows)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        self.col_lo = np.ascontiguousarray(col_lo, dtype=np.uint32)
        self.col_hi = np.ascontiguousarray(col_hi, dtype=np.uint32)
        self.region = np.ascontiguousarray(region, dtype=np.uint32)
        self.nregions = _check_nregions(int(nregions))
        self.names = None if names is None else list(names)
        if self.names is not None and len(self.names) != self.nregions:
            raise ValueError("%d names for %d regions" % (len(self.names), self.nregions))
        ns = len(self.col_lo)
        if len(self.col_hi) != ns or len(self.region) != ns or len(self.row_ptr) != self.nrows + 1:
            raise ValueError("span arrays of different lengths, or row_ptr not of nrows + 1 entries")
        if ns > MAX_SPANS:
            raise ValueError("%d spans; a region set holds at most %d (use a lower zoom, or fewer regions per set)"
                             % (ns, MAX_SPANS))
        if self.nrows > MAX_ROWS:
            raise ValueError("%d rows; a region set covers at most %d" % (self.nrows, MAX_ROWS))
        if self.row_lo < 0 or self.nrows < 0 or self.row_lo + self.nrows > (1 << self.zoom):
            raise ValueError("rows [%d, %d) are not inside zoom %d" % (self.row_lo, self.row_lo + self.nrows, self.zoom))

    @property
    def nspans(self) -> int:
        return len(self.col_lo)

    def rows(self) -> np.ndarray:
        """the row of every span (int64)"""
        return self.row_lo + np.repeat(np.arange(self.nrows, dtype=np.int64), np.diff(self.row_ptr.astype(np.int64)))

    def area(self) -> np.ndarray:
        """cells per region (int64 [nregions])"""
        w = self.col_hi.astype(np.int64) - self.col_lo.astype(np.int64)
        return np.bincount(self.region, weights=w, minlength=self.nregions).astype(np.int64)

    def cells(self, j: int):
        """(rows, cols) of region j's cells (int64, by row then column): for
        tests and small uses"""
        m = self.region == j
        r, lo, hi = self.rows()[m], self.col_lo[m].astype(np.int64), self.col_hi[m].astype(np.int64)
        w = hi - lo
        start = np.cumsum(w) - w
        col = np.arange(int(w.sum()), dtype=np.int64) - np.repeat(start - lo, w)
        return np.repeat(r, w), col

    def bounding_rect(self):
        """(zoom, row_lo, row_hi, col_lo, col_hi) around every span, or None for a set without spans"""
        if not self.nspans:
            return None
        return (self.zoom, self.row_lo, self.row_lo + self.nrows, int(self.col_lo.min()), int(self.col_hi.max()))

    # ---------------------------------------------------------- constructors

    @classmethod
    def _from_spans(cls, zoom, row, lo, hi, region, nregions, names=None):
        """The table of the spans (row, [lo, hi), region), int64 arrays in any
        order: clipped to the square, empty ones dropped, touching or
        overlapping spans of one region in one row merged, sorted."""
        zoom = _check_zoom(zoom)
        side = 1 << zoom
        row, lo, hi, region = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (row, lo, hi, region))
        lo, hi = np.clip(lo, 0, side), np.clip(hi, 0, side)
        m = (row >= 0) & (row < side) & (hi > lo)
        row, lo, hi, region = row[m], lo[m], hi[m], region[m]
        if len(row):
            o = np.lexsort((lo, region, row))
            row, lo, hi, region = row[o], lo[o], hi[o], region[o]
            # a running maximum of hi inside each (row, region) group: the
            # group's number lifts its values above every earlier group's
            new_group = np.ones(len(row), dtype=bool)
            new_group[1:] = (row[1:] != row[:-1]) | (region[1:] != region[:-1])
            lift = (np.cumsum(new_group) - 1) * (side + 1)
            reach = np.maximum.accumulate(hi + lift) - lift
            start = new_group.copy()
            start[1:] |= lo[1:] > reach[:-1]
            first = np.flatnonzero(start)
            row, lo, region = row[first], lo[first], region[first]
            hi = np.maximum.reduceat(hi, first)
            o = np.lexsort((region, lo, row))
            row, lo, hi, region = row[o], lo[o], hi[o], region[o]
            row_lo, nrows = int(row[0]), int(row[-1] - row[0] + 1)
            if nrows > MAX_ROWS:
                raise ValueError("%d rows; a region set covers at most %d" % (nrows, MAX_ROWS))
            row_ptr = np.concatenate([[0], np.cumsum(np.bincount(row - row_lo, minlength=nrows))])
        else:
            row_lo, nrows, row_ptr = 0, 0, np.zeros(1, dtype=np.int64)
        return cls(zoom, row_lo, nrows, row_ptr, lo, hi, region, nregions, names)

    @classmethod
    def from_tile_polygons(cls, regions, zoom, names=None):
        """regions: a list of regions, each a list of rings, each an [n, 2]
        float64 array of continuous tile coordinates (x, y) at `zoom` -- column
        direction, then row direction; the closing edge is implied.  A cell
        (row, col) belongs to a region iff its centre (col + 0.5, row + 0.5) is
        inside under the even-odd rule over all of the region's rings pooled,
        so holes and multipolygons need nothing special.

        The rule, fixed so that two implementations agree bit for bit: for row
        r let yc = r + 0.5.  An edge (x0, y0) -> (x1, y1) crosses iff (y0 <=
        yc) != (y1 <= yc), at x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0) in
        float64, in that operation order.  The crossings sorted ascending pair
        up, and a pair (xa, xb) is the span [ceil(xa - 0.5), ceil(xb - 0.5)),
        clipped to [0, 2^zoom) and dropped if empty.  Non-finite vertices are
        ValueError."""
        zoom = _check_zoom(zoom)
        side = 1 << zoom
        _check_nregions(len(regions))
        rows, los, his, regs = [], [], [], []
        for j, rings in enumerate(regions):
            x0, y0, x1, y1 = _edges(rings)
            # the rows an edge can cross, generously; the rule itself decides
            ymin, ymax = np.minimum(y0, y1), np.maximum(y0, y1)
            ra = np.clip(np.floor(ymin) - 1, 0, side - 1).astype(np.int64)
            rb = np.clip(np.floor(ymax) + 1, 0, side - 1).astype(np.int64)
            keep = (ymax >= 0) & (ymin <= side)
            ra, rb = ra[keep], rb[keep]
            x0, y0, x1, y1 = x0[keep], y0[keep], x1[keep], y1[keep]
            n = rb - ra + 1
            e = np.repeat(np.arange(len(n)), n)
            r = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n - ra, n)
            yc = r + 0.5
            ex0, ey0, ex1, ey1 = x0[e], y0[e], x1[e], y1[e]
            cross = (ey0 <= yc) != (ey1 <= yc)
            r, yc, ex0, ey0, ex1, ey1 = r[cross], yc[cross], ex0[cross], ey0[cross], ex1[cross], ey1[cross]
            with np.errstate(over="ignore", invalid="ignore"):
                x = ex0 + ((yc - ey0) * (ex1 - ex0)) / (ey1 - ey0)
            if not np.isfinite(x).all():
                raise ValueError("region %d: an edge is too long for float64 arithmetic" % j)
            o = np.lexsort((x, r))
            r, x = r[o], x[o]
            # closed rings cross every row an even number of times
            xa, xb, r = x[0::2], x[1::2], r[0::2]
            lo = np.clip(np.ceil(xa - 0.5), 0, side).astype(np.int64)
            hi = np.clip(np.ceil(xb - 0.5), 0, side).astype(np.int64)
            rows.append(r), los.append(lo), his.append(hi), regs.append(np.full(len(r), j, dtype=np.int64))
        cat = (lambda p: np.concatenate(p) if p else np.zeros(0, np.int64))
        return cls._from_spans(zoom, cat(rows), cat(los), cat(his), cat(regs), len(regions), names)

    @classmethod
    def from_polygons(cls, regions, zoom, names=None):
        """from_tile_polygons with rings of (lat, lon) degrees, projected with
        x = (lon + 180) / 360 * 2^zoom and y = (1 - asinh(tan(radians(lat))) /
        pi) / 2 * 2^zoom.  A vertex is an outline, not a point to be binned: it
        goes through numpy, not through the bit-exact projection of the count
        path, so membership is decided at the resolution of one zoom-`zoom`
        cell -- a cell whose centre lies within rounding of an edge may fall on
        either side.  |lat| >= 90 and non-finite vertices are ValueError.  No
        antimeridian handling: longitudes are taken as given and clipped."""
        zoom = _check_zoom(zoom)
        n = float(1 << zoom)
        out = []
        for rings in regions:
            tr = []
            for ring in rings:
                ring = np.asarray(ring, dtype=np.float64)
                if ring.ndim != 2 or ring.shape[1] != 2:
                    raise ValueError("a ring is an [n, 2] array of (lat, lon)")
                lat, lon = ring[:, 0], ring[:, 1]
                if not np.isfinite(ring).all():
                    raise ValueError("non-finite vertex")
                if (np.abs(lat) >= 90.0).any():
                    raise ValueError("|lat| >= 90 has no place on the Mercator square")
                x = (lon + 180.0) / 360.0 * n
                y = (1.0 - np.arcsinh(np.tan(np.radians(lat))) / np.pi) / 2.0 * n
                tr.append(np.stack([x, y], axis=1))
            out.append(tr)
        return cls.from_tile_polygons(out, zoom, names)

    @classmethod
    def from_mask(cls, zoom, row0, col0, mask, names=None):
        """The cells of `mask`, whose element [i, j] is cell (row0 + i, col0 +
        j): a 2-D bool array is one region; a 2-D integer array puts a cell of
        value v > 0 into region v - 1 (max(v) regions); a [R, H, W] bool array
        is R regions that may overlap."""
        mask = np.asarray(mask)
        if mask.ndim == 3:
            if mask.dtype != np.bool_:
                raise ValueError("a [R, H, W] mask is bool")
            planes, nreg = [(j, mask[j]) for j in range(mask.shape[0])], mask.shape[0]
        elif mask.ndim == 2 and mask.dtype == np.bool_:
            planes, nreg = [(0, mask)], 1
        elif mask.ndim == 2 and np.issubdtype(mask.dtype, np.integer):
            planes, nreg = [(None, mask.astype(np.int64))], max(int(mask.max()) if mask.size else 0, 1)
        else:
            raise ValueError("mask must be a 2-D bool or integer array, or a [R, H, W] bool array")
        rows, los, his, regs = [], [], [], []
        for j, m in planes:
            # runs of equal value along each row: between consecutive changes of the zero-padded row
            p = np.pad(m.astype(np.int64), ((0, 0), (1, 1)))
            r, c = np.nonzero(p[:, 1:] != p[:, :-1])
            if not len(r):
                continue
            run = np.flatnonzero(r[1:] == r[:-1])            # boundary k and k + 1 lie in one row
            v = m[r[run], c[run]].astype(np.int64)
            on = v > 0
            run, v = run[on], v[on]
            rows.append(row0 + r[run]), los.append(col0 + c[run]), his.append(col0 + c[run + 1])
            regs.append(np.full(len(run), j, dtype=np.int64) if j is not None else v - 1)
        cat = (lambda p: np.concatenate(p) if p else np.zeros(0, np.int64))
        return cls._from_spans(zoom, cat(rows), cat(los), cat(his), cat(regs), nreg, names)

    @classmethod
    def from_rects(cls, rects, names=None):
        """One region per rectangle (zoom, row_lo, row_hi, col_lo, col_hi) (lo
        inclusive, hi exclusive, clipped to the square), all of one zoom."""
        rects = [tuple(int(v) for v in r) for r in rects]
        if not rects or any(len(r) != 5 for r in rects) or any(r[0] != rects[0][0] for r in rects):
            raise ValueError("from_rects takes rectangles (zoom, row_lo, row_hi, col_lo, col_hi) of one zoom")
        zoom = _check_zoom(rects[0][0])
        side = 1 << zoom
        rows, los, his, regs = [], [], [], []
        for j, (_, rlo, rhi, clo, chi) in enumerate(rects):
            r = np.arange(max(rlo, 0), min(rhi, side), dtype=np.int64)
            rows.append(r), los.append(np.full(len(r), clo)), his.append(np.full(len(r), chi))
            regs.append(np.full(len(r), j, dtype=np.int64))
        return cls._from_spans(zoom, np.concatenate(rows), np.concatenate(los), np.concatenate(his),
                               np.concatenate(regs), len(rects), names)


def _edges(rings):
    """(x0, y0, x1, y1) of every edge of the rings, the closing ones included"""
    xs0, ys0, xs1, ys1 = [], [], [], []
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        if ring.ndim != 2 or ring.shape[1] != 2 or len(ring) < 3:
            raise ValueError("a ring is an [n, 2] array of n >= 3 vertices")
        if not np.isfinite(ring).all():
            raise ValueError("non-finite vertex")
        nxt = np.roll(ring, -1, axis=0)
        xs0.append(ring[:, 0]), ys0.append(ring[:, 1]), xs1.append(nxt[:, 0]), ys1.append(nxt[:, 1])
    if not xs0:
        z = np.zeros(0)
        return z, z, z, z
    return tuple(np.concatenate(p) for p in (xs0, ys0, xs1, ys1))
