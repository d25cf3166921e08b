"""Streaming micro-batches merged into a heatmap resident in HBM (BASELINE
config 5) -- host side of hm_stream_* (include/heatmap_amd.h).

The reference recomputes its pyramid per Spark job (heatmap.py:152-158) and
keys every bin by user group and timespan label (heatmap.py:54-55,62-75; only
'alltime' is live there, the year/month/day labels of build_timespan_label,
heatmap.py:38-52, are commented out).  StreamingHeatmap keeps one device
bucket per (user group, epoch hour); each add() runs ONE count pass over the
batch (however many hours and groups it holds) and folds its cells in.  Every
label is a device rollup of the hour buckets:

  counts(ALLTIME) / hourly()   per-cell counts of every kept point so far
  window(lo, hi)               the same cells summed over the epoch hours
                               lo <= hour < hi (a sliding window such as the
                               last 24 hours; undated points are in none), and
                               window_rows(lo, hi, label) their rows
  view(rects, hours, group)    only the cells inside the rectangles (zoom, rows,
                               cols) of a viewport, for a window of hours or
                               alltime, merged, per group or for one group, and
                               tile_rows(tiles, hours, label, user) the rows of
                               the heatmap tiles on screen (hm_stream_view: one
                               pass over the log's keys)
  tile_raster(tiles, hours, user)  the tiles as dense count grids with a halo
                               (hm_stream_raster: the same filter pass, no
                               merge), and tile_images(...) the same blurred,
                               scaled and coloured into RGBA (heatmap_amd.raster)
  tile_frames(tiles, hours, frame_hours)  the same grids per frame of the hours,
                               for a time slider or an animation, in ONE pass
                               (hm_stream_raster_frames); trailing windows or
                               growth through hm_raster_accumulate;
                               tile_series(...) the tiles' points per frame and
                               tile_frame_images(...) the frames on one scale
  top(k, rects, hours, group)  the k hottest cells of a view in rank order (count
                               descending, then zoom, row, col), selected on the
                               device (hm_stream_top); top_tiles(k, zoom, ...)
                               the busiest cells of one zoom, top_groups /
                               top_users(k, rects, hours) the most active groups
                               there (hm_stream_top_groups)
  visitors(rects, hours, min_visitors)  per cell of a view its points and its
                               distinct visitors (groups), only the cells with
                               at least min_visitors of them (hm_stream_visitors);
                               top_visited(k, ...) the most visited cells,
                               tile_visitors(tiles, ...) the visitors as grids,
                               and tile_raster / tile_images(..., min_users=k)
                               k-anonymous tiles
  region_totals / region_series(regions, hours, ...)  the points inside each
                               region of a region.RegionSet -- polygons, masks:
                               places that are no rectangle -- in all, or per
                               frame of the hours (hm_stream_region_series: one
                               pass, reduced on the device); region_view(...)
                               the cells inside them, region_visitors(...) the
                               distinct visitors per region with a threshold
  expire(before_hour)         retention: the cells of hours < before_hour
                               leave the stream, their buckets are freed
  forget(users, groups, hours)  erasure: the cells of these users or group
                               ids, of these hours or of all time, leave the
                               stream in one pass (hm_stream_forget); export(),
                               snapshot() and merge_from() take the same three
                               arguments and handle only that part
                               (hm_stream_export_select)
  snapshot() / save(path)      the whole state as arrays (hm_stream_export: one
                               record per (group, hour, cell)), and back:
                               load(path), from_snapshot(), restore()
  import_cells(...)            pre-aggregated cells appended (hm_stream_import)
  merge_from(other)            another stream's cells added, groups matched by
                               label: shards of one feed, or a backfill
  rows(timespan)               build_heatmaps' rows, {id: {bin: count}}, for
                               'alltime', 'year', 'month' or 'day' (UTC dates
                               of the epoch hours), with the reference's user
                               groups and level-by-level 'all' weighting
                               (heatmap.heatmap.combine_cells)

so a caller sees the same rows as heatmap.assemble_rows over every point so
far, restricted to the label's period.

Kept points whose zoom-zmax tile lies outside [0, 2^zmax)^2 (|lat| > 85.0511,
lon outside [-180, 180): the reference bins them, tile.py:17,21 never clamp)
do not fit the resident table's keys.  A batch holding any (hm_stream_add
answers HM_E_EXOTIC before inserting anything) is split on the device: the
in-square points go to the table, the out-of-square ones are counted per
(group, hour) by hm_count_grouped and their (rare, pre-aggregated) cell
records are kept beside the table and joined into every rollup.
"""
from __future__ import annotations

import ctypes
import datetime

import numpy as np

from . import _lib, device
from . import heatmap as _hm
from . import raster as _raster
from . import region as _region
from . import top as _top

ALLTIME = -1
EACH_HOUR = -2
MAX_HOURS = 1 << 28
SPANS = {"hour": _lib.HM_SPAN_HOUR, "day": _lib.HM_SPAN_DAY, "month": _lib.HM_SPAN_MONTH,
         "year": _lib.HM_SPAN_YEAR, "alltime": _lib.HM_SPAN_ALLTIME}
NOGROUP = 0xFFFFFFFE      # kept points whose user id makes no group ('x*', or no user ids)
ALLGROUPS = 0xFFFFFFFF    # merged rollups


UNDATED_HOUR = -1         # hour of points added without one (alltime only)


def _sum_records(rec: np.ndarray, w: int) -> np.ndarray:
    """Sum column w of int64 records over equal leading columns [0, w)."""
    if not len(rec):
        return rec
    u, inv = np.unique(rec[:, :w], axis=0, return_inverse=True)
    tot = np.zeros(len(u), dtype=np.int64)
    np.add.at(tot, inv.reshape(-1), rec[:, w])
    return np.concatenate([u, tot[:, None]], axis=1)


def _period(timespan: str, hour: np.ndarray) -> np.ndarray:
    """hm_stream_rollup's period of each epoch hour: the hour, days since
    1970-01-01, year * 12 + month - 1, or the year (UTC civil calendar)."""
    if timespan == "hour":
        return hour
    days = hour // 24
    if timespan == "day":
        return days
    z = days + 719468                    # civil_from_days (H. Hinnant), as k_stream_rollup
    era = np.floor_divide(z, 146097)
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    m = np.where(mp < 10, mp + 3, mp - 9)
    y = yoe + era * 400 + (m <= 2)
    return y * 12 + m - 1 if timespan == "month" else y


def _window_records(x: np.ndarray, hour_lo: int, hour_hi: int, merge_groups: bool) -> np.ndarray:
    """The out-of-square records x (group, hour or UNDATED_HOUR, zoom, row,
    col, count) of a window: the dated ones with hour_lo <= hour < hour_hi,
    summed per (group, zoom, row, col), or over every group (ALLGROUPS)."""
    h = x[:, 1]
    x = x[(h != UNDATED_HOUR) & (h >= hour_lo) & (h < hour_hi)]
    rec = x[:, [0, 2, 3, 4, 5]].copy()
    if merge_groups:
        rec[:, 0] = ALLGROUPS
    return _sum_records(rec, 4)


def _view_records(x: np.ndarray, rects, hours, group) -> np.ndarray:
    """The out-of-square records x (group, hour or UNDATED_HOUR, zoom, row,
    col, count) of a view: those inside any of the (unclipped) rectangles
    (zoom, row_lo, row_hi, col_lo, col_hi), of hours = None (every record,
    undated ones included) or (lo, hi) (the dated ones with lo <= hour < hi),
    and of group = 'merged' (summed over every group: ALLGROUPS), 'each' or
    one group id.  Returns (group, zoom, row, col, count) records."""
    g, h, z, r, c = (x[:, j] for j in range(5))
    m = np.zeros(len(x), dtype=bool)
    for rz, rlo, rhi, clo, chi in rects:
        m |= (z == rz) & (r >= rlo) & (r < rhi) & (c >= clo) & (c < chi)
    if hours is not None:
        m &= (h != UNDATED_HOUR) & (h >= hours[0]) & (h < hours[1])
    if group not in ("merged", "each"):
        m &= g == int(group)
    rec = x[m][:, [0, 2, 3, 4, 5]].copy()
    if group == "merged":
        rec[:, 0] = ALLGROUPS
    return _sum_records(rec, 4)


def _check_min_visitors(min_visitors, what="min_visitors") -> int:
    """The threshold of a visitors query as an int >= 1.  Pure: no device."""
    if isinstance(min_visitors, bool) or not isinstance(min_visitors, (int, np.integer)):
        raise ValueError("%s must be an integer >= 1 (got %r)" % (what, min_visitors))
    if int(min_visitors) < 1:
        raise ValueError("%s must be at least 1 (got %d): a cell with no visitor does not exist"
                         % (what, int(min_visitors)))
    return int(min_visitors)


def _min_users_arg(min_users, user):
    """tile_raster's / tile_images' min_users: None (no threshold: the plain
    raster) or the int >= 1 below which a bin is not drawn.  Together with
    user= it is refused: one user's tile is never k-anonymous.  Pure."""
    if min_users is None:
        return None
    m = _check_min_visitors(min_users, "min_users")
    if user is not None:
        raise ValueError("min_users and user=%r exclude each other: one user's tile is never k-anonymous" % (user,))
    return m


def _visitor_records(x: np.ndarray, rects, hours, min_visitors: int) -> np.ndarray:
    """The out-of-square records x (group, hour or UNDATED_HOUR, zoom, row,
    col, count) of a visitors query: per distinct cell inside the (unclipped)
    rectangles and the hours (as _view_records), its points and the number of
    distinct group ids that own a record of it -- NOGROUP is one id, so the
    records without a group are one visitor together -- kept when that number
    reaches min_visitors.  Returns (zoom, row, col, points, visitors)
    records."""
    rec = _view_records(x, rects, hours, "each")      # one record per (group, cell)
    if not len(rec):
        return np.zeros((0, 5), dtype=np.int64)
    u, inv = np.unique(rec[:, 1:4], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    pts = np.zeros(len(u), dtype=np.int64)
    np.add.at(pts, inv, rec[:, 4])
    vis = np.bincount(inv, minlength=len(u)).astype(np.int64)
    out = np.concatenate([u, pts[:, None], vis[:, None]], axis=1)
    return out[vis >= int(min_visitors)]


def _haloed_rects(tiles, b: int, h: int):
    """The rectangle (zoom, row_lo, row_hi, col_lo, col_hi) of each tile's
    haloed grid: its 2^b x 2^b bins at zoom tz + b and h more on every side,
    not clipped to the square (a view clips)."""
    w = (1 << b) + 2 * h
    return [(tz + b, (tr << b) - h, (tr << b) - h + w, (tc << b) - h, (tc << b) - h + w) for tz, tr, tc in tiles]


def _rects_area(rects) -> int:
    """Cells of the rectangles clipped to the square, overlaps counted twice:
    an upper bound on the distinct cells a view of them returns."""
    return sum((min(rhi, 1 << z) - max(rlo, 0)) * (min(chi, 1 << z) - max(clo, 0))
               for z, rlo, rhi, clo, chi in rects if min(rhi, chi) > 0 and max(rlo, clo) < (1 << z))


def tile_rects(tiles, d: int):
    """The detail-zoom rectangle (zoom, row_lo, row_hi, col_lo, col_hi) of each
    heatmap row tile (tz, tr, tc): its 2^d x 2^d bins at zoom tz + d."""
    return [(tz + d, tr << d, (tr + 1) << d, tc << d, (tc + 1) << d) for tz, tr, tc in tiles]


def _raster_args(zmin: int, zmax: int, index: dict, tiles, hours, user, bins_log2, halo):
    """Validated (tiles, hour_lo, hour_hi, group word or None, bins_log2, halo)
    of StreamingHeatmap.tile_raster on a stream of zooms zmin..zmax whose group
    labels are `index` (label -> id).  The group word is HM_VIEW_MERGED for
    user = None, the label's id, or None for a label the stream has never seen
    (no cell: zero grids).  Pure: needs no device."""
    tiles, b, h = _raster.check_tiles(tiles, bins_log2, halo, zmin, zmax)
    if hours is None:
        lo = hi = _lib.HM_STREAM_ALLTIME
    else:
        lo, hi = int(hours[0]), int(hours[1])
        if hi <= lo:
            raise ValueError("a window needs hour_lo < hour_hi (got %d, %d)" % (lo, hi))
    if user is None:
        gw = _lib.HM_VIEW_MERGED
    elif user == "all":
        raise ValueError("a raster counts points: user='all' (the reference's level-weighted 'all' bins) is a "
                         "property of the row format; use tile_rows(..., user='all'), or user=None for every "
                         "kept point")
    elif not isinstance(user, str):
        raise ValueError("user must be None or a group label (got %r)" % (user,))
    else:
        gw = index.get(user)
    return tiles, lo, hi, gw, b, h


def _frame_args(lo: int, hi: int, frame_hours, trailing):
    """Validated (frame_hours, lead, window) of StreamingHeatmap.tile_frames
    over the hours [lo, hi): `lead` frames are queried before lo and dropped
    after the sums, `window` is raster.accumulate's (None: disjoint frames,
    no sums).  Pure: needs no device."""
    fh = int(frame_hours)
    if fh < 1:
        raise ValueError("frame_hours must be at least 1 (got %r)" % (frame_hours,))
    if trailing is None:
        lead, window = 0, None
    elif trailing == "all":
        lead, window = 0, 0
    elif isinstance(trailing, (int, np.integer)) and not isinstance(trailing, bool) and trailing >= 1:
        lead, window = int(trailing) - 1, int(trailing)
    else:
        raise ValueError("trailing must be None, 'all' or a number of frames >= 1 (got %r)" % (trailing,))
    nf = -((lo - hi) // fh) + lead
    if nf > _lib.HM_RASTER_MAX_FRAMES:
        raise ValueError("%d frames; one call takes at most %d" % (nf, _lib.HM_RASTER_MAX_FRAMES))
    return fh, lead, window


def _check_regions(regions, zmin: int, zmax: int):
    """`regions` as a region.RegionSet a stream of zooms zmin..zmax can query.  Pure."""
    if not isinstance(regions, _region.RegionSet):
        raise ValueError("regions must be a heatmap_amd.region.RegionSet (got %r)" % (type(regions).__name__,))
    if not zmin <= regions.zoom <= zmax:
        raise ValueError("region zoom %d is outside the stream's %d..%d" % (regions.zoom, zmin, zmax))
    return regions


def _region_struct(regions):
    """(hm_regions of a RegionSet, the arrays it points into: keep them alive for the call)"""
    arrays = (regions.row_ptr, regions.col_lo, regions.col_hi, regions.region)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rs = _lib.hm_regions(regions.zoom, regions.row_lo, regions.nrows, regions.nspans, regions.nregions,
                         *(a.ctypes.data_as(u32p) for a in arrays))
    return rs, arrays


def _region_series_args(regions, hours, frame_hours, user, index: dict):
    """Validated (hour_lo, hour_hi, frame_hours, frames, group word or None) of
    StreamingHeatmap.region_series on a stream whose group labels are `index`;
    the group word is tile_raster's (None: a label never seen).  Pure."""
    lo, hi = int(hours[0]), int(hours[1])
    if hi <= lo:
        raise ValueError("a window needs hour_lo < hour_hi (got %d, %d)" % (lo, hi))
    fh = int(frame_hours)
    if fh < 1:
        raise ValueError("frame_hours must be at least 1 (got %r)" % (frame_hours,))
    nf = -((lo - hi) // fh)
    if nf * regions.nregions > _lib.HM_REGION_MAX_TOTALS:
        raise ValueError("%d frames x %d regions; one call takes at most %d totals"
                         % (nf, regions.nregions, _lib.HM_REGION_MAX_TOTALS))
    if user is None:
        gw = _lib.HM_VIEW_MERGED
    elif user == "all":
        raise ValueError("a region total counts points: user='all' (the reference's level-weighted 'all' bins) is a "
                         "property of the row format; use user=None for every kept point")
    elif not isinstance(user, str):
        raise ValueError("user must be None or a group label (got %r)" % (user,))
    else:
        gw = index.get(user)
    return lo, hi, fh, nf, gw


def _cells_subset(cells: "_hm.Cells", m: np.ndarray) -> "_hm.Cells":
    """The bins of cells under the mask m."""
    return _hm.Cells(cells.labels, np.asarray(cells.label)[m], np.asarray(cells.zoom)[m], np.asarray(cells.row)[m],
                     np.asarray(cells.col)[m], np.asarray(cells.value)[m], cells.delta, cells.spans, cells.span[m],
                     tile_override=cells.tile_override)


def _expire_records(x: np.ndarray, before_hour: int):
    """(the records that outlive expire(before_hour), how many are dropped):
    dated records of an hour < before_hour go, undated ones have no time and
    stay."""
    h = x[:, 1]
    gone = (h != UNDATED_HOUR) & (h < before_hour)
    return x[~gone], int(gone.sum())


def _select_labels(users) -> list:
    """Group labels of the reference's user ids, by the rule add(user_id=)
    files them under (_groups): a plain id, 'all' or the literal 'route' is
    its own label.  An 'x...' id never had a group of its own (its points sit
    in the no-group cells, NOGROUP) and an 'rt-...' id was merged into 'route'
    at ingest: neither can be told apart any more, so both are ValueErrors."""
    if isinstance(users, str):
        users = [users]
    out = []
    for u in users:
        if not isinstance(u, str):
            raise TypeError("user id %r is not a string" % (u,))
        if u[:1] == "x":
            raise ValueError("user id %r never had a group of its own: its points are among the cells without a "
                             "group (groups=[NOGROUP] selects all of those)" % (u,))
        if u[:3] == "rt-":
            raise ValueError("user id %r was merged into 'route' when it was added: select 'route'" % (u,))
        out.append(u)
    return out


def _select_ids(users, groups, index: dict):
    """uint32 group ids of a selection: the labels of `users` that `index`
    (label -> id) knows -- one it has never seen selects nothing and is not
    interned -- joined with the explicit ids `groups` (0 .. NOGROUP, NOGROUP:
    the cells without a group), in the order given, repeats kept.  None when
    neither is given: every group."""
    if users is None and groups is None:
        return None
    ids = [index[v] for v in _select_labels(users) if v in index] if users is not None else []
    if groups is not None:
        g = np.atleast_1d(np.asarray(groups))
        if g.size and g.dtype.kind not in "iu":
            raise TypeError("group ids must be integers")
        g = g.reshape(-1).astype(np.uint64 if g.dtype.kind == "u" else np.int64)
        bad = (g < 0) | (g > NOGROUP)
        if bad.any():
            raise ValueError("group id %d is outside 0 .. 0x%X" % (int(g[np.flatnonzero(bad)[0]]), NOGROUP))
        ids += g.tolist()
    if len(ids) > _lib.HM_SELECT_MAX_GROUPS:
        raise ValueError("a selection takes at most %d group ids, not %d" % (_lib.HM_SELECT_MAX_GROUPS, len(ids)))
    return np.array(ids, dtype=np.uint32)


def _select_hours(hours):
    """None (every hour, and the undated cells) or the pair (lo, hi) of a
    selection's hours lo <= hour < hi, as ints"""
    if hours is None:
        return None
    try:
        lo, hi = (int(v) for v in hours)
    except (TypeError, ValueError):
        raise ValueError("hours must be None or a pair (lo, hi), not %r" % (hours,)) from None
    if hi <= lo:
        raise ValueError("hours (%d, %d) hold no hour" % (lo, hi))
    return lo, hi


def _select_records(x: np.ndarray, ids, hours) -> np.ndarray:
    """Mask of the out-of-square records x (group, hour or UNDATED_HOUR, zoom,
    row, col, count) a selection holds: group among ids (None: any) and hour
    in hours = (lo, hi) (None: any, the undated records included; those are
    in no range)."""
    m = np.ones(len(x), dtype=bool)
    if ids is not None:
        m &= np.isin(x[:, 0], np.asarray(ids, dtype=np.int64))
    if hours is not None:
        h = x[:, 1]
        m &= (h != UNDATED_HOUR) & (h >= hours[0]) & (h < hours[1])
    return m


def _forget_records(x: np.ndarray, ids, hours):
    """(the records that outlive forget() of the selection, how many are
    dropped), as _expire_records"""
    gone = _select_records(x, ids, hours)
    return x[~gone], int(gone.sum())


SNAPSHOT_VERSION = 1      # format of snapshot() / save()
_SNAPSHOT_KEYS = ("version", "zmin", "zmax", "base_hour", "labels", "explicit_max", "keys", "counts", "groups",
                  "hours", "x")


def _group_lut(src_labels, index: dict, labels: list) -> np.ndarray:
    """int64 LUT from another stream's group ids (src_labels: its id -> label
    list) to this stream's (index: label -> id, labels: id -> label; labels
    it does not know yet are appended to both).  One more entry than
    src_labels: the last one maps NOGROUP to itself (_remap_groups)."""
    lut = np.empty(len(src_labels) + 1, dtype=np.int64)
    for j, label in enumerate(src_labels):
        label = str(label)
        if label not in index:
            index[label] = len(labels)
            labels.append(label)
        lut[j] = index[label]
    lut[-1] = NOGROUP
    return lut


def _remap_groups(g, lut):
    """Group ids g (int64, a numpy array or a torch tensor) through a
    _group_lut of the same kind: one gather.  NOGROUP passes through; any other
    id without a label is a ValueError naming the first such cell."""
    n = len(lut) - 1
    bad = (g >= n) & (g != NOGROUP)
    if bool(bad.any()):
        i = int(np.flatnonzero(bad)[0]) if isinstance(bad, np.ndarray) else int(bad.nonzero()[0, 0])
        raise ValueError("cell %d: group id %d has no label (the source has %d)" % (i, int(g[i]), n))
    return lut[g.clip(max=n)]


def _explicit_group_max(g) -> int:
    """Largest of the explicit group ids g (int64, numpy or torch) that name a
    group, -1 for none: NOGROUP is a cell without one, and 0xFFFFFFFF is left
    to hm_stream_import, which reports the first invalid cell of any kind."""
    named = g[g < NOGROUP]
    return int(named.max()) if len(named) else -1


def _remap_records(x: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """Out-of-square records x (group, hour, zoom, row, col, count) of another
    stream under this stream's group ids."""
    x = np.array(x, dtype=np.int64).reshape(-1, 6)
    if len(x):
        x[:, 0] = _remap_groups(x[:, 0], lut)
    return x


def _pack_snapshot(zmin, zmax, base_hour, labels, explicit_max, keys, counts, groups, hours, x) -> dict:
    """A stream's state as numpy arrays and plain numbers (snapshot())."""
    return {"version": SNAPSHOT_VERSION, "zmin": int(zmin), "zmax": int(zmax), "base_hour": int(base_hour),
            "labels": np.array([str(v) for v in labels], dtype=np.str_), "explicit_max": int(explicit_max),
            "keys": np.ascontiguousarray(keys, dtype=np.uint64), "counts": np.ascontiguousarray(counts, dtype=np.uint64),
            "groups": np.ascontiguousarray(groups, dtype=np.uint32), "hours": np.ascontiguousarray(hours, dtype=np.uint32),
            "x": np.ascontiguousarray(x, dtype=np.int64).reshape(-1, 6)}


def _unpack_snapshot(snap) -> dict:
    """A snapshot dict or an opened .npz checked and brought to the types
    _pack_snapshot writes; an unknown format version is refused."""
    missing = [k for k in _SNAPSHOT_KEYS if k not in snap]
    if "version" in missing:
        raise ValueError("not a StreamingHeatmap snapshot (no format version)")
    version = int(np.asarray(snap["version"]))
    if version != SNAPSHOT_VERSION:
        raise ValueError("snapshot format version %d is not supported (this package reads version %d)"
                         % (version, SNAPSHOT_VERSION))
    if missing:
        raise ValueError("snapshot lacks %s" % ", ".join(missing))
    out = _pack_snapshot(*(np.asarray(snap[k]) for k in _SNAPSHOT_KEYS[1:4]), np.asarray(snap["labels"]).tolist(),
                         np.asarray(snap["explicit_max"]), snap["keys"], snap["counts"], snap["groups"], snap["hours"],
                         snap["x"])
    n = len(out["keys"])
    if any(len(out[k]) != n for k in ("counts", "groups", "hours")):
        raise ValueError("snapshot arrays differ in length")
    return out


def _save_snapshot(path, snap: dict):
    """np.savez of a snapshot: arrays only, nothing pickled."""
    np.savez(path, **{k: np.asarray(v) for k, v in snap.items()})


def _load_snapshot(path) -> dict:
    with np.load(path, allow_pickle=False) as f:
        return _unpack_snapshot(f)


def _check_zooms(snap: dict, zmin: int, zmax: int):
    if (snap["zmin"], snap["zmax"]) != (zmin, zmax):
        raise ValueError("snapshot holds zooms %d..%d, the stream %d..%d"
                         % (snap["zmin"], snap["zmax"], zmin, zmax))


def span_label(timespan: str, period: int) -> str:
    """build_timespan_label (heatmap.py:38-52) of a rollup period: days since
    1970-01-01, year*12 + month - 1, or the year."""
    if timespan == "alltime":
        return "alltime"
    if timespan == "day":
        d = datetime.date(1970, 1, 1) + datetime.timedelta(days=int(period))
    elif timespan == "month":
        d = datetime.date(int(period) // 12, int(period) % 12 + 1, 1)
    elif timespan == "year":
        d = datetime.date(int(period), 1, 1)
    else:
        raise ValueError("no reference timespan label for %r" % (timespan,))
    return _hm.build_timespan_label(timespan, d)


class StreamingHeatmap:
    def __init__(self, zmin: int = 0, zmax: int = 18, base_hour: int = 0, initial_cells: int = 1 << 20,
                 device_index: int = 0, max_buckets: int = 0):
        self._torch = device._torch()
        self.ctx = device.context(device_index)
        self.device_index = device_index
        self.zmin, self.zmax, self.base_hour = int(zmin), int(zmax), int(base_hour)
        self.labels = ["all"]          # group id -> row-key group (0: the literal user id 'all')
        self._explicit_max = -1        # largest group id passed as group= (those have no label)
        self._index = {"all": 0}
        # cells outside [0, 2^zmax)^2: (group, hour or UNDATED_HOUR, zoom, row, col, count)
        self._x = np.zeros((0, 6), dtype=np.int64)
        self._query_n = {}             # cells of the last query of each kind (_query sizes the next from it)
        p = ctypes.c_void_p()
        rc = self.ctx.L.hm_stream_create(self.ctx.ptr, self.zmin, self.zmax, self.base_hour, int(initial_cells),
                                         int(max_buckets), ctypes.byref(p))
        _lib.raise_for(rc)
        self.ptr = p

    # ------------------------------------------------------------------ input

    def _groups(self, user_id, keep, n):
        """Persistent group ids of a batch's user ids (heatmap.py:64-70): kept
        points only are validated, as heatmap.group_plan does."""
        if len(user_id) != n:
            raise ValueError("user_id must have one entry per point")
        if keep is None:
            kb = np.ones(n, dtype=bool)
        else:
            kb = (keep.cpu().numpy() if hasattr(keep, "cpu") else np.asarray(keep)).astype(bool)
        codes, uniques = _hm._factorize(user_id)
        kept_codes = np.unique(codes[kb])
        if kept_codes.size and kept_codes[0] < 0:
            raise TypeError("'NoneType' object is not subscriptable")
        lut = np.full(len(uniques) + 1, NOGROUP, dtype=np.uint32)   # code -1 -> last entry
        for c in kept_codes.tolist():
            u = uniques[c]
            if not isinstance(u, str):
                raise TypeError("user id %r is not a string" % (u,))
            if _hm.KEY_SEPERATOR in u:
                raise ValueError("user id %r contains the key separator %r" % (u, _hm.KEY_SEPERATOR))
            if u[:1] == "x":
                continue
            label = "route" if u[:3] == "rt-" else u
            if label not in self._index:
                self._index[label] = len(self.labels)
                self.labels.append(label)
            lut[c] = self._index[label]
        return lut[codes]

    def add(self, lat, lon, keep=None, hour=None, user_id=None, group=None):
        """Fold one micro-batch in.  hour: uint32 epoch hours (one per point)
        or None (undated: alltime only).  user_id: the reference's user id per
        point (host strings), or group: explicit uint32 group ids.  Projection
        errors raise as hm_count's do; a failing batch changes no counts."""
        torch = self._torch
        self.ctx.bind_stream()
        la = device._dev(lat, torch.float64, self.device_index)
        lo = device._dev(lon, torch.float64, self.device_index)
        n = la.numel()
        if lo.numel() != n:
            raise ValueError("lat and lon must have the same length")
        if user_id is not None and group is not None:
            raise ValueError("pass user_id or group, not both")
        if user_id is not None:
            group = self._groups(user_id, keep, n)
        elif group is not None:
            # explicit ids: NOGROUP / ALLGROUPS are the table's own markers
            gmax = int((group.to(torch.int64) & 0xFFFFFFFF).max().item()) if isinstance(group, torch.Tensor) and \
                group.numel() else (int(np.asarray(group, dtype=np.uint32).max()) if np.size(group) else 0)
            if gmax >= NOGROUP:
                raise ValueError("group ids must be < 0x%X (0xFFFFFFFE/0xFFFFFFFF are reserved)" % NOGROUP)
            self._explicit_max = max(self._explicit_max, gmax)

        def u32(x, what):
            if x is None:
                return None
            if not isinstance(x, torch.Tensor):
                x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.uint32)).view(np.int32))
            t = device._dev(x, torch.int32, self.device_index)  # uint32 bits
            if t.numel() != n:
                raise ValueError("%s must have one entry per point" % what)
            return t

        hr = u32(hour, "hour")
        gr = u32(group, "group")
        kp = device._dev(keep, torch.uint8, self.device_index) if keep is not None else None
        if kp is not None and kp.numel() != n:
            raise ValueError("keep must have one entry per point")
        rc = self.ctx.L.hm_stream_add(self.ptr, device._ptr(la), device._ptr(lo), device._ptr(kp), device._ptr(hr),
                                      device._ptr(gr), n)
        if rc == _lib.HM_E_EXOTIC:
            self._add_split(la, lo, kp, hr, gr, n)
            return
        self._raise_point(rc)

    def _raise_point(self, rc):
        """raise_for with the index of the batch's first failing point"""
        if rc != _lib.HM_OK:
            _lib.raise_for(rc, self.ctx.last_error()[0])

    def _add_split(self, la, lo, kp, hr, gr, n):
        """The batch holds kept points outside the square: project once on the
        device (zoom zmax), insert the in-square ones, count the others per
        (group, hour) with hm_count_grouped.  A projection error raises before
        anything is inserted (hm_stream_add checks the whole batch)."""
        torch = self._torch
        row = torch.empty(n, dtype=torch.int64, device=la.device)
        col = torch.empty(n, dtype=torch.int64, device=la.device)
        st = torch.empty(n, dtype=torch.uint8, device=la.device)
        rc = self.ctx.L.hm_project(self.ctx.ptr, device._ptr(la), device._ptr(lo), n, self.zmax, device._ptr(row),
                                   device._ptr(col), device._ptr(st))
        self._raise_point(rc)     # before anything is inserted: the batch stays atomic
        lim = 1 << self.zmax
        out = (st == 0) & ((row < 0) | (row >= lim) | (col < 0) | (col >= lim))
        if kp is not None:
            out &= kp != 0
        keep_in = (~out).to(torch.uint8) if kp is None else (kp * (~out).to(torch.uint8))
        rc = self.ctx.L.hm_stream_add(self.ptr, device._ptr(la), device._ptr(lo), device._ptr(keep_in),
                                      device._ptr(hr), device._ptr(gr), n)
        self._raise_point(rc)
        sel = out.nonzero().flatten()
        g = (gr[sel].to(torch.int64) & 0xFFFFFFFF) if gr is not None else torch.full_like(sel, NOGROUP)
        h = (hr[sel].to(torch.int64) & 0xFFFFFFFF) if hr is not None else torch.full_like(sel, UNDATED_HOUR)
        pair, inv = torch.unique(torch.stack([g, h], 1), dim=0, return_inverse=True)
        gc = device.count_grouped(la[sel], lo[sel], inv.to(torch.int32), None, self.zmin, self.zmax,
                                  device=self.device_index)
        pg = pair.cpu().numpy()[gc.group.astype(np.int64)]
        rec = np.stack([pg[:, 0], pg[:, 1], gc.zoom.astype(np.int64), gc.row, gc.col, gc.count.astype(np.int64)],
                       axis=1)
        self._x = _sum_records(np.concatenate([self._x, rec]), 5)

    # ---------------------------------------------------------------- queries

    def cells(self):
        """(distinct (bucket, cell) pairs held, cell-log capacity); compacts
        the log (one bucketed merge) when it holds repeated keys"""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self.ctx.L.hm_stream_cells(self.ptr, ctypes.byref(a), ctypes.byref(b), None)
        _lib.raise_for(rc)
        return a.value, b.value

    def _log_capacity(self) -> int:
        b = ctypes.c_int64(0)
        self.ctx.L.hm_stream_cells(self.ptr, None, ctypes.byref(b), None)
        return b.value

    def buckets(self) -> int:
        """(group, period) buckets in use, rollup labels included"""
        c = ctypes.c_int64(0)
        self.ctx.L.hm_stream_cells(self.ptr, None, None, ctypes.byref(c))
        return c.value

    def _query(self, call, extra: int, cap: int, memo_key=None):
        """A capacity query: call(keys, counts, *extra int32 columns, cap,
        n_out) -> status fills cap-sized CUDA tensors.  HM_E_CAPACITY with n >
        cap: again at n + 1024.  n is remembered under memo_key (None: not) for
        the caller's next starting capacity.  Returns (n, keys, counts,
        *columns)."""
        torch = self._torch
        dev = "cuda:%d" % self.device_index
        while True:
            out = [torch.empty(cap, dtype=torch.int64 if j < 2 else torch.int32, device=dev) for j in range(2 + extra)]
            n = ctypes.c_int64(0)
            rc = call(*(device._ptr(t) for t in out), cap, ctypes.byref(n))
            if rc == _lib.HM_E_CAPACITY and n.value > cap:
                cap = n.value + 1024
                continue
            _lib.raise_for(rc)
            if memo_key is not None:
                self._query_n[memo_key] = n.value
            return (n.value, *out)

    @staticmethod
    def _with_side(out, side):
        """The host columns `out` with the matching columns `side` of the
        out-of-square records (None: the stream holds none) appended."""
        if side is None:
            return out
        return tuple(np.concatenate([a, np.asarray(b).astype(a.dtype)]) for a, b in zip(out, side))

    @classmethod
    def _host_cells(cls, n, keys, counts, columns=(), side=None):
        """A query's first n device cells on the host: (*columns as uint32,
        zoom, row, col, count), then the side records' columns (_with_side)."""
        z, r, c = device.decode_keys(keys[:n].cpu().numpy().view(np.uint64))
        out = (*(t[:n].cpu().numpy().view(np.uint32) for t in columns), z, r, c, counts[:n].cpu().numpy())
        return cls._with_side(out, side)

    def rollup_device(self, timespan: str = "alltime", merge_groups: bool = True, select: int = -1):
        """(n, keys, counts, groups, periods) as torch CUDA tensors: the cells
        of `timespan` summed per (group, period), or over every group."""
        self.ctx.bind_stream()
        span = SPANS[timespan]
        # start from the last rollup of this kind (the log's capacity doubles as
        # batches arrive and can far exceed the distinct cells): a short
        # estimate costs one HM_E_CAPACITY retry with the exact size
        mk = (span, bool(merge_groups), int(select))
        cap = min(max(1024, self._log_capacity()), max(1024, int(self._query_n.get(mk, 1 << 20) * 1.25) + 1024))
        return self._query(lambda *out: self.ctx.L.hm_stream_rollup(self.ptr, span, int(bool(merge_groups)),
                                                                    int(select), *out), 2, cap, mk)

    def rollup(self, timespan: str = "alltime", merge_groups: bool = True, select: int = -1):
        """Host arrays (group u32, period u32, zoom, row, col, count), cells
        outside the square included."""
        n, keys, counts, groups, periods = self.rollup_device(timespan, merge_groups, select)
        return self._host_cells(n, keys, counts, (groups, periods),
                                self._exotic_rollup(timespan, merge_groups, select) if len(self._x) else None)

    def _exotic_rollup(self, timespan, merge_groups, select):
        """The out-of-square records summed per (group, period) of `timespan`
        (the periods hm_stream_rollup uses)."""
        g, h, z, r, c, n = self._x.T
        dated = h != UNDATED_HOUR
        if timespan == "alltime":
            period = np.zeros_like(h)
        else:
            g, h, z, r, c, n = g[dated], h[dated], z[dated], r[dated], c[dated], n[dated]
            period = _period(timespan, h)
        if select >= 0:
            m = period == select
            g, period, z, r, c, n = g[m], period[m], z[m], r[m], c[m], n[m]
        if merge_groups:
            g = np.full_like(g, ALLGROUPS)
        rec = _sum_records(np.stack([g, period, z, r, c, n], axis=1), 5) if len(g) else np.zeros((0, 6), np.int64)
        return (rec[:, 0].astype(np.uint32), rec[:, 1].astype(np.uint32), rec[:, 2].astype(np.int32), rec[:, 3],
                rec[:, 4], rec[:, 5])

    def extract_device(self, hour: int = ALLTIME):
        """(n, keys, counts, hours) as torch CUDA tensors (hm_count key
        layout), summed over groups: hour = ALLTIME, EACH_HOUR or one hour."""
        if hour == ALLTIME:
            n, k, c, _, _ = self.rollup_device("alltime")
            return n, k, c, None
        n, k, c, _, p = self.rollup_device("hour", True, -1 if hour == EACH_HOUR else int(hour))
        return n, k, c, (p if hour == EACH_HOUR else None)

    def counts(self, hour: int = ALLTIME, window=None) -> device.Counts:
        """Cells of every kept point (ALLTIME), of one epoch hour, or of the
        hours window = (lo, hi), lo <= hour < hi (cells outside the square
        included)."""
        if window is not None:
            if hour != ALLTIME:
                raise ValueError("pass hour or window, not both")
            return self.window_counts(*window)
        n, keys, counts, _ = self.extract_device(hour)
        side = self._exotic_rollup("alltime" if hour == ALLTIME else "hour", True,
                                   -1 if hour == ALLTIME else int(hour))[2:] if len(self._x) else None
        return device.Counts(*self._host_cells(n, keys, counts, (), side), 0, [])

    # ------------------------------------------------- windows and retention

    def window_device(self, hour_lo: int, hour_hi: int, merge_groups: bool = True):
        """(n, keys, counts, groups) as torch CUDA tensors: the cells of the
        dated hours hour_lo <= hour < hour_hi summed per group, or over every
        group (hm_stream_window; out-of-square cells not included)."""
        self.ctx.bind_stream()
        if int(hour_hi) <= int(hour_lo):
            raise ValueError("a window needs hour_lo < hour_hi (got %d, %d)" % (hour_lo, hour_hi))
        # sized as rollup_device does: from the last window of this width
        mk = ("window", bool(merge_groups), int(hour_hi) - int(hour_lo))
        cap = min(max(1024, self._log_capacity()), max(1024, int(self._query_n.get(mk, 1 << 20) * 1.25) + 1024))
        return self._query(lambda *out: self.ctx.L.hm_stream_window(self.ptr, int(hour_lo), int(hour_hi),
                                                                    int(bool(merge_groups)), *out), 1, cap, mk)

    def window(self, hour_lo: int, hour_hi: int, merge_groups: bool = True):
        """Host arrays (group u32, zoom, row, col, count) of the window, cells
        outside the square included."""
        n, keys, counts, groups = self.window_device(hour_lo, hour_hi, merge_groups)
        return self._host_cells(n, keys, counts, (groups,),
                                _window_records(self._x, int(hour_lo), int(hour_hi), merge_groups).T
                                if len(self._x) else None)

    def window_counts(self, hour_lo: int, hour_hi: int) -> device.Counts:
        """Cells of every kept point of the hours hour_lo <= hour < hour_hi."""
        _, z, r, c, cnt = self.window(hour_lo, hour_hi, True)
        return device.Counts(z, r, c, cnt, 0, [])

    # -------------------------------------------------- viewports and tiles

    def _view_args(self, rects, hours, group):
        """Validated (int64 rectangle array, hour_lo, hour_hi, group word) of
        hm_stream_view."""
        rects = [tuple(int(v) for v in r) for r in rects]
        if not 1 <= len(rects) <= _lib.HM_VIEW_MAX_RECTS or any(len(r) != 5 for r in rects):
            raise ValueError("a view takes 1..%d rectangles (zoom, row_lo, row_hi, col_lo, col_hi)"
                             % _lib.HM_VIEW_MAX_RECTS)
        for z, rlo, rhi, clo, chi in rects:
            if not self.zmin <= z <= self.zmax:
                raise ValueError("rectangle zoom %d is outside the stream's %d..%d" % (z, self.zmin, self.zmax))
            if rhi <= rlo or chi <= clo:
                raise ValueError("empty rectangle %r (row_hi <= row_lo or col_hi <= col_lo)"
                                 % ((z, rlo, rhi, clo, chi),))
        if hours is None:
            lo = hi = _lib.HM_STREAM_ALLTIME
        else:
            lo, hi = int(hours[0]), int(hours[1])
            if hi <= lo:
                raise ValueError("a window needs hour_lo < hour_hi (got %d, %d)" % (lo, hi))
        if group == "merged":
            gw = _lib.HM_VIEW_MERGED
        elif group == "each":
            gw = _lib.HM_VIEW_EACH
        elif isinstance(group, (int, np.integer)) and 0 <= int(group) <= NOGROUP:
            gw = int(group)
        else:
            raise ValueError("group must be 'merged', 'each' or a group id 0..0x%X (got %r)" % (NOGROUP, group))
        return rects, lo, hi, gw

    def view_device(self, rects, hours=None, group="merged"):
        """(n, keys, counts, groups) as torch CUDA tensors: the cells inside
        any of rects = [(zoom, row_lo, row_hi, col_lo, col_hi)] (lo inclusive,
        hi exclusive, clipped to the square), of hours = None (every cell,
        undated ones included) or (lo, hi), summed over every group
        ('merged'), per group ('each') or of one group id (hm_stream_view;
        out-of-square cells not included)."""
        self.ctx.bind_stream()
        rects, lo, hi, gw = self._view_args(rects, hours, group)
        ra = (ctypes.c_int64 * (5 * len(rects)))(*[v for r in rects for v in r])
        # merged and one-group views hold at most the rectangles' cells; an
        # 'each' view starts from the last one of these rectangles (one
        # HM_E_CAPACITY retry with the exact size when that is short)
        area = _rects_area(rects)
        mk = ("view", tuple(rects), gw if gw < 0 else 0)
        if gw == _lib.HM_VIEW_EACH:
            cap = max(1024, int(self._query_n.get(mk, min(area, 1 << 20)) * 1.25) + 1024)
        else:
            cap = max(1024, min(area, int(self._query_n.get(mk, 1 << 20) * 1.25) + 1024))
        cap = min(max(1024, self._log_capacity()), cap)
        return self._query(lambda *out: self.ctx.L.hm_stream_view(self.ptr, lo, hi, gw, ra, len(rects), *out), 1, cap,
                           mk)

    def view(self, rects, hours=None, group="merged"):
        """Host arrays (group u32, zoom, row, col, count) of the view, with
        the out-of-square cells that lie in the rectangles as given (not
        clipped)."""
        n, keys, counts, groups = self.view_device(rects, hours, group)
        return self._host_cells(n, keys, counts, (groups,),
                                _view_records(self._x, [tuple(int(v) for v in q) for q in rects], hours, group).T
                                if len(self._x) else None)

    def view_counts(self, rects, hours=None) -> device.Counts:
        """Cells of every kept point inside the rectangles (and the hours)."""
        _, z, r, c, cnt = self.view(rects, hours, "merged")
        return device.Counts(z, r, c, cnt, 0, [])

    # ------------------------------------------------------------- visitors

    def visitors_device(self, rects, hours=None, min_visitors=1):
        """(n, keys, points, visitors, withheld_cells, withheld_points): the
        distinct cells of view_device(rects, hours) that at least min_visitors
        different groups produced, as CUDA tensors (int64 keys and points,
        int32 visitors; the first n entries count, in no particular order),
        and how many cells and points stayed below the threshold
        (hm_stream_visitors; out-of-square cells not included).  The records
        without a group are one visitor together, so visitors is a lower
        bound on the distinct people."""
        self.ctx.bind_stream()
        m = _check_min_visitors(min_visitors)
        rects, lo, hi, _ = self._view_args(rects, hours, "merged")
        ra = (ctypes.c_int64 * (5 * len(rects)))(*[v for r in rects for v in r])
        # at most the rectangles' cells, and usually about as many as the last
        # such query of this threshold (one HM_E_CAPACITY retry when short)
        area = _rects_area(rects)
        mk = ("visitors", tuple(rects), m)
        cap = max(1024, min(area, int(self._query_n.get(mk, 1 << 20) * 1.25) + 1024))
        cap = min(max(1024, self._log_capacity()), cap)
        wh = (ctypes.c_int64 * 2)(0, 0)
        n, keys, points, vis = self._query(
            lambda k, c, v, cp, n_out: self.ctx.L.hm_stream_visitors(self.ptr, lo, hi, ra, len(rects), m, k, c, v, cp,
                                                                     n_out, wh), 1, cap, mk)
        return n, keys, points, vis, int(wh[0]), int(wh[1])

    def visitors(self, rects, hours=None, min_visitors=1):
        """Host arrays (zoom, row, col, points, visitors) of the cells inside
        the rectangles (and hours) with at least min_visitors distinct groups,
        with the out-of-square side records that lie in the rectangles as given
        (not clipped, as view's) under the same threshold."""
        n, keys, points, vis, _, _ = self.visitors_device(rects, hours, min_visitors)
        z, r, c = device.decode_keys(keys[:n].cpu().numpy().view(np.uint64))
        out = (z, r, c, points[:n].cpu().numpy(), vis[:n].cpu().numpy().view(np.uint32).astype(np.int64))
        if not len(self._x):
            return out
        # side cells lie outside the square, device cells inside it: the two
        # sets are disjoint, so each part's visitors are already whole
        side = _visitor_records(self._x, [tuple(int(v) for v in q) for q in rects], hours, int(min_visitors))
        return self._with_side(out, side.T)

    def top_visited(self, k, rects, hours=None, min_visitors=1):
        """[((zoom, row, col), visitors, points)]: the k most visited cells
        inside the rectangles (and hours) among those with at least
        min_visitors, in rank order -- visitors descending, then zoom, row,
        col ascending (hm_cells_top over the keys and visitors of
        visitors_device).  The out-of-square side records take part."""
        torch = self._torch
        k = _top.check_k(k)
        n, keys, points, vis, _, _ = self.visitors_device(rects, hours, min_visitors)
        keys, points = keys[:n], points[:n]
        m, tk, tv = _top.top_cells(keys, vis[:n].to(torch.int64) & 0xFFFFFFFF, k, device=self.device_index)
        # the chosen cells' points: their keys are distinct, one masked gather
        chosen = torch.isin(keys, tk) if m else torch.zeros(0, dtype=torch.bool, device=keys.device)
        ck = keys[chosen].cpu().numpy().view(np.uint64) if m else np.zeros(0, np.uint64)
        cp = points[chosen].cpu().numpy() if m else np.zeros(0, np.int64)
        cz, cr, cc = device.decode_keys(ck)
        pts = {(int(a), int(b), int(d)): int(e) for a, b, d, e in zip(cz, cr, cc, cp)}
        z, r, c = device.decode_keys(tk.cpu().numpy().view(np.uint64))
        side = None
        if len(self._x):
            rec = _visitor_records(self._x, [tuple(int(v) for v in q) for q in rects], hours, int(min_visitors))
            side = (rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 4])
            pts.update({(int(a), int(b), int(d)): int(e) for a, b, d, e in rec[:, :4].tolist()})
        z, r, c, v = _top.join_ranked(z, r, c, tv.cpu().numpy(), side, k)
        return [((int(a), int(b), int(d)), int(e), pts[(int(a), int(b), int(d))]) for a, b, d, e in zip(z, r, c, v)]

    def _tile_threshold_raster(self, tiles, hours, bins_log2, halo, min_users, what):
        """int64 CUDA tensor [T, W, W]: the tiles' grids from the cells with at
        least min_users visitors -- their points (what = 'points') or their
        visitors -- through visitors_device over the tiles' haloed rectangles
        and hm_cells_raster.  HM_VIEW_MAX_RECTS tiles per query, and each
        query's cells are drawn only into its own tiles' grids: a cell inside
        the halos of two chunks is in both queries and must not be added
        twice."""
        torch = self._torch
        tiles, _, _, _, b, h = _raster_args(self.zmin, self.zmax, self._index, tiles, hours, None, bins_log2, halo)
        w = (1 << b) + 2 * h
        grid = torch.empty((len(tiles), w, w), dtype=torch.int64, device="cuda:%d" % self.device_index)
        for j in range(0, len(tiles), _lib.HM_VIEW_MAX_RECTS):
            part = tiles[j:j + _lib.HM_VIEW_MAX_RECTS]
            n, keys, points, vis, _, _ = self.visitors_device(_haloed_rects(part, b, h), hours, min_users)
            vals = points[:n] if what == "points" else vis[:n].to(torch.int64) & 0xFFFFFFFF
            grid[j:j + len(part)] = _raster.raster_cells(keys[:n], vals, part, b, h, device=self.device_index)
        return grid

    def tile_visitors(self, tiles, hours=None, bins_log2=5, halo=0, min_users=1):
        """int64 CUDA tensor [T, W, W]: tile_raster's grids holding each bin's
        distinct visitors instead of its points, bins below min_users left 0
        (visitors_device, then hm_cells_raster of the keys and visitors)."""
        return self._tile_threshold_raster(tiles, hours, bins_log2, halo, _check_min_visitors(min_users, "min_users"),
                                           "visitors")

    # -------------------------------------------------------------- regions

    def _region_table(self, regions):
        """(hm_regions struct of a region.RegionSet, the arrays it points into)"""
        return _region_struct(_check_regions(regions, self.zmin, self.zmax))

    def region_series(self, regions, hours, frame_hours=1, user=None):
        """int64 CUDA tensor [F, R]: the kept points inside each region of
        `regions` (a region.RegionSet) per frame of hours = (lo, hi), cut into
        F = ceil((hi - lo) / frame_hours) frames anchored at lo as tile_frames
        cuts them -- one chart line per district, or a choropleth per hour --
        for every group merged (user = None) or the group label `user` (an
        unknown label: zeros).  A cell inside several regions counts in each.
        hm_stream_region_series: ONE filter pass over the log with the sums
        reduced on the device; undated points are in no frame, and the
        out-of-square side records never belong to a region (spans end at the
        square)."""
        torch = self._torch
        self.ctx.bind_stream()
        if hours is None:
            raise ValueError("a series needs hours = (lo, hi): alltime has no first frame (region_totals sums it)")
        lo, hi, fh, nf, gw = _region_series_args(regions, hours, frame_hours, user, self._index)
        rs, keep = self._region_table(regions)
        dev = "cuda:%d" % self.device_index
        if gw is None:
            return torch.zeros((nf, regions.nregions), dtype=torch.int64, device=dev)
        out = torch.empty((nf, regions.nregions), dtype=torch.int64, device=dev)
        rc = self.ctx.L.hm_stream_region_series(self.ptr, lo, hi, fh, gw, ctypes.byref(rs), device._ptr(out))
        _lib.raise_for(rc)
        return out

    def region_totals(self, regions, hours=None, user=None):
        """int64 CUDA tensor [R]: the kept points inside each region, of hours
        = None (every kept point, undated ones included) or (lo, hi) -- the
        sum of region_series over the same hours, as one frame."""
        torch = self._torch
        self.ctx.bind_stream()
        if hours is not None:
            lo, hi = int(hours[0]), int(hours[1])
            return self.region_series(regions, hours, max(hi - lo, 1), user)[0]
        _, _, _, _, gw = _region_series_args(regions, (0, 1), 1, user, self._index)
        rs, keep = self._region_table(regions)
        dev = "cuda:%d" % self.device_index
        if gw is None:
            return torch.zeros(regions.nregions, dtype=torch.int64, device=dev)
        out = torch.empty(regions.nregions, dtype=torch.int64, device=dev)
        rc = self.ctx.L.hm_stream_region_series(self.ptr, _lib.HM_STREAM_ALLTIME, _lib.HM_STREAM_ALLTIME, 1, gw,
                                                ctypes.byref(rs), device._ptr(out))
        _lib.raise_for(rc)
        return out

    def region_view_device(self, regions, hours=None, group="merged"):
        """(n, keys, counts, groups) as torch CUDA tensors, what view_device
        returns: the distinct cells that any region of `regions` covers (a cell
        inside several is listed once), of hours = None or (lo, hi), summed
        over every group ('merged'), per group ('each') or of one group id
        (hm_stream_region_view; out-of-square cells never belong to a
        region)."""
        self.ctx.bind_stream()
        rs, keep = self._region_table(regions)
        _, lo, hi, gw = self._view_args([(self.zmin, 0, 1, 0, 1)], hours, group)
        # sized as view_device does it: at most the regions' cells for a merged
        # or one-group view, else from the last such query
        area = int(regions.area().sum())
        mk = ("region_view", id(regions), gw if gw < 0 else 0)
        if gw == _lib.HM_VIEW_EACH:
            cap = max(1024, int(self._query_n.get(mk, min(area, 1 << 20)) * 1.25) + 1024)
        else:
            cap = max(1024, min(area, int(self._query_n.get(mk, 1 << 20) * 1.25) + 1024))
        cap = min(max(1024, self._log_capacity()), cap)
        return self._query(lambda *out: self.ctx.L.hm_stream_region_view(self.ptr, lo, hi, gw, ctypes.byref(rs), *out),
                           1, cap, mk)

    def region_view(self, regions, hours=None, group="merged"):
        """Host arrays (group u32, zoom, row, col, count) of region_view_device.
        top.top_cells over region_view_device's keys and counts gives the
        hottest cells inside a polygon."""
        n, keys, counts, groups = self.region_view_device(regions, hours, group)
        return self._host_cells(n, keys, counts, (groups,))

    def region_counts(self, regions, hours=None) -> device.Counts:
        """Cells of every kept point inside the regions (and the hours)."""
        _, z, r, c, cnt = self.region_view(regions, hours, "merged")
        return device.Counts(z, r, c, cnt, 0, [])

    def region_visitors(self, regions, hours=None, min_visitors=1):
        """(points [R], visitors [R], withheld_regions, withheld_points): per
        region its kept points and the distinct groups that produced them, as
        numpy int64 arrays; a region with fewer than min_visitors gets 0 and
        0, and the last two numbers count those regions (the ones with at
        least one visitor) and their points.  The records without a group are
        one visitor together, so visitors is a lower bound on the distinct
        people (hm_stream_region_visitors; out-of-square cells never belong to
        a region)."""
        torch = self._torch
        self.ctx.bind_stream()
        m = _check_min_visitors(min_visitors)
        rs, keep = self._region_table(regions)
        _, lo, hi, _ = self._view_args([(self.zmin, 0, 1, 0, 1)], hours, "merged")
        dev = "cuda:%d" % self.device_index
        pts = torch.empty(regions.nregions, dtype=torch.int64, device=dev)
        vis = torch.empty(regions.nregions, dtype=torch.int32, device=dev)
        wh = (ctypes.c_int64 * 2)(0, 0)
        rc = self.ctx.L.hm_stream_region_visitors(self.ptr, lo, hi, ctypes.byref(rs), m, device._ptr(pts),
                                                  device._ptr(vis), wh)
        _lib.raise_for(rc)
        return (pts.cpu().numpy(), vis.cpu().numpy().view(np.uint32).astype(np.int64), int(wh[0]), int(wh[1]))

    # ------------------------------------------------------------- rankings

    def top_device(self, k, rects, hours=None, group="merged"):
        """(n, keys, counts, cells): of the `cells` distinct summed cells that
        view_device(rects, hours, group) would return, the first n = min(k,
        cells) in rank order (count descending, then HM_KEY ascending) as
        int64 CUDA tensors of n entries (hm_stream_top: the view's filter and
        merge, then a device selection that emits k cells, not all of them).
        group is 'merged' or one group id; out-of-square cells not included."""
        torch = self._torch
        self.ctx.bind_stream()
        k = _top.check_k(k)
        if group == "each":
            raise ValueError("a ranking takes group='merged' or one group id (a ranking per group is out of reach "
                             "of one call: rank each group's id in turn)")
        rects, lo, hi, gw = self._view_args(rects, hours, group)
        ra = (ctypes.c_int64 * (5 * len(rects)))(*[v for r in rects for v in r])
        dev = "cuda:%d" % self.device_index
        keys = torch.empty(k, dtype=torch.int64, device=dev)
        counts = torch.empty(k, dtype=torch.int64, device=dev)
        n, cells = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self.ctx.L.hm_stream_top(self.ptr, lo, hi, gw, ra, len(rects), k, device._ptr(keys), device._ptr(counts),
                                      ctypes.byref(n), ctypes.byref(cells))
        _lib.raise_for(rc)
        return n.value, keys[:n.value], counts[:n.value], cells.value

    def top(self, k, rects, hours=None, group="merged"):
        """Host arrays (zoom, row, col, count) of the k hottest cells inside
        the rectangles (and hours, and group), in rank order: count
        descending, then zoom, row, col ascending.  The out-of-square side
        records inside the rectangles as given (not clipped, as view's) take
        part."""
        n, keys, counts, _ = self.top_device(k, rects, hours, group)
        z, r, c = device.decode_keys(keys.cpu().numpy().view(np.uint64))
        side = None
        if len(self._x):
            side = _view_records(self._x, [tuple(int(v) for v in q) for q in rects], hours, group).T[1:]
        return _top.join_ranked(z, r, c, counts.cpu().numpy(), side, k)

    def top_tiles(self, k, zoom, hours=None, user=None, within=None):
        """[((zoom, row, col), count)]: the k busiest cells of one zoom, in
        rank order -- of the whole zoom, or only inside the heatmap tiles
        within = [(tz, tr, tc)] (1..HM_VIEW_MAX_RECTS of them, tz <= zoom) --
        for every kept point (user = None) or the group label `user` (an
        unknown label: no cells)."""
        zoom = int(zoom)
        if not self.zmin <= zoom <= self.zmax:
            raise ValueError("zoom %d is outside the stream's %d..%d" % (zoom, self.zmin, self.zmax))
        if within is None:
            rects = [(zoom, 0, 1 << zoom, 0, 1 << zoom)]
        else:
            tiles = [tuple(int(v) for v in t) for t in within]
            if not 1 <= len(tiles) <= _lib.HM_VIEW_MAX_RECTS or any(len(t) != 3 for t in tiles):
                raise ValueError("within takes 1..%d tiles (tz, tr, tc)" % _lib.HM_VIEW_MAX_RECTS)
            for tz, tr, tc in tiles:
                if not 0 <= tz <= zoom or not (0 <= tr < (1 << tz) and 0 <= tc < (1 << tz)):
                    raise ValueError("tile %r is not a tile of zooms 0..%d inside the square" % ((tz, tr, tc), zoom))
            rects = tile_rects(tiles, 0)
            rects = [(zoom, rlo << (zoom - z), rhi << (zoom - z), clo << (zoom - z), chi << (zoom - z))
                     for z, rlo, rhi, clo, chi in rects]
        # the group word as tile_raster resolves it
        gw = _raster_args(self.zmin, self.zmax, self._index, [(zoom, 0, 0)], hours, user, 0, 0)[3]
        _top.check_k(k)
        if gw is None:
            return []
        z, r, c, n = self.top(k, rects, hours, "merged" if gw == _lib.HM_VIEW_MERGED else gw)
        return [((int(a), int(b), int(d)), int(e)) for a, b, d, e in zip(z, r, c, n)]

    def _top_groups_device(self, k, rects, lo, hi):
        torch = self._torch
        ra = (ctypes.c_int64 * (5 * len(rects)))(*[v for r in rects for v in r])
        dev = "cuda:%d" % self.device_index
        ids = torch.empty(k, dtype=torch.int32, device=dev)
        counts = torch.empty(k, dtype=torch.int64, device=dev)
        n, total = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self.ctx.L.hm_stream_top_groups(self.ptr, lo, hi, ra, len(rects), k, device._ptr(ids),
                                             device._ptr(counts), ctypes.byref(n), ctypes.byref(total))
        _lib.raise_for(rc)
        return (ids[:n.value].cpu().numpy().view(np.uint32).astype(np.int64), counts[:n.value].cpu().numpy(),
                total.value)

    def top_groups(self, k, rects, hours=None):
        """Host arrays (group ids uint32, points): the k most active groups
        inside the rectangles (all of one zoom) and hours, by their kept
        points there -- count descending, then id ascending; the points
        without a group rank as id 0xFFFFFFFE.  A cell in several rectangles
        counts once.  Out-of-square side records inside the rectangles as
        given are counted (hm_stream_top_groups)."""
        self.ctx.bind_stream()
        k = _top.check_k(k)
        rects, lo, hi, _ = self._view_args(rects, hours, "merged")
        if len({r[0] for r in rects}) != 1:
            raise ValueError("the rectangles of a group ranking must be of one zoom: every point is counted once per "
                             "zoom")
        side = _view_records(self._x, rects, hours, "each") if len(self._x) else np.zeros((0, 5), np.int64)
        extra = {}
        for g, n in zip(side[:, 0].tolist(), side[:, 4].tolist()):
            extra[g] = extra.get(g, 0) + n
        ids, counts, total = self._top_groups_device(min(_lib.HM_TOP_MAX_K, k + len(extra)), rects, lo, hi)
        if extra:
            # a group with side records ranks by both parts: its device part
            # when the ranking did not reach it is one group-select view
            have = dict(zip(ids.tolist(), counts.tolist()))
            for g, n in extra.items():
                if g not in have and total > len(ids):
                    nv, _, vc, _ = self.view_device(rects, hours, int(g))
                    have[g] = int(vc[:nv].sum().item())
                have[g] = have.get(g, 0) + n
            ids = np.fromiter(have.keys(), np.int64, len(have))
            counts = np.fromiter(have.values(), np.int64, len(have))
            order = _top.rank_order(ids, counts)[:k]
            ids, counts = ids[order], counts[order]
        return ids[:k].astype(np.uint32), counts[:k]

    def top_users(self, k, rects, hours=None):
        """[(label, points)]: the k most active user groups inside the
        rectangles and hours, in rank order (top_groups without the points
        that have no group: it asks for k + 1 groups and drops that entry; at
        k = HM_TOP_MAX_K, when the entry took one of the places, the totals
        come from a per-group view instead)."""
        k = _top.check_k(k)
        if self._explicit_max >= len(self.labels):
            raise ValueError("rows need a label per group: group id %d was passed as group= and has none "
                             "(feed the stream with user_id= to build rows)" % self._explicit_max)
        if k < _lib.HM_TOP_MAX_K:
            ids, counts = self.top_groups(k + 1, rects, hours)
        else:
            ids, counts = self.top_groups(k, rects, hours)
            if len(ids) == k and NOGROUP in ids.tolist():
                # k + 1 groups are out of a ranking's reach and the no-group entry took a place: every
                # group's total from a view, as before there were rankings
                g, _, _, _, n = self.view(rects, hours, "each")
                tot = _sum_records(np.stack([g.astype(np.int64), n.astype(np.int64)], axis=1), 1)
                order = _top.rank_order(tot[:, 0], tot[:, 1])
                ids, counts = tot[order, 0], tot[order, 1]
        return [(self.labels[g], int(n)) for g, n in zip(ids.tolist(), counts.tolist()) if g != NOGROUP][:k]

    def tile_cells(self, tiles, hours=None, label=None, user=None, max_zoom_level=None, delta=None) -> "_hm.Cells":
        """The bins of the rows of the heatmap row tiles [(tz, tr, tc)]: those
        of window_cells(lo, hi, label) for hours = (lo, hi), of
        heatmap_cells('alltime') for hours = None, restricted to the tiles (and
        to the rows of the group label `user`, when given).  Each tile is one
        rectangle of a device view (tile_rects), 32 tiles per query."""
        d = _hm.DETAIL_ZOOM_DELTA if delta is None else int(delta)
        mz = self.zmax - d if max_zoom_level is None else int(max_zoom_level)
        if mz + d != self.zmax or self.zmin > d + 1:
            raise ValueError("rows need zooms %d..%d; the stream holds %d..%d" % (d + 1, mz + d, self.zmin, self.zmax))
        if hours is None:
            label = "alltime"
        elif not isinstance(label, str) or _hm.KEY_SEPERATOR in label:
            raise ValueError("window label %r must be a string without the key separator %r"
                             % (label, _hm.KEY_SEPERATOR))
        elif int(hours[1]) <= int(hours[0]):
            raise ValueError("a window needs hour_lo < hour_hi (got %d, %d)" % (hours[0], hours[1]))
        if self._explicit_max >= len(self.labels):
            raise ValueError("rows need a label per group: group id %d was passed as group= and has none "
                             "(feed the stream with user_id= to build rows)" % self._explicit_max)
        tiles = sorted({tuple(int(v) for v in t) for t in tiles})
        for tz, tr, tc in tiles:
            if not 1 <= tz <= mz or not (0 <= tr < (1 << tz) and 0 <= tc < (1 << tz)):
                raise ValueError("tile %r is not a heatmap row tile of zooms 1..%d inside the square"
                                 % ((tz, tr, tc), mz))
        gid = None if user is None else self._index.get(user, -1)
        det = self._x[self._x[:, 2] == self.zmax]
        if len(det) and not _hm._in_chain_window(det[:, 3], det[:, 4], self.zmax, d).all():
            # side records outside the chain windows move between tiles (ChainFix):
            # every cell is needed, the rows are filtered afterwards
            cells = (self.heatmap_cells("alltime", max_zoom_level, delta) if hours is None else
                     self.window_cells(hours[0], hours[1], label, max_zoom_level, delta))
            want = set(tiles)
            m = np.array([t in want for t in zip(*(a.tolist() for a in cells.row_tiles()))], dtype=bool)
            return _cells_subset(cells, m if gid is None else m & (np.asarray(cells.label) == gid))
        # one group's rows are its own cells: a group-select query (the literal
        # 'all' rows, group 0, need every group's; an unknown label has none)
        select = gid is not None and gid > 0
        todo = range(0, len(tiles) if gid != -1 else 0, _lib.HM_VIEW_MAX_RECTS)
        parts = [self.view(tile_rects(tiles[j:j + _lib.HM_VIEW_MAX_RECTS], d), hours, gid if select else "each")
                 for j in todo]
        gg, gz, gr, gc, gn = (np.concatenate([p[j] for p in parts]).astype(np.int64) if parts else
                              np.zeros(0, np.int64) for j in range(5))
        if select:
            return _hm.Cells(self.labels, gg, gz, gr, gc, gn.astype(np.float64), d, [label])
        # n: every group's cells summed; the grouped cells: those with a label
        al = _sum_records(np.stack([gz, gr, gc, gn], axis=1), 3)
        q = gg != NOGROUP
        cells = _hm.combine_cells(self.labels, (al[:, 0], al[:, 1], al[:, 2], al[:, 3]),
                                  (gg[q], gz[q], gr[q], gc[q], gn[q]), mz + d, d, label)
        return cells if gid is None else _cells_subset(cells, np.asarray(cells.label) == gid)

    def tile_rows(self, tiles, hours=None, label=None, user=None, max_zoom_level=None, delta=None) -> dict:
        """{row_id: {bin_id: float}}: exactly the entries of window_rows(lo,
        hi, label) (rows('alltime') for hours = None) whose tile is in tiles
        = [(tz, tr, tc)], or those of the group label `user` alone; tiles
        without data have no row."""
        return _hm.cells_to_rows(self.tile_cells(tiles, hours, label, user, max_zoom_level, delta))

    def tile_table(self, tiles, hours=None, label=None, user=None, max_zoom_level=None, delta=None):
        """The same rows as a pyarrow Table(id, heatmap JSON)."""
        return _hm.cells_to_table(self.tile_cells(tiles, hours, label, user, max_zoom_level, delta))

    def tile_raster(self, tiles, hours=None, user=None, bins_log2=5, halo=0, min_users=None):
        """int64 CUDA tensor [T, W, W], W = 2^bins_log2 + 2 halo: the point
        counts of the tiles [(tz, tr, tc)] as dense grids of zoom tz +
        bins_log2 bins, each with a halo of its neighbours' bins, of hours =
        None (every kept point) or (lo, hi), for every group merged (user =
        None) or the group label `user` (an unknown label: zero grids).
        hm_stream_raster: one filter pass over the log, no merge; the
        out-of-square side records are never drawn.

        min_users = k (>= 1): k-anonymous tiles -- a bin that fewer than k
        distinct groups produced stays 0 (hm_stream_visitors over the tiles'
        haloed rectangles, then hm_cells_raster of the emitted cells), so the
        tile can be published; not together with user=."""
        m = _min_users_arg(min_users, user)
        if m is not None:
            return self._tile_threshold_raster(tiles, hours, bins_log2, halo, m, "points")
        torch = self._torch
        self.ctx.bind_stream()
        tiles, lo, hi, gw, b, h = _raster_args(self.zmin, self.zmax, self._index, tiles, hours, user, bins_log2, halo)
        w = (1 << b) + 2 * h
        dev = "cuda:%d" % self.device_index
        if gw is None:
            return torch.zeros((len(tiles), w, w), dtype=torch.int64, device=dev)
        grid = torch.empty((len(tiles), w, w), dtype=torch.int64, device=dev)
        for j in range(0, len(tiles), _lib.HM_RASTER_MAX_TILES):
            part = tiles[j:j + _lib.HM_RASTER_MAX_TILES]
            rc = self.ctx.L.hm_stream_raster(self.ptr, lo, hi, gw, _raster._tile_array(part), len(part), b, h,
                                             device._ptr(grid[j:j + len(part)]))
            _lib.raise_for(rc)
        return grid

    def tile_images(self, tiles, hours=None, user=None, bins_log2=8, radius=2, scale="log", vmax=None, ramp="heat",
                    min_users=None):
        """uint8 CUDA tensor [T, S, S, 4], S = 2^bins_log2: the tiles as RGBA
        images -- tile_raster with halo = radius, then raster.render (binomial
        blur of `radius`, 'log' or 'linear' levels against vmax, or the
        call's own maximum, coloured through ramp).  raster.png_bytes turns
        one into a PNG.  min_users: tile_raster's, the bins below it are not
        drawn."""
        _raster.check_render(bins_log2, radius, radius, scale, vmax)
        grid = self.tile_raster(tiles, hours, user, bins_log2, halo=radius, min_users=min_users)
        return _raster.render(grid, bins_log2, radius, radius, scale, vmax, ramp)[0]

    def tile_frames(self, tiles, hours, frame_hours=1, user=None, bins_log2=5, halo=0, trailing=None):
        """int64 CUDA tensor [F, T, W, W]: tile_raster with a time axis, for a
        time slider or an animation, in ONE pass over the log
        (hm_stream_raster_frames) instead of one per frame.  hours = (lo, hi)
        is cut into F = ceil((hi - lo) / frame_hours) frames anchored at lo;
        frame f holds the hours [lo + f fh, lo + (f + 1) fh), the last one up
        to hi.  Undated points are in no frame.

        trailing = k (an int >= 1): frame f holds the k frame lengths that END
        with it, the hours [lo + (f + 1 - k) fh, lo + (f + 1) fh) -- "the
        trailing 24 hours, advancing hourly" is frame_hours = 1, trailing =
        24.  The frames are queried from lo - (k - 1) fh on, summed with
        raster.accumulate(window = k) and the first k - 1 dropped, so every
        returned frame is a whole window.  trailing = 'all': frame f holds
        [lo, lo + (f + 1) fh), the growth since lo."""
        torch = self._torch
        self.ctx.bind_stream()
        if hours is None:
            raise ValueError("frames need hours = (lo, hi): alltime has no first frame")
        tiles, lo, hi, gw, b, h = _raster_args(self.zmin, self.zmax, self._index, tiles, hours, user, bins_log2, halo)
        fh, lead, window = _frame_args(lo, hi, frame_hours, trailing)
        nf = -((lo - lead * fh - hi) // fh)
        w = (1 << b) + 2 * h
        dev = "cuda:%d" % self.device_index
        if gw is None:
            return torch.zeros((nf - lead, len(tiles), w, w), dtype=torch.int64, device=dev)
        grid = torch.empty((nf, len(tiles), w, w), dtype=torch.int64, device=dev)
        for j in range(0, len(tiles), _lib.HM_RASTER_MAX_TILES):
            part = tiles[j:j + _lib.HM_RASTER_MAX_TILES]
            # a call's frames are contiguous [nf][its tiles]: parts are joined along T
            g = grid if len(part) == len(tiles) else torch.empty((nf, len(part), w, w), dtype=torch.int64, device=dev)
            rc = self.ctx.L.hm_stream_raster_frames(self.ptr, lo - lead * fh, hi, fh, gw, _raster._tile_array(part),
                                                    len(part), b, h, device._ptr(g))
            _lib.raise_for(rc)
            if g is not grid:
                grid[:, j:j + len(part)] = g
        if window is None:
            return grid
        return _raster.accumulate(grid, window)[lead:]

    def tile_series(self, tiles, hours, frame_hours=1, user=None):
        """int64 CUDA tensor [F, T]: the kept points inside each tile (tz, tr,
        tc) per frame of hours = (lo, hi) -- a per-hour chart; a viewport's
        series is the sum over its covering tiles.  tile_frames with bins_log2
        = 0, where a tile's grid is its own cell: no kernel of its own."""
        return self.tile_frames(tiles, hours, frame_hours, user, bins_log2=0, halo=0)[:, :, 0, 0]

    def tile_frame_images(self, tiles, hours, frame_hours=1, user=None, bins_log2=8, radius=2, scale="log", vmax=None,
                          ramp="heat", trailing=None):
        """uint8 CUDA tensor [F, T, S, S, 4]: the frames of tile_frames (halo
        = radius) as RGBA images, every frame on ONE scale so the animation
        does not flicker.  vmax = None finds that scale in two render passes:
        every frame is rendered once on its own to read back its largest
        blurred value vs (in units of 2^-(4 radius)); the largest of them is
        rounded up to a whole count, vmax = ceil(vs / 2^(4 radius)), and every
        frame is rendered again with that fixed vmax.  raster.apng_bytes turns
        one tile's frames, [:, t], into an animated PNG."""
        b, h, r, _, _ = _raster.check_render(bins_log2, radius, radius, scale, vmax)
        grid = self.tile_frames(tiles, hours, frame_hours, user, b, halo=r, trailing=trailing)
        step = _lib.HM_RASTER_MAX_TILES
        if vmax is None:
            vs = max(_raster.render(grid[f, j:j + step], b, r, r, scale, None, ramp)[1]
                     for f in range(grid.shape[0]) for j in range(0, grid.shape[1], step))
            vmax = max(1, -(-vs >> (4 * r)))
        return self._torch.stack([_raster.render(grid[f], b, r, r, scale, vmax, ramp)[0] for f in range(grid.shape[0])])

    def expire(self, before_hour: int):
        """Retention: drop the cells of every hour < before_hour (undated
        points stay) and free their buckets and every rollup label's.
        Returns (cells dropped, bucket slots freed)."""
        self.ctx.bind_stream()
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self.ctx.L.hm_stream_expire(self.ptr, int(before_hour), ctypes.byref(a), ctypes.byref(b))
        _lib.raise_for(rc)
        self._x, gone = _expire_records(self._x, int(before_hour))
        return a.value + gone, b.value

    # ------------------------------------------------------------ selections

    def _selection(self, users, groups, hours):
        """The selection of forget / export / snapshot / merge_from checked:
        (group ids as uint32 or None for every group, (lo, hi) or None for
        every hour and the undated cells), or None when no argument is given.
        users: the reference's user ids as given to add(user_id=)
        (_select_labels); groups: explicit ids, NOGROUP for the cells without
        a group; their union is taken."""
        if users is None and groups is None and hours is None:
            return None
        return _select_ids(users, groups, self._index), _select_hours(hours)

    @staticmethod
    def _select_args(ids, hours):
        """(groups, ngroups, hour_lo, hour_hi) of the C selection, and the
        array the pointer reads"""
        lo, hi = (_lib.HM_STREAM_ALLTIME, _lib.HM_STREAM_ALLTIME) if hours is None else hours
        if ids is None:
            return (None, 0, lo, hi), None
        arr = np.ascontiguousarray(ids, dtype=np.uint32)
        return (arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(arr), lo, hi), arr

    def forget(self, users=None, groups=None, hours=None):
        """Erase a part of the stream (hm_stream_forget): the cells of these
        users (their ids as given to add(user_id=); an 'x...' or 'rt-...' id
        is a ValueError, _select_labels) and explicit group ids (NOGROUP: the
        cells without a group), every group when neither is given, of the
        hours (lo, hi) or, with hours=None, of every hour and the undated
        cells.  One pass over the log; the forgotten buckets and every rollup
        label's are freed as expire() frees them.  Labels keep their ids, and
        a forgotten user's label stays in `labels`.  A later add() may bring
        the same user or hour back.  Returns (cells dropped, bucket slots
        freed)."""
        sel = self._selection(users, groups, hours)
        if sel is None:
            raise ValueError("forget() needs users, groups or hours: nothing is forgotten by default")
        ids, hr = sel
        self.ctx.bind_stream()
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        if ids is None or len(ids):          # (no id left: none of the users is known here)
            args, _alive = self._select_args(ids, hr)
            rc = self.ctx.L.hm_stream_forget(self.ptr, *args, ctypes.byref(a), ctypes.byref(b))
            _lib.raise_for(rc)
        self._x, gone = _forget_records(self._x, ids, hr)
        return a.value + gone, b.value

    # ------------------------------------------------- snapshots and merging

    def export_device(self, users=None, groups=None, hours=None):
        """(n, keys, counts, groups, hours) as torch CUDA tensors: the whole
        resident state, one record per distinct (group, hour, cell)
        (hm_stream_export: hm_count key layout, group NOGROUP for none, hour
        HM_STREAM_UNDATED's bits for an undated cell; out-of-square cells not
        included).  With users, groups or hours (as forget()'s) only that
        selection's records (hm_stream_export_select)."""
        self.ctx.bind_stream()
        sel = self._selection(users, groups, hours)
        if sel is None:
            cap = max(1, self.cells()[0])      # exact: the export compacts the log as cells() does
            return self._query(lambda *out: self.ctx.L.hm_stream_export(self.ptr, *out), 2, cap)
        ids, hr = sel
        if ids is not None and not len(ids):
            dev = "cuda:%d" % self.device_index
            return (0, *(self._torch.empty(0, dtype=t, device=dev)
                         for t in (self._torch.int64,) * 2 + (self._torch.int32,) * 2))
        args, _alive = self._select_args(ids, hr)
        return self._query(lambda *out: self.ctx.L.hm_stream_export_select(self.ptr, *args, *out), 2,
                           self._query_n.get("export_select", 1 << 16) + 1024, "export_select")

    def _side(self, sel):
        """the out-of-square records of a selection (None: all of them)"""
        return self._x if sel is None else self._x[_select_records(self._x, *sel)]

    def export(self, users=None, groups=None, hours=None):
        """Host arrays (group u32, hour int64, zoom, row, col, count) of every
        record held, hour UNDATED_HOUR (-1) for undated cells, cells outside
        the square included; with users, groups or hours (as forget()'s) of
        that selection only."""
        n, keys, counts, grp, hrs = self.export_device(users, groups, hours)
        g, h, z, r, c, cnt = self._host_cells(n, keys, counts, (grp, hrs))
        h = h.astype(np.int64)
        h[h == _lib.HM_STREAM_UNDATED] = UNDATED_HOUR
        x = self._side(self._selection(users, groups, hours))
        return self._with_side((g, h, z, r, c, cnt), x.T if len(x) else None)

    def _cells_u32(self, x, n, what, undated=False):
        """uint32 values per cell as an int32 device tensor (their bits).
        Signed 64-bit input is range-checked (UNDATED_HOUR -> HM_STREAM_UNDATED
        for hours); int32 / uint32 input is taken as bits."""
        torch = self._torch
        if x is None:
            return None
        if not isinstance(x, torch.Tensor):
            a = np.asarray(x)
            if a.dtype.kind not in "iu":
                raise TypeError("%s must be integers" % what)
            if a.dtype.itemsize == 4:
                x = torch.from_numpy(np.ascontiguousarray(a).view(np.int32))
            else:
                x = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
        elif getattr(torch, "uint32", None) is not None and x.dtype == torch.uint32:
            x = x.view(torch.int32)
        if x.numel() != n:
            raise ValueError("%s must have one entry per cell" % what)
        if x.dtype != torch.int32:
            x = device._dev(x, torch.int64, self.device_index)
            if undated:
                x = torch.where(x == UNDATED_HOUR, torch.full_like(x, _lib.HM_STREAM_UNDATED), x)
            bad = (x < 0) | (x > 0xFFFFFFFF)
            if bool(bad.any()):
                raise ValueError("cell %d: %s does not fit 32 bits" % (int(bad.nonzero()[0, 0]), what))
            # the low 32 bits, as int32
            x = torch.where(x >= (1 << 31), x - (1 << 32), x)
        return device._dev(x, torch.int32, self.device_index)

    def import_cells(self, keys, counts, groups=None, hours=None, labels=None, distinct=False):
        """Append pre-aggregated cells (hm_stream_import): keys in hm_count's
        layout and their counts, numpy arrays or CUDA tensors.  groups: uint32
        group ids (None: no cell has a group), hours: epoch hours, UNDATED_HOUR
        or HM_STREAM_UNDATED for an undated cell (None: all undated).  labels:
        the source stream's id -> label list; the ids are then remapped to this
        stream's (unknown labels are appended, NOGROUP passes through).
        Without labels the ids are explicit, as add(group=)'s.  distinct: no
        two cells share (group, hour, key), as an export's.  Equal cells add
        up, in the input and with the stream's.  An invalid cell raises
        ValueError naming the first one's index; nothing is appended then."""
        torch = self._torch
        self.ctx.bind_stream()

        def u64(x):
            if not isinstance(x, torch.Tensor):
                a = np.asarray(x)
                if a.dtype.kind not in "iu" or a.dtype.itemsize != 8:
                    a = a.astype(np.uint64)
                x = torch.from_numpy(np.ascontiguousarray(a).view(np.int64))
            elif getattr(torch, "uint64", None) is not None and x.dtype == torch.uint64:
                x = x.view(torch.int64)
            return device._dev(x, torch.int64, self.device_index)

        k, cn = u64(keys), u64(counts)
        n = k.numel()
        if cn.numel() != n:
            raise ValueError("keys and counts must have the same length")
        gr = self._cells_u32(groups, n, "group")
        hr = self._cells_u32(hours, n, "hour", undated=True)
        index, new_labels, explicit_max = self._index, self.labels, self._explicit_max
        if gr is not None:
            g64 = gr.to(torch.int64) & 0xFFFFFFFF
            if labels is not None:
                index, new_labels = dict(self._index), list(self.labels)    # committed when the import succeeds
                lut = torch.from_numpy(_group_lut(labels, index, new_labels)).to(g64.device)
                g64 = _remap_groups(g64, lut)
                gr = torch.where(g64 >= (1 << 31), g64 - (1 << 32), g64).to(torch.int32)
            else:
                explicit_max = max(explicit_max, _explicit_group_max(g64))
        rc = self.ctx.L.hm_stream_import(self.ptr, device._ptr(k), device._ptr(cn), device._ptr(gr), device._ptr(hr),
                                         n, _lib.HM_IMPORT_DISTINCT if distinct else 0)
        if rc == _lib.HM_E_ARG:
            idx, _ = self.ctx.last_error()
            raise ValueError("cell %d is not a valid cell of this stream (zooms %d..%d, row and col inside the "
                             "square, count >= 1, group <= 0x%X, hour undated or in [%d, %d))"
                             % (idx, self.zmin, self.zmax, NOGROUP, self.base_hour, self.base_hour + MAX_HOURS))
        _lib.raise_for(rc)
        self._index, self.labels, self._explicit_max = index, new_labels, explicit_max

    def snapshot(self, users=None, groups=None, hours=None) -> dict:
        """The stream's whole state as numpy arrays and plain numbers: format
        version, zmin, zmax, base_hour, the group labels, the largest explicit
        group id, the export (keys, counts, groups, hours as hm_stream_export
        writes them) and the out-of-square records.  With users, groups or
        hours (as forget()'s) the records of that selection only, under the
        full label list, so restore() and merge_from() map it as any other."""
        n, keys, counts, grp, hrs = self.export_device(users, groups, hours)
        return _pack_snapshot(self.zmin, self.zmax, self.base_hour, self.labels, self._explicit_max,
                              keys[:n].cpu().numpy().view(np.uint64), counts[:n].cpu().numpy().view(np.uint64),
                              grp[:n].cpu().numpy().view(np.uint32), hrs[:n].cpu().numpy().view(np.uint32),
                              self._side(self._selection(users, groups, hours)))

    def save(self, path):
        """Write snapshot() to `path` (numpy's .npz; no pickled objects)."""
        with open(path, "wb") as f:
            _save_snapshot(f, self.snapshot())

    def _take(self, labels, explicit_max, x, keys, counts, groups, hours, distinct):
        """Another stream's cells (device tensors or host arrays), labels and
        out-of-square records x joined into this one."""
        labels = [str(v) for v in labels]
        if int(explicit_max) >= len(labels):
            # ids passed as group= have no label to remap by: they keep their
            # values, which needs the labelled ids to mean the same here
            m = min(len(labels), len(self.labels))
            if labels[:m] != self.labels[:m]:
                raise ValueError("the source holds explicit group ids (up to %d) and its labels %r do not line up "
                                 "with this stream's %r" % (int(explicit_max), labels, self.labels))
            self.import_cells(keys, counts, groups, hours, None, distinct)
            lut = _group_lut(labels, self._index, self.labels)
            lut = np.concatenate([lut[:-1], np.arange(len(labels), int(explicit_max) + 1), lut[-1:]])
        else:
            self.import_cells(keys, counts, groups, hours, labels, distinct)
            lut = _group_lut(labels, self._index, self.labels)      # (all known by now)
        self._explicit_max = max(self._explicit_max, int(explicit_max))
        if len(x):
            self._x = _sum_records(np.concatenate([self._x, _remap_records(x, lut)]), 5)

    def _check_hours(self, lo, hi, what):
        """ValueError unless the dated hours lo..hi (None: none) fit this stream"""
        if lo is not None and (lo < self.base_hour or hi >= self.base_hour + MAX_HOURS):
            raise ValueError("%s holds hours %d..%d, outside this stream's [%d, %d)"
                             % (what, lo, hi, self.base_hour, self.base_hour + MAX_HOURS))

    def restore(self, snapshot):
        """Join a snapshot() (or an opened .npz of one) into this stream: its
        zooms must be this stream's and its hours must fit; into a fresh
        stream this restores the snapshot's state."""
        snap = _unpack_snapshot(snapshot)
        _check_zooms(snap, self.zmin, self.zmax)
        h = np.concatenate([snap["hours"][snap["hours"] != _lib.HM_STREAM_UNDATED].astype(np.int64),
                            snap["x"][snap["x"][:, 1] != UNDATED_HOUR, 1]])
        self._check_hours(int(h.min()) if len(h) else None, int(h.max()) if len(h) else None, "the snapshot")
        self._take(snap["labels"].tolist(), snap["explicit_max"], snap["x"], snap["keys"], snap["counts"],
                   snap["groups"], snap["hours"], True)
        return self

    @classmethod
    def from_snapshot(cls, snapshot, **create_kwargs):
        """A new stream holding the snapshot's state (zooms and base hour from
        the snapshot unless given; other create_kwargs as the constructor's)."""
        snap = _unpack_snapshot(snapshot)
        kw = dict(zmin=snap["zmin"], zmax=snap["zmax"], base_hour=snap["base_hour"],
                  initial_cells=max(1 << 20, len(snap["keys"]) + len(snap["keys"]) // 4))
        kw.update(create_kwargs)
        _check_zooms(snap, int(kw["zmin"]), int(kw["zmax"]))
        s = cls(**kw)
        try:
            return s.restore(snap)
        except Exception:
            s.close()
            raise

    @classmethod
    def load(cls, path, **create_kwargs):
        """A new stream from a file written by save()."""
        return cls.from_snapshot(_load_snapshot(path), **create_kwargs)

    def merge_from(self, other: "StreamingHeatmap", users=None, groups=None, hours=None):
        """Add every cell of `other` (same zooms; its base hour may differ, its
        hours must fit this stream's) to this stream: shards of one feed, or a
        backfill.  Groups are matched by label.  `other` is left unchanged;
        nothing changes here when its hours do not fit.  With users, groups or
        hours (as forget()'s, in `other`'s ids) only that part of `other`:
        moving users U here is merge_from(other, users=U), then
        other.forget(users=U)."""
        torch = self._torch
        if (other.zmin, other.zmax) != (self.zmin, self.zmax):
            raise ValueError("merge_from needs equal zooms: %d..%d against %d..%d"
                             % (other.zmin, other.zmax, self.zmin, self.zmax))
        n, keys, counts, grp, hrs = other.export_device(users, groups, hours)
        ox = other._side(other._selection(users, groups, hours))
        h = hrs[:n].to(torch.int64) & 0xFFFFFFFF
        h = h[h != _lib.HM_STREAM_UNDATED]
        xh = ox[ox[:, 1] != UNDATED_HOUR, 1]
        ends = ([int(h.min()), int(h.max())] if h.numel() else []) + ([int(xh.min()), int(xh.max())] if len(xh) else [])
        self._check_hours(min(ends, default=None), max(ends, default=None), "the other stream")
        dev = "cuda:%d" % self.device_index
        self.ctx.bind_stream()
        self._take(list(other.labels), other._explicit_max, ox, keys[:n].to(dev), counts[:n].to(dev),
                   grp[:n].to(dev), hrs[:n].to(dev), True)

    def hourly(self):
        """{epoch hour: Counts} for every non-empty hour."""
        _, hr, z, r, c, cnt = self.rollup("hour")
        out = {}
        for h in np.unique(hr).tolist():
            m = hr == h
            out[int(h)] = device.Counts(z[m], r[m], c[m], cnt[m], 0, [])
        return out

    def heatmap_cells(self, timespan: str = "alltime", max_zoom_level=None, delta=None) -> "_hm.Cells":
        """The bins of build_heatmaps' rows for `timespan` ('alltime', 'year',
        'month', 'day'): every period of the span, each with its label."""
        d = _hm.DETAIL_ZOOM_DELTA if delta is None else int(delta)
        mz = self.zmax - d if max_zoom_level is None else int(max_zoom_level)
        if mz + d != self.zmax or self.zmin > d + 1:
            raise ValueError("rows need zooms %d..%d; the stream holds %d..%d" % (d + 1, mz + d, self.zmin, self.zmax))
        if timespan not in ("alltime", "year", "month", "day"):
            raise ValueError("timespan must be 'alltime', 'year', 'month' or 'day'")
        if self._explicit_max >= len(self.labels):
            raise ValueError("rows need a label per group: group id %d was passed as group= and has none "
                             "(feed the stream with user_id= to build rows)" % self._explicit_max)
        _, ap, az, ar, ac, an = self.rollup(timespan, merge_groups=True)
        gg, gp, gz, gr, gc, gn = self.rollup(timespan, merge_groups=False)
        grouped = gg != NOGROUP
        gg, gp, gz, gr, gc, gn = gg[grouped], gp[grouped], gz[grouped], gr[grouped], gc[grouped], gn[grouped]
        parts = []
        for p in np.unique(ap).tolist():
            m, q = ap == p, gp == p
            parts.append(_hm.combine_cells(self.labels, (az[m], ar[m], ac[m], an[m]),
                                           (gg[q].astype(np.int64), gz[q], gr[q], gc[q], gn[q]), mz + d, d,
                                           span_label(timespan, p)))
        return _hm.concat_cells(parts, self.labels, d)

    def window_cells(self, hour_lo: int, hour_hi: int, label: str, max_zoom_level=None, delta=None) -> "_hm.Cells":
        """The bins of build_heatmaps' rows over the window's points, under
        the caller's timespan label (e.g. 'last24h': the reference has none
        for a window)."""
        d = _hm.DETAIL_ZOOM_DELTA if delta is None else int(delta)
        mz = self.zmax - d if max_zoom_level is None else int(max_zoom_level)
        if mz + d != self.zmax or self.zmin > d + 1:
            raise ValueError("rows need zooms %d..%d; the stream holds %d..%d" % (d + 1, mz + d, self.zmin, self.zmax))
        if not isinstance(label, str) or _hm.KEY_SEPERATOR in label:
            raise ValueError("window label %r must be a string without the key separator %r"
                             % (label, _hm.KEY_SEPERATOR))
        if self._explicit_max >= len(self.labels):
            raise ValueError("rows need a label per group: group id %d was passed as group= and has none "
                             "(feed the stream with user_id= to build rows)" % self._explicit_max)
        _, az, ar, ac, an = self.window(hour_lo, hour_hi, merge_groups=True)
        gg, gz, gr, gc, gn = self.window(hour_lo, hour_hi, merge_groups=False)
        q = gg != NOGROUP
        return _hm.combine_cells(self.labels, (az, ar, ac, an), (gg[q].astype(np.int64), gz[q], gr[q], gc[q], gn[q]),
                                 mz + d, d, label)

    def window_rows(self, hour_lo: int, hour_hi: int, label: str, max_zoom_level=None, delta=None) -> dict:
        """{row_id: {bin_id: float}} as build_heatmaps would give over the
        points of the hours hour_lo <= hour < hour_hi, row ids
        '<group>|<label>|<tile>'."""
        return _hm.cells_to_rows(self.window_cells(hour_lo, hour_hi, label, max_zoom_level, delta))

    def window_table(self, hour_lo: int, hour_hi: int, label: str, max_zoom_level=None, delta=None):
        """The same rows as a pyarrow Table(id, heatmap JSON)."""
        return _hm.cells_to_table(self.window_cells(hour_lo, hour_hi, label, max_zoom_level, delta))

    def rows(self, timespan: str = "alltime", max_zoom_level=None, delta=None) -> dict:
        """{row_id: {bin_id: float}} as build_heatmaps would give over every
        point so far, row ids '<group>|<timespan label>|<tile>'."""
        return _hm.cells_to_rows(self.heatmap_cells(timespan, max_zoom_level, delta))

    def table(self, timespan: str = "alltime", max_zoom_level=None, delta=None):
        """The same rows as a pyarrow Table(id, heatmap JSON)."""
        return _hm.cells_to_table(self.heatmap_cells(timespan, max_zoom_level, delta))

    def close(self):
        if getattr(self, "ptr", None):
            self.ctx.L.hm_stream_destroy(self.ptr)
            self.ptr = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
