"""A plain CPU model of the streaming heatmap's state, for the ingest tests.

Test infrastructure only: no GPU code, nothing of heatmap_amd.stream.

Points are integer (row, col) tiles at the stream's zmax.  Fed to the stream
as the lat/lon of their CENTRES (centre(), the construction of
tests/test_gpu_l1_whole_tiles.py: far from every guard band of the
projection), a point's cell at zoom z is exactly

    (z, row >> (zmax - z), col >> (zmax - z))

so the model is integer arithmetic and independent of the projection code
(tests/test_stream_model_host.py checks that against the C oracle).

The state is one record per distinct (group, hour, zoom, row, col) with a
64-bit count, kept as an int64 array of those six columns in lexicographic
order -- the columns and the order of a sorted StreamingHeatmap.export().
NOGROUP stands for "no group", UNDATED_HOUR for an undated cell.
"""
import numpy as np

NOGROUP = 0xFFFFFFFE      # heatmap_amd.stream.NOGROUP
UNDATED_HOUR = -1         # heatmap_amd.stream.UNDATED_HOUR
ALLTIME = -1              # heatmap_amd.stream.ALLTIME


def centre(rows, cols, zoom):
    """lat/lon of the centres of zoom-`zoom` tiles"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    y = np.pi - 2.0 * np.pi * (rows + 0.5) / float(1 << zoom)
    return np.degrees(np.arctan(np.sinh(y))), (cols + 0.5) / float(1 << zoom) * 360.0 - 180.0


def count_keys(zoom, row, col):
    """hm_count's key layout (zoom << 58 | row << 29 | col), what import_cells takes"""
    return ((np.asarray(zoom).astype(np.uint64) << np.uint64(58)) | (np.asarray(row).astype(np.uint64) << np.uint64(29))
            | np.asarray(col).astype(np.uint64))


def sort_records(rec):
    """int64 records [n, w] in lexicographic order of their columns"""
    rec = np.asarray(rec, dtype=np.int64)
    return rec[np.lexsort(rec.T[::-1])] if len(rec) else rec


def sum_records(rec):
    """Sorted records with the last column summed over equal leading columns."""
    rec = sort_records(rec)
    if len(rec) < 2:
        return rec
    first = np.ones(len(rec), dtype=bool)
    first[1:] = (rec[1:, :-1] != rec[:-1, :-1]).any(axis=1)
    start = np.flatnonzero(first)
    out = rec[start].copy()
    out[:, -1] = np.add.reduceat(rec[:, -1], start)
    return out


def batch_keys(n, keep=None, hour=None, group=None):
    """The distinct (group, hour) pairs of a batch's KEPT points, sorted: the
    buckets hm_stream_add sees in it (NOGROUP / UNDATED_HOUR where the batch has
    no group / hour)."""
    g = np.full(n, NOGROUP, np.int64) if group is None else np.asarray(group).astype(np.int64)
    h = np.full(n, UNDATED_HOUR, np.int64) if hour is None else np.asarray(hour).astype(np.int64)
    kb = np.ones(n, dtype=bool) if keep is None else np.asarray(keep).astype(bool)
    pairs = np.stack([g[kb], h[kb]], axis=1)
    return np.unique(pairs, axis=0) if len(pairs) else pairs


class StreamModel:
    def __init__(self, zmin, zmax):
        self.zmin, self.zmax = int(zmin), int(zmax)
        self.rec = np.zeros((0, 6), dtype=np.int64)   # group, hour, zoom, row, col, count

    def copy(self):
        m = StreamModel(self.zmin, self.zmax)
        m.rec = self.rec.copy()
        return m

    # ------------------------------------------------------------ operations

    def add(self, rows, cols, keep=None, hour=None, group=None):
        """One batch of zoom-zmax tiles; keep: per-point mask, hour: per-point
        epoch hours (None: undated), group: per-point ids (None: no group)."""
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        n = len(rows)
        kb = np.ones(n, dtype=bool) if keep is None else np.asarray(keep).astype(bool)
        g = (np.full(n, NOGROUP, np.int64) if group is None else np.asarray(group).astype(np.int64))[kb]
        h = (np.full(n, UNDATED_HOUR, np.int64) if hour is None else np.asarray(hour).astype(np.int64))[kb]
        r, c = rows[kb], cols[kb]
        one = np.ones(len(r), dtype=np.int64)
        parts = [self.rec]
        for z in range(self.zmin, self.zmax + 1):
            sh = self.zmax - z
            parts.append(np.stack([g, h, np.full(len(r), z, np.int64), r >> sh, c >> sh, one], axis=1))
        self.rec = sum_records(np.concatenate(parts))

    def expire(self, before_hour):
        """Dated records of hours < before_hour leave; returns how many."""
        h = self.rec[:, 1]
        gone = (h != UNDATED_HOUR) & (h < int(before_hour))
        self.rec = self.rec[~gone]
        return int(gone.sum())

    def selected(self, groups=None, hours=None):
        """Mask of the records of a forget() / export() selection: group among
        `groups` (None: any), hour in hours = (lo, hi) (None: any hour and the
        undated records; those are in no range)."""
        m = np.ones(len(self.rec), dtype=bool)
        if groups is not None:
            m &= np.isin(self.rec[:, 0], np.asarray(list(groups), dtype=np.int64))
        if hours is not None:
            h = self.rec[:, 1]
            m &= (h != UNDATED_HOUR) & (h >= int(hours[0])) & (h < int(hours[1]))
        return m

    def forget(self, groups=None, hours=None):
        gone = self.selected(groups, hours)
        self.rec = self.rec[~gone]
        return int(gone.sum())

    def import_records(self, rec):
        """Records (group, hour, zoom, row, col, count) added to the state;
        equal ones add up, in the input and with the state's."""
        rec = np.asarray(rec, dtype=np.int64).reshape(-1, 6)
        self.rec = sum_records(np.concatenate([self.rec, rec]))

    # --------------------------------------------------------------- queries

    def records(self):
        """Every record, sorted: what a sorted export() must equal."""
        return self.rec

    def buckets(self):
        """distinct (group, hour) pairs with a record"""
        return len(np.unique(self.rec[:, :2], axis=0)) if len(self.rec) else 0

    def has_undated(self):
        return bool((self.rec[:, 1] == UNDATED_HOUR).any())

    def dated(self):
        """The dated records, sorted: the per-group hour rollup."""
        return self.rec[self.rec[:, 1] != UNDATED_HOUR]

    def group_alltime(self):
        """(group, zoom, row, col, count) summed over hours and the undated
        records: the per-group alltime rollup."""
        return sum_records(self.rec[:, [0, 2, 3, 4, 5]])

    def counts(self, hour=ALLTIME):
        """(zoom, row, col, count) merged over groups, of one epoch hour or of
        everything (ALLTIME), in the order of device.Counts.sorted()."""
        rec = self.rec if hour == ALLTIME else self.rec[self.rec[:, 1] == int(hour)]
        out = sum_records(rec[:, 2:])
        return out[:, 0], out[:, 1], out[:, 2], out[:, 3]
