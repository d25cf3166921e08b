"""hm_stream_add as a state machine: scripted sequences of batches, expiry,
forgetting, imports and compactions, each step mirrored in a plain CPU model
(tests/stream_model.py, checked against the oracle by
tests/test_stream_model_host.py) and compared with it exactly.

Which code a batch runs is decided in hm_stream_add (hm_stream_api.cpp) by

  nparts       the batch's distinct (group, hour) buckets among its KEPT points:
               0       nothing kept, nothing appended
               1       hm_count straight into the log's tail
               2, 3    gathered runs counted at once on helper contexts
                       (stream_fold_parts_par: nparts + 1 <= HMS_PAR = 4),
                       one after the other with HM_STREAM_PAR=0
               4..64   gathered runs counted one after the other
                       (nparts <= HMS_MAX_PARTS = 64)
               65...   one grouped pass (stream_fold_grouped)
  last_nparts  the previous batch's nparts; spec = last_nparts <= 1: the batch
               is first counted as if it were one bucket, and when it is not,
               that tail is dropped and k_stream_buckets runs again to write
               the per-point ids.  A fresh stream, an import and an expire or
               forget that dropped cells set last_nparts = 1.

and whether cells() / export() may trust the log as it is (the host-side
`compact` flag: stream_appended, log_buckets, HMS_ANY_BUCKET, stream_compact,
stream_refile_end, the tail of hm_stream_import) depends on the stream's whole
history.  A wrongly true flag changes no rollup -- rollups merge anyway -- so
every script is checked in two ways:

  after every step, without compacting: the per-group hour rollup equals the
    model's dated records, counts(ALLTIME) equals the model's (and the
    per-group alltime rollup where the script holds undated cells);
  where the script says so and at the end, compacting: cells()[0] is the
    model's record count and the sorted export() IS the model's records, which
    fails on any duplicate (group, hour, cell).

Compacting changes the state the next step starts from, so every script runs
twice: with the compacting checks after every step ("every") and only at the
end ("end").  Bucket counts are asserted from the model before each GPU call,
so an edit of a generator cannot move a case off its boundary unnoticed.

Zooms 0-12 (one script at zmin 3), at most 10 000 points a batch.  The
grid-stride loops of k_stream_buckets, k_stream_part_count and
k_stream_scatter start beyond 8M points a batch and are out of scope here.
"""
import numpy as np
import pytest

import stream_model as sm
from heatmap_amd import _lib
from heatmap_amd.stream import ALLTIME, NOGROUP, UNDATED_HOUR, StreamingHeatmap

pytestmark = pytest.mark.gpu
BASE = 480000   # epoch hour (2024-10-04), the streams' base hour
ZMIN, ZMAX = 0, 12
N = 3000
MODES = ["every", "end"]

assert (sm.NOGROUP, sm.UNDATED_HOUR, sm.ALLTIME) == (NOGROUP, UNDATED_HOUR, ALLTIME)


# ------------------------------------------------------------------ batches

class Batch:
    """n zoom-ZMAX tiles, half of them uniform over the square and half in a
    24 x 24 block that every batch shares (so batches repeat each other's
    cells at every zoom), and per point the index of its key."""

    def __init__(self, n, keys, seed, keep="mask", order="cycle"):
        rng = np.random.default_rng(seed)
        self.n = n
        self.rows = rng.integers(0, 1 << ZMAX, n)
        self.cols = rng.integers(0, 1 << ZMAX, n)
        self.rows[n // 2:] = 1500 + rng.integers(0, 24, n - n // 2)
        self.cols[n // 2:] = 2600 + rng.integers(0, 24, n - n // 2)
        self.lat, self.lon = sm.centre(self.rows, self.cols, ZMAX)
        k = len(keys)
        i = np.arange(n)
        if order == "cycle":          # interleaved point by point
            idx = i % k
        elif order == "sorted":       # one contiguous run per key
            idx = i * k // n
        elif order == "block64":      # a key per 64-lane step
            idx = (i // 64) % k
        elif order == "lonely":       # key 0: one point, keys 2..: two points each, key 1: all the rest
            idx = np.ones(n, dtype=np.int64)
            idx[n // 2] = 0
            for j in range(2, k):
                idx[[3 * j, n - 3 * j]] = j
        else:
            raise ValueError(order)
        self.idx = idx
        if keep == "all":
            self.keep = None
        elif keep == "mask":          # about one point in seven dropped, no period that a cycle of keys could meet
            self.keep = (rng.random(n) > 0.15).astype(np.uint8)
            self.keep[-1] = 1         # (the last point may be the only one of its key)
        elif keep == "none":
            self.keep = np.zeros(n, np.uint8)
        elif keep == "not0":          # every point of key 0 is dropped
            self.keep = (idx != 0).astype(np.uint8)
        else:
            raise ValueError(keep)
        groups, hours = [g for g, _ in keys], [h for _, h in keys]
        assert all(g is None for g in groups) or all(g is not None for g in groups)
        assert all(h is None for h in hours) or all(h is not None for h in hours)
        self.group = None if groups[0] is None else np.array(groups, dtype=np.uint32)[idx]
        self.hour = None if hours[0] is None else np.array(hours, dtype=np.uint32)[idx]

    def keys(self):
        """the batch's buckets: distinct (group, hour) of its kept points"""
        return sm.batch_keys(self.n, self.keep, self.hour, self.group)


def gh_keys(k, first=0):
    """k distinct (group, hour) keys: groups 0..2, hours from BASE"""
    return [(j % 3, BASE + j // 2) for j in range(first, first + k)]


def records(b, zmin=ZMIN):
    """a batch's records as a stream that held only it would export them"""
    m = sm.StreamModel(zmin, ZMAX)
    m.add(b.rows, b.cols, b.keep, b.hour, b.group)
    return m.records()


# ---------------------------------------------------- a stream and its model

def _rec(*cols):
    return sm.sort_records(np.stack([np.asarray(c).astype(np.int64) for c in cols], axis=1))


def _same_records(got, want, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    dup = len(got) - len(np.unique(got[:, :-1], axis=0)) if len(got) else 0
    raise AssertionError("%s: %d records (%d of them repeat an earlier key) against the model's %d"
                         % (what, len(got), dup, len(want)))


class Pair:
    """A StreamingHeatmap and its model, stepped together; every step ends
    with the checks of the module docstring."""

    def __init__(self, mode, zmin=ZMIN, zmax=ZMAX, **kw):
        kw.setdefault("max_buckets", 4096)
        self.every = mode == "every"
        self.s = StreamingHeatmap(zmin, zmax, base_hour=BASE, **kw)
        self.m = sm.StreamModel(zmin, zmax)
        self.buckets_after_add = []

    def have(self):
        return set(map(tuple, self.m.records()[:, :2].tolist()))

    def light(self):
        """the checks that leave the log as it is"""
        g, p, z, r, c, n = self.s.rollup("hour", merge_groups=False)
        _same_records(_rec(g, p, z, r, c, n), self.m.dated(), "per-group hour rollup")
        got = self.s.counts(ALLTIME).sorted()
        for a, b in zip((got.zoom, got.row, got.col, got.count), self.m.counts(ALLTIME)):
            assert np.array_equal(a, b), "counts(ALLTIME)"
        if self.m.has_undated():
            g, _, z, r, c, n = self.s.rollup("alltime", merge_groups=False)
            _same_records(_rec(g, z, r, c, n), self.m.group_alltime(), "per-group alltime rollup")

    def heavy(self):
        """the checks that compact the log"""
        _same_records(_rec(*self.s.export()), self.m.records(), "export()")
        assert self.s.cells()[0] == len(self.m.records()), "cells()"

    def after(self):
        self.light()
        if self.every:
            self.heavy()

    def add(self, b, buckets, new):
        """One batch.  buckets: its bucket count, new: how many of them have
        no cell in the stream yet -- both asserted from the model first."""
        keys = set(map(tuple, b.keys().tolist()))
        assert len(keys) == buckets
        assert len(keys - self.have()) == new
        self.s.add(b.lat, b.lon, b.keep, b.hour, group=b.group)
        self.m.add(b.rows, b.cols, b.keep, b.hour, b.group)
        self.buckets_after_add.append(self.s.buckets())   # before this step's rollups intern their labels
        self.after()

    def expire(self, before, drops):
        gone = self.m.expire(before)
        assert (gone > 0) == drops
        dropped, _ = self.s.expire(before)
        assert dropped >= gone and (dropped > 0) == drops   # (a log that is not compact holds a cell several times)
        self.after()

    def forget(self, groups=None, hours=None, empties=False):
        gone = self.m.forget(groups, hours)
        assert gone > 0 and (len(self.m.records()) == 0) == empties
        dropped, _ = self.s.forget(groups=groups, hours=hours)
        assert dropped >= gone
        self.after()

    def imp(self, rec, distinct, new, dup=False):
        """import_cells of the records rec (a model's export); dup: every third
        record once more, which distinct=False must sum"""
        keys = set(map(tuple, rec[:, :2].tolist()))
        assert len(keys - self.have()) == new
        if dup:
            assert not distinct
            rec = np.concatenate([rec, rec[::3]])
        self.s.import_cells(sm.count_keys(rec[:, 2], rec[:, 3], rec[:, 4]), rec[:, 5].astype(np.uint64), rec[:, 0],
                            rec[:, 1], distinct=distinct)
        self.m.import_records(rec)
        self.after()

    def cells(self):
        """the script's own compaction"""
        self.heavy()
        self.light()

    def end(self):
        self.heavy()
        self.light()
        self.s.close()


def _par(monkeypatch, par):
    if par is None:
        monkeypatch.delenv("HM_STREAM_PAR", raising=False)
    else:
        monkeypatch.setenv("HM_STREAM_PAR", par)


# --------------------------------------------- 1. bucket-count boundaries

# (buckets, keep pattern, HM_STREAM_PAR)
BOUNDARIES = [(0, "none", None), (1, "mask", None), (2, "mask", None), (2, "mask", "0"), (3, "mask", None),
              (3, "mask", "0"), (4, "mask", None), (5, "mask", None), (63, "mask", None), (64, "all", None),
              (64, "mask", None), (65, "mask", None), (66, "mask", None)]


@pytest.mark.parametrize("start", ["empty", "holding-every", "holding-end"])
@pytest.mark.parametrize("k,keep,par", BOUNDARIES, ids=["%d-%s-par%s" % (k, kp, p) for k, kp, p in BOUNDARIES])
def test_bucket_count_boundaries(gpu, monkeypatch, k, keep, par, start):
    """One batch of k buckets on each side of every rule of hm_stream_add:
    k = 0 nothing kept; 1 the tail count; 2, 3 stream_fold_parts_par (with
    HM_STREAM_PAR=0 the sequential loop of stream_fold_parts); 4, 5, 63, 64 the
    sequential loop (4: nparts + 1 > HMS_PAR; 64 = HMS_MAX_PARTS, every one of
    the HMS_MAX_PARTS + 1 LDS counters of k_stream_part_count and
    k_stream_scatter in use -- with every point kept the last of them, the
    run of the points not kept, stays empty, with a mask it does not); 65, 66
    stream_fold_grouped.
    empty: the stream is fresh, so last_nparts = 1 and the batch is counted
    speculatively as one bucket first (for k >= 2 that tail is dropped and
    k_stream_buckets runs again); all its buckets are new.
    holding: a batch of max(2, k / 2) buckets came before (last_nparts >= 2:
    no speculation, ids written by the first pass), half of this batch's
    buckets have cells in the log already; the modes differ in whether that
    log was compacted in between."""
    _par(monkeypatch, par)
    keys = gh_keys(max(k, 1))
    p = Pair("every" if start != "holding-end" else "end")
    old = 0
    if start != "empty":
        pre = (keys + [(9, BASE + 500)])[:max(2, k // 2)] if k < 4 else keys[:k // 2]
        p.add(Batch(N, pre, seed=50 + k), len(pre), len(pre))
        old = 0 if k == 0 else len(set(pre) & set(keys))
        assert old == (min(k, 2) if k < 4 else k // 2)
    p.add(Batch(N, keys, seed=k, keep=keep), k, k - old)
    assert p.m.buckets() == (k if start == "empty" else k + len(pre) - old)
    p.end()


def test_boundary_batches_at_zmin_3(gpu, monkeypatch):
    """The boundaries' paths once more on a stream of zooms 3-12, in one
    script: 1 bucket (tail, speculative), 3 (parallel runs; speculated first,
    since the batch before was one bucket), 64 (sequential runs, not
    speculated), 65 (grouped, not speculated), 1 again (tail, not
    speculated), then a compaction."""
    _par(monkeypatch, None)
    for mode in MODES:
        p = Pair(mode, zmin=3)
        p.add(Batch(N, gh_keys(1), seed=1), 1, 1)
        p.add(Batch(N, gh_keys(3), seed=2), 3, 2)
        p.add(Batch(N, gh_keys(64), seed=3), 64, 61)
        p.add(Batch(N, gh_keys(65, first=10), seed=4), 65, 11)
        p.add(Batch(N, gh_keys(1, first=70), seed=5), 1, 0)
        p.end()


# --------------------------------------------- 2. speculation transitions

CLASSES = {"one": 1, "few": 3, "many": 70}
H0 = BASE + 10


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("prev", ["one", "several", "expire_drop", "forget", "import", "expire_none"])
def test_speculation_transitions(gpu, monkeypatch, prev, cls, mode):
    """spec = last_nparts <= 1 crossed with this batch's class.  Every script
    starts with a three-bucket batch (group 1, hours H0..H0+2; last_nparts =
    3), then `prev`, then the batch under test: one bucket (the tail count),
    three (parallel runs) or 70 (grouped pass), its first bucket (1, H0+2)
    already in the log, the others new.
      several      nothing in between: not speculated, one k_stream_buckets pass
      one          a one-bucket batch (not speculated itself) sets last_nparts = 1:
                   speculated; the few and many batches drop the tail and run
                   k_stream_buckets a second time
      expire_drop  expire(H0+1) drops hour H0 and sets last_nparts = 1: speculated
      forget       forget(group 1, hour H0) likewise: speculated
      import       import_cells sets last_nparts = 1: speculated
      expire_none  expire(BASE+5) runs its pass, drops nothing and leaves the
                   stream as it is, last_nparts = 3 included: not speculated"""
    _par(monkeypatch, None)
    p = Pair(mode)
    p.add(Batch(N, [(1, H0), (1, H0 + 1), (1, H0 + 2)], seed=1), 3, 3)
    if prev == "one":
        p.add(Batch(N, [(1, H0 + 1)], seed=2), 1, 0)
    elif prev == "expire_drop":
        p.expire(H0 + 1, drops=True)
    elif prev == "forget":
        p.forget(groups=[1], hours=(H0, H0 + 1))
    elif prev == "import":
        p.imp(records(Batch(500, [(2, H0 + 5)], seed=3)), True, new=1)
    elif prev == "expire_none":
        p.expire(BASE + 5, drops=False)
    k = CLASSES[cls]
    keys = [(1, H0 + 2)] + [(1, H0 + 20 + j) for j in range(k - 1)]
    p.add(Batch(N, keys, seed=4), k, k - 1)
    # and the state that batch left: a one-bucket batch of an old hour
    p.add(Batch(N, [(1, H0 + 2)], seed=5), 1, 0)
    p.end()


# ------------------------------------------------- 3. compactness history

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("vmm", ["1", "0"])
def test_compactness_history(gpu, monkeypatch, vmm, mode):
    """The `compact` flag through one long history, on a log that starts at
    1024 cells, so that stream_room compacts and grows it inside the batches
    (HM_STREAM_VMM=1: pages mapped behind the cells; 0: copied).  No group;
    h(j) = BASE + j.  Step, path (rule), and what the flag must do:
      1  h0, new                  tail, speculated (fresh stream)       empty log: stays compact
      2  h0 again                 tail, speculated (last_nparts 1)      bucket in log_buckets: NOT compact
      3  cells()                  stream_compact
      4  h1 h2 h3, new            parallel runs, speculated first       three fresh buckets: stays compact
      5  h3 h4 h5                 parallel runs (last_nparts 3)         h3 is in the log: NOT compact
      6  65 hours h10..h74        grouped (65 > HMS_MAX_PARTS)          HMS_ANY_BUCKET joins log_buckets
      7  h80, new                 tail (last_nparts 65: not speculated) ANY_BUCKET: NOT compact, new or not
      8  expire(h3)               drops h0..h2, last_nparts = 1         log_buckets rebuilt from new slot ids
      9  h81 new, then h4         tail, speculated, twice               fresh: as before; h4 survives: NOT compact
      10 import distinct, h90 h91 new, then of h4 h5                    fresh keeps the flag, old clears it
      11 import not distinct, h92, with repeated cells                  NOT compact, whatever the buckets
      12 forget(every hour)       the log is empty                      compact again
      13 h0                       tail, speculated (a forget resets last_nparts)"""
    monkeypatch.setenv("HM_STREAM_VMM", vmm)
    _par(monkeypatch, None)

    def h(*js):
        return [(None, BASE + j) for j in js]

    p = Pair(mode, initial_cells=1024)
    p.add(Batch(N, h(0), seed=1), 1, 1)
    p.add(Batch(N, h(0), seed=2), 1, 0)
    p.cells()
    p.add(Batch(N, h(1, 2, 3), seed=3), 3, 3)
    p.add(Batch(N, h(3, 4, 5), seed=4), 3, 2)
    p.add(Batch(N, h(*range(10, 75)), seed=5), 65, 65)
    p.add(Batch(N, h(80), seed=6), 1, 1)
    p.expire(BASE + 3, drops=True)
    p.add(Batch(N, h(81), seed=7), 1, 1)
    p.add(Batch(N, h(4), seed=8), 1, 0)
    p.imp(records(Batch(N, h(90, 91), seed=9)), True, new=2)
    p.imp(records(Batch(N, h(4, 5), seed=10)), True, new=0)
    p.imp(records(Batch(N, h(92), seed=11)), False, new=1, dup=True)
    p.forget(hours=(BASE, BASE + 1000), empties=True)
    p.add(Batch(N, h(0), seed=12), 1, 1)
    p.end()


def test_compactness_history_undated_and_groups(gpu, monkeypatch):
    """The same bookkeeping where the buckets differ by group and some cells
    are undated (the per-group alltime rollup joins the checks): an undated
    batch without a group (one bucket, the tail, speculated), the same again
    (NOT compact), undated with three groups (parallel runs, fresh buckets),
    a dated 70-bucket batch (grouped: HMS_ANY_BUCKET), an expire that drops
    all of those (the undated cells stay), undated group 1 again (tail,
    speculated: its bucket survived, NOT compact), a forget of group 1."""
    _par(monkeypatch, None)
    for mode in MODES:
        p = Pair(mode, initial_cells=1024)
        p.add(Batch(N, [(None, None)], seed=1), 1, 1)
        p.add(Batch(N, [(None, None)], seed=2), 1, 0)
        p.add(Batch(N, [(0, None), (1, None), (2, None)], seed=3), 3, 3)
        p.add(Batch(N, [(j % 2, BASE + j // 2) for j in range(70)], seed=4), 70, 70)
        p.expire(BASE + 100, drops=True)
        p.add(Batch(N, [(1, None)], seed=5), 1, 0)
        p.forget(groups=[1])
        p.end()


# ---------------------------------------------------------- 4. uneven runs

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4095, 4096, 4097])
@pytest.mark.parametrize("shape", ["lonely", "unkept", "sorted", "interleaved"])
@pytest.mark.parametrize("k", [3, 20])
def test_uneven_runs(gpu, monkeypatch, k, shape, n, mode):
    """The gather of a few-bucket batch (k_stream_part_count, k_stream_scatter:
    blocks of 4096 points, so n = 4095, 4096, 4097 end a block one short, full
    and one over) with k = 3 (parallel runs) and k = 20 (sequential runs):
      lonely       one bucket holds a single point, another nearly all, the
                   others two points each
      unkept       every point of the first key is dropped by keep: the batch
                   has k - 1 buckets and that key is interned nowhere
      sorted       the buckets come as contiguous runs of the input
      interleaved  they alternate point by point
    The batch comes twice: on a fresh stream (speculated first, then
    k_stream_buckets again) and once more with other tiles (last_nparts > 1:
    not speculated; every bucket is in the log)."""
    _par(monkeypatch, None)
    keys = gh_keys(k)
    kw = {"lonely": dict(order="lonely", keep="all"), "unkept": dict(order="cycle", keep="not0"),
          "sorted": dict(order="sorted"), "interleaved": dict(order="cycle")}[shape]
    kb = k - 1 if shape == "unkept" else k
    p = Pair(mode)
    b = Batch(n, keys, seed=n, **kw)
    if shape == "lonely":
        assert np.bincount(b.idx).tolist() == [1, n - 1 - 2 * (k - 2)] + [2] * (k - 2)
    p.add(b, kb, kb)
    assert p.buckets_after_add[0] == kb == p.m.buckets()   # no label interned yet: the dropped key has no bucket
    p.add(Batch(n, keys, seed=n + 10, **kw), kb, 0)
    p.end()


# ------------------- 5. k_stream_buckets and the bucket table at their edges

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193]
PATTERNS = ["one", "block64", "cycle5", "cycle9", "own"]
GROUPS = [0, 0xFFFFFFFD, 7, 123456]      # 0xFFFFFFFD: the largest id add(group=) accepts
LAST_HOUR = BASE + (1 << 28) - 1         # the last hour of a stream whose base is BASE


def _hour(q):
    """distinct hours from both ends of the stream's range: BASE, LAST_HOUR, BASE + 2, LAST_HOUR - 2, ..."""
    return BASE + q if q % 2 == 0 else LAST_HOUR + 1 - q


def edge_keys(flavour, k, first=0):
    """k distinct keys: 'both' explicit groups and hours, 'group' undated,
    'hour' without a group, 'plain' the one key of neither"""
    js = range(first, first + k)
    if flavour == "both":
        return [(GROUPS[j % 4], _hour(j // 4)) for j in js]
    if flavour == "group":
        return [(GROUPS[j] if j < 2 else j, None) for j in js]
    if flavour == "hour":
        return [(None, _hour(j)) for j in js]
    assert flavour == "plain" and k == 1
    return [(None, None)]


def edge_batch(n, pattern, flavour, seed):
    if pattern == "one":
        # the largest group id and the last hour where the flavour has them
        return Batch(n, edge_keys(flavour, 1, first={"both": 5, "group": 1, "hour": 1, "plain": 0}[flavour]), seed)
    if pattern == "block64":
        return Batch(n, edge_keys(flavour, (n + 63) // 64), seed, order="sorted" if n < 64 else "block64")
    if pattern == "own":
        return Batch(n, edge_keys(flavour, n), seed)
    return Batch(n, edge_keys(flavour, min(int(pattern[5:]), n)), seed)


def _edge_case(n, pattern, flavour, spec):
    p = Pair("end", max_buckets=16384)
    pre = 0
    if not spec:
        # two points of two buckets first: last_nparts = 2, so the batch is not
        # speculated on and k_stream_buckets writes the ids in its first pass
        p.add(Batch(2, [(99, BASE + 300), (99, BASE + 301)], seed=1, keep="all"), 2, 2)
        pre = 2
    b = edge_batch(n, pattern, flavour, seed=n)
    k = len(b.keys())
    p.add(b, k, k)
    # the checks of the first batch interned one label (the merged alltime rollup's)
    assert p.buckets_after_add[-1] == k + (3 if pre else 0) and p.m.buckets() == k + pre
    p.end()
    return k


@pytest.mark.parametrize("spec", [True, False], ids=["spec", "nospec"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_bucket_kernel_sizes_and_patterns(gpu, monkeypatch, n, pattern, spec):
    """One add() of n points under each key pattern; export() must equal the
    model and buckets() the model's distinct (group, hour) pairs (compared
    before any merged rollup).  k_stream_buckets gives each wave a range of
    `per` points, per rounded up to 256, in steps of 4 x 64 lanes: the sizes
    put the batch's end one short of, on and one past a lane row (64), a step
    (256), a block's four waves (1024) and the first block (8192).  Its
    HMS_WC = 4 cached (key, bucket) pairs are evicted round-robin:
      one      one key, the largest group id and the stream's last hour: every
               row after the first hits the cache
      block64  a key per lane row: a step brings four keys, the next step evicts all
      cycle5, cycle9  5 and 9 keys alternating lane by lane: every row holds
               more keys than the cache, so keys are evicted and interned again
               within a row.  The cache saves probes; a wrong eviction order
               can cost time but no count, and this test holds for any order
      own      every point its own key (up to 8193 buckets in one batch)
    Path by the kept points' buckets: 1 the tail, 2-3 parallel runs, 4-64
    sequential runs, more the grouped pass; `spec`: on a fresh stream the batch
    is speculated on (k_stream_buckets runs twice for >= 2 buckets), after a
    two-bucket batch it is not (one pass that writes the ids)."""
    _par(monkeypatch, None)
    k = _edge_case(n, pattern, "both", spec)
    want = {"one": 1, "block64": (n + 63) // 64, "cycle5": min(5, n), "cycle9": min(9, n)}
    if pattern in want:
        assert k == want[pattern]
    else:
        assert n - n // 4 <= k <= n      # the keep mask drops about one in seven of the one-point keys


@pytest.mark.parametrize("n", [257, 8193])
@pytest.mark.parametrize("pattern,flavour", [(pt, fl) for fl in ("group", "hour") for pt in PATTERNS] + [("one", "plain")])
def test_bucket_key_components(gpu, monkeypatch, n, pattern, flavour):
    """The key's halves on their own: undated batches with explicit groups
    (0 and 0xFFFFFFFD among them), dated batches without a group (BASE and
    BASE + 2^28 - 1 among them), and a batch with neither (one bucket, no
    k_stream_buckets input at all)."""
    _par(monkeypatch, None)
    _edge_case(n, pattern, flavour, True)


def _hour_keys(lo, hi):
    return [(None, BASE + j) for j in range(lo, hi)]


def test_nearly_full_bucket_table(gpu, monkeypatch):
    """max_buckets = 1 gives the smallest table, 1024 slots.  1000 new hours
    in one batch (three points each, interleaved: every lane row misses the
    cache 64 times; the grouped path), then 16 more (sequential runs) into
    the 24 slots left: probe chains run long and wrap around the table's end.
    Rollups only afterwards: the merged alltime label takes a slot too."""
    _par(monkeypatch, None)
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, max_buckets=1)
    m = sm.StreamModel(ZMIN, ZMAX)
    for b, total in ((Batch(3000, _hour_keys(0, 1000), seed=1, keep="all"), 1000),
                     (Batch(160, _hour_keys(1000, 1016), seed=2, keep="all"), 1016)):
        s.add(b.lat, b.lon, b.keep, b.hour)
        m.add(b.rows, b.cols, b.keep, b.hour)
        assert s.buckets() == m.buckets() == total
        assert s.cells()[0] == len(m.records())
        _same_records(_rec(*s.export()), m.records(), "export()")
    g, h, z, r, c, n = s.rollup("hour", merge_groups=False)      # (its labels are the raw buckets)
    _same_records(_rec(g, h, z, r, c, n), m.dated(), "per-group hour rollup")
    got = s.counts(ALLTIME).sorted()
    for a, b in zip((got.zoom, got.row, got.col, got.count), m.counts(ALLTIME)):
        assert np.array_equal(a, b)
    assert s.buckets() == 1017
    s.close()


@pytest.mark.parametrize("free", ["expire", "forget"])
def test_full_bucket_table(gpu, monkeypatch, free):
    """A batch whose new keys exceed the slots left answers HM_E_CAPACITY and
    leaves no cell behind (buckets it may); expire or forget then frees slots
    and the same batch fits.  The 1024-slot table holds 1000 hours; the batch
    brings 40 new ones.  It comes first right after the 1000-bucket batch
    (not speculated) and, once slots are free, after the expire or forget
    (last_nparts = 1: speculated, tail dropped, sequential runs).  No rollup
    before the capacity assertions: a label needs a slot."""
    _par(monkeypatch, None)
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, max_buckets=1)
    m = sm.StreamModel(ZMIN, ZMAX)
    b = Batch(3000, _hour_keys(0, 1000), seed=1, keep="all")
    s.add(b.lat, b.lon, b.keep, b.hour)
    m.add(b.rows, b.cols, b.keep, b.hour)
    assert s.buckets() == 1000
    over = Batch(400, _hour_keys(1000, 1040), seed=2)
    assert len(over.keys()) == 40 > 1024 - s.buckets()
    with pytest.raises(Exception) as want:
        _lib.raise_for(_lib.HM_E_CAPACITY)
    with pytest.raises(Exception) as got:
        s.add(over.lat, over.lon, over.keep, over.hour)
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    assert 1000 <= s.buckets() <= 1024
    assert s.cells()[0] == len(m.records())
    _same_records(_rec(*s.export()), m.records(), "export() after the failed batch")
    if free == "expire":
        dropped, freed = s.expire(BASE + 100)
        m.expire(BASE + 100)
    else:
        dropped, freed = s.forget(hours=(BASE + 900, BASE + 1000))
        m.forget(hours=(BASE + 900, BASE + 1000))
    # an expire keeps the buckets of surviving cells only; a forget carries every
    # bucket it did not select over, the failed batch's unused ones included
    assert dropped > 0 and freed >= 100 and m.buckets() == 900
    assert s.buckets() == 900 if free == "expire" else 900 <= s.buckets() <= 924
    s.add(over.lat, over.lon, over.keep, over.hour)
    m.add(over.rows, over.cols, over.keep, over.hour)
    assert s.buckets() == m.buckets() == 940
    assert s.cells()[0] == len(m.records())
    _same_records(_rec(*s.export()), m.records(), "export()")
    g, h, z, r, c, n = s.rollup("hour", merge_groups=False)
    _same_records(_rec(g, h, z, r, c, n), m.dated(), "per-group hour rollup")
    got = s.counts(ALLTIME).sorted()
    for a, b in zip((got.zoom, got.row, got.col, got.count), m.counts(ALLTIME)):
        assert np.array_equal(a, b)
    s.close()
