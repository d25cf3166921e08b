"""hm_stream_add's capacity retries on every fold path, against the oracle.

3000 uniform points at zooms 0-18 make 38527 cells (oracle.count): far more
than the 2 n + 1024 = 7024 a count is first given room for, than the 8192
cells the log of initial_cells = 1024 grows to for that, and, split over three
hours (about 13640 cells a run), than a run's first 3024.  So the first
attempt overflows whichever way the batch is folded: one bucket counted into
the log's tail (the first batch speculatively, the second not, since the
first one of several hours turns speculation off), a few buckets as gathered
runs counted concurrently (HM_STREAM_PAR=1) or one after the other (=0), and
more buckets than HMS_MAX_PARTS through the grouped pass."""
import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import device, synth
from heatmap_amd.stream import ALLTIME, StreamingHeatmap

BASE = 480000
N, ZMIN, ZMAX = 3000, 0, 18
CASES = {"one_hour": (1, None), "three_hours_par": (3, "1"), "three_hours_seq": (3, "0"), "seventy_hours": (70, None)}


def _hours(b, nhours):
    """Batch b's hours: nhours of them from BASE + b, so the two batches share all but one"""
    return (BASE + b + np.arange(N) % nhours).astype(np.uint32)


@pytest.fixture(scope="module")
def cloud():
    lat = [synth.generate("uniform", N, seed=11, start=b * N)[0] for b in range(2)]
    lon = [synth.generate("uniform", N, seed=11, start=b * N)[1] for b in range(2)]
    refs = {}

    def ref(nhours, hour):
        """oracle.count of both batches' points of `hour` (ALLTIME: all), computed once"""
        if (nhours, hour) not in refs:
            keep = None if hour == ALLTIME else np.concatenate([_hours(b, nhours) == hour
                                                                for b in range(2)]).astype(np.uint8)
            refs[nhours, hour] = oracle.count(np.concatenate(lat), np.concatenate(lon), keep, ZMIN, ZMAX)
        return refs[nhours, hour]

    return lat, lon, ref


def _same(got, ref):
    got = got.sorted()
    assert ref["status"] == 0
    for a, b in zip((got.zoom, got.row, got.col, got.count), (ref["zoom"], ref["row"], ref["col"], ref["count"])):
        assert np.array_equal(a, b)


def test_the_input_overflows_every_first_attempt(cloud):
    """The sizes the module's docstring relies on, from the oracle (no GPU)."""
    lat, lon, ref = cloud
    one = oracle.count(lat[0], lon[0], None, ZMIN, ZMAX)
    assert len(one["count"]) == 38527 > 8192 > 2 * N + 1024
    for h in range(3):
        run = oracle.count(lat[0], lon[0], (_hours(0, 3) == BASE + h).astype(np.uint8), ZMIN, ZMAX)
        assert len(run["count"]) > 2 * (N // 3) + 1024


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_capacity_retries_match_oracle(gpu, monkeypatch, cloud, case):
    nhours, par = CASES[case]
    if par is not None:
        monkeypatch.setenv("HM_STREAM_PAR", par)
    lat, lon, ref = cloud
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1024)
    for b in range(2):
        s.add(lat[b], lon[b], None, _hours(b, nhours))
    _same(s.counts(ALLTIME), ref(nhours, ALLTIME))
    for hour in (BASE, BASE + 1):
        _same(s.counts(hour), ref(nhours, hour))
    cells, cap = s.cells()
    assert 0 < cells <= cap
    s.close()


@pytest.mark.gpu
def test_failing_second_batch_is_atomic_and_reports_hm_counts_point(gpu, cloud):
    """Three hours a batch, one NaN latitude in the second: the exception and
    hm_last_error are those of hm_count over that batch, and the stream holds
    what it held before."""
    lat, lon, ref = cloud
    bad = lat[1].copy()
    bad[1777] = np.nan
    ctx = device.context(0)
    with pytest.raises(ValueError) as want:
        device.count(bad, lon[1], None, ZMIN, ZMAX)
    want_at = ctx.last_error()
    assert want_at[0] == 1777
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=BASE, initial_cells=1024)
    s.add(lat[0], lon[0], None, _hours(0, 3))
    before = s.counts(ALLTIME).sorted()
    _same(before, oracle.count(lat[0], lon[0], None, ZMIN, ZMAX))
    with pytest.raises(ValueError) as got:
        s.add(bad, lon[1], None, _hours(1, 3))
    assert s.ctx.last_error() == want_at
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    after = s.counts(ALLTIME).sorted()
    for a, b in zip((after.zoom, after.row, after.col, after.count), (before.zoom, before.row, before.col, before.count)):
        assert np.array_equal(a, b)
    s.close()
