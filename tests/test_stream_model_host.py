"""CPU: the stream model of the ingest tests (tests/stream_model.py) against
the C oracle, and its own operations against recomputation.

The model claims that a tile-centre point's cell at zoom z is its zoom-zmax
tile shifted right: checked here field by field against oracle.count over the
centres' lat/lon, for everything and per hour, at zooms 0-12 and 3-12.
expire, forget and import_records are checked against a model rebuilt from
the surviving points alone."""
import numpy as np
import pytest

from oracle import oracle
import stream_model as sm

BASE = 480000
ZMAX = 12
N = 5000


@pytest.fixture(scope="module")
def cloud():
    """5000 zoom-12 tiles: half uniform over the square (its corners
    included), half clustered so that fine cells repeat; 5 hours, 3 groups,
    a keep mask."""
    rng = np.random.default_rng(20240521)
    rows = rng.integers(0, 1 << ZMAX, N)
    cols = rng.integers(0, 1 << ZMAX, N)
    rows[N // 2:] = 1500 + rng.integers(0, 40, N - N // 2)
    cols[N // 2:] = 2600 + rng.integers(0, 40, N - N // 2)
    rows[:4] = [0, 0, (1 << ZMAX) - 1, (1 << ZMAX) - 1]
    cols[:4] = [0, (1 << ZMAX) - 1, 0, (1 << ZMAX) - 1]
    hour = BASE + rng.integers(0, 5, N)
    group = rng.integers(0, 3, N)
    keep = (np.arange(N) % 7 != 3).astype(np.uint8)
    lat, lon = sm.centre(rows, cols, ZMAX)
    return rows, cols, keep, hour, group, lat, lon


def _same(got, ref):
    assert ref["status"] == 0
    for a, k in zip(got, ("zoom", "row", "col", "count")):
        assert np.array_equal(a, ref[k]), k


def _model(cloud, zmin, mask=None, dated=True, grouped=True):
    rows, cols, keep, hour, group, _, _ = cloud
    m = sm.StreamModel(zmin, ZMAX)
    kp = keep if mask is None else keep & mask.astype(np.uint8)
    m.add(rows, cols, kp, hour if dated else None, group if grouped else None)
    return m


@pytest.mark.parametrize("zmin", [0, 3])
def test_model_counts_equal_oracle(cloud, zmin):
    rows, cols, keep, hour, group, lat, lon = cloud
    m = _model(cloud, zmin)
    ref = oracle.count(lat, lon, keep, zmin, ZMAX)
    if zmin == 0:
        assert len(ref["count"]) > 10000      # the uniform half alone: thousands of one-point cells
    _same(m.counts(sm.ALLTIME), ref)
    assert int(m.counts(sm.ALLTIME)[3].sum()) == int(keep.sum()) * (ZMAX - zmin + 1)
    for h in range(BASE, BASE + 5):
        _same(m.counts(h), oracle.count(lat, lon, keep & (hour == h).astype(np.uint8), zmin, ZMAX))
    # without a mask, and split over several add() calls in another order
    m2 = sm.StreamModel(zmin, ZMAX)
    for part in (slice(3000, N), slice(0, 1000), slice(1000, 3000)):
        m2.add(rows[part], cols[part], None, hour[part], group[part])
    _same(m2.counts(sm.ALLTIME), oracle.count(lat, lon, None, zmin, ZMAX))


def test_model_records(cloud):
    """One record per distinct (group, hour, cell), sorted; groups and hours
    partition the counts; NOGROUP and UNDATED_HOUR stand in when absent."""
    rows, cols, keep, hour, group, lat, lon = cloud
    m = _model(cloud, 0)
    rec = m.records()
    assert len(np.unique(rec[:, :5], axis=0)) == len(rec)
    assert np.array_equal(rec, sm.sort_records(rec))
    assert m.buckets() == len(sm.batch_keys(N, keep, hour, group)) == 15
    for g in range(3):
        for h in (BASE, BASE + 4):
            part = rec[(rec[:, 0] == g) & (rec[:, 1] == h)]
            ref = oracle.count(lat, lon, keep & ((hour == h) & (group == g)).astype(np.uint8), 0, ZMAX)
            _same((part[:, 2], part[:, 3], part[:, 4], part[:, 5]), ref)
    ga = m.group_alltime()
    one = ga[ga[:, 0] == 1]
    _same((one[:, 1], one[:, 2], one[:, 3], one[:, 4]), oracle.count(lat, lon, keep & (group == 1).astype(np.uint8), 0, ZMAX))
    assert np.array_equal(m.dated(), rec) and not m.has_undated()
    plain = _model(cloud, 0, dated=False, grouped=False)
    assert plain.has_undated() and plain.buckets() == 1 and len(plain.dated()) == 0
    assert set(plain.records()[:, 0]) == {sm.NOGROUP} and set(plain.records()[:, 1]) == {sm.UNDATED_HOUR}
    _same(plain.counts(sm.ALLTIME), oracle.count(lat, lon, keep, 0, ZMAX))
    assert sm.batch_keys(N, np.zeros(N, np.uint8), hour, group).shape == (0, 2)


def test_expire_forget_import_equal_recomputation(cloud):
    rows, cols, keep, hour, group, _, _ = cloud
    m = _model(cloud, 0)
    total = len(m.records())
    # expire
    gone = m.expire(BASE + 2)
    left = _model(cloud, 0, hour >= BASE + 2)
    assert np.array_equal(m.records(), left.records()) and gone == total - len(left.records())
    assert m.expire(BASE + 2) == 0
    # forget by group, by hours, by both
    m.forget(groups=[1])
    assert np.array_equal(m.records(), _model(cloud, 0, (hour >= BASE + 2) & (group != 1)).records())
    m.forget(hours=(BASE + 3, BASE + 4))
    surv = (hour >= BASE + 2) & (group != 1) & (hour != BASE + 3)
    assert np.array_equal(m.records(), _model(cloud, 0, surv).records())
    m.forget(groups=[0], hours=(BASE + 4, BASE + 9))
    surv &= ~((group == 0) & (hour == BASE + 4))
    assert np.array_equal(m.records(), _model(cloud, 0, surv).records())
    # undated records are in no hour range and outlive every expire
    u = _model(cloud, 0, dated=False)
    n = len(u.records())
    assert u.expire(BASE + 100) == 0 and u.forget(hours=(BASE, BASE + 100)) == 0 and len(u.records()) == n
    assert u.forget(groups=[0, 1, 2]) == n and len(u.records()) == 0
    # import: another model's records add up with this one's, duplicates in the input too
    a, b = _model(cloud, 0, group == 0), _model(cloud, 0, group != 0)
    a.import_records(b.records())
    assert np.array_equal(a.records(), _model(cloud, 0).records())
    twice = sm.StreamModel(0, ZMAX)
    twice.import_records(np.concatenate([b.records(), b.records()[::-1]]))
    want = b.records().copy()
    want[:, 5] *= 2
    assert np.array_equal(twice.records(), want)


def test_count_keys_and_centres():
    k = sm.count_keys([0, 12], [0, 4095], [0, 7])
    assert k.dtype == np.uint64 and k.tolist() == [0, (12 << 58) | (4095 << 29) | 7]
    lat, lon = sm.centre([0, 2047, 4095], [0, 2048, 4095], 12)
    row, col, st, _ = oracle.project(lat, lon, 12)
    assert st.tolist() == [0, 0, 0] and row.tolist() == [0, 2047, 4095] and col.tolist() == [0, 2048, 4095]
