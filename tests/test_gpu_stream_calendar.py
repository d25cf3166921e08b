"""GPU: the calendar of hm_stream_rollup (hms_civil, hms_label and
hms_period_value in csrc/hm_stream.hip) against Python's datetime.

One stream based at hour 0 holds a few points at 00:00 and 23:00 of the days
where a civil-from-days conversion goes wrong first -- the epoch, the turn of
a 400-year leap year (2000), its leap day, an ordinary and a leap February, a
century non-leap year (2100), the next 400-year leap day (2400) and
9999-12-31 -- and at 200 hours drawn from the whole range.  Hour j of the list
holds j % 5 + 1 points, so a period that swallowed or lost an hour has the
wrong sum.  The reference is a dict {(group, period): points} built with
datetime.datetime.fromtimestamp(hour * 3600, tz=utc): the period is the hour,
days since 1970-01-01, year * 12 + month - 1, the year, or 0.

Hours beyond 9999-12-31 23:00 (hour 70_389_527; a stream's base_hour may go up
to 2^32) are not covered: datetime ends there and cannot serve as reference.
"""
import datetime

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import synth
from heatmap_amd.stream import ALLGROUPS, StreamingHeatmap, span_label

pytestmark = pytest.mark.gpu

UTC = datetime.timezone.utc
EPOCH = datetime.date(1970, 1, 1)
ZMIN, ZMAX = 0, 4
GROUPS = (5, 77)
LAST_HOUR = 70_389_527      # 9999-12-31 23:00
SPANS = ("hour", "day", "month", "year", "alltime")
DAYS = [(1970, 1, 1), (1999, 12, 31), (2000, 1, 1), (2000, 2, 28), (2000, 2, 29), (2000, 3, 1), (2023, 2, 28),
        (2023, 3, 1), (2024, 2, 29), (2100, 2, 28), (2100, 3, 1), (2400, 2, 29), (9999, 12, 31)]


def _hour(y, m, d, h=0):
    return (datetime.date(y, m, d) - EPOCH).days * 24 + h


def _period(span, hour):
    """The period of an epoch hour, from datetime alone."""
    t = datetime.datetime.fromtimestamp(int(hour) * 3600, tz=UTC)
    if span == "hour":
        return int(hour)
    if span == "day":
        return (t.date() - EPOCH).days
    if span == "month":
        return t.year * 12 + t.month - 1
    if span == "year":
        return t.year
    return 0


def _points(hours, seed):
    """(lat, lon, hour, group): hour j of the list gets j % 5 + 1 in-square
    points (hotspot cloud: |lat| < 71), groups alternating."""
    per = [j % 5 + 1 for j in range(len(hours))]
    n = sum(per)
    lat, lon = synth.generate("hotspots", n, seed=seed)
    hour = np.repeat(np.asarray(hours, dtype=np.uint32), per)
    group = np.asarray([GROUPS[i % 2] for i in range(n)], dtype=np.uint32)
    return lat, lon, hour, group


class _Data:
    pass


@pytest.fixture(scope="module")
def cal(gpu):
    assert _hour(9999, 12, 31, 23) == LAST_HOUR and LAST_HOUR < (1 << 28)
    hours = [_hour(y, m, d, h) for (y, m, d) in DAYS for h in (0, 23)]
    rnd = np.random.default_rng(2024).integers(0, LAST_HOUR + 1, 200).tolist()
    hours += rnd
    # two batches of more than 64 (group, hour) buckets; the second repeats hours 100..139
    b1 = _points(hours[:140], seed=41)
    b2 = _points(hours[100:], seed=42)
    d = _Data()
    d.s = StreamingHeatmap(ZMIN, ZMAX, base_hour=0)
    for lat, lon, hour, group in (b1, b2):
        assert len(set(zip(hour.tolist(), group.tolist()))) > 64
        d.s.add(lat, lon, None, hour, group=group)
    d.lat, d.lon, d.hour, d.group = (np.concatenate([x, y]) for x, y in zip(b1, b2))
    d.first = b1
    d.random_hour = int(rnd[17])
    d.period = {span: np.asarray([_period(span, h) for h in d.hour.tolist()], dtype=np.int64) for span in SPANS}
    yield d
    d.s.close()


def _want(d, span, merge, sel=None):
    """{(group, period): points} of the points under the mask sel."""
    out = {}
    for i in range(d.hour.size):
        if sel is not None and not sel[i]:
            continue
        k = (ALLGROUPS if merge else int(d.group[i]), int(d.period[span][i]))
        out[k] = out.get(k, 0) + 1
    return out


def _zoom0(res):
    """{(group, period): count} of a rollup's zoom-0 cells; each pair once."""
    g, p, z, r, c, cnt = res
    m = z == 0
    assert not r[m].any() and not c[m].any()
    out = {(int(a), int(b)): int(n) for a, b, n in zip(g[m], p[m], cnt[m])}
    assert len(out) == int(m.sum()), "a (group, period) pair came back twice"
    return out


def _cells(res, group, period, zoom):
    g, p, z, r, c, cnt = res
    m = (g == group) & (p == period) & (z == zoom)
    o = np.lexsort((c[m], r[m]))
    return r[m][o], c[m][o], cnt[m][o]


def _oracle_cells(d, sel, zoom):
    ref = oracle.count(d.lat[sel], d.lon[sel], None, zoom, zoom)
    assert ref["status"] == 0
    return ref["row"], ref["col"], ref["count"]


def _chosen(d, span):
    """The periods holding 2000-02-29, 2100-03-01 and one of the random hours."""
    return [_period(span, _hour(2000, 2, 29, 23)), _period(span, _hour(2100, 3, 1)), _period(span, d.random_hour)]


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("span", SPANS)
def test_rollup_periods_match_datetime(cal, span, merge):
    d = cal
    res = d.s.rollup(span, merge_groups=merge)
    want = _want(d, span, merge)
    assert _zoom0(res) == want
    for p in _chosen(d, span):
        for grp in ((ALLGROUPS,) if merge else GROUPS):
            sel = d.period[span] == p
            if not merge:
                sel = sel & (d.group == grp)
            if not sel.any():
                assert (grp, p) not in want
                continue
            for a, b in zip(_cells(res, grp, p, ZMAX), _oracle_cells(d, sel, ZMAX)):
                assert np.array_equal(a, b), (span, p, grp)


@pytest.mark.parametrize("span", SPANS)
def test_rollup_select(cal, span):
    """select = p returns period p alone, with the cells of the full rollup
    (and of the oracle); a period without data returns nothing."""
    d = cal
    full = d.s.rollup(span, merge_groups=True)
    for p in sorted(set(_chosen(d, span))):
        res = d.s.rollup(span, merge_groups=True, select=p)
        sel = d.period[span] == p
        assert _zoom0(res) == {(ALLGROUPS, p): int(sel.sum())}, (span, p)
        assert set(res[1].tolist()) == {p}
        for zoom in (ZMIN, ZMAX):
            for a, b, c in zip(_cells(res, ALLGROUPS, p, zoom), _cells(full, ALLGROUPS, p, zoom),
                               _oracle_cells(d, sel, zoom)):
                assert np.array_equal(a, b) and np.array_equal(a, c), (span, p, zoom)
        # per group as well: the same select, one record set per group
        resg = d.s.rollup(span, merge_groups=False, select=p)
        assert _zoom0(resg) == _want(d, span, False, sel), (span, p)
    have = set(d.period[span].tolist())
    if span == "alltime":
        empty = 1
    else:   # the day after 2000-02-29 23:00 holds 2000-03-01; take a period nothing falls in
        empty = next(q for q in range(_period(span, _hour(2000, 2, 29)) + 2, 1 << 27) if q not in have)
    res = d.s.rollup(span, merge_groups=True, select=empty)
    assert res[0].size == 0, (span, empty)


def test_rollup_base_hour_far_from_zero(cal):
    """The same hours in a stream based at 2099-12-31 00:00 (period words are
    offsets from the base; the calendar takes base + offset): the periods of
    2100-02-28 .. 2100-03-01 are those of the stream based at hour 0."""
    d = cal
    lat, lon, hour, group = d.first
    lo, hi = _hour(2100, 2, 28), _hour(2100, 3, 1, 23)
    m = (hour >= lo) & (hour <= hi)
    assert len(set(hour[m].tolist())) == 4
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=_hour(2099, 12, 31))
    try:
        s.add(lat[m], lon[m], None, hour[m], group=group[m])
        for span in SPANS:
            want = {}
            for h, g in zip(hour[m].tolist(), group[m].tolist()):
                k = (g, _period(span, h))
                want[k] = want.get(k, 0) + 1
            got = _zoom0(s.rollup(span, merge_groups=False))
            assert got == want, span
            if span != "alltime":   # and they are the periods the first stream gives these hours
                first = _zoom0(d.s.rollup(span, merge_groups=False))
                assert set(got) <= set(first), span
    finally:
        s.close()


@pytest.mark.parametrize("span", ["day", "month", "year"])
def test_rows_label_leap_day(gpu, span):
    """rows(span) labels the 2000-02-29 points with build_timespan_label of
    the datetime-derived period, and the neighbouring days with theirs."""
    lat, lon = synth.generate("hotspots", 12, seed=9)
    hour = np.asarray([_hour(2000, 2, 28, 23)] * 3 + [_hour(2000, 2, 29, 0)] * 3 + [_hour(2000, 2, 29, 23)] * 3 +
                      [_hour(2000, 3, 1, 0)] * 3, dtype=np.uint32)
    users = ["other"] * 3 + ["leap"] * 6 + ["other"] * 3
    s = StreamingHeatmap(ZMIN, ZMAX, base_hour=0)
    try:
        s.add(lat, lon, None, hour, user_id=users)
        rows = s.rows(span, max_zoom_level=ZMAX - 1, delta=1)
    finally:
        s.close()
    want = {"leap": {span_label(span, _period(span, _hour(2000, 2, 29, 12)))},
            "other": {span_label(span, _period(span, _hour(2000, 2, 28))),
                      span_label(span, _period(span, _hour(2000, 3, 1)))}}
    assert want["leap"] == {{"day": "2000-02-29", "month": "2000-02", "year": "2000"}[span]}
    for user in ("leap", "other"):
        assert {k.split("|")[1] for k in rows if k.split("|")[0] == user} == want[user], (span, user)
