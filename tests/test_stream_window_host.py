"""CPU: the host side of the stream's sliding windows and retention -- the
selection of the out-of-square side records (stream._window_records,
stream._expire_records) against a brute-force loop, and the argument checks of
hm_stream_window / hm_stream_expire that need no GPU."""
import os
import subprocess
import sys

import numpy as np

from heatmap_amd.stream import ALLGROUPS, NOGROUP, UNDATED_HOUR, _expire_records, _window_records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H0 = 480000


def _records(seed=3, n=400):
    """(group, hour or UNDATED_HOUR, zoom, row, col, count) records: few
    distinct cells, so several hours and groups share a cell."""
    rng = np.random.default_rng(seed)
    g = rng.choice([1, 2, 3, NOGROUP], n)
    h = np.where(rng.random(n) < 0.2, UNDATED_HOUR, H0 + rng.integers(0, 8, n))
    z = rng.integers(0, 3, n)
    r = rng.integers(-2, 1, n)
    c = (1 << z) + rng.integers(0, 2, n)
    cnt = rng.integers(1, 50, n)
    rec = np.stack([g, h, z, r, c, cnt], axis=1).astype(np.int64)
    # as StreamingHeatmap keeps them: one record per (group, hour, cell)
    u, inv = np.unique(rec[:, :5], axis=0, return_inverse=True)
    tot = np.zeros(len(u), np.int64)
    np.add.at(tot, inv.reshape(-1), rec[:, 5])
    return np.concatenate([u, tot[:, None]], axis=1)


def _brute_window(x, lo, hi, merge):
    out = {}
    for g, h, z, r, c, n in x.tolist():
        if h == UNDATED_HOUR or not (lo <= h < hi):
            continue
        k = (ALLGROUPS if merge else g, z, r, c)
        out[k] = out.get(k, 0) + n
    return out


def _as_dict(rec):
    d = {tuple(row[:4]): row[4] for row in rec.tolist()}
    assert len(d) == len(rec)       # summed: one record per (group, cell)
    return d


def test_window_records_match_brute_force():
    x = _records()
    assert (x[:, 1] == UNDATED_HOUR).any() and (x[:, 0] == NOGROUP).any()
    for lo, hi in [(H0, H0 + 1), (H0 + 2, H0 + 5), (H0 + 7, H0 + 8), (H0 - 10, H0 + 100), (H0 + 8, H0 + 20),
                   (-5, H0), (UNDATED_HOUR, H0 + 3)]:
        for merge in (True, False):
            want = _brute_window(x, lo, hi, merge)
            assert _as_dict(_window_records(x, lo, hi, merge)) == want, (lo, hi, merge)
    # the bounds: lo is in, hi is out
    only = x[(x[:, 1] == H0 + 3)]
    assert _as_dict(_window_records(x, H0 + 3, H0 + 4, False)) == _brute_window(only, H0 + 3, H0 + 4, False)
    assert len(_window_records(x, H0 + 8, H0 + 20, True)) == 0            # no data: empty
    assert len(_window_records(x, UNDATED_HOUR, H0, True)) == 0           # undated records are in no window
    every = _window_records(x, H0, H0 + 8, True)
    assert every[:, 4].sum() == x[x[:, 1] != UNDATED_HOUR][:, 5].sum()
    assert (every[:, 0] == ALLGROUPS).all()


def test_window_records_empty():
    x = np.zeros((0, 6), np.int64)
    assert _window_records(x, 0, 10, True).shape == (0, 5)
    assert _window_records(x, 0, 10, False).shape == (0, 5)
    kept, gone = _expire_records(x, 10)
    assert kept.shape == (0, 6) and gone == 0


def test_expire_records_match_brute_force():
    x = _records(seed=8)
    for cut in (H0 - 1, H0, H0 + 1, H0 + 4, H0 + 8, H0 + 1000):
        kept, gone = _expire_records(x, cut)
        want = [row for row in x.tolist() if row[1] == UNDATED_HOUR or row[1] >= cut]
        assert kept.tolist() == want, cut
        assert gone == len(x) - len(want), cut
    kept, gone = _expire_records(x, H0 + 1000)
    assert len(kept) and (kept[:, 1] == UNDATED_HOUR).all()     # undated records never expire
    kept, gone = _expire_records(x, H0)
    assert gone == 0 and np.array_equal(kept, x)                # nothing below the cut


def test_null_stream_is_an_argument_error():
    """hm_stream_window(NULL, ...) and hm_stream_expire(NULL, ...) answer
    HM_E_ARG before anything touches a device (a child process: the library
    is loaded without a GPU)."""
    code = r"""
import ctypes
from heatmap_amd import _lib
L = _lib.load()
n, a, b = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int64(7)
print("WINDOW", L.hm_stream_window(None, 0, 24, 1, None, None, None, 0, ctypes.byref(n)))
print("EXPIRE", L.hm_stream_expire(None, 100, ctypes.byref(a), ctypes.byref(b)))
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert "WINDOW 16" in r.stdout, r.stdout + r.stderr
    assert "EXPIRE 16" in r.stdout, r.stdout + r.stderr
