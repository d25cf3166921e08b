"""The host side of selections (hm_stream_forget, hm_stream_export_select;
StreamingHeatmap.forget and the users / groups / hours arguments of export,
snapshot and merge_from) on the CPU.

csrc/hm_stream_select.h is plain C: a shim around it is built here with the
host compiler, and the ids it hands the verdict kernel -- sorted, distinct --
and the search that kernel runs over them are compared with Python sets.  The
label rule and the filter of the out-of-square records are module-level pure
functions of heatmap_amd.stream and are checked without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")
HEADER = os.path.join(REPO, "include", "heatmap_amd.h")
MAXG = 1 << 20
NOGROUP = 0xFFFFFFFE
SHIM = """
#include "hm_stream_select.h"
int64_t select_ids(const uint32_t* groups, int64_t n, uint32_t* out) { return hms_select_ids(groups, n, out); }
int select_has(const uint32_t* ids, uint32_t n, uint32_t g) { return hms_select_has(ids, n, g); }
int select_max(void) { return HMS_SELECT_MAX_GROUPS; }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_select")
    src, lib = d / "shim.c", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                    str(src), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.select_ids.argtypes = [u32p, ctypes.c_int64, u32p]
    L.select_ids.restype = ctypes.c_int64
    L.select_has.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32]
    return L


def normalise(shim, ids, n=None):
    """(status, sorted distinct ids) of hms_select_ids over `ids` (None: a NULL pointer, with the count n)"""
    u32p = ctypes.POINTER(ctypes.c_uint32)
    if ids is None:
        return shim.select_ids(None, n, None), None
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    count = len(a) if n is None else n
    out = np.full(max(len(a), 1), 0xABABABAB, dtype=np.uint32)
    m = shim.select_ids(a.ctypes.data_as(u32p) if len(a) else out.ctypes.data_as(u32p), count, out.ctypes.data_as(u32p))
    return m, (out[:m].copy() if m > 0 else None)


def check(shim, ids, probes=()):
    m, out = normalise(shim, ids)
    want = sorted(set(int(v) for v in ids))
    assert m == len(want) and out.tolist() == want
    u32p = ctypes.POINTER(ctypes.c_uint32)
    have = set(want)
    for g in list(probes) + want[:50] + [0, 1, NOGROUP, want[0] + 1, max(want[-1], 1) - 1]:
        assert bool(shim.select_has(out.ctypes.data_as(u32p), m, g)) == (g in have), g


def test_select_max_matches_the_abi(shim):
    assert shim.select_max() == MAXG


def test_every_group_and_refused_counts(shim):
    assert normalise(shim, None, 0)[0] == 0              # NULL, 0: every group
    for n in (1, -1, 5, MAXG + 1):
        assert normalise(shim, None, n)[0] == -1         # NULL with a count
    assert normalise(shim, [], 0)[0] == -1               # a pointer with no id
    assert normalise(shim, [3], -1)[0] == -1
    big = np.zeros(MAXG + 1, dtype=np.uint32)
    assert normalise(shim, big)[0] == -1
    assert normalise(shim, big[:MAXG])[0] == 1           # the limit itself, all one id


def test_one_duplicates_descending_nogroup(shim):
    check(shim, [7])
    check(shim, [0])
    check(shim, [5, 5, 5, 5])
    check(shim, [9, 3, 9, 3, 1, 1, 0])
    check(shim, list(range(300, 0, -1)), probes=[301, 150])
    check(shim, [NOGROUP])
    check(shim, [NOGROUP, 0, NOGROUP, 12], probes=[NOGROUP - 1, 11, 13])


def test_the_merged_marker_is_refused(shim):
    for ids in ([0xFFFFFFFF], [1, 2, 0xFFFFFFFF], [0xFFFFFFFF, 4], [3] * 70 + [0xFFFFFFFF] + [9] * 70):
        assert normalise(shim, ids)[0] == -1


@pytest.mark.parametrize("n", [1, 2, 65, 100000])
def test_random_ids_against_sets(shim, n):
    rng = np.random.default_rng(n)
    wide = rng.integers(0, 0xFFFFFFFF, n, dtype=np.uint64)            # 0 .. 0xFFFFFFFE
    check(shim, wide, probes=rng.integers(0, 0xFFFFFFFF, 200, dtype=np.uint64).tolist())
    narrow = rng.integers(0, max(2, n // 3), n, dtype=np.uint64)      # many repeats
    check(shim, narrow, probes=range(0, max(2, n // 3) + 3, max(1, n // 300)))


# ------------------------------------------------------------------ the ABI

NEW = ("hm_stream_forget", "hm_stream_export_select")


def test_both_names_are_declared_exported_and_listed():
    from heatmap_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    L = _lib.load()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in exported and name in _lib.EXPORTS
        assert getattr(L, name).argtypes
    assert re.search(r"^#define HM_SELECT_MAX_GROUPS \(1 << 20\)$", src, flags=re.M)
    assert re.search(r"^#define HM_ABI_VERSION 7$", src, flags=re.M)
    assert _lib.HM_SELECT_MAX_GROUPS == MAXG


def test_null_handles_answer_e_arg():
    """before any device call: so also on a machine without a GPU"""
    from heatmap_amd import _lib

    L = _lib.load()
    ids = (ctypes.c_uint32 * 2)(1, 2)
    a, b, n = ctypes.c_int64(77), ctypes.c_int64(78), ctypes.c_int64(79)
    out = [(ctypes.c_uint64 * 4)(7, 7, 7, 7), (ctypes.c_uint64 * 4)(7, 7, 7, 7), (ctypes.c_uint32 * 4)(7, 7, 7, 7),
           (ctypes.c_uint32 * 4)(7, 7, 7, 7)]
    ptrs = [ctypes.cast(o, ctypes.c_void_p) for o in out]
    for groups, ng, lo, hi in ((ids, 2, 0, 5), (None, 0, -1, -1), (None, 0, 0, 5)):
        assert L.hm_stream_forget(None, groups, ng, lo, hi, ctypes.byref(a), ctypes.byref(b)) == _lib.HM_E_ARG
        assert L.hm_stream_export_select(None, groups, ng, lo, hi, *ptrs, 4, ctypes.byref(n)) == _lib.HM_E_ARG
    assert (a.value, b.value, n.value) == (77, 78, 79)
    assert all(list(o) == [7] * 4 for o in out)


# ------------------------------------------------- labels and side records

def test_select_labels():
    from heatmap_amd.stream import _select_labels

    assert _select_labels(["u1", "all", "route", "nobody"]) == ["u1", "all", "route", "nobody"]
    assert _select_labels("u1") == ["u1"]                 # one id, not its letters
    assert _select_labels([]) == []
    with pytest.raises(ValueError, match="never had a group"):
        _select_labels(["u1", "xhidden"])
    with pytest.raises(ValueError, match="route"):
        _select_labels(["rt-17"])
    with pytest.raises(TypeError):
        _select_labels([3])


def test_select_ids():
    from heatmap_amd.stream import _select_ids

    index = {"all": 0, "u1": 1, "route": 2, "u2": 3}
    assert _select_ids(None, None, index) is None
    got = _select_ids(["u2", "all", "route", "nobody", "u2"], None, index)
    assert got.dtype == np.uint32 and got.tolist() == [3, 0, 2, 3]
    assert "nobody" not in index                           # an unknown label is not interned
    assert _select_ids(["nobody"], None, index).tolist() == []
    assert _select_ids(["u1"], [NOGROUP, 9, 1], index).tolist() == [1, NOGROUP, 9, 1]
    assert _select_ids(None, np.array([4, 2], dtype=np.uint32), index).tolist() == [4, 2]
    assert _select_ids(None, 5, index).tolist() == [5]
    for bad in ([0xFFFFFFFF], [-1], [1 << 40]):
        with pytest.raises(ValueError, match="outside"):
            _select_ids(None, bad, index)
    with pytest.raises(TypeError):
        _select_ids(None, [1.5], index)
    with pytest.raises(ValueError, match="at most"):
        _select_ids(None, np.zeros(MAXG + 1, dtype=np.uint32), index)
    with pytest.raises(ValueError):
        _select_ids(["xother"], [1], index)
    with pytest.raises(ValueError):
        _select_ids(["rt-1"], None, index)


def test_select_hours():
    from heatmap_amd.stream import _select_hours

    assert _select_hours(None) is None
    assert _select_hours((5, 9)) == (5, 9) and _select_hours([np.int64(5), 6]) == (5, 6)
    for bad in ((5, 5), (9, 5), (-1, -1), (1, 2, 3), 7, "ab"):
        with pytest.raises(ValueError):
            _select_hours(bad)


def test_forget_records_against_a_loop():
    from heatmap_amd.stream import UNDATED_HOUR, _forget_records, _select_records

    rng = np.random.default_rng(5)
    groups = [0, 1, 2, 7, NOGROUP]
    hours = [UNDATED_HOUR, 100, 101, 102, 105, 110]
    x = np.array([(g, h, 18, int(rng.integers(-5, 0)), int(rng.integers(0, 9)), int(rng.integers(1, 9)))
                  for g in groups for h in hours for _ in range(2)], dtype=np.int64)
    x = x[rng.permutation(len(x))]
    for ids in (None, [1], [1, 1, 7], [NOGROUP], [NOGROUP, 0], [3], [], np.array([2, 0], dtype=np.uint32)):
        for hr in (None, (100, 101), (101, 106), (90, 100), (0, 1 << 40), (111, 200), (-5, 101)):
            sel = [bool((ids is None or int(row[0]) in [int(v) for v in ids]) and
                        (hr is None or (row[1] != UNDATED_HOUR and hr[0] <= row[1] < hr[1]))) for row in x]
            assert _select_records(x, ids, hr).tolist() == sel
            kept, gone = _forget_records(x, ids, hr)
            assert gone == sum(sel) and np.array_equal(kept, x[~np.array(sel, dtype=bool)])
    kept, gone = _forget_records(np.zeros((0, 6), np.int64), [1], (0, 5))
    assert gone == 0 and kept.shape == (0, 6)


def test_forget_needs_an_argument():
    """checked before any device call"""
    from heatmap_amd.stream import StreamingHeatmap

    s = StreamingHeatmap.__new__(StreamingHeatmap)
    s._index = {"all": 0}
    with pytest.raises(ValueError, match="needs users, groups or hours"):
        s.forget()
    with pytest.raises(ValueError, match="never had a group"):
        s.forget(users=["xhidden"])
    with pytest.raises(ValueError, match="hold no hour"):
        s.forget(hours=(9, 9))
