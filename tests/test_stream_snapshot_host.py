"""Host side of the streaming heatmap's snapshots and merging (no device): the
snapshot's pack / unpack and file round trip, the group-id remap by label, the
out-of-square records under a remap, and the refusals (format version, zooms)."""
import zipfile

import numpy as np
import pytest

from heatmap_amd import _lib
from heatmap_amd.stream import (NOGROUP, SNAPSHOT_VERSION, UNDATED_HOUR, _check_zooms, _explicit_group_max, _group_lut,
                                _load_snapshot, _pack_snapshot, _remap_groups, _remap_records, _save_snapshot,
                                _sum_records, _unpack_snapshot)


def _snap():
    keys = np.array([(3 << 58) | (5 << 29) | 7, (18 << 58) | (262143 << 29) | 1, 0], dtype=np.uint64)
    counts = np.array([4, 1 << 40, 9], dtype=np.uint64)
    groups = np.array([1, NOGROUP, 2], dtype=np.uint32)
    hours = np.array([480000, _lib.HM_STREAM_UNDATED, 480017], dtype=np.uint32)
    x = np.array([[1, 480003, 18, -4, 262144, 2], [NOGROUP, UNDATED_HOUR, 0, 0, 1, 5]], dtype=np.int64)
    return _pack_snapshot(0, 18, 480000, ["all", "u1", "zoë|x"], -1, keys, counts, groups, hours, x)


def _same_snapshot(a, b):
    assert set(a) == set(b)
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape and np.array_equal(va, vb), k
        else:
            assert type(va) is type(vb) and va == vb, k


def test_pack_unpack_round_trip():
    s = _snap()
    assert s["version"] == SNAPSHOT_VERSION and (s["zmin"], s["zmax"], s["base_hour"]) == (0, 18, 480000)
    assert s["labels"].dtype.kind == "U" and s["labels"].tolist() == ["all", "u1", "zoë|x"]
    assert s["keys"].dtype == np.uint64 and s["groups"].dtype == np.uint32 and s["x"].shape == (2, 6)
    _same_snapshot(_unpack_snapshot(s), s)
    # an empty stream: no cells, no records, the one label
    e = _pack_snapshot(2, 5, 7, ["all"], -1, [], [], [], [], np.zeros((0, 6), np.int64))
    assert e["keys"].shape == (0,) and e["x"].shape == (0, 6)
    _same_snapshot(_unpack_snapshot(e), e)


def test_file_round_trip_holds_no_pickle(tmp_path):
    s = _snap()
    path = tmp_path / "stream.snapshot"
    with open(path, "wb") as f:
        _save_snapshot(f, s)
    _same_snapshot(_load_snapshot(path), s)
    # plain arrays only: every member loads with pickling refused
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(s)
        for k in f.files:
            assert f[k].dtype.kind in "iuU", k
    with zipfile.ZipFile(path) as z:
        assert sorted(n[:-4] for n in z.namelist()) == sorted(s)


def test_unknown_version_and_incomplete_snapshots_are_refused(tmp_path):
    s = _snap()
    bad = dict(s, version=SNAPSHOT_VERSION + 1)
    with pytest.raises(ValueError, match="version %d" % (SNAPSHOT_VERSION + 1)):
        _unpack_snapshot(bad)
    path = tmp_path / "newer.npz"
    with open(path, "wb") as f:
        _save_snapshot(f, bad)
    with pytest.raises(ValueError, match="version"):
        _load_snapshot(path)
    with pytest.raises(ValueError, match="version"):
        _unpack_snapshot({k: v for k, v in s.items() if k != "version"})
    with pytest.raises(ValueError, match="lacks counts"):
        _unpack_snapshot({k: v for k, v in s.items() if k != "counts"})
    with pytest.raises(ValueError, match="length"):
        _unpack_snapshot(dict(s, hours=s["hours"][:2]))


def test_zoom_mismatch_is_refused():
    s = _snap()
    _check_zooms(s, 0, 18)
    for zmin, zmax in ((1, 18), (0, 17), (0, 21)):
        with pytest.raises(ValueError, match="zooms 0..18"):
            _check_zooms(s, zmin, zmax)


def test_group_lut_known_and_new_labels():
    index, labels = {"all": 0, "u2": 1, "u1": 2}, ["all", "u2", "u1"]
    lut = _group_lut(["all", "u1", "u3", "u2", "route"], index, labels)
    assert lut.dtype == np.int64 and lut.tolist() == [0, 2, 3, 1, 4, NOGROUP]
    assert labels == ["all", "u2", "u1", "u3", "route"]
    assert index == {"all": 0, "u2": 1, "u1": 2, "u3": 3, "route": 4}
    # again: everything is known, nothing is appended
    assert _group_lut(["all", "u1", "u3", "u2", "route"], index, labels).tolist() == lut.tolist()
    assert len(labels) == 5
    # numpy unicode labels (a loaded snapshot's) are plain strings afterwards
    _group_lut(np.array(["all", "u9"]), index, labels)
    assert labels[-1] == "u9" and type(labels[-1]) is str


def test_remap_groups_gather_nogroup_and_bound():
    lut = np.array([0, 2, 3, 1, NOGROUP], dtype=np.int64)   # four source labels
    g = np.array([3, 0, NOGROUP, 1, 2, NOGROUP, 3], dtype=np.int64)
    assert _remap_groups(g, lut).tolist() == [1, 0, NOGROUP, 2, 3, NOGROUP, 1]
    assert _remap_groups(np.zeros(0, np.int64), lut).tolist() == []
    # the id bound: 4 has no label, and the merged-rollup marker is no group either
    with pytest.raises(ValueError, match="cell 2: group id 4 "):
        _remap_groups(np.array([0, 3, 4, 9], dtype=np.int64), lut)
    with pytest.raises(ValueError, match="cell 1: group id %d " % 0xFFFFFFFF):
        _remap_groups(np.array([NOGROUP, 0xFFFFFFFF], dtype=np.int64), lut)


def test_remap_groups_on_torch_tensors():
    torch = pytest.importorskip("torch")
    lut = torch.tensor([0, 2, 3, 1, NOGROUP], dtype=torch.int64)
    g = torch.tensor([3, 0, NOGROUP, 1, 2], dtype=torch.int64)
    assert _remap_groups(g, lut).tolist() == [1, 0, NOGROUP, 2, 3]
    with pytest.raises(ValueError, match="cell 1: group id 7 "):
        _remap_groups(torch.tensor([0, 7], dtype=torch.int64), lut)
    assert _explicit_group_max(g) == 3


def test_explicit_ids():
    assert _explicit_group_max(np.array([5, 0, NOGROUP, 17, 2], dtype=np.int64)) == 17
    assert _explicit_group_max(np.array([NOGROUP, NOGROUP], dtype=np.int64)) == -1
    assert _explicit_group_max(np.zeros(0, np.int64)) == -1
    # 0xFFFFFFFF names no group: the import kernel reports that cell
    assert _explicit_group_max(np.array([3, 0xFFFFFFFF], dtype=np.int64)) == 3
    assert _explicit_group_max(np.array([NOGROUP - 1], dtype=np.int64)) == NOGROUP - 1


def test_out_of_square_records_merge_under_a_remap():
    mine = np.array([[1, 480003, 18, -4, 7, 2], [2, UNDATED_HOUR, 18, -4, 7, 1]], dtype=np.int64)
    other = np.array([[2, 480003, 18, -4, 7, 10],          # the other's 2 is this stream's 1: sums with mine[0]
                      [1, UNDATED_HOUR, 18, -4, 7, 20],    # its 1 is this stream's 2: sums with mine[1]
                      [NOGROUP, 480003, 18, -4, 7, 5],     # stays without a group
                      [3, 480004, 0, 0, 1, 6]], dtype=np.int64)   # a label this stream did not know
    index, labels = {"all": 0, "a": 1, "b": 2}, ["all", "a", "b"]
    lut = _group_lut(["all", "b", "a", "c"], index, labels)
    got = _sum_records(np.concatenate([mine, _remap_records(other, lut)]), 5)
    want = np.array([[1, 480003, 18, -4, 7, 12], [2, UNDATED_HOUR, 18, -4, 7, 21], [3, 480004, 0, 0, 1, 6],
                     [NOGROUP, 480003, 18, -4, 7, 5]], dtype=np.int64)
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    assert other[0, 0] == 2                      # the source's records are left as they were
    assert _remap_records(np.zeros((0, 6), np.int64), lut).shape == (0, 6)
    with pytest.raises(ValueError, match="group id 4 "):
        _remap_records(np.array([[4, 1, 0, 0, 1, 1]]), lut)


def test_binding_lists_the_new_entry_points():
    assert {"hm_stream_export", "hm_stream_import"} <= set(_lib.EXPORTS)
    assert _lib.HM_STREAM_UNDATED == 0xFFFFFFFF and _lib.HM_IMPORT_DISTINCT == 1
