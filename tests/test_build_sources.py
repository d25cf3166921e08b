"""heatmap_amd/build.py against csrc/: every translation unit is built, and the
staleness check sees every source and header there (no hand-kept list)."""
import os

import pytest

from heatmap_amd import build


def test_sources_are_the_translation_units_of_csrc():
    units = sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp", ".c")) and f != build.SCALAR_SRC)
    assert sorted(build.SOURCES) == units
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    for f in build.SOURCES:
        assert os.path.isfile(os.path.join(build.CSRC, f)), f


def _fake_products(tmp_path, monkeypatch, when):
    """a library and a scalar module of mtime `when`, in place of the real ones"""
    lib = tmp_path / "libheatmap_amd.so"
    mod = tmp_path / "_hm_scalar.so"
    for p in (lib, mod):
        p.write_bytes(b"")
        os.utime(p, (when, when))
    monkeypatch.setattr(build, "LIB", str(lib))
    monkeypatch.setattr(build, "scalar_module_path", lambda: str(mod))


def _newest_dependency():
    deps = [os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC)]
    deps.append(os.path.join(os.path.dirname(build.HERE), "include", "heatmap_amd.h"))
    return max(os.path.getmtime(d) for d in deps)


def test_fresh_library_is_not_stale(tmp_path, monkeypatch):
    _fake_products(tmp_path, monkeypatch, _newest_dependency() + 10)
    assert not build._stale()


@pytest.mark.parametrize("header", ["hm_genkey.h", "hm_runs.h", "hm_stamps.h", "hm_pipeline.h"])
def test_library_older_than_one_header_is_stale(tmp_path, monkeypatch, header):
    """only `header` is newer than the library: a copy of csrc/ whose other
    files are all older"""
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for f in os.listdir(build.CSRC):
        (csrc / f).write_bytes(b"")
        os.utime(csrc / f, (1000, 1000))
    monkeypatch.setattr(build, "CSRC", str(csrc))
    inc = os.path.getmtime(os.path.join(os.path.dirname(build.HERE), "include", "heatmap_amd.h"))
    os.utime(csrc / header, (inc + 20, inc + 20))
    _fake_products(tmp_path, monkeypatch, inc + 10)
    assert build._stale()
    os.utime(csrc / header, (1000, 1000))
    assert not build._stale()
