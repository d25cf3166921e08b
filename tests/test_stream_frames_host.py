"""The host side of frames (hm_stream_raster_frames, hm_raster_accumulate,
raster.apng_bytes) on the CPU.

csrc/hm_stream_frames.h is plain C: a shim around it is built here with the
host compiler, and the frame its plan gives every hour of a range -- what the
kernel computes from (lo, hi, phase, fh) and the host's frame0 -- is compared
with the frame the specification assigns: (h - hour_lo) / frame_hours for
hour_lo <= h < hour_hi, anchored at the caller's hour_lo."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")
HEADER = os.path.join(REPO, "include", "heatmap_amd.h")
MAXF = 1 << 16
CAP = 1 << 28
SHIM = """
#include "hm_stream_frames.h"
int frame_plan(int64_t base, int64_t lo, int64_t hi, int64_t fh, int64_t max_frames, int64_t* out)
{
    HmsFramePlan p;
    const int rc = hms_frame_plan(base, lo, hi, fh, max_frames, &p);
    if (rc) return rc;
    out[0] = p.nframes;
    out[1] = p.frame0;
    out[2] = p.lo;
    out[3] = p.hi;
    out[4] = p.fh;
    out[5] = p.phase;
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_frames")
    src, lib = d / "shim.c", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                    str(src), "-o", str(lib)], check=True)
    fn = ctypes.CDLL(str(lib)).frame_plan
    fn.argtypes = [ctypes.c_int64] * 5 + [ctypes.POINTER(ctypes.c_int64)]
    fn.restype = ctypes.c_int

    def call(base, lo, hi, fh, max_frames=MAXF):
        """(nframes, frame0, lo, hi, fh, phase), or None where the plan is refused"""
        out = (ctypes.c_int64 * 6)()
        return tuple(out) if fn(base, lo, hi, fh, max_frames, out) == 0 else None

    return call


def kernel_frame(p, x):
    """the frame k_stream_raster_frames gives a cell of hour offset x, or None"""
    nframes, frame0, lo, hi, fh, phase = p
    if not lo <= x < hi:
        return None
    assert 1 <= fh <= CAP and 0 <= phase < fh and x - lo + phase < 1 << 32     # the kernel's 32-bit words
    return frame0 + (x - lo + phase) // fh


def spec_frame(hour_lo, hour_hi, fh, h):
    return (h - hour_lo) // fh if hour_lo <= h < hour_hi else None


def check(plan, base, hour_lo, hour_hi, fh, offsets):
    """every offset: plan == specification; returns the frames met"""
    p = plan(base, hour_lo, hour_hi, fh)
    assert p is not None
    assert p[0] == -(-(hour_hi - hour_lo) // fh)
    assert 0 <= p[2] <= p[3] <= CAP
    met = set()
    for x in offsets:
        want = spec_frame(hour_lo, hour_hi, fh, base + x)
        assert kernel_frame(p, x) == want, (base, hour_lo, hour_hi, fh, x)
        if want is not None:
            assert 0 <= want < p[0]
            met.add(want)
    return met


BASE = 480000


@pytest.mark.parametrize("hour_lo,hour_hi,fh,frames", [
    (BASE, BASE + 18, 1, 18),            # frame_hours 1: a frame per hour
    (BASE, BASE + 18, 5, 4),             # does not divide the span: a 3-hour last frame
    (BASE + 4, BASE + 11, 3, 3),         # a one-hour last frame
    (BASE, BASE + 18, 40, 1),            # larger than the span
    (BASE - 3, BASE + 6, 4, 3),          # below the base by less than one frame
    (BASE - 7, BASE + 6, 4, 3),          # ... by more than one: frame 1 is [BASE - 3, BASE + 1), hour BASE only
    (BASE - 50, BASE + 30, 7, 5),        # ... by several frames
    (BASE - 8, BASE + 8, 8, 1),          # ... by exactly one
])
def test_every_hour_of_a_small_range(plan, hour_lo, hour_hi, fh, frames):
    met = check(plan, BASE, hour_lo, hour_hi, fh, range(0, 64))
    assert len(met) == frames            # the frames that hold an hour of the stream


def test_anchored_at_hour_lo_not_at_the_base(plan):
    p = plan(BASE, BASE - 7, BASE + 6, 4)
    assert [kernel_frame(p, x) for x in range(7)] == [1, 2, 2, 2, 2, 3, None]


def test_hour_hi_beyond_the_streams_hours(plan):
    """only the bounds handed to the kernel are clamped: nframes counts the caller's window"""
    hi = BASE + CAP + 1000
    p = plan(BASE, BASE + CAP - 100, hi, 30)
    assert p[0] == -(-1100 // 30) and (p[2], p[3]) == (CAP - 100, CAP)
    check(plan, BASE, BASE + CAP - 100, hi, 30, range(CAP - 130, CAP))
    # from below the base to beyond the end, frames of a million hours
    check(plan, BASE, BASE - 12345, hi, 1000003, list(range(0, 5000)) + list(range(987658 - 50, 987658 + 50)) +
          list(range(CAP - 5000, CAP)))


def test_a_window_outside_the_streams_hours_selects_nothing(plan):
    for lo, hi in ((BASE - 90, BASE - 10), (BASE - 1, BASE), (BASE + CAP, BASE + CAP + 9), (0, 5)):
        p = plan(BASE, lo, hi, 3)
        assert p is not None and p[0] == -(-(hi - lo) // 3) and p[2] == p[3]
        assert all(kernel_frame(p, x) is None for x in (0, 1, 77, CAP - 1))


def test_frames_longer_than_every_offset(plan):
    """frame_hours above 2^28: at most one edge is inside the offsets, and 32-bit words still find it"""
    big = (1 << 40) + 7
    spots = list(range(0, 300)) + list(range(CAP - 300, CAP))
    assert check(plan, BASE, BASE - 5, BASE + big, big, spots) == {0}
    # the edge between frames 0 and 1 at offset 100, then at the last offset, then just out of reach
    for edge in (100, CAP - 1, CAP):
        lo = BASE + edge - big
        met = check(plan, BASE, lo, lo + 3 * big, big, spots + list(range(max(edge - 50, 0), min(edge + 50, CAP))))
        assert met == ({0, 1} if edge < CAP else {0})
    assert check(plan, BASE, BASE + 10, BASE + 10 + big, CAP + 1, spots) == {0}
    assert check(plan, BASE, BASE - 10, BASE + big, CAP + 1, spots) == {0, 1}
    assert check(plan, BASE, -(1 << 62), 1 << 62, 1 << 50, spots) == {(BASE + (1 << 62)) >> 50}


def test_the_frame_cap(plan):
    assert plan(BASE, BASE, BASE + MAXF, 1)[0] == MAXF
    assert plan(BASE, BASE, BASE + MAXF + 1, 1) is None
    assert plan(BASE, BASE - 5, BASE - 5 + 3 * MAXF, 3)[0] == MAXF
    assert plan(BASE, BASE - 5, BASE - 5 + 3 * MAXF + 1, 3) is None
    assert plan(BASE, -(1 << 63), (1 << 63) - 1, 1) is None                       # 2^64 - 1 hours
    assert plan(BASE, -(1 << 63), (1 << 63) - 1, 1 << 48)[0] == MAXF
    check(plan, BASE, BASE, BASE + MAXF, 1, list(range(0, 40)) + list(range(MAXF - 40, MAXF + 40)))


def test_refused_plans(plan):
    for lo, hi, fh in ((BASE, BASE, 1), (BASE + 1, BASE, 1), (BASE, BASE + 5, 0), (BASE, BASE + 5, -1),
                       (BASE, BASE + 5, -(1 << 63))):
        assert plan(BASE, lo, hi, fh) is None


# ------------------------------------------------------------------ the ABI

NEW = ("hm_stream_raster_frames", "hm_raster_accumulate")


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
    assert re.search(r"^#define HM_RASTER_MAX_FRAMES \(1 << 16\)$", src, flags=re.M)
    assert _lib.HM_RASTER_MAX_FRAMES == MAXF


def test_null_handles_answer_e_arg():
    """before any device call: so also on a machine without a GPU"""
    from heatmap_amd import _lib

    L = _lib.load()
    tiles = (ctypes.c_int64 * 3)(0, 0, 0)
    grid = (ctypes.c_uint64 * 4)(7, 7, 7, 7)      # never touched: the handle is refused first
    assert L.hm_stream_raster_frames(None, 0, 5, 1, _lib.HM_VIEW_MERGED, tiles, 1, 0, 0, grid) == _lib.HM_E_ARG
    assert L.hm_raster_accumulate(None, grid, 2, 2, 0, grid) == _lib.HM_E_ARG
    assert list(grid) == [7] * 4


# --------------------------------------------------------------- apng_bytes

def chunks(png):
    """[(tag, data)] of a PNG, every length and CRC checked"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, i = [], 8
    while i < len(png):
        n, tag = struct.unpack(">I4s", png[i:i + 8])
        data = png[i + 8:i + 8 + n]
        assert len(data) == n
        assert struct.unpack(">I", png[i + 8 + n:i + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        out.append((tag, data))
        i += 12 + n
    assert i == len(png)
    return out


def rows(data, hgt, wid):
    raw = np.frombuffer(zlib.decompress(data), np.uint8).reshape(hgt, 1 + 4 * wid)
    assert not raw[:, 0].any()           # filter type 0
    return raw[:, 1:].reshape(hgt, wid, 4)


@pytest.mark.parametrize("nf,hgt,wid", [(1, 3, 5), (2, 1, 1), (5, 16, 9)])
def test_apng_chunks(nf, hgt, wid):
    from heatmap_amd import raster

    frames = np.random.default_rng(nf).integers(0, 256, (nf, hgt, wid, 4), dtype=np.uint8)
    ch = chunks(raster.apng_bytes(frames, delay_ms=250, loops=3))
    tags = [t for t, _ in ch]
    assert tags == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (nf - 1) + [b"IEND"]
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (wid, hgt, 8, 6, 0, 0, 0)
    assert struct.unpack(">II", ch[1][1]) == (nf, 3)
    seq, shown = [], []
    for tag, data in ch:
        if tag == b"fcTL":
            s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", data)
            assert (w, h, x, y, num, den, dispose, blend) == (wid, hgt, 0, 0, 250, 1000, 0, 0)
            seq.append(s)
        elif tag == b"IDAT":
            shown.append(rows(data, hgt, wid))
        elif tag == b"fdAT":
            seq.append(struct.unpack(">I", data[:4])[0])
            shown.append(rows(data[4:], hgt, wid))
    assert seq == list(range(2 * nf - 1))
    assert np.array_equal(np.stack(shown), frames)
    assert ch[-1] == (b"IEND", b"")


def test_apng_first_frame_is_the_still_png():
    """IHDR and IDAT are png_bytes' own: a viewer without APNG shows frame 0"""
    from heatmap_amd import raster

    frames = np.arange(2 * 4 * 4 * 4, dtype=np.uint8).reshape(2, 4, 4, 4)
    still, anim = chunks(raster.png_bytes(frames[0])), chunks(raster.apng_bytes(frames))
    assert anim[0] == still[0] and anim[3] == still[1]
    assert struct.unpack(">II", anim[1][1]) == (2, 0)                             # loops = 0: for ever


def test_apng_refuses_other_shapes():
    from heatmap_amd import raster

    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 4, 4), np.uint8), np.zeros((2, 4, 4, 3), np.uint8),
                np.zeros((2, 4, 4, 4), np.int32)):
        with pytest.raises(ValueError):
            raster.apng_bytes(bad)
    with pytest.raises(ValueError):
        raster.apng_bytes(np.zeros((1, 2, 2, 4), np.uint8), delay_ms=70000)


def test_frame_args_are_checked_without_a_device():
    from heatmap_amd.stream import _frame_args

    assert _frame_args(10, 28, 1, None) == (1, 0, None)
    assert _frame_args(10, 28, 5, 3) == (5, 2, 3)
    assert _frame_args(10, 28, 5, "all") == (5, 0, 0)
    assert _frame_args(0, MAXF, 1, None) == (1, 0, None)
    for fh, trailing in ((0, None), (-2, None), (1, 0), (1, -1), (1, "some"), (1, True), (1, 2.5)):
        with pytest.raises(ValueError):
            _frame_args(10, 28, fh, trailing)
    with pytest.raises(ValueError):
        _frame_args(0, MAXF + 1, 1, None)
    with pytest.raises(ValueError):
        _frame_args(0, MAXF, 1, 2)       # the leading frame counts
