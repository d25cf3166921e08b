"""Frames of the resident streaming heatmap (hm_stream_raster_frames,
hm_raster_accumulate; StreamingHeatmap.tile_frames / tile_series /
tile_frame_images) vs the oracle: frame f equals one oracle count over the
points of ITS hours densified by the model (tests/raster_model.py), and equals
tile_raster of those hours.  The tiles sit on the oracle's heaviest cells and
the expected grids are asserted non-zero.

The streams are those of tests/test_gpu_stream_view.py (hours BASE .. BASE +
17): the main one holds well over 4 x 8192 cells (several blocks and a ragged
last chunk), the tiny one is one partial chunk, the zooms 6-12 one has pyramid
offsets that do not start at 0."""
import ctypes

import numpy as np
import pytest

import raster_model as model
from oracle import oracle
from heatmap_amd import _lib, device, raster, synth
from heatmap_amd.stream import StreamingHeatmap
from test_gpu_stream_view import BASE, ZMAX, ZMIN, Data, _heaviest

pytestmark = pytest.mark.gpu
END = BASE + 18                       # the data's hours are [BASE, END)


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def main(gpu, data):
    """the main stream with user groups; the tests that use it leave it as it is"""
    s = data.stream()
    assert s.cells()[0] > 4 * 8192
    s.state_at_start = (s.cells(), s.buckets())
    yield s
    s.close()


def _expect(ref, tiles, b, h):
    assert ref["status"] == 0
    return model.densify_arrays(ref["zoom"], ref["row"], ref["col"], ref["count"], tiles, b, h)


def _tiles_on(ref, b):
    """tests/test_gpu_stream_raster.py's tiles: the tile of zoom 18 - b on the
    oracle's heaviest zoom-18 cell, two of its neighbours (the halos overlap)
    and the tile of zoom 13 - b on the heaviest zoom-13 cell"""
    r, c = _heaviest(ref, 18)
    tz = 18 - b
    tr, tc = r >> b, c >> b
    nr, nc = (tr + 1 if tr + 1 < (1 << tz) else tr - 1), (tc + 1 if tc + 1 < (1 << tz) else tc - 1)
    r13, c13 = _heaviest(ref, 13)
    return [(tz, tr, tc), (tz, tr, nc), (tz, nr, nc), (13 - b, r13 >> b, c13 >> b)]


def _frames(lo, hi, fh):
    """the hours [a, b) of every frame of (lo, hi) cut by fh"""
    return [(a, min(a + fh, hi)) for a in range(lo, hi, fh)]


def _want(data, spans, tiles, b, h, extra=None):
    """[F, T, W, W]: the oracle's densified count of each span of hours"""
    w = (1 << b) + 2 * h
    out = np.zeros((len(spans), len(tiles), w, w), dtype=np.int64)
    for f, (a, e) in enumerate(spans):
        a, e = max(a, BASE), min(e, END)
        if a < e:                     # else: no point has such an hour
            out[f] = _expect(data.ref(a, e, extra), tiles, b, h)
    return out


WINDOWS = [(BASE, END, 1), (BASE, END, 3), (BASE, END, 5), (BASE, END, 18), (BASE, END, 40),
           (BASE + 4, BASE + 11, 3), (BASE - 7, BASE + 6, 4), (BASE + 10, BASE + 400, 100)]


@pytest.mark.parametrize("user", [None, "u2"])
@pytest.mark.parametrize("b,h", [(5, 2), (3, 8), (0, 0)])
@pytest.mark.parametrize("lo,hi,fh", WINDOWS)
def test_equals_the_oracle_and_tile_raster(main, data, lo, hi, fh, b, h, user):
    extra = None if user is None else data.users == user
    tiles = _tiles_on(data.ref(max(lo, BASE), min(hi, END), extra), b)    # on the window's own heaviest cells
    spans = _frames(lo, hi, fh)
    want = _want(data, spans, tiles, b, h, extra)
    assert want[:, 0].any() and want[:, 3].any()
    if (lo, hi, fh) == (BASE - 7, BASE + 6, 4):          # anchored at hour_lo: frame 1 is hour BASE alone
        assert spans[1] == (BASE - 3, BASE + 1)
        assert np.array_equal(want[1], _expect(data.ref(BASE, BASE + 1, extra), tiles, b, h)) and want[1].any()
    if len(spans) > 1 and hi <= END:
        assert want[-1].any() and (want[0] != want[-1]).any()
    got = main.tile_frames(tiles, (lo, hi), fh, user, bins_log2=b, halo=h)
    assert str(got.dtype) == "torch.int64" and tuple(got.shape) == want.shape and got.is_contiguous()
    got = got.cpu().numpy()
    for f, span in enumerate(spans):
        assert np.array_equal(got[f], want[f]), (f, span)
        assert np.array_equal(main.tile_raster(tiles, span, user, bins_log2=b, halo=h).cpu().numpy(), want[f]), span
    # conservation: the frames sum to the raster of the whole window
    whole = main.tile_raster(tiles, (lo, hi), user, bins_log2=b, halo=h).cpu().numpy()
    assert whole.any() and np.array_equal(got.sum(axis=0), whole)


def test_late_batch_and_undated_cells(gpu, data):
    """tests/test_gpu_stream_raster.py's recipe: a late batch of old hours (its
    keys repeat in the log, which no query compacts) adds to its own hours'
    frames; undated cells have no hour and are in no frame"""
    s = data.stream()
    lat0, lon0, keep0, hour0, us0 = data.batches[0]
    lat1, lon1, keep1, _, us1 = data.batches[1]
    s.add(lat0, lon0, keep0, hour0, user_id=us0)          # the same points again, hours already in the log
    s.add(lat1, lon1, keep1, None, user_id=us1)           # undated
    try:
        lat, lon = np.concatenate([data.lat, lat0]), np.concatenate([data.lon, lon0])
        keep = np.concatenate([data.keep, keep0]) == 1
        hour = np.concatenate([data.hour, hour0.astype(np.int64)])
        b, h, fh = 5, 1, 2
        tiles = _tiles_on(data.ref(), b)
        spans = _frames(BASE, END, fh)
        want = np.stack([_expect(oracle.count(lat, lon, (keep & (hour >= a) & (hour < e)).astype(np.uint8), ZMIN, ZMAX),
                                 tiles, b, h) for a, e in spans])
        alone = _want(data, spans, tiles, b, h)
        assert set(np.unique(hour0)) == {BASE, BASE + 1, BASE + 2}
        assert (want[0] > alone[0]).any() and (want[1] > alone[1]).any()      # the late batch, in frames 0 and 1
        assert np.array_equal(want[2:], alone[2:]) and want[2:].any()         # ... and in no other
        got = s.tile_frames(tiles, (BASE, END), fh, None, b, h).cpu().numpy()
        assert np.array_equal(got, want)
        # the undated points: in alltime, in no frame
        every = s.tile_raster(tiles, None, None, b, h).cpu().numpy()
        assert (every > got.sum(axis=0)).any()
        assert np.array_equal(got.sum(axis=0), s.tile_raster(tiles, (BASE, END), None, b, h).cpu().numpy())
        # one group, with the late batch in it
        m = np.concatenate([data.users, np.array(us0)]) == "u1"
        want1 = np.stack([_expect(oracle.count(lat, lon, (keep & m & (hour >= a) & (hour < e)).astype(np.uint8), ZMIN,
                                               ZMAX), tiles, b, h) for a, e in spans[:2]])
        assert want1.any() and (want1 != want[:2]).any()
        assert np.array_equal(s.tile_frames(tiles, (BASE, BASE + 4), fh, "u1", b, h).cpu().numpy(), want1)
    finally:
        s.close()


def test_tiny_and_empty_streams(gpu):
    """50 points of one hour: one partial chunk of one block; an empty stream;
    windows that hold nothing; a base hour above and below hour_lo"""
    lat, lon = synth.generate("hotspots", 50, seed=3)
    ref = oracle.count(lat, lon, np.ones(50, np.uint8), ZMIN, ZMAX)
    for base in (BASE, BASE - 100):
        s = StreamingHeatmap(ZMIN, ZMAX, base_hour=base)
        try:
            tiles = [(0, 0, 0), (5, 3, 3)]
            g = s.tile_frames(tiles, (BASE, BASE + 3), 1, None, 4, 2)         # the empty stream
            assert tuple(g.shape) == (3, 2, 20, 20) and not g.any()
            s.add(lat, lon, None, np.full(50, BASE + 1, np.uint32))
            for b in (0, 4, 8):
                r, c = _heaviest(ref, 10 + b)
                tiles = [(0, 0, 0), (10, r >> b, c >> b), (10, r >> b, c >> b)]
                want = _expect(ref, tiles, b, 2)
                assert want[0].any() and want[1].any() and np.array_equal(want[1], want[2])
                # hour BASE + 1 is frame 1 of hourly frames from BASE, and frame (1 + 10) // 4 = 2 from BASE - 10
                for lo, hi, fh, f in ((BASE, BASE + 4, 1, 1), (BASE - 10, BASE + 5, 4, 2), (BASE - 50, BASE + 9, 17, 3)):
                    got = s.tile_frames(tiles, (lo, hi), fh, None, b, 2).cpu().numpy()
                    assert got.shape[0] == -(-(hi - lo) // fh)
                    assert np.array_equal(got[f], want), (base, b, lo, hi, fh)
                    assert not np.delete(got, f, axis=0).any()
            # a window that holds nothing, and windows outside the stream's hours
            for hours in ((BASE + 2, BASE + 7), (BASE - 9, BASE - 1), (BASE - 500, BASE - 100), (0, 3)):
                g = s.tile_frames(tiles, hours, 2, None, 4, 2)
                assert g.shape[0] == -(-(hours[1] - hours[0]) // 2) and not g.any()
        finally:
            s.close()


def test_zooms_6_to_12_stream(gpu, data):
    """pyramid offsets that do not start at 0; bin zooms at both ends of the stream's range"""
    s = StreamingHeatmap(6, 12, base_hour=BASE)
    try:
        for lat, lon, keep, hour, _ in data.batches[:2]:
            s.add(lat, lon, keep, hour)
        n = 2 * len(data.batches[0][0])
        whole = oracle.count(data.lat[:n], data.lon[:n], data.keep[:n], 6, 12)
        spans = _frames(BASE - 1, BASE + 6, 3)            # hours BASE .. BASE + 5 in frames of 2, 3 and 1 of them
        refs = [oracle.count(data.lat[:n], data.lon[:n],
                             ((data.keep[:n] == 1) & (data.hour[:n] >= a) & (data.hour[:n] < e)).astype(np.uint8), 6, 12)
                for a, e in spans]
        for tz, b, h in ((6, 0, 8), (12, 0, 3), (1, 5, 8), (4, 8, 1)):
            r, c = _heaviest(whole, tz + b)
            tiles = [(tz, r >> b, c >> b), (tz, 0, 0), (tz, (1 << tz) - 1, (1 << tz) - 1)]
            want = np.stack([_expect(ref, tiles, b, h) for ref in refs])
            assert all(want[f, 0].any() for f in range(3))
            assert np.array_equal(s.tile_frames(tiles, (BASE - 1, BASE + 6), 3, None, b, h).cpu().numpy(), want)
        for tiles, b in (([(0, 0, 0)], 5), ([(5, 0, 0)], 8), ([(13, 0, 0)], 0)):
            with pytest.raises(ValueError):
                s.tile_frames(tiles, (BASE, BASE + 2), 1, None, b, 0)
    finally:
        s.close()


def _cell_count(ref, z, r, c):
    m = (np.asarray(ref["zoom"]) == z) & (np.asarray(ref["row"]) == r) & (np.asarray(ref["col"]) == c)
    return int(np.asarray(ref["count"]).astype(np.int64)[m].sum())


@pytest.mark.parametrize("user", [None, "u3"])
def test_series(main, data, user):
    extra = None if user is None else data.users == user
    own = data.ref(BASE, END, extra)
    tiles = [(13,) + _heaviest(own, 13), (18,) + _heaviest(own, 18), (0, 0, 0)]
    for lo, hi, fh in ((BASE, END, 3), (BASE - 2, BASE + 25, 1)):
        spans = _frames(lo, hi, fh)
        want = np.array([[_cell_count(data.ref(max(a, BASE), min(e, END), extra), *t) if max(a, BASE) < min(e, END)
                          else 0 for t in tiles] for a, e in spans], dtype=np.int64)
        assert (want[:, 0] > 0).sum() > 2 and want[:, 1].any() and len(set(want[:, 2])) > 2
        got = main.tile_series(tiles, (lo, hi), fh, user)
        assert str(got.dtype) == "torch.int64" and tuple(got.shape) == (len(spans), 3)
        assert np.array_equal(got.cpu().numpy(), want)
        frames = main.tile_frames(tiles, (lo, hi), fh, user, bins_log2=0)
        assert tuple(frames.shape) == (len(spans), 3, 1, 1)
        assert np.array_equal(frames[:, :, 0, 0].cpu().numpy(), want)


@pytest.mark.parametrize("lo,hi,fh,k", [(BASE + 1, BASE + 12, 2, 3),      # queried from BASE - 3: below the base
                                        (BASE + 8, BASE + 16, 2, 3),      # queried from BASE + 4
                                        (BASE + 2, BASE + 9, 1, 1)])      # a window of one frame: the frames
def test_trailing_windows_and_growth(main, data, lo, hi, fh, k):
    b, h = 5, 2
    tiles = _tiles_on(data.ref(), b)
    nf = -(-(hi - lo) // fh)
    got = main.tile_frames(tiles, (lo, hi), fh, None, b, h, trailing=k)
    assert tuple(got.shape) == (nf, 4, 36, 36)
    grown = main.tile_frames(tiles, (lo, hi), fh, None, b, h, trailing="all")
    assert tuple(grown.shape) == (nf, 4, 36, 36)
    for f in range(nf):
        a, e = lo + (f + 1 - k) * fh, min(lo + (f + 1) * fh, hi)
        want = main.tile_raster(tiles, (a, e), None, b, h)
        assert want.any() and gpu_equal(got[f], want), (f, a, e)
        want = main.tile_raster(tiles, (lo, e), None, b, h)
        assert want.any() and gpu_equal(grown[f], want), (f, lo, e)
    assert not gpu_equal(got[0], got[-1]) and not gpu_equal(grown[0], grown[-1])
    for bad in (0, -1, "some", 1.5):
        with pytest.raises(ValueError):
            main.tile_frames(tiles, (lo, hi), fh, None, b, h, trailing=bad)


def gpu_equal(a, b):
    import torch

    return bool(torch.equal(a, b))


def _as_dev(torch, x):
    return torch.from_numpy(x.view(np.int64)).cuda()


def test_accumulate_on_random_u64_grids(gpu):
    torch = gpu
    rng = np.random.default_rng(5)
    ctx = device.context(0)
    for nf in (1, 2, 7, 33):
        for elems in (1, 63, 64 * 256 + 5):
            x = rng.integers(0, 2 ** 64, (nf, elems), dtype=np.uint64)
            x[rng.random((nf, elems)) < 0.2] = 2 ** 64 - 1                     # sums that wrap
            x[rng.random((nf, elems)) < 0.2] = 0
            csum = np.concatenate([np.zeros((1, elems), np.uint64), np.cumsum(x, axis=0, dtype=np.uint64)])
            xin = _as_dev(torch, x)
            for window in sorted({0, 1, 2, nf - 1, nf, nf + 5}):
                k = nf if window == 0 or window > nf else window
                want = np.stack([csum[f + 1] - csum[max(0, f + 1 - k)] for f in range(nf)])   # modulo 2^64
                out = torch.full((nf + 1, elems), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
                rc = ctx.L.hm_raster_accumulate(ctx.ptr, device._ptr(xin), nf, elems, window, device._ptr(out))
                assert rc == _lib.HM_OK
                got = out.cpu().numpy().view(np.uint64)
                assert np.array_equal(got[:nf], want), (nf, elems, window)
                assert (got[nf] == 0x5A5A5A5A).all()                           # nothing behind the last frame
                if window == 1:
                    assert np.array_equal(want, x)
            # the Python form, on a tensor of more axes
            if elems == 63:
                y = raster.accumulate(xin.reshape(nf, 7, 3, 3), 2)
                assert tuple(y.shape) == (nf, 7, 3, 3)
                assert np.array_equal(y.cpu().numpy().view(np.uint64).reshape(nf, 63),
                                      np.stack([csum[f + 1] - csum[max(0, f - 1)] for f in range(nf)]))


def test_accumulate_bad_arguments_leave_the_output_untouched(gpu):
    torch = gpu
    ctx = device.context(0)
    nf, elems = 4, 100
    buf = torch.full((3 * nf * elems,), 0x1234567, dtype=torch.int64, device="cuda")
    ref = buf.clone()
    base = buf.data_ptr()
    size = nf * elems * 8

    def call(gin=base, nframes=nf, frame_elems=elems, window=2, gout=base + size):
        return ctx.L.hm_raster_accumulate(ctx.ptr, gin, nframes, frame_elems, window, gout)

    for kw in (dict(gin=None), dict(gout=None), dict(nframes=0), dict(nframes=-1), dict(frame_elems=0),
               dict(frame_elems=-5), dict(window=-1), dict(gout=base), dict(gout=base + 8), dict(gout=base + size - 8),
               dict(gin=base + size, gout=base + 8), dict(gin=base + size, gout=base + 2 * size - 8),
               dict(nframes=1 << 40, frame_elems=1 << 40)):
        assert call(**kw) == _lib.HM_E_ARG, kw
    assert ctx.L.hm_raster_accumulate(None, base, nf, elems, 2, base + size) == _lib.HM_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, ref)
    assert call() == _lib.HM_OK and call(gin=base + size, gout=base) == _lib.HM_OK   # side by side: no overlap
    torch.cuda.synchronize()
    assert torch.equal(buf[2 * nf * elems:], ref[2 * nf * elems:])
    with pytest.raises(ValueError):
        raster.accumulate(buf.reshape(3, -1), -1)


def test_seventy_tiles_by_three_frames(main, data):
    """more than HM_RASTER_MAX_TILES tiles go in parts, joined along T"""
    r, c = _heaviest(data.ref(), 16)
    b, h = 3, 1
    tr, tc = max((r >> b) - 3, 0), max((c >> b) - 5, 0)
    tiles = [(13, tr + i // 10, tc + i % 10) for i in range(70)]
    spans = _frames(BASE, END, 6)
    want = _want(data, spans, tiles, b, h)
    assert all(want[f, :64].any() and want[f, 64:].any() for f in range(3))
    got = main.tile_frames(tiles, (BASE, END), 6, None, b, h)
    assert tuple(got.shape) == (3, 70, 10, 10) and np.array_equal(got.cpu().numpy(), want)
    series = main.tile_series(tiles, (BASE, END), 6)
    assert tuple(series.shape) == (3, 70) and series[:, 64:].any()


def test_frame_images_share_one_scale(main, data):
    """the documented two-pass rule: vmax = ceil(the largest frame's vs / 2^4R)"""
    lo, hi, fh = BASE + 2, BASE + 12, 5
    b, radius = 5, 2
    r, c = _heaviest(data.ref(lo, hi), 17)
    tiles = [(17 - b, r >> b, c >> b), (17 - b, r >> b, (c >> b) ^ 1)]
    grids = _want(data, _frames(lo, hi, fh), tiles, b, radius)
    lut = raster.RAMPS["heat"]
    vs = [model.render(g, b, radius, radius, "log", None)[1] for g in grids]
    assert vs[0] != vs[1] and min(vs) > 0                 # each frame alone would take its own scale
    vmax = -(-max(vs) >> (4 * radius))
    want = [model.render(g, b, radius, radius, "log", vmax, lut) for g in grids]
    assert all(len(np.unique(lev)) > 3 for lev, _, _ in want)
    got = main.tile_frame_images(tiles, (lo, hi), fh, None, bins_log2=b, radius=radius)
    assert str(got.dtype) == "torch.uint8" and tuple(got.shape) == (2, 2, 32, 32, 4)
    for f in range(2):
        assert np.array_equal(got[f].cpu().numpy(), want[f][2]), f
    # a fixed vmax, linear
    fixed = main.tile_frame_images(tiles, (lo, hi), fh, None, bins_log2=b, radius=radius, scale="linear", vmax=40)
    for f in range(2):
        assert np.array_equal(fixed[f].cpu().numpy(), model.render(grids[f], b, radius, radius, "linear", 40, lut)[2])
    # growth since lo: the last frame is the whole window
    grown = main.tile_frame_images(tiles, (lo, hi), fh, None, bins_log2=b, radius=radius, vmax=40, trailing="all")
    assert gpu_equal(grown[1], main.tile_images(tiles, (lo, hi), None, bins_log2=b, radius=radius, vmax=40))
    png = raster.apng_bytes(got[:, 0])
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and b"acTL" in png[:64]


def test_user_selection(main, data):
    tiles = _tiles_on(data.ref(), 5)
    with pytest.raises(ValueError, match="tile_rows"):
        main.tile_frames(tiles, (BASE, END), 3, "all")
    with pytest.raises(ValueError):
        main.tile_frames(tiles, None)
    with pytest.raises(ValueError):
        main.tile_frames(tiles, (BASE, END), 0)
    for user in ("nobody", "xhidden"):                    # 'x...' ids make no group: no label either
        g = main.tile_frames(tiles, (BASE, END), 4, user, 5, 1)
        assert tuple(g.shape) == (5, 4, 34, 34) and not g.any()
        g = main.tile_frames(tiles, (BASE, END), 4, user, 5, 1, trailing=3)
        assert tuple(g.shape) == (5, 4, 34, 34) and not g.any()
        assert tuple(main.tile_series(tiles, (BASE, END), 4, user).shape) == (5, 4)


def test_raw_errors_leave_the_grid_untouched(main, data, gpu):
    torch = gpu
    SENT = 0x1234567
    g = torch.full((400,), SENT, dtype=torch.int64, device="cuda")
    ref = g.clone()
    M = _lib.HM_RASTER_MAX_FRAMES
    r, c = _heaviest(data.ref(), 8)
    on_data = (5, r >> 3, c >> 3)

    def call(lo=BASE, hi=BASE + 3, fh=1, group=_lib.HM_VIEW_MERGED, tiles=(on_data,), ntiles=1, b=3, h=1, s=main.ptr,
             grid=g):
        flat = [int(v) for t in tiles for v in t]
        ta = (ctypes.c_int64 * len(flat))(*flat)
        return main.ctx.L.hm_stream_raster_frames(s, lo, hi, fh, group, ta, ntiles, b, h, device._ptr(grid))

    for kw in (dict(fh=0), dict(fh=-1), dict(lo=-1, hi=-1), dict(lo=BASE + 2, hi=BASE + 2), dict(lo=BASE + 3, hi=BASE + 2),
               dict(hi=BASE + M + 1), dict(lo=BASE - 1, hi=BASE + 2 * M, fh=2), dict(group=_lib.HM_VIEW_EACH), dict(s=None),
               # the tile errors of hm_stream_raster
               dict(group=-3), dict(group=0xFFFFFFFF), dict(ntiles=0), dict(ntiles=65), dict(b=-1), dict(b=9),
               dict(h=-1), dict(h=9), dict(tiles=((-1, 0, 0),)), dict(tiles=((5, 32, 0),)), dict(tiles=((5, 0, -1),)),
               dict(tiles=((16, 0, 0),)), dict(tiles=((5, 1, 1), (5, 1, 32)), ntiles=2),
               dict(grid=torch.zeros(0, dtype=torch.int64, device="cuda"))):
        assert call(**kw) == _lib.HM_E_ARG, kw
    torch.cuda.synchronize()
    assert torch.equal(g, ref)
    # HM_OK zeroes exactly its nframes * ntiles * W * W = 3 * 1 * 10 * 10 elements
    assert call(lo=BASE - 50, hi=BASE - 47) == _lib.HM_OK
    torch.cuda.synchronize()
    assert not g[:300].any() and torch.equal(g[300:], ref[300:])
    g[:300] = SENT
    assert call(lo=BASE - 1, hi=BASE + 5, fh=2) == _lib.HM_OK         # hours with cells in them
    torch.cuda.synchronize()
    want = main.tile_frames([on_data], (BASE - 1, BASE + 5), 2, None, 3, 1)
    assert all(want[f].any() for f in range(3))
    assert torch.equal(g[:300], want.reshape(-1)) and torch.equal(g[300:], ref[300:])
    assert call(group=0xFFFFFFFE) == _lib.HM_OK                       # the cells without a group
    torch.cuda.synchronize()
    assert torch.equal(g[300:], ref[300:])


def test_the_stream_is_left_as_it_is(main, data):
    """nothing above compacted the log or interned a bucket, and nor does this"""
    tiles = _tiles_on(data.ref(), 5)
    main.tile_frames(tiles, (BASE - 7, BASE + 30), 4, "u2", 5, 2)
    main.tile_frames(tiles, (BASE, END), 1, None, 5, 2, trailing=3)
    main.tile_series(tiles, (BASE, END), 1)
    main.tile_frame_images(tiles[:1], (BASE + 2, BASE + 9), 3, None, bins_log2=5, radius=1)
    gpu_sync()
    assert (main.cells(), main.buckets()) == main.state_at_start


def gpu_sync():
    import torch

    torch.cuda.synchronize()
