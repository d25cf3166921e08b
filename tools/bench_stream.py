#!/usr/bin/env python3
"""Config 5 (BASELINE.json): streaming micro-batches of 10M points with uint32
epoch-hour timestamps merged into a resident multi-zoom heatmap (hm_stream_*).

One step = one hm_stream_add of a 10M-point hotspot batch (device-resident,
synthesised outside the timed region) whose points carry `--hours` distinct
hours; the heatmap keeps growing across steps, as a stream's would.  Prints
one JSON line (points/s over the timed batches, ms per batch, resident cells).

    python tools/bench_stream.py --batches 18 --warmup 2

With the defaults (2 + 18 batches of 10M hotspot points, one hour each) the
alltime cells are checked against the C oracle's digest of the same 200M
points (tests/golden/big_digests.json, hotspots_2e8_z0-18_stream20x10M).

    python tools/bench_stream.py --retain 24 --batches 40 --warmup 0

Retention mode: one-hour batches, each followed by expire(newest - H) and one
window(newest - H, newest + 1) query (hm_stream_expire / hm_stream_window).
The JSON line then carries ms per add, per expire and per window (median and
range over the batches that expired something), the expire pass's effective
GB/s over 16 B per log cell read plus 16 B per survivor written, next to the
library's read-stream kernel over the same bytes (hm_bench_read), and the
log's cells, capacity and the bucket count after every batch: with retention
they stop growing once H + 1 hours are resident.

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --view --out profiles/stream_view.json

--view: on the steady retained log, window(newest - H, newest + 1) against
view (hm_stream_view) of the same hours for two viewports -- (a) one heatmap
tile, the 32 x 32 block of detail zoom 13 around the heaviest zoom-13 cell, and
(b) a 4 x 3-tile screen at each of the detail zooms 8, 13 and 18 (3
rectangles) -- as host ms around the call, 15 repetitions each (interleaved),
median and range, with the cells out and a check that the view's cells equal
the window's filtered by rectangle on the host.  --window-only times the
window alone (the script then needs nothing newer than hm_stream_window, so a
checkout of an earlier commit can run it on the same log); --parent-json FILE
puts that run's "window" into this one's result as "parent_window".

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --snapshot --out profiles/stream_snapshot.json

--snapshot: on the steady retained log, hm_stream_export of the whole log and
hm_stream_import of that export into a fresh stream whose log is sized for it
(7 interleaved repetitions after one warm-up pair, host ms around the C call,
median and range, and the effective GB/s over 40 B per cell), one save() +
load() round trip through a file, and the only restore there is without
snapshots: the retained one-hour batches of raw points added again to a fresh
stream (3 repetitions).  "check": every restored stream's window over the
retained hours and its cell count equal the original's.  The yardsticks of the
same session are in the same JSON line: "ms_expire" (the nearest existing pass
over the same log) and "read_stream_GBps".  --readd-only times the re-adding
alone (nothing newer than hm_stream_window is needed, so a checkout of the
parent commit can run it); --parent-json FILE puts that run's "readd_ms" into
this one's result as "parent_readd_ms".

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --raster --out profiles/stream_raster.json

--raster: on the steady retained log, tile rasters (hm_stream_raster) and
rendered tiles (hm_raster_render) against the view (hm_stream_view) of the same
haloed rectangles, over the same hours, interleaved in one process, 15
repetitions each: (a) one heatmap tile, the 32 x 32 bins of zoom 13 around the
heaviest zoom-13 cell; (b) a 4 x 3-tile screen of 256 x 256-bin tiles of zoom
18 around the heaviest zoom-18 cell, halo = radius = 2.  Host ms around the C
call plus a synchronise (and the device ms between two events around the
raster), median and range; "check": every grid equals the view's cells
densified in numpy.  --view-only times the views alone (nothing newer than
hm_stream_view is needed, so a checkout of the parent commit can run it);
--parent-json FILE puts that run's view times into this one's result as
"parent_view_ms".

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --frames --out profiles/stream_frames.json

--frames: on the steady retained log, --raster's 4 x 3-tile screen of 256 x
256 zoom-18 bins with halo 2 as 24 hourly frames over the last 24 hours: one
hm_stream_raster_frames call ("frames_ms"), the same call with bins_log2 = 0
(the 12 tiles' hourly series, "series_ms"), hm_raster_accumulate with window =
6 over the frames and the render of all 24 frames (24 hm_raster_render calls),
against the only way there was before -- 24 hm_stream_raster calls, one per
hour ("loop_ms") -- and one hm_stream_raster of the whole window
("one_raster_pass_ms"); all interleaved in one process, 15 repetitions each,
host ms around the call(s) plus a synchronise, median and range.  "check":
every frame equals the hm_stream_raster grid of its hour, the series equal
the frames' interiors summed, the accumulated frames equal torch's.  The
accumulate is also given as GB/s over the bytes it must move (8 B read and 8 B
written per element), next to "read_stream_GBps".  --loop-only times the two
hm_stream_raster items alone (nothing newer is needed, so a checkout of the
parent commit can run it); --parent-json FILE puts that run's times into this
one's result as "parent_loop_ms" and "parent_one_raster_pass_ms".

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --forget --out profiles/stream_forget.json

--forget: the steady retained log is exported once to device arrays; every
timed call then runs on a fresh stream that imported them and ran one expire
that drops nothing, which makes the alternate arrays (both untimed), the calls
taking turns within a repetition: hm_stream_expire of a cut in the middle of the
retained hours; hm_stream_forget of the same hours (every group): the same
cells dropped, the same bytes moved; hm_stream_forget of one middle hour, and
the only path there was before for that (export, mask in torch, import into a
fresh stream); hm_stream_export_select of that one hour against the full
hm_stream_export; and, on the same cells imported with group = a hash of the
cell % 1000, hm_stream_forget of 10 of the 1000 groups against export + mask +
import.  Host ms around each call, which ends in its own wait; 2 warm-up
repetitions dropped.  --expire-only times the expire alone (no newer API is
needed, so a checkout of the parent commit can run it); --parent-json FILE puts
that run's times into this one's result as "parent_expire_ms".

--retain H --top ranks on the steady retained log, each ranking against the
route a caller had before it: the 100 hottest zoom-14 cells of the trailing 24
hours (top_device against view_device, a two-key device sort with torch and a
slice of 100), the same inside the 4 x 3-tile screen of --raster at its detail
zoom, and the 10 most active groups on that screen (hm_stream_top_groups
against view_device(..., 'each'), a per-group sum and the sort) on the same
cells imported with group = a hash of the cell % 1000.  Both routes are warmed,
then take TOP_REPS alternating repetitions; host ms around each, which ends in
a synchronise; median and min-max of each, and "not distinguishable" when the
ranges overlap; for the two cell rankings also the selection alone
(hm_cells_top) against the sort alone, on the view's cells.  --sort-only times the earlier route alone (nothing newer than
hm_stream_view and hm_stream_import is needed, so a checkout of the parent
commit can run it); --parent-json FILE puts that run's times into this one's
result as "parent_sort_ms".

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --visitors --out profiles/stream_visitors.json

--retain H --visitors: distinct visitors on the steady retained log, on the
same cells imported with group = a hash of the cell % 1000 (--top's groups):
the cells with at least 5 visitors in the trailing 24 hours, their points and
visitors and the withheld totals (visitors_device(min_visitors=5); those groups
are a function of the cell, so every cell has one visitor and all of it is
withheld: min_visitors=1, where all of it is emitted, is timed beside it),
against the
route a caller had before it -- view_device(rects, hours, 'each'), one record
per (group, cell), then a device torch.unique(return_inverse, return_counts)
over the keys, a scatter_add of the points, the mask and the gathers -- for
--top's two selections: the whole of zoom 14 and the 4 x 3-tile screen at the
detail zoom.  Both routes are warmed, then take VISITORS_REPS alternating
repetitions; host ms around each, which ends in a synchronise; median and
min-max of each, "not distinguishable" when the ranges overlap, and the two
results compared record by record.  --each-only times the earlier route alone
(nothing newer than hm_stream_view and hm_stream_import is needed, so a
checkout of the parent commit can run it); --parent-json FILE puts that run's
times into this one's result as "parent_each_unique_ms".

    python tools/bench_stream.py --retain 24 --batches 30 --warmup 0 --regions --out profiles/stream_regions.json

--retain H --regions: polygon regions (heatmap_amd.region, hm_stream_region_*)
on the steady retained log, trailing 24 hours: (a) one polygon, the ellipse
inscribed in --top's 4 x 3-tile screen at the detail zoom: its total
(region_totals) and its cells (region_view_device); (b) a choropleth of about
1000 polygons, a jittered 32 x 32 mesh of quadrilaterals over the 256 x 256
zoom-14 cells around the heaviest one: totals and a 24-frame hourly series
(region_series); (c) region_visitors(min_visitors=5) on (b), on --top's
grouped copy of the log.  Each against the route a caller had before:
view_device of the bounding rectangle, every returned cell looked up in a
dense region-id image in torch, scatter_add (24 such calls for the series;
view_device(..., 'each'), torch.unique of (region, group) and scatter_add for
the visitors).  Both routes are warmed, then take REGION_REPS alternating
repetitions, timed and reported as above, and the two results are compared
entry for entry (the cells record for record).  --bbox-only times the earlier
routes alone (nothing newer than hm_stream_view is called; region.py is host
code); --parent-json FILE puts that run's times into this one's result as
"parent_bbox_ms".
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from heatmap_amd import device  # noqa: E402
from heatmap_amd.stream import ALLTIME, StreamingHeatmap  # noqa: E402

BASE = 480000


def _ms(f):
    """host ms of f(), device work included (the calls end in a synchronise
    of their own; one more makes that explicit)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _stats(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1], "n": len(x)} if x else None


def read_rate(s, nbytes, reps=5):
    """GB/s of the library's read-stream kernel (k_read_stream, 16-B loads)
    over nbytes of HBM, best of reps: what a pass that only read the log
    would reach in this session"""
    half = max(1 << 20, nbytes // 2 // 16 * 16)
    a = torch.zeros(half // 8, dtype=torch.int64, device="cuda")
    b = torch.zeros(half // 8, dtype=torch.int64, device="cuda")
    sink = torch.zeros(4096, dtype=torch.int64, device="cuda")
    best = 0.0
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = s.ctx.L.hm_bench_read(s.ctx.ptr, a.data_ptr(), b.data_ptr(), half, sink.data_ptr())
        e1.record()
        e1.synchronize()
        assert rc == 0, rc
        best = max(best, 2.0 * half / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return best


VIEW_REPS = 15


def _screen(key, tiles_rows, tiles_cols):
    """(zoom, row_lo, row_hi, col_lo, col_hi) of tiles_rows x tiles_cols
    heatmap tiles (32 x 32 cells each) around the tile of the cell `key`"""
    z, r, c = key >> 58, (key >> 29) & 0x1FFFFFFF, key & 0x1FFFFFFF
    tr, tc = (r >> 5) - (tiles_rows - 1) // 2, (c >> 5) - (tiles_cols - 1) // 2
    return (z, tr << 5, (tr + tiles_rows) << 5, tc << 5, (tc + tiles_cols) << 5)


def view_bench(s, a, lo, hi):
    """--view (module docstring) on the stream as it stands"""
    import numpy as np

    n, keys, counts, _ = s.window_device(lo, hi)
    k, cnt = keys[:n], counts[:n]
    out = {"hours": [lo, hi], "reps": VIEW_REPS, "log_cells": s.cells()[0], "window_cells": n,
           "timing": "host ms around the call (ends in a synchronise), window and views interleaved"}
    t_win = []
    if a.window_only:
        for _ in range(VIEW_REPS):
            t_win.append(_ms(lambda: s.window_device(lo, hi))[0])
        out["window"] = _stats(t_win)
        return out
    heavy = {}
    for z in (8, 13, 18):
        m = (k >> 58) == z
        heavy[z] = int(k[torch.argmax(torch.where(m, cnt, torch.full_like(cnt, -1)))].item())
    ports = {"a_one_tile_z13": [_screen(heavy[13], 1, 1)],
             "b_screen_4x3_z8_z13_z18": [_screen(heavy[z], 3, 4) for z in (8, 13, 18)]}
    hk, hc = k.cpu().numpy(), cnt.cpu().numpy()
    hz, hr, hcol = hk >> 58, (hk >> 29) & 0x1FFFFFFF, hk & 0x1FFFFFFF
    t_view = {name: [] for name in ports}
    for name, rects in ports.items():
        s.view_device(rects, (lo, hi))          # warm: code object, the capacity memo
    for _ in range(VIEW_REPS):
        t_win.append(_ms(lambda: s.window_device(lo, hi))[0])
        for name, rects in ports.items():
            t_view[name].append(_ms(lambda: s.view_device(rects, (lo, hi)))[0])
    out["window"] = _stats(t_win)
    ok = True
    for name, rects in ports.items():
        nv, vk, vc, _ = s.view_device(rects, (lo, hi))
        m = np.zeros(hk.size, dtype=bool)
        for z, rlo, rhi, clo, chi in rects:
            m |= (hz == z) & (hr >= rlo) & (hr < rhi) & (hcol >= clo) & (hcol < chi)
        gk, gc = vk[:nv].cpu().numpy(), vc[:nv].cpu().numpy()
        og, ow = np.argsort(gk), np.argsort(hk[m])
        same = nv == int(m.sum()) and nv > 0 and np.array_equal(gk[og], hk[m][ow]) and \
            np.array_equal(gc[og], hc[m][ow])
        ok &= bool(same)
        out[name] = {"rects": [list(map(int, q)) for q in rects], "cells_out": nv, "ms": _stats(t_view[name]),
                     "equals_filtered_window": bool(same)}
    out["check"] = "ok" if ok else "FAIL"
    if a.parent_json:
        pj = json.load(open(a.parent_json))
        out["parent_window"] = pj["view"]["window"]
        out["parent_window_note"] = ("this script with --window-only run by a checkout of the parent commit (its "
                                     "library and package) on the same seeded log, in the same session")
        assert pj["view"]["window_cells"] == n and pj["view"]["log_cells"] == out["log_cells"]
    return out


def _ev_ms(f):
    """device ms between two events around f() (the launches' own time, without the host's)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _densify(hk, hc, tiles, b, h):
    """numpy: cells (hm_count keys, counts) added into the haloed grids of tiles"""
    import numpy as np

    w = (1 << b) + 2 * h
    z, r, c = hk >> 58, (hk >> 29) & 0x1FFFFFFF, hk & 0x1FFFFFFF
    grid = np.zeros((len(tiles), w, w), dtype=np.int64)
    for t, (tz, tr, tc) in enumerate(tiles):
        y, x = r - ((tr << b) - h), c - ((tc << b) - h)
        m = (z == tz + b) & (y >= 0) & (y < w) & (x >= 0) & (x < w)
        np.add.at(grid[t], (y[m], x[m]), hc[m])
    return grid


def raster_bench(s, a, lo, hi):
    """--raster (module docstring) on the stream as it stands"""
    import ctypes

    if not a.view_only:     # the views alone need nothing newer than hm_stream_view
        from heatmap_amd import _lib, raster

    n, keys, counts, _ = s.window_device(lo, hi)
    k, cnt = keys[:n], counts[:n]
    out = {"hours": [lo, hi], "reps": VIEW_REPS, "log_cells": s.cells()[0], "window_cells": n,
           "timing": "host ms around the call plus one synchronise (raster_dev_ms: device ms between two events "
                     "around the same call); raster, render and view interleaved"}
    heavy = {}
    for z in (13, 18):
        m = (k >> 58) == z
        heavy[z] = int(k[torch.argmax(torch.where(m, cnt, torch.full_like(cnt, -1)))].item())
    del keys, counts, k, cnt
    r13, c13 = (heavy[13] >> 29) & 0x1FFFFFFF, heavy[13] & 0x1FFFFFFF
    r18, c18 = (heavy[18] >> 29) & 0x1FFFFFFF, heavy[18] & 0x1FFFFFFF
    tr, tc = (r18 >> 8) - 1, (c18 >> 8) - 1
    cases = {"a_one_tile_z13_32x32": ([(8, r13 >> 5, c13 >> 5)], 5, 0, None),
             "b_screen_4x3_tiles_256x256_r2": ([(10, tr + i, tc + j) for i in range(3) for j in range(4)], 8, 2, 2)}
    L, ok = s.ctx.L, True
    for name, (tiles, b, h, radius) in cases.items():
        w, side = (1 << b) + 2 * h, 1 << b
        rects = [(tz + b, (y << b) - h, (y << b) - h + w, (x << b) - h, (x << b) - h + w) for tz, y, x in tiles]
        grid = torch.empty((len(tiles), w, w), dtype=torch.int64, device="cuda")
        rgba = torch.empty((len(tiles), side, side, 4), dtype=torch.uint8, device="cuda")
        used = ctypes.c_uint64(0)
        if not a.view_only:
            ta = raster._tile_array(tiles)
            lut = raster._lut("heat", torch, grid.device)

        def do_raster():
            rc = L.hm_stream_raster(s.ptr, lo, hi, _lib.HM_VIEW_MERGED, ta, len(tiles), b, h, grid.data_ptr())
            assert rc == 0, rc

        def do_render():
            rc = L.hm_raster_render(s.ctx.ptr, grid.data_ptr(), len(tiles), b, h, radius, _lib.HM_SCALE_LOG, 0,
                                    lut.data_ptr(), rgba.data_ptr(), None, ctypes.byref(used))
            assert rc == 0, rc

        t_view, t_ras, t_dev, t_ren = [], [], [], []
        s.view_device(rects, (lo, hi))              # warm: code objects, the capacity memo
        if not a.view_only:
            do_raster()
            if radius is not None:
                do_render()
        for _ in range(VIEW_REPS):
            t_view.append(_ms(lambda: s.view_device(rects, (lo, hi)))[0])
            if a.view_only:
                continue
            t_ras.append(_ms(do_raster)[0])
            t_dev.append(_ev_ms(do_raster))
            if radius is not None:
                t_ren.append(_ms(do_render)[0])
        nv, vk, vc, _ = s.view_device(rects, (lo, hi))
        res = {"tiles": [list(t) for t in tiles], "bins_log2": b, "halo": h, "view_rects": [list(q) for q in rects],
               "view_cells_out": nv, "view_ms": _stats(t_view)}
        if not a.view_only:
            do_raster()
            want = _densify(vk[:nv].cpu().numpy(), vc[:nv].cpu().numpy(), tiles, b, h)
            same = nv > 0 and bool((grid.cpu().numpy() == want).all())
            ok &= same
            res.update({"raster_ms": _stats(t_ras), "raster_dev_ms": _stats(t_dev), "grid_sum": int(grid.sum()),
                        "grid_equals_densified_view": same})
            if radius is not None:
                res.update({"radius": radius, "render_ms": _stats(t_ren), "vmax_used": used.value,
                            "pixels_drawn": int((rgba[..., 3] != 0).sum())})
        out[name] = res
    if not a.view_only:
        out["check"] = "ok" if ok else "FAIL"
    if a.parent_json:
        pj = json.load(open(a.parent_json))["raster"]
        assert pj["window_cells"] == n and pj["log_cells"] == out["log_cells"]
        for name in cases:
            assert pj[name]["view_cells_out"] == out[name]["view_cells_out"]
            out[name]["parent_view_ms"] = pj[name]["view_ms"]
        out["parent_view_note"] = ("this script with --raster --view-only run by a checkout of the parent commit (its "
                                   "library and package) on the same seeded log, in the same session")
    return out


FRAMES = 24


def frames_bench(s, a, hi):
    """--frames (module docstring) on the stream as it stands: the hours [hi - 24, hi)"""
    import ctypes

    from heatmap_amd import _lib, raster

    lo = hi - FRAMES
    n, keys, counts, _ = s.window_device(lo, hi)
    k, cnt = keys[:n], counts[:n]
    heavy = int(k[torch.argmax(torch.where((k >> 58) == 18, cnt, torch.full_like(cnt, -1)))].item())
    del keys, counts, k, cnt
    tr, tc = (((heavy >> 29) & 0x1FFFFFFF) >> 8) - 1, ((heavy & 0x1FFFFFFF) >> 8) - 1
    tiles = [(10, tr + i, tc + j) for i in range(3) for j in range(4)]
    b, h, radius, window = 8, 2, 2, 6
    w, side, nt = (1 << b) + 2 * h, 1 << b, len(tiles)
    L, ta = s.ctx.L, raster._tile_array(tiles)
    out = {"hours": [lo, hi], "frames": FRAMES, "frame_hours": 1, "reps": VIEW_REPS, "log_cells": s.cells()[0],
           "window_cells": n, "tiles": [list(t) for t in tiles], "bins_log2": b, "halo": h,
           "timing": "host ms around the call(s) plus one synchronise; every timed item interleaved in one process"}
    loop_grid = torch.empty((FRAMES, nt, w, w), dtype=torch.int64, device="cuda")

    def do_loop():          # the only way there was: one hm_stream_raster call, one pass over the log, per hour
        for f in range(FRAMES):
            rc = L.hm_stream_raster(s.ptr, lo + f, lo + f + 1, _lib.HM_VIEW_MERGED, ta, nt, b, h,
                                    loop_grid[f].data_ptr())
            assert rc == 0, rc

    def do_pass():          # one raster of the whole window: what one pass over this log costs
        rc = L.hm_stream_raster(s.ptr, lo, hi, _lib.HM_VIEW_MERGED, ta, nt, b, h, loop_grid[0].data_ptr())
        assert rc == 0, rc

    timed = {"loop_ms": do_loop, "one_raster_pass_ms": do_pass}
    if not a.loop_only:
        grid = torch.empty((FRAMES, nt, w, w), dtype=torch.int64, device="cuda")
        acc = torch.empty_like(grid)
        series = torch.empty((FRAMES, nt), dtype=torch.int64, device="cuda")
        rgba = torch.empty((FRAMES, nt, side, side, 4), dtype=torch.uint8, device="cuda")
        lut = raster._lut("heat", torch, grid.device)
        used = ctypes.c_uint64(0)

        def do_frames():
            rc = L.hm_stream_raster_frames(s.ptr, lo, hi, 1, _lib.HM_VIEW_MERGED, ta, nt, b, h, grid.data_ptr())
            assert rc == 0, rc

        def do_series():
            rc = L.hm_stream_raster_frames(s.ptr, lo, hi, 1, _lib.HM_VIEW_MERGED, ta, nt, 0, 0, series.data_ptr())
            assert rc == 0, rc

        def do_acc():
            rc = L.hm_raster_accumulate(s.ctx.ptr, grid.data_ptr(), FRAMES, nt * w * w, window, acc.data_ptr())
            assert rc == 0, rc

        def do_render():    # one render pass: every frame on its own scale (a shared scale is a second such pass)
            for f in range(FRAMES):
                rc = L.hm_raster_render(s.ctx.ptr, grid[f].data_ptr(), nt, b, h, radius, _lib.HM_SCALE_LOG, 0,
                                        lut.data_ptr(), rgba[f].data_ptr(), None, ctypes.byref(used))
                assert rc == 0, rc

        do_frames()         # the accumulate and the render read its grid
        timed.update({"frames_ms": do_frames, "series_ms": do_series, "accumulate_ms": do_acc, "render_ms": do_render})
    for f in timed.values():    # warm: code objects
        f()
    t = {name: [] for name in timed}
    for _ in range(VIEW_REPS):
        for name, f in timed.items():
            t[name].append(_ms(f)[0])
    out.update({name: _stats(x) for name, x in t.items()})
    do_loop()               # do_pass wrote over frame 0
    torch.cuda.synchronize()
    out["grid_sum"] = int(loop_grid.sum())
    if not a.loop_only:
        do_frames()
        do_series()
        do_acc()
        torch.cuda.synchronize()
        same = out["grid_sum"] > 0 and all(bool(torch.equal(grid[f], loop_grid[f])) for f in range(FRAMES))
        # a tile's series is its grid's interior summed: the 256 x 256 bins of zoom 18 are the tile's zoom-10 cell
        same &= bool(torch.equal(series, grid[:, :, h:h + side, h:h + side].sum(dim=(2, 3))))
        csum = torch.cumsum(grid, dim=0)
        csum[window:] -= csum[:-window].clone()
        same &= bool(torch.equal(acc, csum))
        nbytes = 16 * grid.numel()
        out.update({"check": "ok" if same else "FAIL", "frames_equal_the_loops_grids": same,
                    "accumulate_window": window, "accumulate_min_bytes": nbytes,
                    "accumulate_min_bytes_note": "8 B read and 8 B written per element; the kernel reads the leaving "
                                                 "frame again: 8 B more for the frames past the window",
                    "accumulate_GBps_over_min_bytes": nbytes / (out["accumulate_ms"]["median"] * 1e-3) / 1e9,
                    "series_sum": int(series.sum()), "pixels_drawn": int((rgba[..., 3] != 0).sum())})
    if a.parent_json:
        pj = json.load(open(a.parent_json))["frames"]
        assert pj["log_cells"] == out["log_cells"] and pj["grid_sum"] == out["grid_sum"] and pj["tiles"] == out["tiles"]
        out["parent_loop_ms"] = pj["loop_ms"]
        out["parent_one_raster_pass_ms"] = pj["one_raster_pass_ms"]
        out["parent_note"] = ("this script with --frames --loop-only run by a checkout of the parent commit (its "
                              "library and package) on the same seeded log, in the same session")
    return out


SNAP_REPS = 7
READD_REPS = 3


def _sorted_cells(n, keys, counts):
    k, order = torch.sort(keys[:n])
    return k, counts[:n][order]


def readd_bench(a, lat, lon, retained, cap):
    """the restore a user has without snapshots: the retained one-hour batches
    of raw points added again to a fresh stream whose log is sized for them
    (READD_REPS fresh streams; the last one is returned for the check)"""
    pool, n = len(lat), int(a.batch)
    hours = [torch.full((n,), BASE + b, dtype=torch.int32, device="cuda") for b in retained]
    t, s2 = [], None
    for _ in range(READD_REPS):
        if s2 is not None:
            s2.close()
        s2 = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=cap)
        t.append(_ms(lambda: [s2.add(lat[b % pool], lon[b % pool], hour=h) for b, h in zip(retained, hours)])[0])
    return t, s2


def snapshot_bench(s, a, lat, lon, retained):
    """--snapshot (module docstring) on the stream as it stands"""
    import ctypes
    import shutil
    import tempfile

    from heatmap_amd import _lib

    lo, hi = BASE + retained[0], BASE + retained[-1] + 1
    n, cap = s.cells()
    out = {"hours": [lo, hi], "log_cells": n, "log_capacity": cap, "batches_retained": len(retained),
           "timing": "host ms around the call (ends in a synchronise); export and import interleaved"}
    t_readd, s2 = readd_bench(a, lat, lon, retained, cap)
    out["readd_ms"] = _stats(t_readd)
    out["readd_note"] = "%d hm_stream_add calls of %d raw points each into a fresh stream" % (len(retained), int(a.batch))
    wn, wk, wc, _ = s.window_device(lo, hi)
    want = _sorted_cells(wn, wk, wc)
    del wk, wc

    def same_window(x):
        xn, xk, xc, _ = x.window_device(lo, hi)
        if xn != wn:
            return False
        got = _sorted_cells(xn, xk, xc)
        return bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))

    ok = same_window(s2) and s2.cells()[0] == n
    s2.close()
    if a.readd_only:
        out["check"] = "ok" if ok else "FAIL"
        return out
    L = s.ctx.L
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    groups = torch.empty(n, dtype=torch.int32, device="cuda")
    hours = torch.empty(n, dtype=torch.int32, device="cuda")
    m = ctypes.c_int64(0)

    def export():
        rc = L.hm_stream_export(s.ptr, keys.data_ptr(), counts.data_ptr(), groups.data_ptr(), hours.data_ptr(), n,
                                ctypes.byref(m))
        assert rc == 0 and m.value == n, (rc, m.value)

    def imported(x):
        rc = L.hm_stream_import(x.ptr, keys.data_ptr(), counts.data_ptr(), groups.data_ptr(), hours.data_ptr(), n,
                                _lib.HM_IMPORT_DISTINCT)
        assert rc == 0, rc

    t_exp, t_imp, s3 = [], [], None
    for rep in range(SNAP_REPS + 1):        # the first pair warms up and is dropped
        if s3 is not None:
            s3.close()
        s3 = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=cap)
        t_exp.append(_ms(export)[0])
        t_imp.append(_ms(lambda: imported(s3))[0])
        print("snapshot rep %d: export %.2f ms, import %.2f ms" % (rep, t_exp[-1], t_imp[-1]), file=sys.stderr, flush=True)
    out["export_ms"], out["import_ms"] = _stats(t_exp[1:]), _stats(t_imp[1:])
    out["export_GBps"] = 40.0 * n / (out["export_ms"]["median"] * 1e-3) / 1e9
    out["import_GBps"] = 40.0 * n / (out["import_ms"]["median"] * 1e-3) / 1e9
    out["bytes"] = ("export: 16 B per log cell read + 24 B written (key, count, group, hour); import: the same 24 B "
                    "read + 16 B written at the log's tail")
    ok = ok and same_window(s3) and s3.cells()[0] == n
    s3.close()
    del keys, counts, groups, hours
    tmp = tempfile.mkdtemp(prefix="hm_snapshot_")
    try:
        path = os.path.join(tmp, "stream.npz")
        out["save_ms"] = _ms(lambda: s.save(path))[0]
        out["file_bytes"] = os.path.getsize(path)
        print("snapshot saved: %.0f ms, %d bytes" % (out["save_ms"], out["file_bytes"]), file=sys.stderr, flush=True)
        out["load_ms"], s4 = _ms(lambda: StreamingHeatmap.load(path, initial_cells=cap))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    ok = ok and same_window(s4) and s4.cells()[0] == n
    s4.close()
    out["check"] = "ok" if ok else "FAIL"
    if a.parent_json:
        pj = json.load(open(a.parent_json))["snapshot"]
        assert pj["log_cells"] == n and pj["check"] == "ok" and pj["hours"] == [lo, hi]
        out["parent_readd_ms"] = pj["readd_ms"]
        out["parent_readd_note"] = ("this script with --readd-only run by a checkout of the parent commit (its library "
                                    "and package) on the same seeded batches, in the same session")
    return out


FORGET_REPS = 7     # after 2 warm-up repetitions


def forget_bench(s, a, lo, hi):
    """--forget / --expire-only (module docstring) on the log of the stream as it stands"""
    import ctypes

    from heatmap_amd import _lib

    L = s.ctx.L
    n, cap = s.cells()
    n0, keys, counts, groups, hours = s.export_device()
    assert n0 == n
    keys, counts, groups, hours = keys[:n], counts[:n], groups[:n], hours[:n]
    cut, mid = lo + (hi - lo) // 2, lo + (hi - lo) // 2
    h64 = hours.to(torch.int64) & 0xFFFFFFFF
    below, at_mid = int((h64 < cut).sum()), int((h64 == mid).sum())
    g1000 = ((keys ^ (keys >> 23)) * 2654435761 % 1000).to(torch.int32)     # a hash of the cell
    ten = list(range(7, 1000, 100))
    in_ten = int(torch.isin(g1000, torch.tensor(ten, dtype=torch.int32, device="cuda")).sum())
    out = {"hours": [lo, hi], "log_cells": n, "log_capacity": cap, "cut": cut, "cells_below_cut": below,
           "one_hour": mid, "cells_of_one_hour": at_mid, "cells_of_10_of_1000_groups": in_ten,
           "repetitions": "%d after 2 warm-up ones; the calls take turns within a repetition" % FORGET_REPS,
           "timing": "host ms around the call, which ends in its own wait; each call on a fresh stream that imported "
                     "the exported log (untimed)"}
    a64, b64, m64 = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    ok = []

    def fresh(grp):
        x = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=cap)
        rc = L.hm_stream_import(x.ptr, keys.data_ptr(), counts.data_ptr(), grp.data_ptr(), hours.data_ptr(), n,
                                _lib.HM_IMPORT_DISTINCT)
        assert rc == 0, rc
        # a stream in service has its alternate log arrays and table: a fresh one makes them in its first expire
        # or forget (mapping a few GB took 0.3 - 1.7 s now and then), so one that drops nothing runs here, untimed
        assert L.hm_stream_expire(x.ptr, BASE + 1, ctypes.byref(a64), ctypes.byref(b64)) == 0 and a64.value == 0
        return x

    def expire(x):
        assert L.hm_stream_expire(x.ptr, cut, ctypes.byref(a64), ctypes.byref(b64)) == 0
        ok.append(a64.value == below)

    def forget(x, ids, h_lo, h_hi, want):
        arr = (ctypes.c_uint32 * len(ids))(*ids) if ids else None
        assert L.hm_stream_forget(x.ptr, arr, len(ids), h_lo, h_hi, ctypes.byref(a64), ctypes.byref(b64)) == 0
        ok.append(a64.value == want)

    ko, co, go, ho = (torch.empty(n, dtype=t, device="cuda") for t in (torch.int64,) * 2 + (torch.int32,) * 2)

    def export_full(x):
        rc = L.hm_stream_export(x.ptr, ko.data_ptr(), co.data_ptr(), go.data_ptr(), ho.data_ptr(), n, ctypes.byref(m64))
        assert rc == 0 and m64.value == n, (rc, m64.value)

    def export_select(x):
        rc = L.hm_stream_export_select(x.ptr, None, 0, mid, mid + 1, ko.data_ptr(), co.data_ptr(), go.data_ptr(),
                                       ho.data_ptr(), n, ctypes.byref(m64))
        ok.append(rc == 0 and m64.value == at_mid)

    def rebuild(x, gone):
        """the path there was before: the whole export, a mask in torch, an import into a fresh stream"""
        export_full(x)
        m = ~gone(go, ho)
        k, c, g, h = ko[m], co[m], go[m], ho[m]
        y = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=cap)
        rc = L.hm_stream_import(y.ptr, k.data_ptr(), c.data_ptr(), g.data_ptr(), h.data_ptr(), k.numel(),
                                _lib.HM_IMPORT_DISTINCT)
        assert rc == 0, rc
        rebuilt.append((y, k.numel()))

    rebuilt = []
    tens = torch.tensor(ten, dtype=torch.int32, device="cuda")
    calls = [("expire_ms", groups, expire)]
    if not a.expire_only:
        calls += [
            ("forget_same_cut_ms", groups, lambda x: forget(x, [], BASE, cut, below)),
            ("forget_one_hour_ms", groups, lambda x: forget(x, [], mid, mid + 1, at_mid)),
            ("rebuild_without_one_hour_ms", groups, lambda x: rebuild(x, lambda g, h: h == mid)),
            ("export_select_one_hour_ms", groups, export_select),
            ("export_full_ms", groups, export_full),
            ("forget_10_of_1000_groups_ms", g1000, lambda x: forget(x, ten, -1, -1, in_ten)),
            ("rebuild_without_10_of_1000_groups_ms", g1000, lambda x: rebuild(x, lambda g, h: torch.isin(g, tens))),
        ]
    t = {name: [] for name, _, _ in calls}
    for rep in range(FORGET_REPS + 2):
        for name, grp, call in calls:
            x = fresh(grp)
            t[name].append(_ms(lambda: call(x))[0])
            x.close()
            while rebuilt:
                y, left = rebuilt.pop()
                ok.append(y.cells()[0] == left)
                y.close()
        print("forget rep %d: %s" % (rep, ", ".join("%s %.2f" % (k, v[-1]) for k, v in t.items())), file=sys.stderr,
              flush=True)
    for name in t:
        out[name] = _stats(t[name][2:])
        out[name]["all"] = t[name][2:]
    out["check"] = "ok" if all(ok) else "FAIL"
    out["bytes"] = ("expire and forget of the cut: 16 B per log cell read + 16 B per survivor written; export: 16 B "
                    "read + 24 B written per record")
    if a.parent_json:
        pj = json.load(open(a.parent_json))["forget"]
        assert pj["log_cells"] == n and pj["check"] == "ok" and pj["cut"] == cut
        out["parent_expire_ms"] = pj["expire_ms"]
        out["parent_note"] = ("this script with --forget --expire-only run by a checkout of the parent commit (its "
                              "library and package) on the same seeded log, in the same session")
    return out


TOP_REPS = 25


def _two_key_top(keys, counts, k):
    """the first k of (keys, counts) by count descending, then key ascending: two stable device sorts"""
    ks, i = torch.sort(keys, stable=True)
    cs, j = torch.sort(counts[i], descending=True, stable=True)
    return ks[j][:k], cs[:k]


def _hot_screen(s, a, h24):
    """the 4 x 3 tiles of 256 x 256 detail-zoom cells around the heaviest cell of the hours h24"""
    n, keys, counts, _ = s.window_device(*h24)
    k18 = keys[:n][(keys[:n] >> 58) == a.zmax]
    c18 = counts[:n][(keys[:n] >> 58) == a.zmax]
    heavy = int(k18[torch.argmax(c18)].item())
    r, c = (heavy >> 29) & 0x1FFFFFFF, heavy & 0x1FFFFFFF
    tr, tc = (r >> 8) - 1, (c >> 8) - 1
    return [(a.zmax, (tr + i) << 8, (tr + i + 1) << 8, (tc + j) << 8, (tc + j + 1) << 8)
            for i in range(3) for j in range(4)]


def _grouped_copy(s, a):
    """the log's cells under group = a hash of the cell % 1000, in a stream of their own"""
    ne, ek, ec, eg, eh = s.export_device()
    g1000 = ((ek[:ne] ^ (ek[:ne] >> 23)) * 2654435761 % 1000).to(torch.int32)
    g = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=max(1024, ne))
    rc = s.ctx.L.hm_stream_import(g.ptr, ek.data_ptr(), ec.data_ptr(), g1000.data_ptr(), eh.data_ptr(), ne, 1)
    assert rc == 0, rc
    return g


def top_bench(s, a, lo, hi):
    """--top / --sort-only (module docstring) on the stream as it stands"""
    import ctypes

    L = s.ctx.L
    h24 = (max(lo, hi - 24), hi)
    screen = _hot_screen(s, a, h24)
    zw = min(14, a.zmax)
    out = {"hours": list(h24), "reps": TOP_REPS, "log_cells": s.cells()[0],
           "timing": "host ms around the route plus one synchronise; both routes warmed, then alternating"}
    g = _grouped_copy(s, a)

    def sort_cells(rects, k):
        nv, vk, vc, _ = s.view_device(rects, h24)
        return (nv, *_two_key_top(vk[:nv], vc[:nv], k))

    def sort_groups(rects, k):
        nv, vk, vc, vg = g.view_device(rects, h24, "each")
        ids, inv = torch.unique(vg[:nv], return_inverse=True)
        tot = torch.zeros(ids.numel(), dtype=torch.int64, device="cuda").scatter_add_(0, inv, vc[:nv])
        return (ids.numel(), *_two_key_top(ids.to(torch.int64) & 0xFFFFFFFF, tot, k))

    gi = torch.empty(16, dtype=torch.int32, device="cuda")
    gc = torch.empty(16, dtype=torch.int64, device="cuda")
    n64, t64 = ctypes.c_int64(0), ctypes.c_int64(0)

    def top_groups(rects, k):
        ra = (ctypes.c_int64 * (5 * len(rects)))(*[v for q in rects for v in q])
        rc = L.hm_stream_top_groups(g.ptr, h24[0], h24[1], ra, len(rects), k, gi.data_ptr(), gc.data_ptr(),
                                    ctypes.byref(n64), ctypes.byref(t64))
        assert rc == 0, rc
        return t64.value, gi[:n64.value].to(torch.int64) & 0xFFFFFFFF, gc[:n64.value]

    def top_cells(rects, k):
        nt, tk, tcnt, total = s.top_device(k, rects, h24)
        return total, tk, tcnt

    cases = [("a_whole_z%d_top100" % zw, [(zw, 0, 1 << zw, 0, 1 << zw)], 100, sort_cells, top_cells),
             ("b_screen_4x3_tiles_z%d_top100" % a.zmax, screen, 100, sort_cells, top_cells),
             ("c_screen_4x3_tiles_top_groups10", screen, 10, sort_groups, top_groups)]
    ok = True
    for name, rects, k, old, new in cases:
        routes = [("sort_ms", old)] + ([] if a.sort_only else [("top_ms", new)])
        t = {key: [] for key, _ in routes}
        last = {}
        for key, f in routes:
            f(rects, k)                       # warm: code objects, the capacity memo, the scratch
            f(rects, k)
        for _ in range(TOP_REPS):
            for key, f in routes:
                ms, last[key] = _ms(lambda: f(rects, k))
                t[key].append(ms)
        res = {"rects": [list(map(int, q)) for q in rects], "k": k, "selected": int(last["sort_ms"][0])}
        for key in t:
            res[key] = _stats(t[key])
        if not a.sort_only:
            same = all(torch.equal(x, y) for x, y in zip(last["sort_ms"][1:], last["top_ms"][1:])) and \
                last["sort_ms"][0] == last["top_ms"][0] and last["top_ms"][1].numel() == min(k, last["top_ms"][0])
            ok &= bool(same)
            res["top_equals_sorted_view"] = bool(same)
            o, w = res["sort_ms"], res["top_ms"]
            res["verdict"] = ("not distinguishable" if w["min"] <= o["max"] and o["min"] <= w["max"] else
                              "top faster" if w["median"] < o["median"] else "top slower")
            if new is top_cells:
                # the selection by itself against the sort by itself, on the view's cells (filter and merge left out)
                nv, vk, vc, _ = s.view_device(rects, h24)
                vk, vc = vk[:nv].clone(), vc[:nv].clone()
                ko, co = torch.empty(k, dtype=torch.int64, device="cuda"), torch.empty(k, dtype=torch.int64, device="cuda")

                def select_alone():
                    rc = L.hm_cells_top(s.ctx.ptr, vk.data_ptr(), vc.data_ptr(), nv, k, ko.data_ptr(), co.data_ptr(),
                                        ctypes.byref(n64))
                    assert rc == 0, rc

                ta = {"select_alone_ms": [], "sort_alone_ms": []}
                for rep in range(TOP_REPS + 2):
                    ta["select_alone_ms"].append(_ms(select_alone)[0])
                    ta["sort_alone_ms"].append(_ms(lambda: _two_key_top(vk, vc, k))[0])
                sk, sc = _two_key_top(vk, vc, k)
                ok &= bool(torch.equal(sk, ko) and torch.equal(sc, co))
                for key in ta:
                    res[key] = _stats(ta[key][2:])
        out[name] = res
    g.close()
    if not a.sort_only:
        out["check"] = "ok" if ok else "FAIL"
    if a.parent_json:
        pj = json.load(open(a.parent_json))["top"]
        assert pj["log_cells"] == out["log_cells"] and pj["hours"] == out["hours"]
        for name, *_ in cases:
            assert pj[name]["selected"] == out[name]["selected"]
            out[name]["parent_sort_ms"] = pj[name]["sort_ms"]
            o, w = pj[name]["sort_ms"], out[name]["top_ms"]
            out[name]["verdict_vs_parent"] = ("not distinguishable" if w["min"] <= o["max"] and o["min"] <= w["max"]
                                              else "top faster" if w["median"] < o["median"] else "top slower")
        out["parent_sort_note"] = ("this script with --top --sort-only run by a checkout of the parent commit (its "
                                   "library and package) on the same seeded log, in the same session")
    return out


VISITORS_REPS = 25
VISITORS_MIN = (5, 1)     # the k-anonymity threshold measured, and 1: every cell emitted


def visitors_bench(s, a, lo, hi):
    """--visitors / --each-only (module docstring) on the stream as it stands"""
    h24 = (max(lo, hi - 24), hi)
    screen = _hot_screen(s, a, h24)
    zw = min(14, a.zmax)
    out = {"hours": list(h24), "reps": VISITORS_REPS, "log_cells": s.cells()[0],
           "groups": "1000, group = a hash of the cell: every cell belongs to one group, so min_visitors = 5 "
                     "withholds all of it and min_visitors = 1 emits all of it",
           "timing": "host ms around the route plus one synchronise; both routes warmed, then alternating"}
    g = _grouped_copy(s, a)

    def each_route(rects, m):
        """the route before hm_stream_visitors: one record per (group, cell), then unique, mask and gathers"""
        nv, vk, vc, _ = g.view_device(rects, h24, "each")
        cells, inv, vis = torch.unique(vk[:nv], return_inverse=True, return_counts=True)
        pts = torch.zeros(cells.numel(), dtype=torch.int64, device="cuda").scatter_add_(0, inv, vc[:nv])
        keep = vis >= m
        return nv, cells[keep], pts[keep], vis[keep], int((~keep).sum().item()), int(pts[~keep].sum().item())

    def visitors_route(rects, m):
        n, vk, vp, vv, wc, wp = g.visitors_device(rects, h24, m)
        return n, vk[:n], vp[:n], vv[:n].to(torch.int64) & 0xFFFFFFFF, wc, wp

    cases = [("%s_min%d" % (name, m), rects, m)
             for name, rects in (("a_whole_z%d" % zw, [(zw, 0, 1 << zw, 0, 1 << zw)]),
                                 ("b_screen_4x3_tiles_z%d" % a.zmax, screen)) for m in VISITORS_MIN]
    ok = True
    for name, rects, m in cases:
        routes = [("each_unique_ms", each_route)] + ([] if a.each_only else [("visitors_ms", visitors_route)])
        t = {key: [] for key, _ in routes}
        last = {}
        for key, f in routes:
            f(rects, m)                       # warm: code objects, the capacity memo, the scratch, the labels
            f(rects, m)
        for _ in range(VISITORS_REPS):
            for key, f in routes:
                ms, last[key] = _ms(lambda: f(rects, m))
                t[key].append(ms)
        e = last["each_unique_ms"]
        res = {"rects": [list(map(int, q)) for q in rects], "min_visitors": m, "group_cell_records": int(e[0]),
               "emitted": int(e[1].numel()), "withheld_cells": e[4], "withheld_points": e[5]}
        for key in t:
            res[key] = _stats(t[key])
        if not a.each_only:
            v = last["visitors_ms"]
            order = torch.argsort(v[1])       # the call's order is unspecified; unique's is by key
            same = v[0] == e[1].numel() and v[4:] == e[4:] and \
                all(torch.equal(x[order], y) for x, y in zip(v[1:4], e[1:4]))
            ok &= bool(same)
            res["visitors_equals_each_route"] = bool(same)
            o, w = res["each_unique_ms"], res["visitors_ms"]
            res["verdict"] = ("not distinguishable" if w["min"] <= o["max"] and o["min"] <= w["max"] else
                              "visitors faster" if w["median"] < o["median"] else "visitors slower")
        out[name] = res
    g.close()
    if not a.each_only:
        out["check"] = "ok" if ok else "FAIL"
    if a.parent_json:
        pj = json.load(open(a.parent_json))["visitors"]
        assert pj["log_cells"] == out["log_cells"] and pj["hours"] == out["hours"]
        for name, *_ in cases:
            assert pj[name]["emitted"] == out[name]["emitted"]
            out[name]["parent_each_unique_ms"] = pj[name]["each_unique_ms"]
            o, w = pj[name]["each_unique_ms"], out[name]["visitors_ms"]
            out[name]["verdict_vs_parent"] = ("not distinguishable" if w["min"] <= o["max"] and o["min"] <= w["max"]
                                              else "visitors faster" if w["median"] < o["median"] else
                                              "visitors slower")
        out["parent_note"] = ("this script with --visitors --each-only run by a checkout of the parent commit (its "
                              "library and package) on the same seeded log, in the same session")
    return out


REGION_REPS = 25


def _region_image(rs):
    """(bounding rectangle, int32 CUDA image of it: region + 1 per cell, 0 outside) of a RegionSet whose
    regions do not overlap: what the bounding-box route looks cells up in"""
    import numpy as np

    box = rs.bounding_rect()
    w = box[4] - box[3]
    d = np.zeros((rs.nrows, w + 1), dtype=np.int64)
    rows = rs.rows() - rs.row_lo
    np.add.at(d, (rows, rs.col_lo.astype(np.int64) - box[3]), rs.region.astype(np.int64) + 1)
    np.add.at(d, (rows, rs.col_hi.astype(np.int64) - box[3]), -(rs.region.astype(np.int64) + 1))
    return box, torch.from_numpy(np.cumsum(d, axis=1)[:, :w].astype(np.int32)).cuda()


def _choropleth(s, a, h24, zb):
    """about 1000 polygons tiling the 256 x 256 zoom-zb cells around the heaviest zoom-zb cell of the hours:
    a 32 x 32 mesh of quadrilaterals with jittered inner corners, rasterised (RegionSet.from_tile_polygons)
    and made disjoint through the region image, so the bounding-box route can hold it"""
    import numpy as np

    from heatmap_amd.region import RegionSet

    n, keys, counts, _ = s.window_device(*h24)
    kb, cb = keys[:n][(keys[:n] >> 58) == zb], counts[:n][(keys[:n] >> 58) == zb]
    heavy = int(kb[torch.argmax(cb)].item())
    side = 1 << zb
    r0 = min(max(((heavy >> 29) & 0x1FFFFFFF) - 128, 0), max(side - 256, 0))
    c0 = min(max((heavy & 0x1FFFFFFF) - 128, 0), max(side - 256, 0))
    rng = np.random.default_rng(14)
    gy, gx = np.meshgrid(np.arange(33) * 8.0, np.arange(33) * 8.0, indexing="ij")
    jit = rng.uniform(-2.5, 2.5, (2, 33, 33))
    jit[:, [0, -1], :] = 0
    jit[:, :, [0, -1]] = 0
    px, py = c0 + gx + jit[0], r0 + gy + jit[1]
    polys = [[np.array([[px[i, j], py[i, j]], [px[i, j + 1], py[i, j + 1]], [px[i + 1, j + 1], py[i + 1, j + 1]],
                        [px[i + 1, j], py[i + 1, j]]])] for i in range(32) for j in range(32)]
    rs = RegionSet.from_tile_polygons(polys, zb)
    img = np.zeros((min(256, side), min(256, side)), dtype=np.int64)
    for j in range(rs.nregions):                  # a cell two quadrilaterals claim (rounding on a shared edge) stays one's
        r, c = rs.cells(j)
        img[r - r0, c - c0] = j + 1
    return RegionSet.from_mask(zb, r0, c0, img)


def _region_checksum(b):
    """one number of a route's result, to tell that two runs answered the same question"""
    if torch.is_tensor(b):
        return int(b.sum().item())
    if torch.is_tensor(b[1]):
        return int(b[1].sum().item())
    return int(b[0].sum() + b[1].sum())


def regions_bench(s, a, lo, hi):
    """--regions / --bbox-only (module docstring) on the stream as it stands"""
    import numpy as np

    from heatmap_amd.region import RegionSet

    h24 = (max(lo, hi - 24), hi)
    screen = _hot_screen(s, a, h24)
    r0, r1 = min(q[1] for q in screen), max(q[2] for q in screen)
    c0, c1 = min(q[3] for q in screen), max(q[4] for q in screen)
    t = np.linspace(0.0, 2.0 * np.pi, 256, endpoint=False)
    ring = np.stack([(c0 + c1) / 2 + (c1 - c0) / 2 * np.cos(t), (r0 + r1) / 2 + (r1 - r0) / 2 * np.sin(t)], axis=1)
    ell = RegionSet.from_tile_polygons([[ring]], a.zmax)
    zb = min(14, a.zmax)
    cho = _choropleth(s, a, h24, zb)
    g = _grouped_copy(s, a)
    out = {"hours": list(h24), "reps": REGION_REPS, "log_cells": s.cells()[0],
           "timing": "host ms around the route plus one synchronise; both routes warmed, then alternating",
           "bbox_route": "view_device of the bounding rectangle, a lookup of every returned cell in a dense "
                         "region-id image in torch, scatter_add (24 such calls for the series; "
                         "view_device(..., 'each'), torch.unique of (region, group) and scatter_add for visitors)",
           "groups": "visitors: 1000 groups, group = a hash of the cell (the --visitors copy of the log)"}

    def lookup(img, box, k):
        return img[((k >> 29) & 0x1FFFFFFF) - box[1], (k & 0x1FFFFFFF) - box[3]].to(torch.int64)

    def bbox_totals(rs, img, box, hours=h24):
        nv, vk, vc, _ = s.view_device([box], hours)
        tot = torch.zeros(rs.nregions + 1, dtype=torch.int64, device="cuda")
        return tot.scatter_add_(0, lookup(img, box, vk[:nv]), vc[:nv])[1:]

    def bbox_cells(rs, img, box):
        nv, vk, vc, _ = s.view_device([box], h24)
        m = lookup(img, box, vk[:nv]) > 0
        return vk[:nv][m], vc[:nv][m]

    def bbox_series(rs, img, box):
        return torch.stack([bbox_totals(rs, img, box, (h, h + 1)) for h in range(*h24)])

    def bbox_visitors(rs, img, box):
        nv, vk, vc, vg = g.view_device([box], h24, "each")
        reg = lookup(img, box, vk[:nv])
        m = reg > 0
        pairs = torch.unique(((reg[m] - 1) << 32) | (vg[:nv][m].to(torch.int64) & 0xFFFFFFFF))
        vis = torch.bincount(pairs >> 32, minlength=rs.nregions)
        pts = torch.zeros(rs.nregions + 1, dtype=torch.int64, device="cuda").scatter_add_(0, reg, vc[:nv])[1:]
        low = (vis >= 1) & (vis < 5)
        wr, wp = int(low.sum().item()), int(pts[low].sum().item())
        return torch.where(vis < 5, 0, pts).cpu().numpy(), torch.where(vis < 5, 0, vis).cpu().numpy(), wr, wp

    def region_cells(rs, img, box):
        n, k, c, _ = s.region_view_device(rs, h24)
        return k[:n], c[:n]

    def same_cells(x, y):
        ox, oy = torch.argsort(x[0]), torch.argsort(y[0])
        return torch.equal(x[0][ox], y[0][oy]) and torch.equal(x[1][ox], y[1][oy])

    def same_visitors(x, y):
        return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:]

    cases = [("a_ellipse_z%d_totals" % a.zmax, ell, bbox_totals, lambda rs, i, b: s.region_totals(rs, h24), torch.equal),
             ("a_ellipse_z%d_cells" % a.zmax, ell, bbox_cells, region_cells, same_cells),
             ("b_choropleth_z%d_totals" % zb, cho, bbox_totals, lambda rs, i, b: s.region_totals(rs, h24), torch.equal),
             ("b_choropleth_z%d_series24" % zb, cho, bbox_series, lambda rs, i, b: s.region_series(rs, h24, 1),
              torch.equal),
             ("c_choropleth_z%d_visitors_min5" % zb, cho, bbox_visitors,
              lambda rs, i, b: g.region_visitors(rs, h24, 5), same_visitors)]
    images = {id(rs): _region_image(rs) for rs in (ell, cho)}
    ok = True
    for name, rs, old, new, same in cases:
        box, img = images[id(rs)]
        routes = [("bbox_ms", old)] + ([] if a.bbox_only else [("region_ms", new)])
        t = {key: [] for key, _ in routes}
        last = {}
        for key, f in routes:
            f(rs, img, box)                   # warm: code objects, the capacity memo, the scratch
            f(rs, img, box)
        for _ in range(REGION_REPS):
            for key, f in routes:
                ms, last[key] = _ms(lambda: f(rs, img, box))
                t[key].append(ms)
        res = {"regions": rs.nregions, "spans": rs.nspans, "rows": rs.nrows, "region_cells": int(rs.area().sum()),
               "bounding_rect": [int(v) for v in box]}
        res["checksum"] = _region_checksum(last["bbox_ms"])
        for key in t:
            res[key] = _stats(t[key])
        if not a.bbox_only:
            eq = bool(same(last["bbox_ms"], last["region_ms"]))
            ok &= eq
            res["region_equals_bbox_route"] = eq
            o, w = res["bbox_ms"], res["region_ms"]
            res["verdict"] = ("not distinguishable" if w["min"] <= o["max"] and o["min"] <= w["max"] else
                              "region faster" if w["median"] < o["median"] else "region slower")
        out[name] = res
    g.close()
    if not a.bbox_only:
        out["check"] = "ok" if ok else "FAIL"
    if a.parent_json:
        pj = json.load(open(a.parent_json))["regions"]
        assert pj["log_cells"] == out["log_cells"] and pj["hours"] == out["hours"]
        for name, *_ in cases:
            assert pj[name]["checksum"] == out[name]["checksum"]
            out[name]["parent_bbox_ms"] = pj[name]["bbox_ms"]
            o, w = pj[name]["bbox_ms"], out[name]["region_ms"]
            out[name]["verdict_vs_parent"] = ("not distinguishable" if w["min"] <= o["max"] and o["min"] <= w["max"]
                                              else "region faster" if w["median"] < o["median"] else "region slower")
        out["parent_note"] = ("this script with --regions --bbox-only run by a checkout of the parent commit (its "
                              "library and package, this commit's heatmap_amd/region.py beside it) on the same seeded "
                              "log, in the same session")
    return out


def retain(a):
    """--retain H: a stream under retention (module docstring)"""
    n, H = int(a.batch), a.retain
    total = a.warmup + a.batches
    pool = min(total, 8)          # the input batches, reused in turn: the stream's size is what is measured
    lat = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(pool)]
    lon = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(pool)]
    for b in range(pool):
        device.synth(a.kind, lat[b], lon[b], seed=0, start=b * n)
    s = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=int(a.initial_cells))
    t_add, t_exp, t_win, gbps, series = [], [], [], [], []
    for b in range(total):
        hour = torch.full((n,), BASE + b, dtype=torch.int32, device="cuda")
        ms_add, _ = _ms(lambda: s.add(lat[b % pool], lon[b % pool], hour=hour))
        llen = s.cells()[0]
        ms_exp, (dropped, freed) = _ms(lambda: s.expire(BASE + b - H))
        ms_win, w = _ms(lambda: s.window_device(BASE + b - H, BASE + b + 1))
        cells, cap = s.cells()
        series.append({"batch": b, "cells": cells, "log_capacity": cap, "buckets": s.buckets(), "dropped": dropped,
                       "buckets_freed": freed, "window_cells": w[0], "ms_add": ms_add, "ms_expire": ms_exp,
                       "ms_window": ms_win})
        if b >= a.warmup:
            t_add.append(ms_add)
            t_win.append(ms_win)
            if dropped:
                t_exp.append(ms_exp)
                gbps.append(16.0 * (2 * llen - dropped) / (ms_exp * 1e-3) / 1e9)
    steady = [x for x in series if x["batch"] > H]
    view = view_bench(s, a, BASE + total - 1 - H, BASE + total) if a.view else None
    snap = snapshot_bench(s, a, lat, lon, list(range(total - 1 - H, total))) if a.snapshot or a.readd_only else None
    ras = raster_bench(s, a, BASE + total - 1 - H, BASE + total) if a.raster else None
    fra = frames_bench(s, a, BASE + total) if a.frames else None
    fgt = forget_bench(s, a, BASE + total - 1 - H, BASE + total) if a.forget or a.expire_only else None
    top = top_bench(s, a, BASE + total - 1 - H, BASE + total) if a.top or a.sort_only else None
    vis = visitors_bench(s, a, BASE + total - 1 - H, BASE + total) if a.visitors or a.each_only else None
    reg = regions_bench(s, a, BASE + total - 1 - H, BASE + total) if a.regions or a.bbox_only else None
    result = json.dumps({
        "metric": "stream under retention: expire(newest - H) and window(newest - H, newest + 1) per one-hour batch",
        "retain_hours": H, "batch_points": n, "batches": a.batches, "warmup": a.warmup, "zooms": [a.zmin, a.zmax],
        "kind": a.kind, "ms_add": _stats(t_add), "ms_expire": _stats(t_exp), "ms_window": _stats(t_win),
        "expire_GBps": _stats(gbps),
        "expire_bytes": "16 B per log cell read + 16 B per surviving cell written; host time of the call "
                        "(the pass, the table listing, one synchronise)",
        "read_stream_GBps": read_rate(s, 16 * max(x["cells"] for x in series)),
        "flat_after_H": {"log_capacity": sorted({x["log_capacity"] for x in steady}),
                         "buckets": sorted({x["buckets"] for x in steady}),
                         "cells_min_max": [min(x["cells"] for x in steady), max(x["cells"] for x in steady)]}
        if steady else None,
        "view": view,
        "snapshot": snap,
        "raster": ras,
        "frames": fra,
        "forget": fgt,
        "top": top,
        "visitors": vis,
        "regions": reg,
        "series": series,
        "data": "synthetic (heatmap_amd.synth, generated on device, resident in HBM)"})
    print(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(result + "\n")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=float, default=1e7)
    ap.add_argument("--batches", type=int, default=18)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hours", type=int, default=1, help="distinct hours per batch")
    ap.add_argument("--zmin", type=int, default=0)
    ap.add_argument("--zmax", type=int, default=18)
    ap.add_argument("--kind", default="hotspots")
    ap.add_argument("--initial-cells", type=float, default=float(1 << 26),
                    help="the resident log's first capacity (it doubles when full)")
    ap.add_argument("--retain", type=int, default=0, metavar="H",
                    help="retention mode: one-hour batches, expire(newest - H) and one window query after each")
    ap.add_argument("--view", action="store_true",
                    help="with --retain: window vs viewport queries on the steady log (module docstring)")
    ap.add_argument("--window-only", action="store_true", help="with --view: time the window alone")
    ap.add_argument("--snapshot", action="store_true",
                    help="with --retain: export, import and save/load of the steady log (module docstring)")
    ap.add_argument("--raster", action="store_true",
                    help="with --retain: tile rasters and rendered tiles vs views of the same rectangles (module "
                         "docstring)")
    ap.add_argument("--view-only", action="store_true", help="with --raster: time the views alone")
    ap.add_argument("--frames", action="store_true",
                    help="with --retain 24 or more: 24 hourly frames of a screen in one call vs one raster call per "
                         "hour (module docstring)")
    ap.add_argument("--loop-only", action="store_true", help="with --frames: time the per-hour raster calls alone")
    ap.add_argument("--forget", action="store_true",
                    help="with --retain: forget and selective export on the steady log against expire, the full "
                         "export and export + mask + import (module docstring)")
    ap.add_argument("--expire-only", action="store_true", help="with --retain: --forget's expire alone")
    ap.add_argument("--top", action="store_true",
                    help="with --retain 24 or more: the 100 hottest cells and the 10 most active groups against a view "
                         "and a device sort (module docstring)")
    ap.add_argument("--sort-only", action="store_true", help="with --retain: --top's view-and-sort routes alone")
    ap.add_argument("--visitors", action="store_true",
                    help="with --retain 24 or more: the cells with at least 5 distinct visitors (hm_stream_visitors) "
                         "against a per-group view, a device unique and a mask (module docstring)")
    ap.add_argument("--each-only", action="store_true", help="with --retain: --visitors' view-and-unique route alone")
    ap.add_argument("--regions", action="store_true",
                    help="with --retain 24 or more: totals, cells, a 24-hour series and visitors of polygon regions "
                         "(hm_stream_region_*) against a view of the bounding rectangle and a lookup in a region-id "
                         "image (module docstring)")
    ap.add_argument("--bbox-only", action="store_true", help="with --retain: --regions' bounding-box routes alone")
    ap.add_argument("--readd-only", action="store_true",
                    help="with --retain: time only the re-adding of the retained batches to a fresh stream")
    ap.add_argument("--parent-json", default=None, metavar="FILE",
                    help="with --view: a --window-only result of the parent commit, kept as parent_window; with "
                         "--snapshot: its --readd-only result, kept as parent_readd_ms; with --raster: its "
                         "--view-only result, kept as parent_view_ms; with --frames: its --loop-only result, kept as "
                         "parent_loop_ms; with --forget: its --expire-only result, kept as parent_expire_ms; with "
                         "--top: its --sort-only result, kept as parent_sort_ms; with --visitors: its --each-only result, kept as "
                         "parent_each_unique_ms; with --regions: its --bbox-only result, kept as parent_bbox_ms")
    ap.add_argument("--out", default=None, metavar="FILE", help="with --retain: also write the JSON line to FILE")
    a = ap.parse_args()
    if a.retain > 0:
        return retain(a)
    n = int(a.batch)
    total = a.warmup + a.batches
    lat = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(total)]
    lon = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(total)]
    hrs = []
    for b in range(total):
        device.synth(a.kind, lat[b], lon[b], seed=0, start=b * n)
        h = BASE + b * a.hours + (torch.arange(n, device="cuda", dtype=torch.int64) % a.hours)
        hrs.append(h.to(torch.int32))
    s = StreamingHeatmap(a.zmin, a.zmax, base_hour=BASE, initial_cells=int(a.initial_cells))
    for b in range(a.warmup):
        s.add(lat[b], lon[b], hour=hrs[b])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(a.warmup, total):
        s.add(lat[b], lon[b], hour=hrs[b])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cells, cap = s.cells()
    nall, akeys, acounts = s.extract_device(ALLTIME)[:3]
    # the whole stream (warm-up batches included) against the C oracle's digest
    # of the same points, when one is committed for this configuration
    check = None
    gold = os.path.join(REPO, "tests", "golden", "big_digests.json")
    name = "%s_%.0e_z%d-%d_stream%dx10M" % (a.kind, total * n, a.zmin, a.zmax, total)
    name = name.replace("e+0", "e")
    if n == 10_000_000 and os.path.exists(gold):   # alltime: the same points whatever the hours
        g = json.load(open(gold)).get(name)
        if g is not None:
            sys.path.insert(0, os.path.join(REPO, "tests"))
            from digest import device_digest

            check = "ok" if device_digest(torch, akeys[:nall], acounts[:nall]) == g["digest"] else "FAIL"
    print(json.dumps({
        "metric": "points streamed into a resident heatmap/sec (config 5)", "value": a.batches * n / dt,
        "unit": "points/s", "ms_per_batch": dt * 1e3 / a.batches, "batch_points": n, "batches": a.batches,
        "warmup": a.warmup, "hours_per_batch": a.hours, "zooms": [a.zmin, a.zmax], "kind": a.kind,
        "resident_cells_all_buckets": cells, "alltime_cells": nall, "log_capacity": cap,
        "check": check if check is not None else "no digest for this configuration",
        "data": "synthetic (heatmap_amd.synth, generated on device, resident in HBM)"}))
    s.close()


if __name__ == "__main__":
    main()
