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
    print(json.dumps({
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
        "series": series,
        "data": "synthetic (heatmap_amd.synth, generated on device, resident in HBM)"}))
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
