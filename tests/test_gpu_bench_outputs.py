"""bench.py on the GPU at a small size: a plain run's line, `--dump-outputs`
(the same files from run to run, equal to the oracle's cells) and `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from heatmap_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
pytestmark = pytest.mark.gpu

N = 300_000
# none of the synthetic clouds has a point outside the square, so no run writes outside_cells.npy
NAMES = ["zoom_totals", "cells_index", "cells_zoom", "cells_row", "cells_col", "cells_count"]


def _bench(*extra):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HM_BENCH_DRY")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--points", str(N)]
                       + list(extra), env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.split("\n") if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module", params=["hotspots", "uniform"])
def plain(request, gpu, tmp_path_factory):
    """Two plain runs with the same arguments, each with its own dump:
    hotspots has fewer than DUMP_CELLS cells (all are written), uniform more
    (the seeded sample)."""
    dirs = [str(tmp_path_factory.mktemp("dump%d" % i)) for i in range(2)]
    return [_bench("--kind", request.param, "--dump-outputs", d) for d in dirs], dirs, request.param


def test_plain_line(plain):
    line = plain[0][0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["unit"] == "points/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["cpu_baseline"] is None
    assert line["pipeline"]["check"] is None
    assert line["roofline"]["measured_peak"] is None


def test_dump_is_reproducible(plain):
    _, (a, b), _ = plain
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in NAMES)
    total = 0
    for n in NAMES:
        x, y = np.load(os.path.join(a, n + ".npy")), np.load(os.path.join(b, n + ".npy"))
        assert x.dtype == np.float64
        assert x.shape == y.shape and np.array_equal(x, y), n
        total += os.path.getsize(os.path.join(a, n + ".npy"))
    assert total <= 64 << 20


def test_dump_matches_oracle(plain):
    """The dumped cells are the oracle's for the same cloud (heatmap_amd.synth
    is bit-identical to the device generator)."""
    _, (a, _), kind = plain
    d = {n: np.load(os.path.join(a, n + ".npy")) for n in NAMES}
    lat, lon = synth.generate(kind, N, seed=0)
    ref = oracle.count(lat, lon, None, 0, 18)
    assert ref["status"] == 0
    z, r, c, k = (np.asarray(ref[x]).astype(np.int64) for x in ("zoom", "row", "col", "count"))
    side = np.int64(1) << z
    inside = (r >= 0) & (r < side) & (c >= 0) & (c < side)
    o = np.lexsort((c[inside], r[inside], z[inside]))
    zi, ri, ci, ki = z[inside][o], r[inside][o], c[inside][o], k[inside][o]
    zs = np.arange(0, 19)
    assert np.array_equal(d["zoom_totals"][:, 0], zs)
    assert np.array_equal(d["zoom_totals"][:, 1], np.bincount(zi, minlength=19))
    assert np.array_equal(d["zoom_totals"][:, 2], np.bincount(zi, weights=ki, minlength=19))
    assert not (~inside).any() and not d["zoom_totals"][:, 3:].any()
    assert np.array_equal(d["zoom_totals"][:, 2], np.full(19, N))
    idx = d["cells_index"].astype(np.int64)
    assert (len(zi) > 1 << 20) == (kind == "uniform")
    assert len(idx) == min(len(zi), 1 << 20) and np.all(np.diff(idx) > 0)
    assert np.array_equal(d["cells_zoom"], zi[idx]) and np.array_equal(d["cells_row"], ri[idx])
    assert np.array_equal(d["cells_col"], ci[idx]) and np.array_equal(d["cells_count"], ki[idx])


def test_dump_with_cells_outside_the_square(gpu, tmp_path):
    """dump_outputs on buffers that hold cells outside the square: their
    per-zoom totals and the sorted records are written too."""
    import types

    import bench

    torch = gpu
    z, r, c = np.array([3, 1, 3, 2]), np.array([5, 0, 2, 3]), np.array([1, 1, 7, 0])
    keys = torch.tensor(((z << 58) | (r << 29) | c).astype(np.int64), device="cuda")
    counts = torch.tensor([4, 9, 2, 5], device="cuda")
    x = torch.tensor([3, -1, 2, 6, 1, 0, 2, 1, 3, -1, 1, 2], device="cuda")
    bench.dump_outputs(torch, str(tmp_path), types.SimpleNamespace(keys=keys, counts=counts, xcells=x, nx=3), 4, 1, 3)
    d = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in NAMES + ["outside_cells"]}
    assert np.array_equal(d["zoom_totals"], [[1, 1, 9, 1, 1], [2, 1, 5, 0, 0], [3, 2, 6, 2, 8]])
    assert np.array_equal(d["cells_index"], [0, 1, 2, 3])
    assert np.array_equal(d["cells_zoom"], [1, 2, 3, 3]) and np.array_equal(d["cells_row"], [0, 3, 2, 5])
    assert np.array_equal(d["cells_col"], [1, 0, 7, 1]) and np.array_equal(d["cells_count"], [9, 5, 2, 4])
    assert np.array_equal(d["outside_cells"], [[1, 0, 2, 1], [3, -1, 1, 2], [3, -1, 2, 6]])
    # a later dump without such cells into the same directory leaves no stale file
    bench.dump_outputs(torch, str(tmp_path), types.SimpleNamespace(keys=keys, counts=counts, xcells=x, nx=0), 4, 1, 3)
    assert not os.path.exists(os.path.join(str(tmp_path), "outside_cells.npy"))


def test_full_line(gpu):
    line = _bench("--full", "--cpu-sample", "100000")
    assert line["full"] is True
    assert line["pipeline"]["check"] == "ok"
    assert line["roofline"]["measured_peak"]["GBps"] > 0
    assert line["cpu_baseline"]["value"] > 0
