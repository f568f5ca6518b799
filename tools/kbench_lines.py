"""grid_tessellateexplode over lines (Mosaic.lineFill) timing: mosaic_tessellate_lines_gpu against the host
producer mosaic_tessellate_lines (its own threads, 16 at the most) over 20,000 seeded random-walk
"trips" of 50 vertices in the NYC bbox, at H3 res 9 and res 11.  Per resolution: one warm-up call of the
GPU producer (code objects, allocations), then the best wall ms of --reps further calls, the three
device phases of the last of them (mosaic_tess_lines_last: walk, sort, clip; HIP events), the host
producer's best wall ms, and whether the two chip sets are identical (every column, byte for byte).
There is no earlier line path to compare against: a record, not a gate.  Writes one JSON document (--out).
Usage: python tools/kbench_lines.py [--out profiles/line_fill.json] [--reps 3] [--trips 20000]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mosaic_amd import MosaicContext  # noqa: E402
from mosaic_amd import _native as N  # noqa: E402
from mosaic_amd.context import tessellate  # noqa: E402
from mosaic_amd.data import NYC_BBOX, SEED_BASE, LineSet  # noqa: E402


def trips(n, n_vertices=50, step=0.0012, seed=SEED_BASE + 7):
    """Random walks with a slowly turning heading: steps of 20-130 m (a GPS fix every few seconds of
    city driving), rounded to 1e-6 degrees, clipped to the bbox."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x0, y0, x1, y1 = NYC_BBOX
    start = np.column_stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)])
    heading = np.cumsum(rng.normal(0.0, 0.5, (n, n_vertices - 1)), axis=1) + rng.uniform(0, 2 * np.pi, (n, 1))
    length = step * rng.uniform(0.15, 1.0, (n, n_vertices - 1))
    d = np.stack([np.cos(heading) * length, np.sin(heading) * length], axis=2)
    pts = np.concatenate([start[:, None, :], start[:, None, :] + np.cumsum(d, axis=1)], axis=1)
    pts[..., 0] = np.clip(pts[..., 0], x0, x1)
    pts[..., 1] = np.clip(pts[..., 1], y0, y1)
    pts = np.round(pts * 1e6) / 1e6
    offs = np.arange(n + 1, dtype=np.int64) * n_vertices
    return LineSet(pts.reshape(-1, 2), offs, np.arange(n + 1, dtype=np.int64))


def best_ms(fn, reps):
    best, r = float("inf"), None
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        best = min(best, (time.perf_counter() - t) * 1e3)
    return best, r


def same(a, b):
    n = int(a["wkb"][0][-1]) if len(a["wkb"][0]) else 0
    return bool(all(np.array_equal(a[c], b[c]) for c in ("is_core", "index_id", "polygon_key")) and
                np.array_equal(a["wkb"][0], b["wkb"][0]) and
                np.array_equal(np.asarray(a["wkb"][1])[:n], np.asarray(b["wkb"][1])[:n]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trips", type=int, default=20000)
    a = ap.parse_args()
    ctx = MosaicContext.build("H3", "JTS")
    lines = trips(a.trips)
    doc = {"workload": f"{a.trips} random-walk trips of 50 vertices, NYC bbox", "runs": []}
    for res in (9, 11):
        tessellate("H3", lines, res, ctx=ctx)  # warm-up
        gpu_ms, dev = best_ms(lambda: tessellate("H3", lines, res, ctx=ctx), a.reps)
        n, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 3)()
        N.check(N.lib().mosaic_tess_lines_last(n, ms))
        host_ms, host = best_ms(lambda: tessellate("H3", lines, res), max(1, a.reps - 1))
        doc["runs"].append({
            "resolution": res, "chips": int(len(dev["index_id"])), "wkb_bytes": int(dev["wkb"][0][-1]),
            "segments": int(n[0]), "groups": int(n[1]), "groups_to_host": int(n[2]), "pairs": int(n[3]),
            "gpu_wall_ms": round(gpu_ms, 1), "device_walk_ms": round(ms[0], 2), "device_sort_ms": round(ms[1], 2),
            "device_clip_ms": round(ms[2], 2), "host_wall_ms": round(host_ms, 1), "identical": same(dev, host)})
        print(json.dumps(doc["runs"][-1]), flush=True)
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
