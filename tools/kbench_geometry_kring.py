"""grid_geometrykring timing: mosaic_geometry_kring / mosaic_chips_kring (one multi-source search on
the GPU) over the 263 NYC taxi zones at H3 res 9, k = 1, 3, 10, against the composition a caller had
to write before, measured in the same process: tessellate(ctx) + grid_cellkring over the border
cells + a numpy union per geometry.  Reports wall ms of both, the device ms of the search
(mosaic_geometry_kring_last_ms), the search from pre-computed chips, the output cell counts and
whether the two agree as sets.  Writes one JSON document (--out).
Usage: python tools/kbench_geometry_kring.py [--out profiles/geometry_kring.json] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mosaic_amd import MosaicContext  # noqa: E402
from mosaic_amd import _native as N  # noqa: E402
from mosaic_amd.context import tessellate  # noqa: E402
from mosaic_amd.data import PolygonSet  # noqa: E402


def composition(ctx, zones, res, k):
    chips = tessellate(ctx.index_system, zones, res, keep_core_geom=False, ctx=ctx)
    core, ids, key = chips["is_core"] != 0, chips["index_id"], chips["polygon_key"]
    border = np.flatnonzero(~core)
    rings = np.concatenate(ctx.grid_cellkring(ids[border], k)).reshape(len(border), -1)
    out = []
    for g in range(len(zones)):
        out.append(np.union1d(ids[core & (key == g)], rings[key[border] == g].ravel()))
    return out


def best_ms(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        best = min(best, (time.perf_counter() - t) * 1e3)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = MosaicContext.build("H3", "JTS")
    zones = PolygonSet.load("nyc_taxi_zones")
    res = 9
    chips = tessellate(ctx.index_system, zones, res, keep_core_geom=False, ctx=ctx)
    tess_ms, _ = best_ms(lambda: tessellate(ctx.index_system, zones, res, keep_core_geom=False, ctx=ctx), a.reps)
    doc = {"workload": "263 NYC taxi zones, H3 res 9", "chips": int(len(chips["index_id"])),
           "border_chips": int((chips["is_core"] == 0).sum()), "tessellate_wall_ms": round(tess_ms, 2), "runs": []}
    for k in (1, 3, 10):
        ctx.grid_geometrykring(zones, res, k)  # warm-up (code object, allocations)
        composition(ctx, zones, res, k)
        wall, rows = best_ms(lambda: ctx.grid_geometrykring(zones, res, k), a.reps)
        dev = N.lib().mosaic_geometry_kring_last_ms()
        chips_wall, rows_c = best_ms(lambda: ctx.grid_geometrykring(dict(chips, n_geoms=len(zones)), res, k), a.reps)
        base, want = best_ms(lambda: composition(ctx, zones, res, k), a.reps)
        equal = all(np.array_equal(np.sort(r), w) for r, w in zip(rows, want)) and \
            all(np.array_equal(r, c) for r, c in zip(rows, rows_c))
        run = {"k": k, "cells": int(sum(len(r) for r in rows)), "search_wall_ms": round(wall, 2),
               "search_device_ms": round(dev, 3), "search_from_chips_wall_ms": round(chips_wall, 2),
               "composition_wall_ms": round(base, 2), "composition_ring_cells": int(doc["border_chips"] * (1 + 3 * k * (k + 1))),
               "equal_sets": bool(equal)}
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
    ctx.close()
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
