"""st_intersects_aggregate over line chips x polygon chips timing: mosaic_line_intersects_aggregate
against the host restatement mosaic_line_intersects_aggregate_host (its own threads, 16 at the most)
for 20,000 seeded random-walk "trips" (tools/kbench_lines.py) against the 263 NYC taxi zones, at H3
res 9 and res 11.  Per resolution: both chip sets from the GPU producers, the two table builds (wall
ms), one warm-up call of the join, then the best wall ms of --reps further calls and the counters and
device times of the last of them (mosaic_line_join_last: k_lj_probe, k_lj_test; HIP events), for each
team width of k_lj_test (64: one wave per pair; 16: four pairs per wave); the host restatement's best
wall ms; whether the results are identical (key columns and flags).
There is no earlier line join to compare against: a record, not a gate.  Writes one JSON document (--out).
Usage: python tools/kbench_line_join.py [--out profiles/line_join.json] [--reps 3] [--trips 20000]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)

from kbench_lines import best_ms, trips  # noqa: E402
from mosaic_amd import MosaicContext, line_intersects_aggregate_host  # noqa: E402
from mosaic_amd import _native as N  # noqa: E402
from mosaic_amd.context import tessellate  # noqa: E402
from mosaic_amd.data import PolygonSet  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trips", type=int, default=20000)
    a = ap.parse_args()
    ctx = MosaicContext.build("H3", "JTS")
    zones = PolygonSet.load("nyc_taxi_zones")
    lines = trips(a.trips)
    doc = {"workload": f"{a.trips} random-walk trips of 50 vertices against the {len(zones)} NYC taxi zones", "runs": []}
    for res in (9, 11):
        lc = tessellate("H3", lines, res, ctx=ctx)
        pc = tessellate("H3", zones, res, ctx=ctx)
        line_ms, lt = timed(lambda: ctx.line_chip_table(lc["is_core"], lc["index_id"], lc["wkb"], lc["polygon_key"], res))
        poly_ms, pt = timed(lambda: ctx.chip_table(pc["is_core"], pc["index_id"], pc["wkb"], pc["polygon_key"], res))
        run = {"resolution": res, "line_chips": int(len(lc["index_id"])), "polygon_chips": int(len(pc["index_id"])),
               "line_table_build_ms": round(line_ms, 1), "polygon_table_build_ms": round(poly_ms, 1)}
        got = {}
        for team in (64, 16):
            prev = N.lib().mosaic_line_join_team(team)
            ctx.st_intersects_aggregate(lt, pt)  # warm-up
            wall, got[team] = best_ms(lambda: ctx.st_intersects_aggregate(lt, pt), a.reps)
            n, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 2)()
            N.check(N.lib().mosaic_line_join_last(n, ms))
            N.lib().mosaic_line_join_team(prev)
            run[f"team{team}"] = {"gpu_wall_ms": round(wall, 2), "device_probe_ms": round(ms[0], 3),
                                  "device_test_ms": round(ms[1], 3), "line_chips_probed": int(n[0]), "chip_pairs": int(n[1]),
                                  "pairs_tested": int(n[2]), "groups": int(n[3])}
        host_ms, host = best_ms(lambda: line_intersects_aggregate_host("H3", lc, pc, res), max(1, a.reps - 1))
        run.update(groups=int(len(host[0])), true_groups=int(host[2].sum()), host_wall_ms=round(host_ms, 1),
                   identical=bool(all(np.array_equal(x, y) for t in got.values() for x, y in zip(t, host))))
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        lt.close()
        pt.close()
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
