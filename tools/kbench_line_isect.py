"""st_intersection_aggregate over line chips x polygon chips timing: mosaic_line_intersection_aggregate
(lengths) and mosaic_line_intersection_aggregate_geometry (lengths and WKB) against the host
restatement mosaic_line_intersection_aggregate_host (its own threads, 16 at the most) for 20,000 seeded
random-walk "trips" (tools/kbench_lines.py) against the 263 NYC taxi zones, at H3 res 9 and res 11.
Per resolution: both chip sets from the GPU producers, one warm-up call, then the best wall ms of
--reps further calls of each form with the counters and device times of the last of them
(mosaic_line_intersection_last: k_lx_probe, k_lx_chip_len + k_lx_clip, the run fill pass; HIP events);
the host restatement's best wall ms; bit-equality of the three results (asserted); and k_lx_clip's
GB/s against its algorithmic bytes: per clipped pair the vertices of the line chip and of the polygon
chip (16 bytes each, counted from the WKB lengths), the 24-byte pair record and the 12 bytes written.
The device time of that figure includes k_lx_chip_len, which shares k_lx_clip's event pair.
There is no earlier implementation to compare against: a record, not a gate.  With --deviation the
host-side maximum deviation from the exact flat lengths on the two invariant workloads of
tests/test_line_intersection.py is recorded too (CPU only).  Writes one JSON document (--out).
Usage: python tools/kbench_line_isect.py [--out profiles/line_intersection.json] [--reps 3] [--trips 20000]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)

from kbench_lines import best_ms, trips  # noqa: E402
from mosaic_amd import MosaicContext, line_intersection_aggregate_host  # noqa: E402
from mosaic_amd import _native as N  # noqa: E402
from mosaic_amd.context import tessellate  # noqa: E402
from mosaic_amd.data import PolygonSet  # noqa: E402


def last():
    n, ms = (ctypes.c_int64 * 6)(), (ctypes.c_double * 3)()
    N.check(N.lib().mosaic_line_intersection_last(n, ms))
    return [int(v) for v in n], [float(v) for v in ms]


def clip_bytes(lc, pc):
    """Algorithmic bytes of k_lx_clip: per pair with a non-core polygon chip, both chips' vertices,
    the pair record and the outputs."""
    lv = np.maximum((np.diff(lc["wkb"][0]) - 9) // 16, 0)
    pv = np.maximum((np.diff(pc["wkb"][0]) - 13) // 16, 0)
    plain = np.asarray(pc["is_core"]) == 0
    cells, inv = np.unique(np.asarray(pc["index_id"])[plain], return_inverse=True)
    cnt = np.bincount(inv, minlength=len(cells))
    sumv = np.bincount(inv, weights=pv[plain], minlength=len(cells))
    at = np.searchsorted(cells, lc["index_id"])
    hit = (at < len(cells)) & (cells[np.minimum(at, len(cells) - 1)] == lc["index_id"])
    at = at[hit]
    return int((cnt[at] * (lv[hit] * 16 + 36) + sumv[at] * 16).sum())


def same_bits(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
                np.array_equal(np.ascontiguousarray(a[2]).view(np.uint64), np.ascontiguousarray(b[2]).view(np.uint64)) and
                (len(a) < 5 or len(b) < 5 or a[4] == b[4]))


def deviation():
    from tests import line_clip_cases as CC
    from tests import line_join_cases as JC

    out = {}
    for name in ("H3", "BNG"):
        _, _, lines, polys, res = JC.invariant_case(name)
        got = CC.as_dict(*line_intersection_aggregate_host(name, lines, polys, res))
        truth = CC.flat_lengths(name)
        out[name] = {"groups": len(got), "bound": CC.bound(name),
                     "max_abs_deviation": max(abs(v[0] - truth.get(g, 0.0)) for g, v in got.items())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trips", type=int, default=20000)
    ap.add_argument("--deviation", action="store_true")
    a = ap.parse_args()
    ctx = MosaicContext.build("H3", "JTS")
    zones = PolygonSet.load("nyc_taxi_zones")
    lines = trips(a.trips)
    doc = {"workload": f"{a.trips} random-walk trips of 50 vertices against the {len(zones)} NYC taxi zones", "runs": []}
    for res in (9, 11):
        lc = tessellate("H3", lines, res, ctx=ctx)
        pc = tessellate("H3", zones, res, ctx=ctx)
        lt = ctx.line_chip_table(lc["is_core"], lc["index_id"], lc["wkb"], lc["polygon_key"], res)
        pt = ctx.chip_table(pc["is_core"], pc["index_id"], pc["wkb"], pc["polygon_key"], res)
        run = {"resolution": res, "line_chips": int(len(lc["index_id"])), "polygon_chips": int(len(pc["index_id"]))}
        ctx.st_intersection_aggregate_length(lt, pt)  # warm-up
        len_ms, short = best_ms(lambda: ctx.st_intersection_aggregate_length(lt, pt), a.reps)
        n, ms = last()
        nbytes = clip_bytes(lc, pc)
        run["length_call"] = {"gpu_wall_ms": round(len_ms, 2), "device_probe_ms": round(ms[0], 3), "device_clip_ms": round(ms[1], 3)}
        run.update(chip_pairs=n[0], pairs_clipped=n[1], pairs_finished_on_host=n[2], runs=n[3], groups=n[4], cut_cap=n[5],
                   clip_algorithmic_bytes=nbytes, clip_gb_per_s=round(nbytes / (ms[1] * 1e-3) / 1e9, 2) if ms[1] > 0 else None)
        geo_ms, full = best_ms(lambda: ctx.st_intersection_aggregate(lt, pt), a.reps)
        n, ms = last()
        run["geometry_call"] = {"gpu_wall_ms": round(geo_ms, 2), "device_probe_ms": round(ms[0], 3), "device_clip_ms": round(ms[1], 3),
                                "device_run_fill_ms": round(ms[2], 3), "wkb_bytes": int(sum(len(w) for w in full[4]))}
        host_ms, host = best_ms(lambda: line_intersection_aggregate_host("H3", lc, pc, res), max(1, a.reps - 1))
        identical = same_bits(short, host) and same_bits(full, host)
        run.update(host_wall_ms_16_threads=round(host_ms, 1), positive_groups=int((host[2] > 0).sum()), identical_bits=identical)
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        lt.close()
        pt.close()
        assert identical, "the GPU and the host restatement differ"
    if a.deviation:
        doc["host_deviation_from_exact_flat_length"] = deviation()
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
