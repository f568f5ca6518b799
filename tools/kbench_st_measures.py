"""Timing of st_measures on one GPU (mosaic_st_measures over device-resident geometry columns, device
outputs) and of the resolution analyzer end to end, written to profiles/st_measures.json:

    zones          the 263 NYC taxi zones (rings up to 7,814 vertices)
    buildings_2e5  synthetic_buildings(2e5)
    buildings_1e6  synthetic_buildings(1e6)
    trips          the seeded 20,000-trip LineSet of tools/kbench_lines.py

Per column: one combined call (every output), area only and centroid only, each as the best and the
median of --reps calls after a warm-up call, timed with device events on the context's stream around
the call, with a host clock around the same calls beside them; the split between the lane and the wave
kernel; the same three under "every row on the lane kernel" and under "every row on the wave kernel", and
the combined call at each --wave-mins value of "meas_wave_min"; the sequential definition on --host-threads host threads
(tests/native/st_measures_host.cpp), whose bits the GPU's are compared with; and the combined lane
call's share of the 16 B/vertex HBM roofline (--hbm-tbs, the device's peak rate).  No earlier
implementation exists to compare with.  The analyzer (MosaicAnalyzer.get_optimal_resolution, all rows)
is timed with a host clock on the zones and on the 2e5 buildings.

    python tools/kbench_st_measures.py [--columns zones buildings_2e5 buildings_1e6 trips] [--reps 5]
                                       [--host-threads 16] [--out profiles/st_measures.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = dict(meas_tile=256, meas_wave_min=128)  # the library's defaults
VARIANTS = {
    "default": {},
    "all_lane": dict(meas_wave_min=1 << 40),
    "all_wave": dict(meas_wave_min=0),
}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--columns", nargs="*", default=["zones", "buildings_2e5", "buildings_1e6", "trips"])
    p.add_argument("--trips", type=int, default=20000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--hbm-tbs", type=float, default=8.0, help="the device's peak HBM rate, TB/s")
    p.add_argument("--no-analyzer", action="store_true")
    p.add_argument("--wave-mins", type=int, nargs="*", default=[16, 32, 48, 64, 96, 128, 192, 256, 512, 1024])
    p.add_argument("--slow-variants-below", type=float, default=3e5,
                   help="columns with more rows than this skip the all-wave variant (one wave per tiny row)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "st_measures.json"))
    args = p.parse_args()
    import torch

    from mosaic_amd import MosaicAnalyzer, MosaicContext
    from mosaic_amd import _native as N
    from mosaic_amd.data import PolygonSet, synthetic_buildings
    from tests.measures_cases import host_measures
    from tests.test_st_distance_lines import LCol
    from tools.kbench_lines import trips as make_trips

    ctx = MosaicContext.build("H3")
    stream = torch.cuda.ExternalStream(ctx.stream())
    lib = N.lib()
    records = []

    def emit(**rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(table, n, outs):
        ev, host = [], []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            N.check(lib.mosaic_st_measures(ctx.handle, table.handle, None, n, *[N.ptr(o) for o in outs], None))
            e1.record(stream)
            e1.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        ev, host = sorted(ev[1:]), sorted(host[1:])  # the first call warms up
        return dict(device_ms=round(ev[0], 4), device_median_ms=round(ev[len(ev) // 2], 4), wall_ms=round(host[0], 4))

    def column(name, src, col):
        with ctx.geometry_table(src) as table:
            n, nv = len(table), table.info()["n_vertices"]
            f = lambda: torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
            area, length, cx, cy, x0, y0, x1, y1 = (f() for _ in range(8))
            npts = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
            calls = {"combined": [area, length, cx, cy, npts, x0, y0, x1, y1],
                     "area": [area] + [None] * 8,
                     "centroid": [None, None, cx, cy] + [None] * 5}
            rec = dict(column=name, rows=n, vertices=nv)
            try:
                for vname, opts in VARIANTS.items():
                    if vname == "all_wave" and n > args.slow_variants_below:
                        continue
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    rec[vname] = {c: timed(table, n, outs) for c, outs in calls.items()}
                    rec[vname]["lane_rows"], rec[vname]["wave_rows"] = ctx.st_measures_last_split()
                    for k, v in DEFAULTS.items():
                        ctx.set_option(k, v)
                if n <= args.slow_variants_below:
                    rec["combined_device_ms_by_wave_min"] = {}
                    for wm in args.wave_mins:
                        ctx.set_option("meas_wave_min", wm)
                        rec["combined_device_ms_by_wave_min"][str(wm)] = timed(table, n, calls["combined"])["device_ms"]
                    ctx.set_option("meas_wave_min", DEFAULTS["meas_wave_min"])
            finally:
                for k, v in DEFAULTS.items():
                    ctx.set_option(k, v)
            timed(table, n, calls["combined"])
            got = dict(area=area, length=length, cx=cx, cy=cy, numpoints=npts, xmin=x0, ymin=y0, xmax=x1, ymax=y1)
            got = {k: v[:n].cpu().numpy() for k, v in got.items()}
            host = {}
            for c, fields in (("combined", None), ("area", ("area",)), ("centroid", ("cx", "cy"))):
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    want = host_measures(col, threads=args.host_threads) if fields is None else host_measures(col, fields=fields, threads=args.host_threads)
                    ms = (time.perf_counter() - t0) * 1e3
                    best = ms if best is None else min(best, ms)
                host[c] = round(best, 3)
                if fields is None:
                    rec["gpu_equals_host_bits"] = all(
                        bool((got[k].view(np.uint64) == want[k].view(np.uint64)).all()) if got[k].dtype == np.float64
                        else bool((got[k] == want[k]).all()) for k in got)
            rec["host_threads"] = args.host_threads
            rec["host_ms"] = host
            rec["host_over_gpu_device"] = {c: round(host[c] / rec["default"][c]["device_ms"], 2) for c in host}
            rec["host_over_gpu_wall"] = {c: round(host[c] / rec["default"][c]["wall_ms"], 2) for c in host}
            lane = rec["all_lane"]["combined"]["device_ms"]
            rec["lane_kernel_call_roofline"] = dict(
                bytes_per_vertex=16, hbm_tbs=args.hbm_tbs, achieved_tbs=round(16.0 * nv / (lane * 1e-3) / 1e12, 4),
                share=round(16.0 * nv / (lane * 1e-3) / 1e12 / args.hbm_tbs, 4),
                note="whole call (plan + lane kernel + the host's wait for the plan counts), every row on the lane kernel")
            emit(**rec)

    def analyzer(name, src, runs=2):
        best = None
        for _ in range(runs):
            t0 = time.perf_counter()
            with MosaicAnalyzer(ctx, src) as an:
                res = an.get_optimal_resolution()
            s = time.perf_counter() - t0
            best = s if best is None else min(best, s)
        emit(analyzer=name, rows=len(src), optimal_resolution=int(res), wall_s=round(best, 3))

    zones = PolygonSet.load("nyc_taxi_zones")
    host_measures(LCol.from_polyset(zones))  # compiles the host library before anything is timed
    b2e5 = None
    for name in args.columns:
        if name == "zones":
            column(name, zones, LCol.from_polyset(zones))
        elif name.startswith("buildings_"):
            b = synthetic_buildings(int(float(name.split("_", 1)[1])))
            if name == "buildings_2e5":
                b2e5 = b
            column(name, b, LCol.from_polyset(b))
        elif name == "trips":
            t = make_trips(args.trips)
            column(name, t, LCol.from_lineset(t))
        else:
            raise SystemExit(f"unknown column {name}")
    if not args.no_analyzer:
        analyzer("zones", zones)
        analyzer("buildings_2e5", b2e5 if b2e5 is not None else synthetic_buildings(200000), runs=1)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
