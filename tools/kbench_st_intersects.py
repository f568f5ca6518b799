"""Timing of st_intersects on one GPU (mosaic_st_intersects over device-resident geometry columns, device
pair lists and outputs) on the line workloads of tools/dist_bench.py, so the numbers sit beside those of
profiles/st_distance_lines.json, plus the candidate list a chip join produces:

    (d) point - trip pairs                                            --pt 1e6
    (e) trip - zone pairs                                             --tz 1e6
    (f) trip - trip pairs                                             --tt 1e6
    (g) the (trip, zone) groups of st_intersects_aggregate at --res 9 (every pair of geometries that
        share a cell: what a chip join hands to a flat predicate)

The trips are the seeded random walks of tools/kbench_lines.py (--trips 20000 of 50 vertices in the NYC
bbox); (d)-(f) draw the seeded pair lists of tools/dist_bench.py.  Per workload: the share of pairs the
plan kernel ends (null, empty or box-disjoint), the split of the rest between the one-lane and the
workgroup list, ms per call, the same pairs through mosaic_st_distance (what a user could do before:
`st_distance(...) == 0.0`), and the header's sequential driver on --host-threads threads
(tests/native/st_intersects_host.cpp), whose answers the GPU's are compared with.

A call is timed with device events on the context's stream around the call, after a warm-up call; the
best and the median of --reps calls are kept, and a host clock around the same calls is recorded beside
them.  Prints one JSON line per record and writes them all to --out.

    python tools/kbench_st_intersects.py [--cases defg] [--pt 1e6] [--tz 1e6] [--tt 1e6] [--res 9] [--reps 7]
                                         [--small-works ...] [--host-threads 16] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pt", type=float, default=1e6)
    p.add_argument("--tz", type=float, default=1e6)
    p.add_argument("--tt", type=float, default=1e6)
    p.add_argument("--trips", type=int, default=20000)
    p.add_argument("--res", type=int, default=9)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--zones", default="nyc_taxi_zones")
    p.add_argument("--cases", default="defg")
    p.add_argument("--small-works", type=int, nargs="*", default=[], help="dist_small_work values to time each case at as well")
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--out", default="")
    args = p.parse_args()
    import torch

    from mosaic_amd import MosaicContext
    from mosaic_amd import _native as N
    from mosaic_amd.context import tessellate
    from mosaic_amd.data import PolygonSet, uniform_points_device
    from tests.intersects_cases import host_intersects
    from tests.test_st_distance_lines import LCol
    from tools.kbench_lines import trips as make_trips

    zones = PolygonSet.load(args.zones)
    nz = len(zones)
    ctx = MosaicContext.build("H3")
    stream = torch.cuda.ExternalStream(ctx.stream())
    lib = N.lib()
    records = []

    def emit(**rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(entry, lt, rt, li, ri, n, out):
        ev, host = [], []
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            N.check(entry(ctx.handle, lt.handle, rt.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), None))
            e1.record(stream)
            e1.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        ev, host = sorted(ev[1:]), sorted(host[1:])  # the first call warms up
        return ev[0], ev[len(ev) // 2], host[0]

    def split():
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(lib.mosaic_st_intersects_last_split(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def case(name, lt, rt, li, ri, n, work, host, **extra):
        rec = dict(case=name, pairs=n, segment_pairs=int(work), **extra)
        out = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        dist = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        best, med, host_clock = timed(lib.mosaic_st_intersects, lt, rt, li, ri, n, out)
        ended, one_lane, workgroup = split()
        got = out[:n].cpu().numpy().astype(bool)
        rec.update(intersects_ms=round(best, 3), intersects_median_ms=round(med, 3), intersects_host_clock_ms=round(host_clock, 3),
                   ended_in_plan=ended, ended_in_plan_share=round(ended / max(n, 1), 4), one_lane_pairs=one_lane,
                   workgroup_pairs=workgroup, true_pairs=int(got.sum()))
        for sw in args.small_works:
            ctx.set_option("dist_small_work", sw)
            b, m, _ = timed(lib.mosaic_st_intersects, lt, rt, li, ri, n, out)
            rec[f"intersects_ms_small_work_{sw}"] = round(b, 3)
            rec[f"same_answers_small_work_{sw}"] = bool((out[:n].cpu().numpy().astype(bool) == got).all())
        ctx.set_option("dist_small_work", 512)
        best_d, med_d, _ = timed(lib.mosaic_st_distance, lt, rt, li, ri, n, dist)
        d = dist[:n].cpu().numpy()
        rec.update(distance_ms=round(best_d, 3), distance_median_ms=round(med_d, 3), distance_over_intersects=round(best_d / best, 2),
                   distance_zero_pairs=int((d == 0.0).sum()), distance_zero_differs_on=int(((d == 0.0) != got).sum()))
        if not args.no_host:
            hl, hr, hli, hri = host
            t0 = time.perf_counter()
            want = host_intersects(hl, hr, hli, hri, threads=args.host_threads)
            host_ms = (time.perf_counter() - t0) * 1e3
            rec.update(host_threads=args.host_threads, host_ms=round(host_ms, 1), host_over_gpu=round(host_ms / best, 1),
                       gpu_equals_host=bool((got == want).all()))
        emit(**rec)

    zt = ctx.geometry_table(zones)
    zh = LCol.from_polyset(zones)
    if not args.no_host:
        host_intersects(zh, zh, [0], [0])  # compiles the host library before anything is timed
    zfac = zh.status()[1].astype(np.int64)
    x0, y0, x1, y1 = zones.bbox()
    trips = make_trips(args.trips)
    nt = len(trips)
    tt = ctx.geometry_table(trips)
    th = LCol.from_lineset(trips)
    tfac = th.status()[1].astype(np.int64)
    g = torch.Generator(device="cuda")

    def pair_list(seed, n, n_left, n_right):
        g.manual_seed(seed)
        return (torch.randint(0, n_left, (n,), generator=g, device="cuda", dtype=torch.int64),
                torch.randint(0, n_right, (n,), generator=g, device="cuda", dtype=torch.int64))

    if "d" in args.cases:
        n = int(args.pt)
        npts = min(n, 1 << 20)
        px, py = uniform_points_device((x0, y0, x1, y1), npts, seed=6)
        pt_t = ctx.geometry_table((px, py))
        li, ri = pair_list(7, n, npts, nt)
        li_h, ri_h = li.cpu().numpy(), ri.cpu().numpy()
        case("d point-trip", pt_t, tt, li, ri, n, int(tfac[ri_h].sum()),
             (LCol.from_points(px.cpu().numpy(), py.cpu().numpy()), th, li_h, ri_h), trips=nt)
        pt_t.close()
    if "e" in args.cases:
        n = int(args.tz)
        li, ri = pair_list(8, n, nt, nz)
        li_h, ri_h = li.cpu().numpy(), ri.cpu().numpy()
        case("e trip-zone", tt, zt, li, ri, n, int((tfac[li_h] * zfac[ri_h]).sum()), (th, zh, li_h, ri_h), trips=nt)
    if "f" in args.cases:
        n = int(args.tt)
        li, ri = pair_list(10, n, nt, nt)
        li_h, ri_h = li.cpu().numpy(), ri.cpu().numpy()
        case("f trip-trip", tt, tt, li, ri, n, int((tfac[li_h] * tfac[ri_h]).sum()), (th, th, li_h, ri_h), trips=nt)
    if "g" in args.cases:
        polys = tessellate("H3", zones, args.res)
        lines = tessellate("H3", trips, args.res, ctx=ctx)
        lt = ctx.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], args.res)
        pt_c = ctx.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], args.res)
        lk, pk, fl = ctx.st_intersects_aggregate(lt, pt_c)
        lt.close()
        pt_c.close()
        li_h, ri_h = np.ascontiguousarray(lk, np.int64), np.ascontiguousarray(pk, np.int64)
        li, ri = torch.from_numpy(li_h).cuda(), torch.from_numpy(ri_h).cuda()
        n = len(li_h)
        case("g chip-join candidates", tt, zt, li, ri, n, int((tfac[li_h] * zfac[ri_h]).sum()), (th, zh, li_h, ri_h), trips=nt,
             resolution=args.res, aggregate_true_groups=int(np.asarray(fl).astype(bool).sum()))
        flat = records[-1]
        if not args.no_host:
            want = host_intersects(th, zh, li_h, ri_h, threads=args.host_threads)
            flat["aggregate_flags_differ_from_flat_on"] = int((np.asarray(fl).astype(bool) != want).sum())
            print(json.dumps({"case": flat["case"], "aggregate_flags_differ_from_flat_on": flat["aggregate_flags_differ_from_flat_on"]}), flush=True)
    tt.close()
    zt.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
