"""Timing of st_contains over geometry columns on one GPU (mosaic_st_contains_geoms, device pair lists and
outputs), written to profiles/st_contains.json:

    (a) building - zone pairs          --bz 1e6   st_contains(zone, building), seeded random pairs
    (b) trip - zone pairs              --tz 1e6   st_contains(zone, trip), seeded random pairs
    (c) the candidate pairs of st_dwithin_join(buildings, zones, 0.0): every (building, zone) that touch or
        overlap -- what "which buildings lie wholly in which zone" hands to the predicate

Buildings are mosaic_amd.data.synthetic_buildings (--buildings 200000), trips the seeded walks of
tools/kbench_lines.py (--trips 20000 of 50 vertices), zones the 263 NYC taxi zones.  Per workload: ms per
call, the same pairs through mosaic_st_intersects, the sequential definition on --host-threads threads
(tests/native/st_contains_host.cpp; out and status are compared with the GPU's), the five split counts of
mosaic_st_contains_last_split and the undecided share.  A call is timed with device events on the
context's stream, after a warm-up call; best and median of --reps calls.  Nothing is promised: the
record says where the GPU loses.  The host baseline and the column builders are the test suite's
(tests/contains_cases.py, tests/native/st_contains_host.cpp), as in tools/kbench_st_intersects.py, so
the script runs from a full checkout.

    python profiles/st_contains.py [--cases abc] [--bz 1e6] [--tz 1e6] [--reps 7] [--host-threads 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bz", type=float, default=1e6)
    p.add_argument("--tz", type=float, default=1e6)
    p.add_argument("--buildings", type=int, default=200000)
    p.add_argument("--trips", type=int, default=20000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--zones", default="nyc_taxi_zones")
    p.add_argument("--cases", default="abc")
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "st_contains.json"))
    args = p.parse_args()
    import torch

    from mosaic_amd import MosaicContext
    from mosaic_amd import _native as N
    from mosaic_amd.data import PolygonSet, synthetic_buildings
    from tests.contains_cases import host_contains
    from tests.test_st_distance_lines import LCol
    from tools.kbench_lines import trips as make_trips

    zones = PolygonSet.load(args.zones)
    nz = len(zones)
    ctx = MosaicContext.build("H3")
    stream = torch.cuda.ExternalStream(ctx.stream())
    lib = N.lib()
    records = []

    def timed(entry, lt, rt, li, ri, n, out, status):
        ev = []
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            N.check(entry(ctx.handle, lt.handle, rt.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), N.ptr(status)))
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        ev = sorted(ev[1:])  # the first call warms up
        return ev[0], ev[len(ev) // 2]

    def case(name, lt, rt, li, ri, host, **extra):
        n = len(li)
        rec = dict(case=name, pairs=n, **extra)
        out = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        st = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        best, med = timed(lib.mosaic_st_contains_geoms, lt, rt, li, ri, n, out, st)
        five = np.zeros(5, np.int64)
        N.check(lib.mosaic_st_contains_last_split(N.ptr(five)))
        got, got_st = out[:n].cpu().numpy().astype(bool), st[:n].cpu().numpy()
        undecided = int((got_st == N.PAIR_UNDECIDED).sum())
        rec.update(contains_ms=round(best, 3), contains_median_ms=round(med, 3), ended_in_plan=int(five[0]),
                   decided_by_crossing_or_exterior=int(five[1]), decided_without_contact=int(five[2]), undecided=int(five[3]),
                   workgroup_pairs=int(five[4]), undecided_share=round(undecided / max(n, 1), 6), contained_pairs=int(got.sum()))
        best_i, med_i = timed(lib.mosaic_st_intersects, lt, rt, li, ri, n, out, st)
        rec.update(intersects_ms=round(best_i, 3), intersects_median_ms=round(med_i, 3), contains_over_intersects=round(best / best_i, 2),
                   intersecting_pairs=int(out[:n].sum().item()))
        if not args.no_host:
            hl, hr = host
            li_h, ri_h = li.cpu().numpy(), ri.cpu().numpy()
            t0 = time.perf_counter()
            want, want_st = host_contains(hl, hr, li_h, ri_h, threads=args.host_threads)
            host_ms = (time.perf_counter() - t0) * 1e3
            rec.update(host_threads=args.host_threads, host_ms=round(host_ms, 1), host_over_gpu=round(host_ms / best, 2),
                       gpu_equals_host=bool((got == want).all() and (got_st == want_st).all()))
        records.append(rec)
        print(json.dumps(rec), flush=True)

    zt = ctx.geometry_table(zones)
    zh = LCol.from_polyset(zones)
    if not args.no_host:
        host_contains(zh, zh, [0], [0])  # compiles the host library before anything is timed
    g = torch.Generator(device="cuda")

    def pair_list(seed, n, n_left, n_right):
        g.manual_seed(seed)
        return (torch.randint(0, n_left, (n,), generator=g, device="cuda", dtype=torch.int64),
                torch.randint(0, n_right, (n,), generator=g, device="cuda", dtype=torch.int64))

    if "a" in args.cases or "c" in args.cases:
        buildings = synthetic_buildings(args.buildings)
        bt = ctx.geometry_table(buildings)
        bh = LCol.from_polyset(buildings)
        if "a" in args.cases:
            li, ri = pair_list(21, int(args.bz), nz, len(buildings))
            case("a zone contains building, random pairs", zt, bt, li, ri, (zh, bh), buildings=len(buildings), zones=nz)
        if "c" in args.cases:
            ctx.st_dwithin_join(bt, zt, 0.0)  # warms the join up
            t0 = time.perf_counter()
            bi, zi, _ = ctx.st_dwithin_join(bt, zt, 0.0)
            join_ms = (time.perf_counter() - t0) * 1e3  # a host clock around the second call, export included
            li, ri = torch.from_numpy(np.ascontiguousarray(zi)).cuda(), torch.from_numpy(np.ascontiguousarray(bi)).cuda()
            case("c zone contains building, candidates of st_dwithin_join(buildings, zones, 0.0)", zt, bt, li, ri, (zh, bh),
                 buildings=len(buildings), zones=nz, join_warm_host_clock_ms=round(join_ms, 1))
        bt.close()
    if "b" in args.cases:
        trips = make_trips(args.trips)
        tt = ctx.geometry_table(trips)
        th = LCol.from_lineset(trips)
        li, ri = pair_list(22, int(args.tz), nz, len(trips))
        case("b zone contains trip, random pairs", zt, tt, li, ri, (zh, th), trips=len(trips), zones=nz)
        tt.close()
    zt.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
