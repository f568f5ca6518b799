"""Timing of st_distance on one GPU (mosaic_st_distance over device-resident geometry columns, device
pair lists and outputs): six cases, each with and without pruning, against the header's sequential
driver on host threads (tests/native/st_distance_host.cpp; for the line cases the kind-aware driver of
tests/native/st_distance_lines_host.cpp), the only baseline there is.

    (a) point - point pairs                       --pp 1e7
    (b) point - zone pairs on the NYC zones       --pz 1e6
    (c) every zone against every zone             (263 x 263)
    (d) point - trip pairs                        --pt 1e6
    (e) trip - zone pairs                         --tz 1e6
    (f) trip - trip pairs                         --tt 1e6

The trips are the seeded random walks of tools/kbench_lines.py (--trips 20000 of 50 vertices in the NYC
bbox); (d)-(f) draw seeded pair lists over them.  The host runs (c) and (e) on a seeded share of the
pairs (--host-fraction) and its time is scaled up by the share of the work; the GPU's bits are compared
with the host's on the pairs the host ran.

A call is timed with a host clock around mosaic_st_distance, which returns after its stream has
drained; the best and the median of --reps calls after a warm-up are kept.  "segment pairs" is the work
of the unpruned definition, sum over the pairs of facets(left) x facets(right), whatever pruning skips.
--sweep times case (b) and (c) over dist_tile and dist_small_work.  Prints one JSON line per record and
writes them all to --out.

    python tools/dist_bench.py [--cases abcdef] [--pp 1e7] [--pz 1e6] [--pt 1e6] [--tz 1e6] [--tt 1e6] [--reps 5] [--sweep]
                               [--host-threads 16] [--out FILE]
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
    p.add_argument("--pp", type=float, default=1e7)
    p.add_argument("--pz", type=float, default=1e6)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--zones", default="nyc_taxi_zones")
    p.add_argument("--pt", type=float, default=1e6)
    p.add_argument("--tz", type=float, default=1e6)
    p.add_argument("--tt", type=float, default=1e6)
    p.add_argument("--trips", type=int, default=20000)
    p.add_argument("--cases", default="abcdef")
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--tiles", type=int, nargs="*", default=[8, 16, 32, 64, 128, 256, 512, 1024], help="dist_tile values of --sweep")
    p.add_argument("--small-works", type=int, nargs="*", default=[0, 64, 256, 512, 1024, 2048, 4096, 16384, 1 << 20],
                   help="dist_small_work values of --sweep")
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--host-fraction", type=float, default=0.25,
                   help="share of case (c)'s pairs the host baseline runs (a seeded sample; its time is scaled up)")
    p.add_argument("--tile", type=int, default=0)
    p.add_argument("--small-work", type=int, default=-1)
    p.add_argument("--out", default="")
    args = p.parse_args()
    import torch

    from mosaic_amd import MosaicContext
    from mosaic_amd import _native as N
    from mosaic_amd.data import PolygonSet, uniform_points_device
    from tests.test_st_distance import HostCol, host_distance

    zones = PolygonSet.load(args.zones)
    nz = len(zones)
    ctx = MosaicContext.build("H3")
    if args.tile:
        ctx.set_option("dist_tile", args.tile)
    if args.small_work >= 0:
        ctx.set_option("dist_small_work", args.small_work)
    records = []

    def emit(**rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def gpu_time(lt, rt, li, ri, n):
        out = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ms = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            N.check(N.lib().mosaic_st_distance(ctx.handle, lt.handle, rt.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), None))
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[1:])  # the first call warms up
        return ms[0], ms[len(ms) // 2], out

    def case(name, lt, rt, li, ri, n, work, host=None, host_scale=1.0, variants=((1, "pruned"), (0, "unpruned")),
             host_fn=host_distance, host_pick=None, **extra):
        rec = dict(case=name, pairs=n, segment_pairs=int(work), **extra)
        ref = None
        for prune, label in variants:
            ctx.set_option("dist_prune", prune)
            best, med, out = gpu_time(lt, rt, li, ri, n)
            rec[label + "_ms"] = round(best, 3)
            rec[label + "_median_ms"] = round(med, 3)
            rec[label + "_segment_pairs_per_s"] = float(f"{work / (best * 1e-3):.4g}")
            got = out[:n].cpu().numpy()
            if ref is None:
                ref = got
            rec[label + "_same_bits"] = bool((got.view(np.int64) == ref.view(np.int64)).all())
        ctx.set_option("dist_prune", 1)
        if host is not None and not args.no_host:
            hl, hr, hli, hri = host
            t0 = time.perf_counter()
            want = host_fn(hl, hr, hli, hri, threads=args.host_threads)
            host_ms = (time.perf_counter() - t0) * 1e3 * host_scale
            rec["host_threads"] = args.host_threads
            rec["host_ms"] = round(host_ms, 1)
            rec["host_scaled_from_share"] = round(1.0 / host_scale, 4)
            rec["host_over_gpu"] = round(host_ms / rec[variants[0][1] + "_ms"], 1)
            if host_scale == 1.0:
                rec["gpu_equals_host_bits"] = bool((ref.view(np.int64) == want.view(np.int64)).all())
            elif host_pick is not None:  # the pairs the host ran
                rec["gpu_equals_host_bits_on_share"] = bool((ref[host_pick].view(np.int64) == want.view(np.int64)).all())
                rec["host_pairs"] = int(len(host_pick))
        emit(**rec)
        return rec

    zt = ctx.geometry_table(zones)
    zh = HostCol.from_polyset(zones)
    zfac = zh.status()[1].astype(np.int64)
    x0, y0, x1, y1 = zones.bbox()

    if "a" in args.cases:
        n = int(args.pp)
        ax, ay = uniform_points_device((x0, y0, x1, y1), n, seed=1)
        bx, by = uniform_points_device((x0, y0, x1, y1), n, seed=2)
        lt, rt = ctx.geometry_table((ax, ay)), ctx.geometry_table((bx, by))
        host = None
        if not args.no_host:
            host = (HostCol.from_points(ax.cpu().numpy(), ay.cpu().numpy()), HostCol.from_points(bx.cpu().numpy(), by.cpu().numpy()),
                    None, None)
        case("a point-point", lt, rt, None, None, n, n, host, variants=((1, "pruned"),))
        lt.close()
        rt.close()

    if "b" in args.cases:
        n = int(args.pz)
        npts = min(n, 1 << 20)
        px, py = uniform_points_device((x0, y0, x1, y1), npts, seed=3)
        pt_t = ctx.geometry_table((px, py))
        g = torch.Generator(device="cuda")
        g.manual_seed(4)
        li = torch.randint(0, npts, (n,), generator=g, device="cuda", dtype=torch.int64)
        ri = torch.randint(0, nz, (n,), generator=g, device="cuda", dtype=torch.int64)
        work = int(zfac[ri.cpu().numpy()].sum())
        host = (HostCol.from_points(px.cpu().numpy(), py.cpu().numpy()), zh, li.cpu().numpy(), ri.cpu().numpy())
        case("b point-zone", pt_t, zt, li, ri, n, work, host)
        if args.sweep:
            for sw in args.small_works:
                ctx.set_option("dist_small_work", sw)
                case("b point-zone", pt_t, zt, li, ri, n, work, variants=((1, "pruned"),), dist_small_work=sw)
            ctx.set_option("dist_small_work", args.small_work if args.small_work >= 0 else 512)
        pt_t.close()

    if "c" in args.cases:
        li_h, ri_h = np.repeat(np.arange(nz), nz), np.tile(np.arange(nz), nz)
        li, ri = torch.from_numpy(li_h).cuda(), torch.from_numpy(ri_h).cuda()
        work = int(zfac.sum()) ** 2
        rng = np.random.default_rng(5)
        share = min(1.0, max(args.host_fraction, 1e-3))
        pick = np.flatnonzero(rng.random(len(li_h)) < share) if share < 1 else np.arange(len(li_h))
        scale = float(work) / float((zfac[li_h[pick]] * zfac[ri_h[pick]]).sum())  # by the sample's share of the work
        case("c zone-zone", zt, zt, li, ri, len(li_h), work, (zh, zh, li_h[pick], ri_h[pick]), host_scale=scale)
        if args.sweep:
            for tile in args.tiles:
                ctx.set_option("dist_tile", tile)
                case("c zone-zone", zt, zt, li, ri, len(li_h), work, dist_tile=tile)
            ctx.set_option("dist_tile", args.tile or 16)
    if set("def") & set(args.cases):
        from tests.test_st_distance_lines import LCol
        from tests.test_st_distance_lines import host_distance as host_distance_lines
        from tools.kbench_lines import trips as make_trips

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
            work = int(tfac[ri.cpu().numpy()].sum())
            host = (LCol.from_points(px.cpu().numpy(), py.cpu().numpy()), th, li.cpu().numpy(), ri.cpu().numpy())
            case("d point-trip", pt_t, tt, li, ri, n, work, host, host_fn=host_distance_lines, trips=nt)
            pt_t.close()

        if "e" in args.cases:
            n = int(args.tz)
            li, ri = pair_list(8, n, nt, nz)
            li_h, ri_h = li.cpu().numpy(), ri.cpu().numpy()
            pair_work = tfac[li_h] * zfac[ri_h]
            work = int(pair_work.sum())
            share = min(1.0, max(args.host_fraction, 1e-3))
            pick = np.flatnonzero(np.random.default_rng(9).random(n) < share) if share < 1 else np.arange(n)
            scale = float(work) / float(pair_work[pick].sum())
            case("e trip-zone", tt, zt, li, ri, n, work, (th, LCol.from_polyset(zones), li_h[pick], ri_h[pick]), host_scale=scale,
                 host_fn=host_distance_lines, host_pick=pick, trips=nt)

        if "f" in args.cases:
            n = int(args.tt)
            li, ri = pair_list(10, n, nt, nt)
            li_h, ri_h = li.cpu().numpy(), ri.cpu().numpy()
            work = int((tfac[li_h] * tfac[ri_h]).sum())
            case("f trip-trip", tt, tt, li, ri, n, work, (th, th, li_h, ri_h), host_fn=host_distance_lines, trips=nt)
        tt.close()
    zt.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
