"""Timing of st_distance on one GPU (mosaic_st_distance over device-resident geometry columns, device
pair lists and outputs): three cases, each with and without pruning, against the header's sequential
driver on host threads (tests/native/st_distance_host.cpp, the only baseline there is).

    (a) point - point pairs                       --pp 1e7
    (b) point - zone pairs on the NYC zones       --pz 1e6
    (c) every zone against every zone             (263 x 263)

A call is timed with a host clock around mosaic_st_distance, which returns after its stream has
drained; the best and the median of --reps calls after a warm-up are kept.  "segment pairs" is the work
of the unpruned definition, sum over the pairs of facets(left) x facets(right), whatever pruning skips.
--sweep times case (b) and (c) over dist_tile and dist_small_work.  Prints one JSON line per record and
writes them all to --out.

    python tools/dist_bench.py [--pp 1e7] [--pz 1e6] [--reps 5] [--sweep] [--host-threads 16] [--out FILE]
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
    p.add_argument("--cases", default="abc")
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

    def case(name, lt, rt, li, ri, n, work, host=None, host_scale=1.0, variants=((1, "pruned"), (0, "unpruned")), **extra):
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
            want = host_distance(hl, hr, hli, hri, threads=args.host_threads)
            host_ms = (time.perf_counter() - t0) * 1e3 * host_scale
            rec["host_threads"] = args.host_threads
            rec["host_ms"] = round(host_ms, 1)
            rec["host_scaled_from_share"] = round(1.0 / host_scale, 4)
            rec["host_over_gpu"] = round(host_ms / rec[variants[0][1] + "_ms"], 1)
            if host_scale == 1.0:
                rec["gpu_equals_host_bits"] = bool((ref.view(np.int64) == want.view(np.int64)).all())
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
    zt.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
