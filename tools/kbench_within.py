"""The distance-within join (mosaic_within_neighbours) and SpatialKNN.transform_exact, timed on the GPU.

Workloads:
  (a) 19,800 jittered pickups (200 copies of each fixture pickup) against the 263 NYC taxi zones;
  (b) the same 19,800 points against 20,000 seeded trips (tools/kbench_lines.py);
  (c) 2e5 synthetic buildings against themselves at one small radius;
  (s) with --only s: the 99 fixture pickups against the zones at one radius, a size at which every figure
      is an overhead.
For (a) and (b): transform and transform_exact on one model, alternated; then the within-join alone at
the exact pass's radii, in the exact pass's batches.  For all three: the join against the composition it
replaces, written as a caller would --
    a numpy box filter over all (landmark, candidate) envelopes (the boxes grown by the radius),
    st_distance(pairs=...) on the same geometry tables, the radius cut, np.lexsort --
alternated in one process, best of --reps each with the spread, and whether the two give the same rows.
The composition of (c) runs on the first --comp-rows landmarks only (all pairs of 2e5 x 2e5 envelopes
are out of numpy's reach); the join runs on those rows and on all of them.

For the filter kernels: the device ms of the join's first phase (HIP events: k_wn_count, the scan,
k_wn_emit), the box tests they make (both kernels walk every (requested row, candidate row) pair), and
that time against the compute bound: tests x OPS_PER_TEST f64 operations over the f64 vector peak.
Writes one JSON document (--out).
Usage: python tools/kbench_within.py [--out profiles/within_join.json] [--reps 5] [--only s a b c]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mosaic_amd import MosaicContext, SpatialKNN  # noqa: E402
from mosaic_amd.data import GOLDEN, PolygonSet, synthetic_buildings  # noqa: E402
from mosaic_amd.knn import knn_exact_batches, within_neighbours_last_ms  # noqa: E402

# dist::box_lower_bound and its comparison, counted as f64 vector operations: 8 compares + 4 subtractions
# + 4 selects for dx / dy, 4 compares / selects + 2 subtractions for the extents, 2 multiplications + 1
# addition + 1 square root for the gap, 2 multiplications + 1 addition + 1 subtraction for the bound, 1 compare
OPS_PER_TEST = 31
# MI355X: 157.3 TFLOPS f32 vector (the microarchitecture notes); AMD's datasheet gives the f64 vector rate as half of it
F64_VECTOR_PEAK = 78.6e12


def stats(ms):
    ms = sorted(ms)
    return {"best_ms": round(ms[0], 3), "median_ms": round(ms[len(ms) // 2], 3), "worst_ms": round(ms[-1], 3), "reps": len(ms)}


def alternate(fns, reps):
    """every function once per round, `reps` rounds after one warm-up round: ({name: [wall ms]}, {name: last result})"""
    out, res = {k: [] for k in fns}, {}
    for r in range(reps + 1):
        for k, fn in fns.items():
            t = time.perf_counter()
            res[k] = fn()
            if r:
                out[k].append((time.perf_counter() - t) * 1e3)
    return out, res


def boxes_of(ctx, tab):
    m = ctx.st_measures(tab, what=("xmin", "ymin", "xmax", "ymax"))
    return np.stack([np.asarray(m[k], np.float64) for k in ("xmin", "ymin", "xmax", "ymax")], axis=1)


def numpy_box_filter(lb, cb, radius, rows, cells_per_chunk=1 << 24):
    """all (landmark, candidate) pairs whose envelopes, the landmark's grown by its radius, meet"""
    step = max(1, cells_per_chunk // max(len(cb), 1))
    ls, cs = [], []
    for a in range(0, len(rows), step):
        r = rows[a:a + step]
        with np.errstate(over="ignore"):  # DBL_MAX grows to inf: every candidate
            grow = (radius[a:a + step] * (1 + 1e-9) + 1e-12)[:, None]
        b = lb[r]
        keep = ((cb[None, :, 0] - b[:, None, 2] <= grow) & (b[:, None, 0] - cb[None, :, 2] <= grow) &
                (cb[None, :, 1] - b[:, None, 3] <= grow) & (b[:, None, 1] - cb[None, :, 3] <= grow))
        i, c = np.nonzero(keep)
        ls.append(r[i])
        cs.append(c)
    return np.concatenate(ls).astype(np.int64), np.concatenate(cs).astype(np.int64)


def composition(ctx, ltab, rtab, lb, cb, radius, rows):
    l, c = numpy_box_filter(lb, cb, radius, rows)
    d = ctx.st_distance(ltab, rtab, pairs=(l, c)) if len(l) else np.zeros(0)
    at = np.searchsorted(rows, l)
    keep = d <= radius[at]
    l, c, d = l[keep], c[keep], d[keep]
    order = np.lexsort((c, d.view(np.int64), l))
    return l[order], c[order], d[order]


def join_in_batches(ctx, ltab, rtab, radius, rows, batches):
    parts, split = [], np.zeros(3)
    for a, b in batches:
        parts.append(ctx.st_dwithin_join(ltab, rtab, radius[a:b], rows[a:b]))
        split += within_neighbours_last_ms()
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), split


def compare(ctx, name, ltab, rtab, radius, rows, reps, pair_budget=1 << 24):
    """the join against the composition on the given rows"""
    lb, cb = boxes_of(ctx, ltab), boxes_of(ctx, rtab)
    counts = ctx.st_dwithin_candidates(ltab, rtab, radius, rows)
    batches = knn_exact_batches(counts, pair_budget)
    splits = []

    def join():
        got, split = join_in_batches(ctx, ltab, rtab, radius, rows, batches)
        splits.append(split)
        return got

    ms, res = alternate({"join": join, "composition": lambda: composition(ctx, ltab, rtab, lb, cb, radius, rows)}, reps)
    got, want = res["join"], res["composition"]
    same = all(np.array_equal(g.view(np.int64), w.view(np.int64)) for g, w in zip(got, want))
    split = min(splits[1:], key=lambda s: s.sum())
    tests = 2 * len(rows) * len(cb)  # k_wn_count and k_wn_emit each walk every pair
    bound_ms = tests * OPS_PER_TEST / F64_VECTOR_PEAK * 1e3
    doc = {"case": name, "rows": int(len(rows)), "candidates": int(len(cb)), "batches": len(batches),
           "candidate_pairs": int(counts.sum()), "pairs_within": int(len(got[0])), "same_rows": bool(same),
           "join_wall": stats(ms["join"]), "composition_wall": stats(ms["composition"]),
           "join_over_composition_best": round(min(ms["join"]) / min(ms["composition"]), 4),
           "join_device_ms": {"filter_and_self": round(float(split[0]), 3), "distance_and_select": round(float(split[1]), 3),
                              "order": round(float(split[2]), 3)},
           "filter_kernels": {"box_tests": int(tests), "ops_per_test": OPS_PER_TEST, "f64_vector_peak_flops": F64_VECTOR_PEAK,
                              "device_ms_count_scan_emit": round(float(split[0]), 3), "compute_bound_ms": round(bound_ms, 4),
                              "bound_over_device": round(bound_ms / max(float(split[0]), 1e-9), 4),
                              "bound_that_applies": "compute (f64 vector): each candidate box is read once per workgroup from L2 "
                                                    "and tested by 256 lanes, 32 bytes per 256 tests"}}
    print(json.dumps(doc), flush=True)
    return doc


def knn_workload(ctx, name, points, candidates, res, k, max_iterations, reps):
    doc = {"workload": name, "k_neighbours": k, "index_resolution": res, "max_iterations": max_iterations}
    with SpatialKNN(ctx, candidates, k_neighbours=k, index_resolution=res, max_iterations=max_iterations) as model:
        ms, out = alternate({"transform": lambda: model.transform(points), "transform_exact": lambda: model.transform_exact(points)},
                            max(2, reps // 2))
        doc["transform_wall"], doc["transform_exact_wall"] = stats(ms["transform"]), stats(ms["transform_exact"])
        doc["exact_stats"] = model.exact_stats
        doc["rows"] = {"transform": int(len(out["transform"]["distance"])), "transform_exact": int(len(out["transform_exact"]["distance"]))}
        radius = model.exact_radius.copy()
        ltab = ctx.geometry_table(points)
        doc["within_join_at_the_exact_radii"] = compare(ctx, name, ltab, model._right.table, radius,
                                                        np.arange(len(radius), dtype=np.int64), reps)
        ltab.close()
    print(json.dumps({k: v for k, v in doc.items() if k != "within_join_at_the_exact_radii"}), flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=200)
    ap.add_argument("--trips", type=int, default=20000)
    ap.add_argument("--buildings", type=float, default=2e5)
    ap.add_argument("--radius", type=float, default=1e-4, help="workload (c): degrees, about 10 m")
    ap.add_argument("--comp-rows", type=int, default=2000)
    ap.add_argument("--only", nargs="*", default=["a", "b", "c"])
    a = ap.parse_args()
    ctx = MosaicContext.build("H3", "JTS")
    p = np.load(os.path.join(GOLDEN, "nyctaxi_yellow_trips_pickups.npy"))
    rng = np.random.default_rng(20250301)
    x = np.repeat(p[:, 0], a.scale) + rng.normal(0, 0.01, len(p) * a.scale)
    y = np.repeat(p[:, 1], a.scale) + rng.normal(0, 0.01, len(p) * a.scale)
    docs = []
    if "s" in a.only:  # a size at which every figure is an overhead
        ltab, rtab = ctx.geometry_table((p[:, 0].copy(), p[:, 1].copy())), ctx.geometry_table(PolygonSet.load("nyc_taxi_zones"))
        docs.append({"workload": f"(s) the {len(p)} fixture pickups against 263 NYC taxi zones, radius 0.01 degrees",
                     "against_the_composition": compare(ctx, "(s)", ltab, rtab, np.full(len(p), 0.01), np.arange(len(p), dtype=np.int64),
                                                        a.reps)})
        ltab.close()
        rtab.close()
    if "a" in a.only:
        docs.append(knn_workload(ctx, f"(a) {len(x)} jittered pickups against 263 NYC taxi zones", (x, y),
                                 PolygonSet.load("nyc_taxi_zones"), 9, 5, 10, a.reps))
    if "b" in a.only:
        from tools.kbench_lines import trips

        docs.append(knn_workload(ctx, f"(b) {len(x)} jittered pickups against {a.trips} seeded trips", (x, y), trips(a.trips), 9, 5, 10,
                                 a.reps))
    if "c" in a.only:
        n = int(a.buildings)
        tab = ctx.geometry_table(synthetic_buildings(n))
        radius = np.full(n, a.radius)
        rows = np.arange(n, dtype=np.int64)
        m = min(a.comp_rows, n)
        doc = {"workload": f"(c) {n} synthetic buildings against themselves, radius {a.radius} degrees",
               "first_rows_against_the_composition": compare(ctx, f"(c) first {m} rows", tab, tab, radius[:m], rows[:m], a.reps)}
        ms, res = alternate({"join": lambda: (ctx.st_dwithin_join(tab, tab, radius), within_neighbours_last_ms())}, a.reps)
        got, split = res["join"]
        tests = 2 * n * n
        bound_ms = tests * OPS_PER_TEST / F64_VECTOR_PEAK * 1e3
        doc["all_rows"] = {"pairs_within": int(len(got[0])), "join_wall": stats(ms["join"]),
                           "join_device_ms": {"filter_and_self": round(split[0], 3), "distance_and_select": round(split[1], 3),
                                              "order": round(split[2], 3)},
                           "filter_kernels": {"box_tests": tests, "ops_per_test": OPS_PER_TEST, "compute_bound_ms": round(bound_ms, 3),
                                              "bound_over_device": round(bound_ms / max(split[0], 1e-9), 4)},
                           "composition": "not measured: 4e10 envelope pairs are out of numpy's reach"}
        print(json.dumps(doc["all_rows"]), flush=True)
        docs.append(doc)
        tab.close()
    ctx.close()
    text = json.dumps({"device": "one MI355X, one session, whole calls timed with a host clock around calls that end in a device "
                                 "synchronise, device ms from HIP events", "workloads": docs}, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
