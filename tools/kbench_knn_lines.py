"""SpatialKNN timing with line candidates: points as landmarks against the seeded trips of
tools/kbench_lines.py (20,000 random walks of 50 vertices in the NYC bbox) at H3 res 9, k = 5 -- "the k
nearest trips to each point", the reference's documented KNN case with the sides' kinds swapped in
(docs/source/models/spatial-knn.rst:113-152).  The landmarks are --scale seeded jittered copies of each
pickup of the fixture (the generator of tools/kbench_ring_neighbours.py).

Reports the wall ms of the candidates' preparation (geometry column, lineFill chips, cell index: once per
model), of transform (best of --reps, the landmarks' column and chips included), the iterations run and
the active landmarks of each, and the matches.  There is no earlier GPU form to compare with; the host
figure is the brute force a caller without the model would run: dist::distance of every (landmark,
trip) pair on --host-threads threads, measured on --check seeded landmarks and scaled to all of them.
The same sample gives the quality of the approximate model: the share of sampled landmarks whose
neighbours are exactly the k nearest trips, and the GPU distances' bits against the host's.
Writes one JSON document (--out).
Usage: python tools/kbench_knn_lines.py [--out profiles/knn_lines.json] [--reps 3] [--scale 200] [--trips 20000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mosaic_amd import MosaicContext, SpatialKNN  # noqa: E402
from mosaic_amd.data import GOLDEN  # noqa: E402
from tools.kbench_lines import trips as make_trips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=200)
    ap.add_argument("--trips", type=int, default=20000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--res", type=int, default=9)
    ap.add_argument("--max-iterations", type=int, default=10)
    ap.add_argument("--check", type=int, default=200)
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    from tests.test_st_distance_lines import LCol, host_distance

    ctx = MosaicContext.build("H3", "JTS")
    trips = make_trips(a.trips)
    p = np.load(os.path.join(GOLDEN, "nyctaxi_yellow_trips_pickups.npy"))
    rng = np.random.default_rng(20250301)
    x = np.repeat(p[:, 0], a.scale) + rng.normal(0, 0.01, len(p) * a.scale)
    y = np.repeat(p[:, 1], a.scale) + rng.normal(0, 0.01, len(p) * a.scale)
    n = len(x)

    model = SpatialKNN(ctx, trips, k_neighbours=a.k, index_resolution=a.res, max_iterations=a.max_iterations)
    t0 = time.perf_counter()
    model._prepare()
    prepare_ms = (time.perf_counter() - t0) * 1e3
    model.transform((x, y))  # warm-up (code objects, allocations)
    best, got = float("inf"), None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = model.transform((x, y))
        best = min(best, (time.perf_counter() - t0) * 1e3)
    per_landmark = np.bincount(got["landmark_row"], minlength=n)
    doc = {"workload": f"{n} points ({a.scale} jittered copies of each pickup, sigma 0.01 degrees) as landmarks against "
                       f"{len(trips)} seeded trips of 50 vertices, H3 res {a.res}, k = {a.k}, max_iterations {a.max_iterations}",
           "landmarks": n, "candidates": len(trips), "candidate_chips": int(len(model._right.index_id)),
           "cell_index": model._index.info(), "prepare_candidates_wall_ms": round(prepare_ms, 1),
           "transform_wall_ms": round(best, 1), "iterations": len(model.active_sets),
           "active_landmarks": [int(len(s)) for s in model.active_sets], "matches": int(len(got["distance"])),
           "landmarks_with_k": int((per_landmark >= a.k).sum()), "landmarks_without_a_match": int((per_landmark == 0).sum()),
           "metrics": model.metrics()}
    if a.check > 0:
        pick = np.sort(np.random.default_rng(11).choice(n, min(a.check, n), replace=False))
        li, ri = np.repeat(np.arange(len(pick)), len(trips)), np.tile(np.arange(len(trips)), len(pick))
        hp, ht = LCol.from_points(x[pick], y[pick]), LCol.from_lineset(trips)
        t0 = time.perf_counter()
        d = host_distance(hp, ht, li, ri, threads=a.host_threads).reshape(len(pick), len(trips))
        host_ms = (time.perf_counter() - t0) * 1e3
        exact, same_bits = 0, True
        for j, l in enumerate(pick.tolist()):
            m = got["landmark_row"] == l
            c, dd = got["candidate_row"][m], got["distance"][m]
            same_bits &= bool((d[j, c].view(np.int64) == dd.view(np.int64)).all())
            order = np.lexsort((np.arange(len(trips)), d[j]))[:a.k]
            exact += int(len(c) == a.k and np.array_equal(c, order))
        doc["check"] = {"sampled_landmarks": int(len(pick)), "host_threads": a.host_threads,
                        "host_all_pairs_ms_on_sample": round(host_ms, 1),
                        "host_all_pairs_ms_scaled_to_all_landmarks": round(host_ms * n / len(pick), 1),
                        "host_scaled_over_transform": round(host_ms * n / len(pick) / best, 1),
                        "gpu_distance_bits_equal_host": same_bits,
                        "landmarks_whose_neighbours_are_the_k_nearest": exact}
    model.close()
    ctx.close()
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
