"""Pose-candidate sweep measurement (not part of bench.py): fuse the benchmark stream at 5 cm, take the submap's isosurface
registration points and its ESDF, then time cox_align_sweep on it against the only route the engine offered before it.

    python scripts/align_bench.py [--frames N] [--voxel V] [--samples M] [--reps R] [--warmup W] [--tsdf] [--out FILE]

Per case -- the level-0 grid of a search (+-1.2 m, +-0.4 m, +-170 deg in steps of 0.4 m and 10 deg: 5 145 candidates) and one
refinement level (8 kept poses x 81: 648 candidates), both on M stored samples of the point set:

  sweep      SubmapAligner.sweep: wall time of the call (pose upload, launch, download) and HIP-event time of its kernels, median,
             min and max over R runs after W warm-ups; point evaluations (candidates x samples) per second of each.
  loop       the same candidates scored one by one with Registration.normal_eq (one launch and one synchronisation each), wall time.
             The costs of both routes are compared (max relative difference).
  search     the whole coarse-to-fine search (4 refinement levels, keep 8), wall time.

One JSON line per case.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HALF = (1.2, 1.2, 0.4, math.radians(170.0))
STEP = (0.4, 0.4, 0.4, math.radians(10.0))


def spread(ms):
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--tsdf", action="store_true", help="read the TSDF instead of the ESDF")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer, RegPoints, Registration, SubmapAligner, align_grid
    eng = coxgraph_amd.load_engine()

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    layer = Layer(eng, args.voxel, capacity_blocks=1 << 16)
    integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(args.voxel)), "merged")
    for t in range(args.frames):
        T, pts, rgba, _ = synth.make_frame(t)
        integ.integrate_points(T, pts, rgba)
    integ.sync()
    reading = layer if args.tsdf else layer.esdf(max_distance_m=2.0)
    ref = RegPoints.from_isosurface(eng, layer)
    rng = np.random.default_rng(12)
    samples = rng.integers(0, ref.n, args.samples).astype(np.uint32)
    tau = 8 * args.voxel
    al = SubmapAligner(eng, ref, reading, inlier_distance=tau)
    al.set_samples(samples)
    reg = Registration(eng, ref, reading, 0.0)
    reg.set_samples(samples)
    zero = np.zeros(4)
    base = dict(voxel=args.voxel, frames=args.frames, blocks=layer.stats()[0], points=ref.n, samples=args.samples, reading="tsdf" if args.tsdf else "esdf",
                inlier_distance=tau)

    level0 = align_grid(eng, zero, HALF, STEP)
    rec0 = al.sweep(level0)
    kept = level0[np.argsort(-rec0["score"].astype(np.int64), kind="stable")[:8]]
    fine = np.concatenate([align_grid(eng, p, [s / 2 for s in STEP], [s / 2 for s in STEP]) for p in kept])
    for name, poses in (("level0", level0), ("refinement", fine)):
        M = len(poses)
        evals = M * args.samples
        wall, kern = [], []
        for i in range(args.warmup + args.reps):
            al.kernel_time(reset=True)
            t0 = time.perf_counter()
            rec = al.sweep(poses)
            t1 = time.perf_counter()
            if i >= args.warmup:
                wall.append((t1 - t0) * 1e3)
                kern.append(al.kernel_time()[0])
        loop = []
        for i in range(args.loop_reps):
            t0 = time.perf_counter()
            costs = np.array([reg.normal_eq(p, zero)[2] for p in poses])
            loop.append((time.perf_counter() - t0) * 1e3)
        w, k, lp = spread(wall), spread(kern), spread(loop)
        denom = np.maximum(np.abs(costs), 1e-300)
        emit(dict(base, case=name, candidates=M, point_evaluations=evals,
                  sweep_wall=dict(w, evaluations_per_s=evals / (w["ms_median"] * 1e-3)), sweep_kernel=dict(k, evaluations_per_s=evals / (k["ms_median"] * 1e-3)),
                  loop_wall=dict(lp, evaluations_per_s=evals / (lp["ms_median"] * 1e-3), us_per_candidate=lp["ms_median"] * 1e3 / M),
                  loop_over_sweep_wall=lp["ms_median"] / w["ms_median"], loop_over_sweep_kernel=lp["ms_median"] / k["ms_median"],
                  cost_max_relative_difference=float(np.max(np.abs(rec["cost"] - costs) / denom)), best_score=int(rec["score"].max())))
    ms = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = al.search(zero, HALF, STEP, levels=4, keep=8, min_corr=args.samples // 4, tau_min=2 * args.voxel)
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    emit(dict(base, case="search", levels=4, keep=8, candidates=len(level0) + 4 * 648, wall=spread(ms), best=[float(v) for v in out["best"]] if out["n_found"] else None,
              best_record=[int(out["scores"][0][k]) for k in ("score", "n_corr", "n_inlier")] if out["n_found"] else None))


if __name__ == "__main__":
    main()
