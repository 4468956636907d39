"""Layer-compare measurement (not part of bench.py): two 150-frame submaps of the synthetic stream, then cox_compare_run for 1, 8 and
64 transforms in both sample modes, beside the only route the engine offered before it.

    python scripts/compare_bench.py [--frames N] [--voxel V] [--reps R] [--warmup W] [--out FILE]

Submap A fuses frames 0 .. N-1, submap B frames N/2 .. N/2 + N-1, both with `merged`.  The transforms are small seeded 6-DoF
perturbations of the identity (the candidates a search hands over sit around one pose).

  compare    LayerComparer.run: HIP-event time of its kernels and wall time of the call, median, min and max over R runs after W
             warm-ups.  The rate is bytes of A and B words read per second of kernel time, counted from the records: per transform
             8 bytes (distance, weight) for every observed voxel of A, and for every overlapping voxel the words of B behind its
             sample, 8 bytes for NEAREST and 8 corners x 8 bytes for TRILINEAR.  Samples that fail early read less and are not counted.
  parent     the route before this unit, once, for ONE transform: cox_layer_merge of A into an empty layer under T_B_A (a resample
             onto B's grid), two downloads, and numpy over the blocks both layers have.  Wall time.  It resamples B's grid out of A
             where the compare samples B at A's voxels, so its counts are those of a similar, not the same, comparison.

One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def spread(ms):
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer, LayerComparer, words_to_fields
    eng = coxgraph_amd.load_engine()

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    def submap(first):
        layer = Layer(eng, args.voxel, capacity_blocks=1 << 16)
        integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(args.voxel)), "merged")
        for t in range(first, first + args.frames):
            T, pts, rgba, _ = synth.make_frame(t)
            integ.integrate_points(T, pts, rgba)
        integ.sync()
        return layer

    A, B = submap(0), submap(args.frames // 2)
    rng = np.random.default_rng(31)
    T = np.zeros((64, 7), np.float32)
    for i in range(64):
        axis = rng.normal(size=3)
        angle = rng.uniform(-0.05, 0.05)
        qv = np.sin(0.5 * angle) * axis / np.linalg.norm(axis)
        T[i] = np.concatenate([[np.cos(0.5 * angle)], qv, rng.uniform(-0.1, 0.1, 3)])
    base = dict(voxel=args.voxel, frames=args.frames, blocks_a=A.stats()[0], blocks_b=B.stats()[0])
    cmp = LayerComparer(eng, A, B)
    for sample, per_overlap in (("nearest", 8), ("trilinear", 64)):
        for n in (1, 8, 64):
            wall, kern = [], []
            for i in range(args.warmup + args.reps):
                cmp.kernel_time(reset=True)
                t0 = time.perf_counter()
                rec = cmp.run(T[:n], "all", sample)
                t1 = time.perf_counter()
                if i >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    kern.append(cmp.kernel_time()[0])
            nbytes = int(8 * rec["n_a_observed"].astype(np.int64).sum() + per_overlap * rec["n_overlap"].astype(np.int64).sum())
            k, w = spread(kern), spread(wall)
            emit(dict(base, case="compare", sample=sample, transforms=n, bytes_read=nbytes, observed_a=int(rec["n_a_observed"][0]), overlap_first=int(rec["n_overlap"][0]),
                      kernel=dict(k, gbytes_per_s=nbytes / (k["ms_median"] * 1e-3) / 1e9), wall=dict(w, gbytes_per_s=nbytes / (w["ms_median"] * 1e-3) / 1e9)))
    # the parent commit's only route, once, one transform
    t0 = time.perf_counter()
    tmp = Layer(eng, args.voxel, capacity_blocks=1 << 16)
    tmp.merge_from(A, T[0])
    ia, va = tmp.download()
    ib, vb = B.download()
    rows = {tuple(int(v) for v in i): j for j, i in enumerate(ib)}
    pairs = [(j, rows[tuple(int(v) for v in i)]) for j, i in enumerate(ia) if tuple(int(v) for v in i) in rows]
    ja, jb = (np.array(p, np.int64) for p in zip(*pairs)) if pairs else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    da, wa, _ = words_to_fields(va[ja])
    db, wb, _ = words_to_fields(vb[jb])
    both = (wa > 1e-6) & (wb > 1e-6)
    e = np.abs(da - db)[both]
    s = np.float32(args.voxel)
    conflicts = int(((np.abs(da) <= s) & (db >= 2 * s) & both).sum() + ((np.abs(db) <= s) & (da >= 2 * s) & both).sum())
    ms = (time.perf_counter() - t0) * 1e3
    emit(dict(base, case="parent_route", transforms=1, wall_ms=round(ms, 2), overlap=int(both.sum()), rmse=float(np.sqrt(np.mean(e.astype(np.float64) ** 2))) if len(e) else None,
              conflicts=conflicts, common_blocks=len(pairs)))


if __name__ == "__main__":
    main()
