"""View-gain measurement (not part of bench.py): fuse the benchmark stream, then time cox_viewgain_evaluate on the resulting layer.

    python scripts/viewgain_bench.py [--frames N] [--reps R] [--warmup W] [--only 0.05,0.01] [--batches 1,12,256,3072]
                                     [--workspace-mib M] [--cpu-ref] [--out FILE]

Per layer (the 150-frame 5 cm and 1 cm layers of scripts/query_bench.py) and per batch (1, 12, 256 and 3072 views: up to 256
positions x 12 yaw directions, the configured 35 x 96 ray grid with 5 m rays): the HIP-event time of the call's kernels
(cox_viewgain_stats.kernel_ms: box, clears, march launches, records), median and spread over R runs after W warm-up runs; views/s and
samples/s; the share of samples that fell into a voxel the view had already seen; the bitmap's bytes per view and the number of
chunks.  With --cpu-ref the single-thread time of the test-side reference (tests/cpp/viewgain_reference.cpp) on the 12-view batch,
the only CPU statement of this loop the repository has.  One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def fuse(eng, voxel, frames, w, h):
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer
    layer = Layer(eng, voxel, capacity_blocks=1 << 16)
    integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(voxel)), "merged")
    for t in range(frames):
        T, pts, rgba, _ = synth.make_frame(t, w=w, h=h)
        integ.integrate_points(T, pts, rgba)
    integ.sync()
    return layer, integ


def candidate_poses(n_positions, n_yaws, rng):
    """n_positions x n_yaws camera poses: positions uniform in the part of the room the stream's cameras stand in, 12 yaws each
    (ContinuousYawPlanningEvaluator), optical axis horizontal."""
    from coxgraph_amd import synth
    poses = []
    R_opt = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    for p in rng.uniform((-1.5, -1.5, 1.0), (3.0, 2.0, 2.0), size=(n_positions, 3)):
        for k in range(n_yaws):
            a = 2.0 * np.pi * k / n_yaws
            Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
            poses.append(np.concatenate([synth.quat_from_matrix(Rz @ R_opt), p]))
    return np.array(poses, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="0.05,0.01")
    ap.add_argument("--batches", default="1,12,256,3072")
    ap.add_argument("--workspace-mib", type=int, default=0, help="cox_viewgain_config.workspace_bytes in MiB (0: the default, 256)")
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd.capi import ViewGain
    eng = coxgraph_amd.load_engine()
    ref = None
    if args.cpu_ref:
        import viewgain_ref
        out_dir = os.path.join(ROOT, "build")
        os.makedirs(out_dir, exist_ok=True)
        ref = viewgain_ref.build(out_dir)
    poses = candidate_poses(256, 12, np.random.default_rng(5))
    for voxel in [float(v) for v in args.only.split(",")]:
        layer, integ = fuse(eng, voxel, args.frames, 640, 480)
        vg = ViewGain(eng, layer, workspace_bytes=args.workspace_mib << 20)
        for n in [int(b) for b in args.batches.split(",")]:
            batch = poses[:n]
            kern = []
            for i in range(args.warmup + args.reps):
                out = vg.evaluate(batch)
                if i >= args.warmup:
                    kern.append(out["stats"]["kernel_ms"])
            km = statistics.median(kern)
            samples, visible = out["stats"]["n_samples"], int(out["n_visible"].sum())
            line = dict(voxel=voxel, frames=args.frames, blocks=layer.n_blocks(), grid=[vg.cfg.w, vg.cfg.h], ray_length=vg.cfg.ray_length, views=n,
                        chunks=out["stats"]["n_chunks"], workspace_mib=args.workspace_mib or 256, bitmap_bytes_per_view=vg.view_bytes(),
                        samples=samples, samples_per_view=samples / n, visible_per_view=visible / n, duplicate_share=1.0 - visible / max(1, samples),
                        frontier_per_view=float(out["n_frontier"].mean()), occupied_per_view=float(out["n_occupied"].mean()),
                        kernel_ms_median=round(km, 4), kernel_ms_spread=[round(min(kern), 4), round(max(kern), 4)],
                        views_per_s=n / (km * 1e-3), samples_per_s=samples / (km * 1e-3))
            if ref is not None and n == 12:
                r = ref.layer(voxel, *layer.download()).evaluate(batch)
                line["cpu_ref_seconds"] = r["seconds"]
                line["cpu_ref_samples_per_s"] = float(r["n_samples"].sum()) / r["seconds"]
                line["gpu_over_cpu_ref"] = line["samples_per_s"] / line["cpu_ref_samples_per_s"]
            s = json.dumps(line)
            print(s, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(s + "\n")
        vg.close()
        del layer, integ


if __name__ == "__main__":
    main()
