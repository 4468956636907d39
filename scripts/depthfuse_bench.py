"""Depth-image fusion measurement (not part of bench.py): the benchmark's 640x480 depth stream into a fresh layer, frame by frame.

    python scripts/depthfuse_bench.py --integrator depthfuse|merged [--only 0.05,0.02] [--frames N] [--warmup W] [--repeats R] [--out FILE]

ONE integrator per process: `depthfuse` is the voxel-projective integrator of DESIGN.md section 7m (cox_depthfuse_integrate_dev),
`merged` the ray caster fed the same device images through cox_integrate_depth_dev, as the comparison.  They are never both in
one process, and there is no 1 cm shape (section 7m says why).  Per voxel size: W warm-up frames, then N frames in a timed window
that ends in a sync -- R times, each on a fresh layer, for the spread.  For `depthfuse` one more pass reads the statistics after
every frame (a sync per frame, so it is not timed): candidate, touched and new blocks and the frame's HIP-event kernel time; the
wall time per frame of the timed window minus that kernel time is what the frame's single host read costs.  One JSON line per case.
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

W, H = 640, 480
BLOCK_BYTES = 2 * 4096 * 12  # a touched block is read and written once: 96 KB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--integrator", choices=("depthfuse", "merged"), required=True)
    ap.add_argument("--only", default="0.05,0.02")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer
    eng = coxgraph_amd.load_engine()
    K = np.asarray(synth.INTRINSICS[(W, H)], np.float32)
    n_frames = args.warmup + args.frames
    poses, depths = [], []
    for t in range(n_frames):
        T, _, _, depth = synth.make_frame(t)
        poses.append(T)
        depths.append(torch.from_numpy(np.ascontiguousarray(depth)).cuda())
    rgba = torch.from_numpy(np.ascontiguousarray(synth.frame_colors(W, H))).cuda()
    torch.cuda.synchronize()
    for voxel in [float(v) for v in args.only.split(",")]:
        if voxel < 0.015:
            raise SystemExit("no 1 cm shape in this measurement (DESIGN.md section 7m)")
        ov = synth.integrator_overrides(voxel)

        def fresh():
            layer = Layer(eng, voxel, capacity_blocks=1 << 15)
            if args.integrator == "depthfuse":
                integ = layer.depth_integrator(truncation_distance=ov["default_truncation_distance"], max_weight=ov["max_weight"], min_depth_m=ov["min_ray_length_m"],
                                               max_depth_m=ov["max_ray_length_m"], voxel_carving_enabled=ov["voxel_carving_enabled"],
                                               use_const_weight=ov["use_const_weight"], use_weight_dropoff=ov["use_weight_dropoff"])
                step = lambda t: integ.integrate_dev(poses[t], depths[t], rgba, W, H, K)  # noqa: E731
            else:
                integ = Integrator(eng, layer, eng.default_config(**ov), "merged")
                step = lambda t: integ.integrate_depth_dev(poses[t], depths[t].data_ptr(), rgba.data_ptr(), W, H, K)  # noqa: E731
            return layer, integ, step

        fps, blocks = [], 0
        for _ in range(args.repeats):
            layer, integ, step = fresh()
            for t in range(args.warmup):
                step(t)
            integ.sync()
            t0 = time.perf_counter()
            for t in range(args.warmup, n_frames):
                step(t)
            integ.sync()
            fps.append(args.frames / (time.perf_counter() - t0))
            blocks = layer.n_blocks()
            integ.close()
            layer.close()
        line = dict(integrator=args.integrator, voxel=voxel, wh=[W, H], warmup=args.warmup, frames=args.frames, repeats=args.repeats, blocks=blocks,
                    frames_per_s_median=round(statistics.median(fps), 1), frames_per_s_spread=[round(min(fps), 1), round(max(fps), 1)],
                    wall_ms_per_frame=round(1e3 / statistics.median(fps), 4))
        if args.integrator == "depthfuse":
            layer, integ, step = fresh()
            per = []
            for t in range(n_frames):
                step(t)
                st = integ.last_stats()
                if t >= args.warmup:
                    per.append(st)
            mean = lambda k: statistics.fmean(s[k] for s in per)  # noqa: E731
            line.update(candidate_blocks=round(mean("n_candidate_blocks"), 1), touched_blocks=round(mean("n_touched_blocks"), 1),
                        new_blocks=round(mean("n_new_blocks"), 2), updated_voxels=round(mean("n_updated_voxels")), kernel_ms_per_frame=round(mean("kernel_ms"), 4),
                        host_read_ms_per_frame=round(line["wall_ms_per_frame"] - mean("kernel_ms"), 4), update_bytes_per_frame=round(mean("n_touched_blocks") * BLOCK_BYTES))
            integ.close()
            layer.close()
        out = json.dumps(line)
        print(out, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(out + "\n")


if __name__ == "__main__":
    main()
