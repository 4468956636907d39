"""Scan-to-map registration measurement (not part of bench.py): fuse a stretch of the benchmark stream, then time the tracker on it.

    python scripts/track_bench.py [--frames 80:121] [--reps R] [--warmup W] [--only 0.05,0.01] [--strides 1,4] [--min-inlier-ratio 0.1] [--out FILE]

Per layer (5 cm and 1 cm, fused from the given frames at 640x480), stride and parameterisation, with the depth image of the middle
frame as the scan and a prior 1 voxel / 1 degree off: the HIP-event time of ONE iteration (a tracker with max_iterations = 1: one
launch of k_track_step), of a whole refine call (all launches, the idle ones after the stop included) and its wall time, median and
spread over R calls after W warm-up calls.  Beside it the event time of k_query<INTERPOLATE> (cox_layer_query_dev, distance only) over
the same p_G: the same gather without the sums, the natural floor of an iteration.  min_inlier_ratio is lowered from its default
(0.3) to 0.1: the 1 cm configuration fuses rays of up to 3 m only, so a third of this view meets the map, and the default would stop
the loop as lost.  One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="80:121")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="0.05,0.01")
    ap.add_argument("--strides", default="1,4")
    ap.add_argument("--min-inlier-ratio", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    import track_ref
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer, Tracker
    eng = coxgraph_amd.load_engine()
    f0, f1 = (int(x) for x in args.frames.split(":"))
    mid = (f0 + f1) // 2
    T, pts, _, depth = synth.make_frame(mid)
    w, h = 640, 480
    d_depth = torch.from_numpy(depth).cuda()
    stream = torch.cuda.Stream()
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    for voxel in [float(v) for v in args.only.split(",")]:
        layer = Layer(eng, voxel, capacity_blocks=1 << 16)
        integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(voxel)), "merged")
        for t in range(f0, f1):
            Tf, p, rgba, _ = synth.make_frame(t)
            integ.integrate_points(Tf, p, rgba)
        integ.sync()
        nb = layer.n_blocks()
        for dof in (4, 6):
            T0 = track_ref.start_pose(T, voxel, dof, 1.0, 1.0)
            for stride in [int(s) for s in args.strides.split(",")]:
                one = Tracker(eng, layer, dof=dof, stride=stride, max_iterations=1, min_inlier_ratio=args.min_inlier_ratio)
                full = Tracker(eng, layer, dof=dof, stride=stride, min_inlier_ratio=args.min_inlier_ratio)
                it_ms, call_ms, wall_ms = [], [], []
                res = None
                for i in range(args.warmup + args.reps):
                    a = one.refine_depth_dev(T0, d_depth, w, h)
                    t0 = time.perf_counter()
                    res = full.refine_depth_dev(T0, d_depth, w, h)
                    t1 = time.perf_counter()
                    if i >= args.warmup:
                        it_ms.append(a["kernel_ms"])
                        call_ms.append(res["kernel_ms"])
                        wall_ms.append((t1 - t0) * 1e3)
                # the interpolated query over the same p_G
                ev = one.evaluate(T0, synth.depth_to_points(depth))
                cons = (ev["status"] & 1) != 0
                pg = torch.from_numpy(np.ascontiguousarray(ev["pG"][cons])).cuda()
                dist = torch.empty(len(pg), device="cuda")
                st = torch.empty(len(pg), dtype=torch.uint8, device="cuda")
                q_ms = []
                for i in range(args.warmup + args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        layer.query_dev(pg, mode="interpolate", distance=dist, status=st, stream=stream)
                        e1.record(stream)
                    e1.synchronize()
                    if i >= args.warmup:
                        q_ms.append(e0.elapsed_time(e1))
                n_cand = -(-w * h // stride)
                line = dict(voxel=voxel, wh=[w, h], frames=[f0, f1], blocks=nb, dof=dof, stride=stride, candidates=n_cand,
                            considered=res["first_n_considered"], used=res["first_n_used"], status=res["status_name"], iterations=res["iterations"],
                            max_iterations=int(full.cfg.max_iterations), min_inlier_ratio=args.min_inlier_ratio, iteration_ms_median=med(it_ms), iteration_ms_spread=[round(min(it_ms), 4), round(max(it_ms), 4)],
                            refine_kernel_ms_median=med(call_ms), refine_kernel_ms_spread=[round(min(call_ms), 4), round(max(call_ms), 4)],
                            refine_wall_ms_median=med(wall_ms), query_points=len(pg), query_ms_median=med(q_ms),
                            query_ms_spread=[round(min(q_ms), 4), round(max(q_ms), 4)],
                            candidates_per_s=n_cand / (statistics.median(it_ms) * 1e-3))
                out = json.dumps(line)
                print(out, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(out + "\n")
        del layer, integ


if __name__ == "__main__":
    main()
