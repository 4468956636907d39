"""Renderer measurement (not part of bench.py): fuse the benchmark stream, then time cox_layer_render_dev on the resulting layer.

    python scripts/render_bench.py [--frames N] [--reps R] [--warmup W] [--cpu-ref] [--only 0.05,0.02,0.01] [--sizes 640x480,1280x720] [--out FILE]

Per layer (5 cm, 2 cm, 1 cm, fused from N frames at 640x480) and image size, from the pose of the middle frame: the kernel's
HIP-event time (cox_layer_render_dev on a torch stream, depth + normal + colour + status), median and spread over R calls
after W warm-up calls; samples per ray and rays per second; with --cpu-ref the single-thread rate of the test-side reference
(tests/cpp/render_reference.cpp) on the same view at 5 cm.  One JSON line per case.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--only", default="0.05,0.02,0.01")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer
    eng = coxgraph_amd.load_engine()
    ref = None
    if args.cpu_ref:
        import render_ref
        out_dir = os.path.join(ROOT, "build")
        os.makedirs(out_dir, exist_ok=True)
        ref = render_ref.build(out_dir)
    stream = torch.cuda.Stream()
    T = synth.camera_pose(args.frames // 2)[2]
    for voxel in [float(v) for v in args.only.split(",")]:
        layer = Layer(eng, voxel, capacity_blocks=1 << 16)
        integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(voxel)), "merged")
        for t in range(args.frames):
            Tf, pts, rgba, _ = synth.make_frame(t)
            integ.integrate_points(Tf, pts, rgba)
        integ.sync()
        nb = layer.n_blocks()
        max_depth = synth.integrator_overrides(voxel)["max_ray_length_m"]
        for size in args.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            K = np.asarray(synth.INTRINSICS[(w, h)], np.float32)
            d = torch.empty((h, w), device="cuda")
            n = torch.empty((h, w, 3), device="cuda")
            c = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            st = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            kern = []
            for i in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record(stream)
                    layer.render_dev(T, w, h, K, depth=d, normal=n, rgba=c, status=st, stream=stream, max_depth=max_depth)
                    e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    kern.append(e0.elapsed_time(e1))
            host = layer.render(T, w, h, K, max_depth=max_depth)
            s = host["stats"]
            km = statistics.median(kern)
            line = dict(voxel=voxel, wh=[w, h], frames=args.frames, blocks=nb, max_depth=max_depth, rays=w * h, hit_share=s["n_hits"] / (w * h),
                        samples_per_ray=s["n_samples"] / (w * h), block_skips_per_ray=s["n_block_skips"] / (w * h), budget=s["n_budget"],
                        kernel_ms_median=round(km, 4), kernel_ms_spread=[round(min(kern), 4), round(max(kern), 4)],
                        rays_per_s=w * h / (km * 1e-3), samples_per_s=s["n_samples"] / (km * 1e-3))
            if ref is not None and voxel == 0.05 and (w, h) == (640, 480):
                r = ref.layer(voxel, *layer.download()).render(T, w, h, K, max_depth=max_depth)
                line["cpu_ref_rays_per_s"] = w * h / r["stats"]["seconds"]
                line["gpu_over_cpu_ref"] = line["rays_per_s"] / line["cpu_ref_rays_per_s"]
            out = json.dumps(line)
            print(out, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(out + "\n")
        del layer, integ


if __name__ == "__main__":
    main()
