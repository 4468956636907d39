"""Map-query measurement (not part of bench.py): fuse the benchmark stream, then time cox_layer_query on the resulting layer.

    python scripts/query_bench.py [--frames N] [--queries Q] [--reps R] [--warmup W] [--cpu-ref] [--only 0.05,0.02,0.01] [--out FILE]

Per layer (5 cm and 1 cm at 640x480, 2 cm at 1280x720 -- configs[3]'s shape), per query set (surface band: the layer's
registration voxels plus N(0, voxel / 2) noise; uniform in the box of those voxels grown by 1 m) and per mode (interpolated
distance; adaptive with gradient; nearest distance): the kernel's HIP-event time (cox_layer_query_dev on a torch stream) and
the whole host call (cox_layer_query, host buffers in and out), median and spread over R runs after W warm-up runs; queries/s;
the modelled bytes and their share of the 8 TB/s peak; with --cpu-ref (5 cm only) the single-thread rate of the test-side
reference (tests/cpp/map_reference.cpp) on 200 k of the same queries.  One JSON line per case.

Modelled bytes per query: per sample 8 voxels x 8 B (distance + weight words), one hash probe (16 B)
per query, 16 B of I/O (12 B point in, 4 B distance out).  A distance query is 1 sample, a query with gradient 7.
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

HBM_PEAK_GBPS = 8000.0
CASES = (("interpolate", False), ("adaptive", True), ("nearest", False))


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


def query_sets(layer, voxel, n, rng):
    surf = layer.registration_points(1.0, voxel)[:, :3]
    band = (surf[rng.integers(0, len(surf), n)] + rng.normal(0, 0.5 * voxel, size=(n, 3))).astype(np.float32)
    lo, hi = surf.min(axis=0) - 1.0, surf.max(axis=0) + 1.0
    uniform = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    return {"band": band, "uniform": uniform}


def spread(v):
    return [round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--queries", type=int, default=4 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--only", default="0.05,0.02,0.01")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    eng = coxgraph_amd.load_engine()
    ref = None
    if args.cpu_ref:
        import map_ref
        out_dir = os.path.join(ROOT, "build")
        os.makedirs(out_dir, exist_ok=True)
        ref = map_ref.build(out_dir)
    shapes = {0.05: (640, 480), 0.02: (1280, 720), 0.01: (640, 480)}
    rng = np.random.default_rng(5)
    stream = torch.cuda.Stream()
    for voxel in [float(v) for v in args.only.split(",")]:
        w, h = shapes[voxel]
        layer, integ = fuse(eng, voxel, args.frames, w, h)
        nb = layer.n_blocks()
        ref_layer = None
        if ref is not None and voxel == 0.05:
            idx, vox = layer.download()
            ref_layer = ref.layer(voxel, idx, vox)
        for set_name, q in query_sets(layer, voxel, args.queries, rng).items():
            n = len(q)
            x = torch.from_numpy(q).cuda()
            d = torch.empty(n, device="cuda")
            wt = torch.empty(n, device="cuda")
            g = torch.empty((n, 3), device="cuda")
            st = torch.empty(n, dtype=torch.uint8, device="cuda")
            for mode, grad in CASES:
                kern, wall = [], []
                for i in range(args.warmup + args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        layer.query_dev(x, mode=mode, gradient=grad, distance=d, grad=g if grad else None, status=st, stream=stream)
                        e1.record(stream)
                    e1.synchronize()
                    t0 = time.perf_counter()
                    out = layer.query(q, mode, gradient=grad)
                    t1 = time.perf_counter()
                    if i >= args.warmup:
                        kern.append(e0.elapsed_time(e1))
                        wall.append(1e3 * (t1 - t0))
                km, wm = statistics.median(kern), statistics.median(wall)
                samples = 7 if grad else 1
                bytes_q = samples * 64 + 16 + 16 + (12 if grad else 0)
                line = dict(voxel=voxel, wh=[w, h], frames=args.frames, blocks=nb, set=set_name, mode=mode, gradient=grad, queries=n,
                            valid=float(np.mean(out["status"] & 1 > 0)), trilinear=float(np.mean(out["status"] & 2 > 0)),
                            kernel_ms_median=round(km, 4), kernel_ms_spread=spread(kern), call_ms_median=round(wm, 3), call_ms_spread=spread(wall),
                            kernel_queries_per_s=n / (km * 1e-3), call_queries_per_s=n / (wm * 1e-3), model_bytes_per_query=bytes_q,
                            model_gbps=n * bytes_q / (km * 1e-3) / 1e9)
                line["model_frac_of_peak"] = line["model_gbps"] / HBM_PEAK_GBPS
                if ref_layer is not None:
                    m = min(n, 200_000)
                    r = ref_layer.query(q[:m], mode, gradient=grad)
                    line["cpu_ref_queries_per_s"] = m / r["seconds"]
                    line["gpu_over_cpu_ref"] = line["kernel_queries_per_s"] / line["cpu_ref_queries_per_s"]
                s = json.dumps(line)
                print(s, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(s + "\n")
        del layer, integ


if __name__ == "__main__":
    main()
