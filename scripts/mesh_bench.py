"""Mesher measurement (not part of bench.py): fuse the benchmark stream, then time the GPU mesher on the resulting layer.

    python scripts/mesh_bench.py [--frames N] [--reps R] [--warmup W] [--cpu-ref] [--only 0.05,0.02,0.01]

Per layer (5 cm and 1 cm at 640x480, 2 cm at 1280x720 -- configs[3]'s shape): blocks and triangles; the two mesh kernels'
HIP-event time (count + write) and the whole cox_meshlayer_from_layer call, median and spread over R calls after W warm-up
calls, one mesher in flight; the modelled HBM bytes of the two kernels and their share of the 8 TB/s peak; the connected-mesh
time; with --cpu-ref the single-thread time of the test-side reference (tests/cpp/mesh_reference.cpp) beside them.
One JSON line per layer.

Modelled bytes: the count pass reads every allocated block once (48 KiB of voxel words; the +x/+y/+z
neighbour samples are the next blocks' own words and are served from L2/MALL); the write pass reads the blocks with triangles
once more and writes 27 B per vertex (12 position + 12 normal + 3 colour).
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
BLOCK_BYTES = 4096 * 12

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

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--only", default="0.05,0.02,0.01")
    args = ap.parse_args()
    import coxgraph_amd
    from coxgraph_amd.capi import MeshLayer
    eng = coxgraph_amd.load_engine()
    ref = None
    if args.cpu_ref:
        import mesh_ref
        out_dir = os.path.join(ROOT, "build")
        os.makedirs(out_dir, exist_ok=True)
        ref = mesh_ref.build(out_dir)
    shapes = {0.05: (640, 480), 0.02: (1280, 720), 0.01: (640, 480)}
    for voxel in [float(v) for v in args.only.split(",")]:
        w, h = shapes[voxel]
        layer, integ = fuse(eng, voxel, args.frames, w, h)
        nb_alloc = layer.n_blocks()
        kern, wall = [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            m = MeshLayer.from_layer(eng, layer, min_weight=1e-4)
            t1 = time.perf_counter()
            _, ms = m.stats()
            if i >= args.warmup:
                kern.append(ms)
                wall.append(1e3 * (t1 - t0))
            nb, ntri, nv = m.n_blocks, m.n_triangles, m.n_vertices
            if i < args.warmup + args.reps - 1:
                m.close()
        conn = []
        for i in range(args.warmup + min(args.reps, 5)):
            t0 = time.perf_counter()
            c = MeshLayer.connected(eng, [m], None, 0.5 * voxel)
            if i >= args.warmup:
                conn.append(1e3 * (time.perf_counter() - t0))
        count_ms = statistics.median(k[0] for k in kern)
        write_ms = statistics.median(k[1] for k in kern)
        bytes_count = nb_alloc * BLOCK_BYTES
        bytes_write = nb * BLOCK_BYTES + 27 * nv
        rec = dict(voxel=voxel, shape=[w, h], frames=args.frames, blocks=nb_alloc, mesh_blocks=nb, triangles=ntri, connected_vertices=len(c["xyz"]),
                   count_kernel_ms=round(count_ms, 4), write_kernel_ms=round(write_ms, 4),
                   kernel_ms_min_max=[round(min(k[0] + k[1] for k in kern), 4), round(max(k[0] + k[1] for k in kern), 4)],
                   from_layer_call_ms=round(statistics.median(wall), 3), connected_ms=round(statistics.median(conn), 3),
                   modelled_bytes=dict(count=bytes_count, write=bytes_write),
                   hbm_fraction=dict(count=round(bytes_count / (count_ms * 1e-3) / (HBM_PEAK_GBPS * 1e9), 4),
                                     write=round(bytes_write / (write_ms * 1e-3) / (HBM_PEAK_GBPS * 1e9), 4),
                                     both=round((bytes_count + bytes_write) / ((count_ms + write_ms) * 1e-3) / (HBM_PEAK_GBPS * 1e9), 4)),
                   reps=args.reps, warmup=args.warmup)
        if ref is not None:
            idx, vox = layer.download()
            r = ref.mesh(voxel, idx, vox, 1e-4)
            rec["cpu_reference_single_thread_ms"] = round(1e3 * r["seconds"], 1)
            rec["cpu_reference_same_triangles"] = bool(len(r["xyz"]) == nv)
        print(json.dumps(rec), flush=True)
        m.close()
        integ.close()
        layer.close()

if __name__ == "__main__":
    main()
