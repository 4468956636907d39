"""Observation-history measurement (not part of bench.py).

    python scripts/history_bench.py [--frames N] [--reps R] [--warmup W] [--mesh-frames M] [--skip-mesh] [--out FILE]

One JSON line per case, appended to profiles/history_bench.jsonl (or --out):
  mark     k_obs_mark on one 640x480 frame per voxel size: HIP-event time on the caller's stream around cox_obs_record_dev (which
           makes that stream wait for the record's), median and spread over R runs after W warm-up runs, frames rotating so the
           marks are not all repeats; the modelled 12 B x points read and its share of the 8 TB/s peak; atomics before (one per
           marking point) and after the wave-level merge (one per distinct cell per wave).
  stream   `merged` at 5 cm over N frames through cox_integrate_points_async, with and without a history attached: frames/s
           (wall clock, whole stream, best of three), and the ratio.
  extract  the 1 cm / M-frame mesh: HIP-event time of k_tri_mask + scan as cox_meshlayer_history_size reports it and the whole
           cox_meshlayer_history call, next to the mesher's own kernel time.
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

HBM_PEAK_GBPS = 8000.0


def emit(line, path):
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(s + "\n")


def bench_mark(eng, torch, voxel, args, out):
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Layer, ObservationHistory
    ov = synth.integrator_overrides(voxel)
    layer = Layer(eng, voxel, capacity_blocks=64)
    obs = ObservationHistory(eng, layer, 1 << 15)
    frames = [synth.make_frame(5 * k)[:2] for k in range(8)]
    dev = [(T, torch.from_numpy(p).cuda()) for T, p in frames]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ms, counts = [], []
    for i in range(args.warmup + args.reps):
        T, x = dev[i % len(dev)]
        obs.set_frame(i % 256)
        c0 = obs.counts()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        obs.record_dev(T, x, ov["min_ray_length_m"], ov["max_ray_length_m"], stream=stream)
        e1.record(stream)
        e1.synchronize()
        c1 = obs.counts()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
            counts.append((c1[0] - c0[0], c1[1] - c0[1], x.shape[0]))
    obs.sync()
    med = statistics.median(ms)
    n = int(statistics.median(c[2] for c in counts))
    line = dict(case="mark", voxel=voxel, points=n, ms_median=round(med, 4), ms_spread=[round(min(ms), 4), round(max(ms), 4)], reps=args.reps,
                model_bytes=12 * n, model_gbps=12 * n / (med * 1e-3) / 1e9, atomics_before_merge=int(statistics.median(c[0] for c in counts)),
                atomics_after_merge=int(statistics.median(c[1] for c in counts)), **obs.stats())
    line["model_frac_of_peak"] = line["model_gbps"] / HBM_PEAK_GBPS
    emit(line, out)


def bench_stream(eng, torch, args, out):
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer, ObservationHistory
    voxel = 0.05
    frames = [synth.make_frame(t)[:3] for t in range(args.frames)]
    pinned = [(T, torch.from_numpy(p).pin_memory(), torch.from_numpy(c).pin_memory()) for T, p, c in frames]
    rates = {}
    for attached in (False, True, False, True, False, True):
        layer = Layer(eng, voxel, capacity_blocks=1 << 15)
        integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(voxel)), "merged")
        obs = ObservationHistory(eng, layer, 1 << 14)
        if attached:
            integ.attach_history(obs)
        for T, p, c in pinned[:3]:
            integ.integrate_points_async(T, p.data_ptr(), c.data_ptr(), p.shape[0])
        integ.sync()
        t0 = time.perf_counter()
        for k, (T, p, c) in enumerate(pinned):
            if attached:
                obs.set_frame(k % 256)
            integ.integrate_points_async(T, p.data_ptr(), c.data_ptr(), p.shape[0])
        integ.sync()
        obs.sync()
        rates.setdefault(attached, []).append(len(pinned) / (time.perf_counter() - t0))
        integ.attach_history(None)
        del integ, obs, layer
    line = dict(case="stream", method="merged", voxel=voxel, frames=args.frames, fps_without=[round(v, 1) for v in rates[False]],
                fps_attached=[round(v, 1) for v in rates[True]], attached_over_without=max(rates[True]) / max(rates[False]))
    emit(line, out)


def bench_extract(eng, torch, args, out):
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer, MeshLayer, ObservationHistory
    voxel = 0.01
    layer = Layer(eng, voxel, capacity_blocks=1 << 16)
    integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(voxel)), "merged")
    obs = ObservationHistory(eng, layer, 1 << 16)
    integ.attach_history(obs)
    for t in range(args.mesh_frames):
        T, pts, rgba, _ = synth.make_frame(t)
        obs.set_frame(t % 256)
        integ.integrate_points(T, pts, rgba)
    integ.sync()
    obs.sync()
    mesh = MeshLayer.from_layer(eng, layer, min_weight=1e-4)
    kern, call = [], []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        h = mesh.history(obs, with_time=True)
        t1 = time.perf_counter()
        if i >= args.warmup:
            kern.append(h["kernel_ms"])
            call.append(1e3 * (t1 - t0))
    line = dict(case="extract", voxel=voxel, frames=args.mesh_frames, triangles=mesh.n_triangles, history_words=int(len(h["history"])),
                mask_scan_ms_median=round(statistics.median(kern), 4), mask_scan_ms_spread=[round(min(kern), 4), round(max(kern), 4)],
                call_ms_median=round(statistics.median(call), 3), mesher_kernel_ms=[round(v, 4) for v in mesh.stats()[1]], **obs.stats())
    emit(line, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--mesh-frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-mesh", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_bench.jsonl"))
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    eng = coxgraph_amd.load_engine()
    for voxel in (0.10, 0.05, 0.02):
        bench_mark(eng, torch, voxel, args, args.out)
    bench_stream(eng, torch, args, args.out)
    if not args.skip_mesh:
        bench_extract(eng, torch, args, args.out)


if __name__ == "__main__":
    main()
