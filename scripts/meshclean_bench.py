"""Mesh clean-up measurement (not part of bench.py): fuse the benchmark stream at 1 cm, mesh and weld it (the connected mesh of
DESIGN.md section 7d), then time each clean-up operation of section 7h on it.

    python scripts/meshclean_bench.py [--frames N] [--reps R] [--warmup W] [--voxel V] [--no-cpu-ref]

Per operation, one JSON line: the HIP-event time of the whole call (events on the null stream, which the library uses, around the
call; median, min and max of R calls after W warm-up calls, every call on a fresh upload of the same mesh), for the smoothing also
the library's own event time of the 2 x iterations half-step launches, the modelled bytes, and the CPU time of the test-side numpy
reference (tests/meshclean_ref.py, float64).

Modelled bytes.  A stable LSD sort of n elements by one word of b bits: 12 n for the gather (permutation, word, key) plus
ceil(b / 11) passes of 20 n (histogram 4 n, scatter 8 n in, 8 n out).  clean: canonical triples 28 nt, three word sorts, flags and
compaction 40 nt + 8 nv, scans 16 (nt + nv), output 12 nt' + 54 nv'.  smooth: the neighbour list once (two word sorts of 6 nt edges,
48 nt to emit, 24 nt scan, 60 nt fill), then per half-step 32 nv + 16 nnz (own position, row bounds, per neighbour an index and
a position, the new position).  normals: one word sort of 3 nt corners, 12 nt of row bounds, per corner 4 + 3 x 16 gathered, 20 nv.
cluster: bounds 12 nv, cells 24 nv, three word sorts of nv, flags / ids 40 nv, averages 31 nv + 27 nc, re-index 24 nt, then clean.
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


HBM_PEAK_GBPS = 8000.0


def bits_for(n):
    return max(0, int(n - 1).bit_length())


def sort_bytes(n, bits):
    return sum(n * (12 + 20 * -(-b // 11)) for b in bits if b > 0)


def clean_bytes(nv, nt, nv2, nt2):
    return 28 * nt + sort_bytes(nt, [bits_for(nv)] * 3) + 40 * nt + 8 * nv + 16 * (nt + nv) + 12 * nt2 + 54 * nv2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--cell", type=float, default=0.05)
    ap.add_argument("--no-cpu-ref", action="store_true")
    args = ap.parse_args()
    import torch
    import coxgraph_amd
    import meshclean_ref as R
    from coxgraph_amd import synth
    from coxgraph_amd.capi import ConnectedMesh, Integrator, Layer, MeshLayer
    torch.zeros(1, device="cuda")
    eng = coxgraph_amd.load_engine()
    layer = Layer(eng, args.voxel, capacity_blocks=1 << 16)
    integ = Integrator(eng, layer, eng.default_config(**synth.integrator_overrides(args.voxel)), "merged")
    for t in range(args.frames):
        T, pts, rgba, _ = synth.make_frame(t)
        integ.integrate_points(T, pts, rgba)
    integ.sync()
    part = MeshLayer.from_layer(eng, layer, min_weight=1e-4)
    base = MeshLayer.connected(eng, [part], None, 0.5 * args.voxel)
    cleaned = R.clean(base)[0]

    def fresh(m):
        return ConnectedMesh.from_arrays(eng, m["xyz"], m["triangles"], m["normals"], m["rgb"])

    ops = [
        ("clean", base, lambda c: c.clean(), lambda m: R.clean(m)),
        ("smooth_taubin", cleaned, lambda c: c.smooth_taubin(args.iterations), lambda m: R.smooth_taubin(m, args.iterations)),
        ("simplify_clustering", cleaned, lambda c: c.simplify_clustering(args.cell), lambda m: R.simplify_clustering(m, args.cell)),
        ("compute_normals", cleaned, lambda c: c.compute_normals(), lambda m: R.compute_normals(m)),
    ]
    for name, m, op, ref in ops:
        mv, mt = len(m["xyz"]), len(m["triangles"])
        ms, own = [], []
        for i in range(args.warmup + args.reps):
            c = fresh(m)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = op(c)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
                if name == "smooth_taubin":
                    own.append(r)
            after = c.size
            c.close()
        if name == "clean":
            nbytes = clean_bytes(mv, mt, *after)
        elif name == "smooth_taubin":
            nbytes = 48 * mt + sort_bytes(6 * mt, [bits_for(mv)] * 2) + 84 * mt + 2 * args.iterations * (32 * mv + 16 * nnz_of(R, m))
        elif name == "compute_normals":
            nbytes = sort_bytes(3 * mt, [bits_for(mv)]) + 12 * mt + 3 * mt * 52 + 20 * mv
        else:
            span = (m["xyz"].max(axis=0) - m["xyz"].min(axis=0)) / args.cell + 1
            nbytes = 36 * mv + sort_bytes(mv, [bits_for(int(s) + 1) for s in span]) + 71 * mv + 27 * after[0] + 24 * mt + clean_bytes(after[0], mt, *after)
        med = statistics.median(ms)
        rec = dict(op=name, voxel=args.voxel, frames=args.frames, vertices=mv, triangles=mt, vertices_after=after[0], triangles_after=after[1],
                   call_event_ms=round(med, 4), call_event_ms_min_max=[round(min(ms), 4), round(max(ms), 4)], modelled_bytes=int(nbytes),
                   hbm_fraction=round(nbytes / (med * 1e-3) / (HBM_PEAK_GBPS * 1e9), 5), reps=args.reps, warmup=args.warmup)
        if own:
            k = statistics.median(own)
            rec.update(iterations=args.iterations, half_step_launches=2 * args.iterations, launches_event_ms=round(k, 4),
                       launches_event_ms_min_max=[round(min(own), 4), round(max(own), 4)], us_per_launch=round(1e3 * k / (2 * args.iterations), 3),
                       half_step_bytes=int(32 * mv + 16 * nnz_of(R, m)),
                       half_step_hbm_fraction=round((32 * mv + 16 * nnz_of(R, m)) / (k * 1e-3 / (2 * args.iterations)) / (HBM_PEAK_GBPS * 1e9), 5))
        if not args.no_cpu_ref:
            t0 = time.perf_counter()
            ref(m)
            rec["cpu_reference_numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        print(json.dumps(rec), flush=True)


_NNZ = {}


def nnz_of(R, m):
    key = id(m)
    if key not in _NNZ:
        _NNZ[key] = len(R.adjacency(m["triangles"], len(m["xyz"]))[2])
    return _NNZ[key]


if __name__ == "__main__":
    main()
