"""Collision-check measurement (not part of bench.py): fuse the benchmark stream, build the ESDF, then time the checks of
include/coxgraph_hip_collide.h on it against the route the engine offered before them.

    python scripts/collide_bench.py [--frames N] [--reps R] [--warmup W] [--only 0.05,0.01] [--batches 1,256,4096,65536]
                                    [--tree-nodes 20000] [--radius 0.3] [--cpu-ref] [--single] [--out FILE]

Per layer (the ESDF, 4 m band, of the 150-frame 5 cm and 1 cm layers of scripts/query_bench.py), per batch of straight segments
of the configured shape (<= 1.5 m, 5 cm spacing, starts in observed space) and for a tree of 30-point stored trajectories, each
in three mixes -- all feasible, about half blocked, all blocked at the first sample:

  fused      cox_collide_segments_dev / cox_collide_tree_dev with 32 and with 64 lanes per item: HIP-event time of the call's
             kernels, median, min and max over R runs after W warm-ups; segments/s and samples/s (samples of the rule, looked at
             or skipped).
  yardstick  the same answer by the older route, timed the same way: the samples expanded on the device with torch,
             cox_layer_query_dev twice (NEAREST for "observed", INTERPOLATE for the distance), the reduction in torch (and for
             the tree the pointer jumping in torch).  first_blocked / keep of both routes are compared (first_blocked_equal).

With --cpu-ref the single-thread time of the test-side reference (tests/cpp/collide_reference.cpp) on the 4 096-segment batch.
--single runs the fused 65 536-segment half-blocked batch only (for a kernel trace of one batch).  One JSON line per case.
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

MIXES = ("feasible", "half", "blocked")
TRAJ_POINTS = 30


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


def candidates(esdf, voxel, n, rng):
    """Segments of the configured shape that start in observed space: starts at free-space voxel centres moved by up to half a
    voxel, ends uniform in the ball of 1.5 m."""
    xyz, _ = esdf.free_points(0.0)
    a = xyz[rng.integers(0, len(xyz), n)] + rng.uniform(-0.5, 0.5, size=(n, 3)) * voxel
    d = rng.normal(size=(n, 3))
    d *= (1.5 * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return a.astype(np.float32), (a + d).astype(np.float32)


def pick(mix, feasible, blocked0, n, rng):
    """Indices of n candidates in the mix (with repetition when the pool is smaller than n)."""
    f, b = np.flatnonzero(feasible), np.flatnonzero(blocked0)
    nf = f if len(f) else b
    if mix == "feasible":
        return rng.choice(f, n)
    if mix == "blocked":
        return rng.choice(b, n)
    other = np.flatnonzero(~feasible)
    sel = np.concatenate([rng.choice(nf, n - n // 2), rng.choice(other, n // 2)])
    rng.shuffle(sel)
    return sel


def timed(fn, stream, reps, warmup):
    import torch
    ms = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


class OldRoute:
    """What a caller did before the fused entry points: expand, query twice, reduce -- all on the device."""

    def __init__(self, layer, radius, ds=0.05, max_ext=1.5):
        import torch
        self.torch, self.layer, self.radius, self.ds, self.max_ext = torch, layer, radius, ds, max_ext

    def _blocked(self, p, stream):
        torch = self.torch
        n = p.shape[0]
        st_n = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st_t = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d = torch.zeros(n, device="cuda")
        self.layer.query_dev(p, mode="nearest", status=st_n, stream=stream)
        self.layer.query_dev(p, mode="interpolate", distance=d, status=st_t, stream=stream)
        ok = ((st_n & 1) != 0) & ((st_t & 1) != 0) & (d > self.radius)
        return ~ok

    def segments(self, a, b, stream):
        """first_blocked[n] (n + 1 of the segment when none) and the number of samples."""
        torch = self.torch
        dirv = b - a
        length = torch.sqrt((dirv[:, 0] * dirv[:, 0] + dirv[:, 1] * dirv[:, 1]) + dirv[:, 2] * dirv[:, 2])
        s = torch.where(length > self.max_ext, self.max_ext / length, torch.ones_like(length))
        clamp = length > self.max_ext
        dirv = torch.where(clamp[:, None], dirv * s[:, None], dirv)
        length = torch.where(clamp, torch.sqrt((dirv[:, 0] * dirv[:, 0] + dirv[:, 1] * dirv[:, 1]) + dirv[:, 2] * dirv[:, 2]), length)
        n = torch.clamp(torch.ceil(length / self.ds), min=1.0).to(torch.int64)
        count = n + 1
        seg = torch.repeat_interleave(torch.arange(len(a), device="cuda"), count)
        start = torch.cumsum(count, 0) - count
        i = torch.arange(seg.shape[0], device="cuda") - start[seg]
        t = i.to(torch.float32) / n[seg].to(torch.float32)
        p = (a[seg] + t[:, None] * dirv[seg]).contiguous()
        blocked = self._blocked(p, stream)
        first = count.clone()
        first.scatter_reduce_(0, seg[blocked], i[blocked], reduce="amin")
        return first, int(seg.shape[0])

    def tree(self, offsets, parent, xyz, stream):
        """keep[n] (1 / 0; the trees of the benchmark are proper forests)."""
        torch = self.torch
        count = offsets[1:] - offsets[:-1]
        node = torch.repeat_interleave(torch.arange(len(parent), device="cuda"), count)
        blocked = self._blocked(xyz, stream)
        bad = torch.zeros(len(parent), dtype=torch.int64, device="cuda")
        bad.scatter_add_(0, node, blocked.to(torch.int64))
        ok = bad == 0
        anc = parent.to(torch.int64)
        for _ in range(int(np.ceil(np.log2(max(len(parent), 2)))) + 1):
            has = anc >= 0
            safe = torch.where(has, anc, torch.zeros_like(anc))
            ok = ok & torch.where(has, ok[safe], torch.ones_like(ok))
            anc = torch.where(has, anc[safe], anc)
        return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="0.05,0.01")
    ap.add_argument("--batches", default="1,256,4096,65536")
    ap.add_argument("--tree-nodes", type=int, default=20000)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd.capi import COLLIDE_RECORD_DTYPE, CollisionChecker
    eng = coxgraph_amd.load_engine()
    stream = torch.cuda.Stream()
    batches = [65536] if args.single else [int(b) for b in args.batches.split(",")]

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    for voxel in [float(v) for v in args.only.split(",")]:
        rng = np.random.default_rng(9)
        tsdf, integ = fuse(eng, voxel, args.frames, 640, 480)
        esdf = tsdf.esdf(max_distance_m=4.0, min_distance_m=0.1)
        base = dict(voxel=voxel, frames=args.frames, blocks=esdf.n_blocks(), radius=args.radius)
        checkers = {g: CollisionChecker(eng, esdf, group_size=g, collision_radius=args.radius) for g in (32, 64)}
        old = OldRoute(esdf, args.radius)
        # candidates, classified by the checker itself
        ca, cb = candidates(esdf, voxel, 1 << 20, rng)
        rec = checkers[32].segments(ca, cb)
        feasible, blocked0 = (rec["flags"] & 1) != 0, (rec["flags"] & 1 == 0) & (rec["first_blocked"] == 0)
        emit(dict(base, case="candidates", n=len(ca), feasible=float(feasible.mean()), blocked_at_first=float(blocked0.mean())))
        ref_layer = None
        if args.cpu_ref and voxel == 0.05:
            import collide_ref
            out_dir = os.path.join(ROOT, "build")
            os.makedirs(out_dir, exist_ok=True)
            idx, vox = esdf.download()
            ref_layer = collide_ref.build(out_dir).layer(voxel, idx, vox)
        for n in batches:
            for mix in (("half",) if args.single else MIXES):
                sel = pick(mix, feasible, blocked0, n, rng)
                a, b = torch.from_numpy(ca[sel]).cuda(), torch.from_numpy(cb[sel]).cuda()
                out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                n_samples = int((rec["n_samples"][sel].astype(np.int64) + 1).sum())
                line = dict(base, case="segments", mix=mix, segments=n, samples=n_samples, feasible=float(feasible[sel].mean()))
                for g, cc in checkers.items():
                    t = timed(lambda: cc.segments_dev(a, b, out, stream=stream), stream, args.reps, args.warmup)
                    line[f"fused{g}"] = dict(t, segments_per_s=n / (t["ms_median"] * 1e-3), samples_per_s=n_samples / (t["ms_median"] * 1e-3))
                got = out.cpu().numpy().view(COLLIDE_RECORD_DTYPE)
                if not args.single:
                    t = timed(lambda: old.segments(a, b, stream), stream, args.reps, args.warmup)
                    with torch.cuda.stream(stream):
                        first, expanded = old.segments(a, b, stream)
                    stream.synchronize()
                    line["yardstick"] = dict(t, segments_per_s=n / (t["ms_median"] * 1e-3), samples_per_s=n_samples / (t["ms_median"] * 1e-3),
                                             samples_expanded=expanded)
                    line["first_blocked_equal"] = bool(np.array_equal(first.cpu().numpy(), got["first_blocked"].astype(np.int64)))
                    line["fused_over_yardstick"] = {g: t["ms_median"] / line[f"fused{g}"]["ms_median"] for g in (32, 64)}
                if ref_layer is not None and n == 4096:
                    r = ref_layer.segments(ca[sel], cb[sel], collision_radius=args.radius)
                    line["cpu_ref_seconds"] = r["seconds"]
                    line["cpu_ref_segments_per_s"] = n / r["seconds"]
                    line["cpu_ref_records_equal"] = collide_ref.records_equal(got, r["records"]) is None
                emit(line)
        if args.single:
            continue
        # the tree: a random forest whose nodes own 30 points along a candidate segment each
        n = args.tree_nodes
        ta, tb = ca[: 4 * n], cb[: 4 * n]
        steps = (np.arange(TRAJ_POINTS, dtype=np.float32) / np.float32(TRAJ_POINTS - 1))[None, :, None]
        pts = (ta[:, None, :] + steps * (tb - ta)[:, None, :]).astype(np.float32)
        offs = np.arange(0, 4 * n * TRAJ_POINTS + 1, TRAJ_POINTS, dtype=np.uint64)
        trec = checkers[32].trajectories(offs, pts.reshape(-1, 3))
        t_feasible, t_blocked0 = (trec["flags"] & 1) != 0, trec["first_blocked"] == 0
        order = rng.permutation(n)
        parent = np.full(n, -1, np.int32)
        for i in range(8, n):
            parent[order[i]] = order[rng.integers(max(0, i - 64), i)]  # deep and narrow, as an RRT* grows
        for mix in MIXES:
            sel = pick(mix, t_feasible, t_blocked0 & ~t_feasible, n, rng)
            xyz = torch.from_numpy(np.ascontiguousarray(pts[sel].reshape(-1, 3))).cuda()
            d_off = torch.arange(0, n * TRAJ_POINTS + 1, TRAJ_POINTS, dtype=torch.int64, device="cuda")
            d_par = torch.from_numpy(parent).cuda()
            out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
            keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
            line = dict(base, case="tree", mix=mix, nodes=n, points=n * TRAJ_POINTS, feasible=float(t_feasible[sel].mean()))
            for g, cc in checkers.items():
                t = timed(lambda: cc.tree_dev(d_off, d_par, n, xyz, n * TRAJ_POINTS, out, keep, stream=stream), stream, args.reps, args.warmup)
                line[f"fused{g}"] = dict(t, nodes_per_s=n / (t["ms_median"] * 1e-3), samples_per_s=n * TRAJ_POINTS / (t["ms_median"] * 1e-3))
            t = timed(lambda: old.tree(d_off, d_par, xyz, stream), stream, args.reps, args.warmup)
            with torch.cuda.stream(stream):
                ok = old.tree(d_off, d_par, xyz, stream)
            stream.synchronize()
            line["yardstick"] = dict(t, nodes_per_s=n / (t["ms_median"] * 1e-3))
            line["kept"] = float((keep == 1).float().mean().item())
            line["keep_equal"] = bool(torch.equal(ok, keep == 1))
            line["fused_over_yardstick"] = {g: t["ms_median"] / line[f"fused{g}"]["ms_median"] for g in (32, 64)}
            emit(line)
        for g, cc in checkers.items():
            emit(dict(base, case="stats", group=g, **cc.stats()))
            cc.close()
        del esdf, tsdf, integ


if __name__ == "__main__":
    main()
