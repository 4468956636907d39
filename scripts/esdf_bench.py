"""Incremental ESDF measurement (not part of bench.py): follow the benchmark stream with an EsdfIntegrator and time every update
against the batch on the same layer.

    python scripts/esdf_bench.py [--frames 150] [--only 0.05,0.1] [--max 2,4] [--every 1,5,15] [--subsample 1] [--out FILE]
                                 [--local-side 24] [--local-only]

Per voxel size, maximum distance (default_distance = max, min_distance 0.1 m, coxgraph_client.yaml:68-69) and update period: the
stream is fused with the merged integrator; after every `period` frames cox_esdf_update runs (frames still in flight) and, in the
same run on the same layer, cox_esdf_from_tsdf -- unchanged from before the incremental path existed, so it is the baseline.  Host
wall time of both calls (the update's own `ms` as well), every field of cox_esdf_update_stats, and whether the two layers hold the
same words (checked at the last update of a run).  One JSON line per update, one summary line per run, appended to
profiles/esdf_bench.jsonl.

The synthetic stream turns in one room, so every frame re-observes most of the map.  --local-side N adds the other end of the
range: an N x N x 3-block slab at 10 cm around a wavy floor (uploaded, not fused), maximum 2 m, in which one block at a time is
overwritten -- the share of the map out of view is all but one block.  Only blocks of the middle layer are edited, the one the
floor runs through, and the floor moves by at least 5 cm, so every edit changes content (n_dirty_blocks is recorded per edit and
`all_edits_dirty` in the summary).  Same two timings per edit (kind "local"), and after each a second update that finds nothing
changed (`noop_update_ms`).
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


def run(eng, voxel, max_d, period, frames, subsample, out):
    from coxgraph_amd import synth
    from coxgraph_amd.capi import Integrator, Layer
    cfg = dict(max_distance_m=max_d, min_distance_m=0.1)
    tsdf = Layer(eng, voxel, capacity_blocks=1 << 14)
    integ = Integrator(eng, tsdf, eng.default_config(**synth.integrator_overrides(voxel)), "merged")
    inc = tsdf.esdf_integrator(**cfg)
    rows = []
    for t in range(frames):
        T, pts, rgba, _ = synth.make_frame(t)
        integ.integrate_points(T, pts[::subsample], rgba[::subsample])
        if (t + 1) % period:
            continue
        integ.sync()   # the frame's own time stays out of both measurements
        t0 = time.perf_counter()
        st = inc.update()
        t1 = time.perf_counter()
        batch = tsdf.esdf(**cfg)
        t2 = time.perf_counter()
        row = dict(kind="update", voxel=voxel, max_distance_m=max_d, period=period, frame=t, update_ms=1e3 * (t1 - t0), batch_ms=1e3 * (t2 - t1), **st)
        last = t + period >= frames
        if last:
            (ia, va), (ib, vb) = inc.layer.download(), batch.download()
            row["same_words"] = bool(np.array_equal(ia, ib) and np.array_equal(va, vb))
        batch.close()
        rows.append(row)
        out.write(json.dumps(row) + "\n")
    steady = rows[1:] or rows   # the first update is a rebuild
    summary = dict(kind="summary", voxel=voxel, max_distance_m=max_d, period=period, n_updates=len(rows), n_blocks=rows[-1]["n_blocks"],
                   update_ms_median=statistics.median(r["update_ms"] for r in steady), batch_ms_median=statistics.median(r["batch_ms"] for r in steady),
                   update_ms_max=max(r["update_ms"] for r in steady), swept_share_median=statistics.median(r["n_swept_blocks"] / max(1, r["n_blocks"]) for r in steady),
                   dirty_share_median=statistics.median(r["n_dirty_blocks"] / max(1, r["n_blocks"]) for r in steady),
                   raise_sweeps_median=statistics.median(r["n_raise_sweeps"] for r in steady), lower_sweeps_median=statistics.median(r["n_lower_sweeps"] for r in steady),
                   first_update_ms=rows[0]["update_ms"], same_words=rows[-1].get("same_words"))
    summary["speedup_median"] = summary["batch_ms_median"] / summary["update_ms_median"]
    out.write(json.dumps(summary) + "\n")
    out.flush()
    print(json.dumps(summary), flush=True)
    inc.close()


def run_local(eng, side, n_edits, out):
    from coxgraph_amd.capi import Layer
    voxel, cfg = 0.10, dict(max_distance_m=2.0, min_distance_m=0.15)
    idx = np.array([[x, y, z] for z in range(3) for y in range(side) for x in range(side)], np.int32)
    lin = np.arange(4096)
    loc = np.stack([lin % 16, (lin // 16) % 16, lin // 256], axis=1)

    def field(blocks, z0):
        c = ((blocks[:, None, :].astype(np.int64) * 16 + loc[None]).astype(np.float32) + 0.5) * np.float32(voxel)
        d = c[..., 2] - z0 + 0.1 * np.sin(1.3 * c[..., 0]) * np.cos(0.9 * c[..., 1])
        vox = np.zeros(d.shape + (3,), np.uint32)
        vox[..., 0] = np.clip(d, -3 * voxel, 3 * voxel).astype(np.float32).view(np.uint32)
        vox[..., 1] = np.float32(5.0).view(np.uint32)
        return vox
    tsdf = Layer(eng, voxel, capacity_blocks=len(idx))
    for part in np.array_split(np.arange(len(idx)), max(1, len(idx) // 256)):
        tsdf.upload(idx[part], field(idx[part], 2.37))
    inc = tsdf.esdf_integrator(**cfg)
    rng = np.random.default_rng(3)
    rows = []
    for e in range(n_edits + 1):
        if e:
            mid = idx[idx[:, 2] == 1]   # the floor (z = 2.37 +- 0.4) runs through the middle layer (z in 1.6 .. 3.2) only
            b = mid[rng.integers(len(mid))][None]
            tsdf.upload(b, field(b, 2.37 + rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 0.3)))
        t0 = time.perf_counter()
        st = inc.update()
        t1 = time.perf_counter()
        batch = tsdf.esdf(**cfg)
        t2 = time.perf_counter()
        noop = inc.update()
        t3 = time.perf_counter()
        assert noop["n_dirty_blocks"] == 0
        row = dict(kind="local", voxel=voxel, max_distance_m=cfg["max_distance_m"], edit=e, update_ms=1e3 * (t1 - t0), batch_ms=1e3 * (t2 - t1),
                   noop_update_ms=1e3 * (t3 - t2), **st)
        if e == n_edits:
            (ia, va), (ib, vb) = inc.layer.download(), batch.download()
            row["same_words"] = bool(np.array_equal(ia, ib) and np.array_equal(va, vb))
        batch.close()
        rows.append(row)
        out.write(json.dumps(row) + "\n")
    steady = rows[1:]
    summary = dict(kind="local_summary", side=side, n_blocks=rows[-1]["n_blocks"], n_edits=n_edits, first_update_ms=rows[0]["update_ms"],
                   update_ms_median=statistics.median(r["update_ms"] for r in steady), update_ms_max=max(r["update_ms"] for r in steady),
                   batch_ms_median=statistics.median(r["batch_ms"] for r in steady), noop_update_ms_median=statistics.median(r["noop_update_ms"] for r in steady),
                   all_edits_dirty=all(r["n_dirty_blocks"] == 1 for r in steady), swept_blocks_min=min(r["n_swept_blocks"] for r in steady),
                   swept_blocks_max=max(r["n_swept_blocks"] for r in steady),
                   raise_sweeps_median=statistics.median(r["n_raise_sweeps"] for r in steady), lower_sweeps_median=statistics.median(r["n_lower_sweeps"] for r in steady),
                   swept_blocks_median=statistics.median(r["n_swept_blocks"] for r in steady), same_words=rows[-1]["same_words"])
    summary["speedup_median"] = summary["batch_ms_median"] / summary["update_ms_median"]
    out.write(json.dumps(summary) + "\n")
    out.flush()
    print(json.dumps(summary), flush=True)
    inc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--only", default="0.05,0.1")
    ap.add_argument("--max", default="2,4")
    ap.add_argument("--every", default="1,5,15")
    ap.add_argument("--subsample", type=int, default=1)
    ap.add_argument("--local-side", type=int, default=0)
    ap.add_argument("--local-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_bench.jsonl"))
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    eng = coxgraph_amd.load_engine()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        if a.local_side:
            run_local(eng, a.local_side, 10, out)
        for voxel in (float(v) for v in a.only.split(",") if not a.local_only):
            for max_d in (float(v) for v in a.max.split(",")):
                for period in (int(v) for v in a.every.split(",")):
                    run(eng, voxel, max_d, period, a.frames, a.subsample, out)


if __name__ == "__main__":
    main()
