"""Dense-stereo measurement (not part of bench.py): EuRoC-sized pairs, 752 x 480, through the EuRoC rectification maps.

    python scripts/stereo_bench.py [--disparities 128,64] [--paths 8,4] [--frames 20] [--warmup 3] [--filters] [--cpu-ref] [--out FILE]

Per shape (disparities x paths) one matcher (cox_stereo_t) and two passes over the same pair, each W warm-up
frames and then N frames, a sync and a read of the statistics after every frame:
  resident   the pair is on the device (cox_stereo_compute_dev): the HIP-event time per stage and per frame;
  host       the pair and the three outputs are in pinned host memory (cox_stereo_compute): the HIP-event time of the frame with its
             copies, and the wall time of call + sync.  EuRoC's cameras run at 20 Hz: this one has to stay under 50 ms.
Median, min and max of the N frames.  Beside them the bytes each pass has to move at least (computed from the shape, below), what
share of the measured copy rate of the chip (6.29 TB/s) that is, and with --cpu-ref the time tests/stereo_ref.py takes for the same
frame on one thread.  One JSON line per shape.  --filters switches the median and the speckle filter on (steps 7a and 7b: median 3,
window 20, range 16) and adds their two stage times, their modelled bytes and the filter counts to the line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

W, H = 752, 480
COPY_RATE = 6.29e12  # bytes/s, the chip's measured float4 copy
STAGES = ("remap_ms", "census_ms", "paths_ms", "winner_ms", "depth_ms", "frame_ms")
FILTER_STAGES = ("median_ms", "speckle_ms")
FILTERS = dict(median_size=3, speckle_window=20, speckle_range16=16)


def modelled_bytes(n, D, P, lr):
    """what each pass reads and writes at least, every buffer counted once per launch that touches it"""
    return dict(remap_ms=2 * n * (1 + 8 + 1) + n,                          # image, map, rectified image; the left mask
                census_ms=2 * n * (1 + 8),
                paths_ms=P * 2 * n * 8 + (2 * P - 1) * n * D * 2,          # both census images per direction; S written once, then read and written
                winner_ms=n * D * 2 + n * 4 + (n * D * 2 + n * 2 if lr else 0),
                depth_ms=n * (4 + 2 + 8 + 1 + 1) + n * (4 + 4 + 2 + 2))


def modelled_filter_bytes(n):
    """the same for the two filter stages: the median reads and writes a u16 image; the labelling reads it in four launches (the
    border pass touches an eighth of it at most), writes parents and sizes, reads and writes the parents, adds to and reads the
    sizes, and writes the final image"""
    return dict(median_ms=n * (2 + 2), speckle_ms=n * (2 + 4 + 4) + n * (2 + 4) // 8 + n * (2 + 4 + 4 + 4) + n * (2 + 4 + 4 + 2))


def summary(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", default="128,64")
    ap.add_argument("--paths", default="8,4")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--filters", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    import stereo_ref as sr
    from coxgraph_amd import capi
    eng = coxgraph_amd.load_engine()
    if eng.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    chain = sr.euroc_camchain()
    left, right, _ = sr.scene(W, H)
    n = W * H
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    depth_d = torch.empty((H, W), dtype=torch.float32, device="cuda")
    rgba_d = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    disp_d = torch.empty((H, W), dtype=torch.int16, device="cuda")
    pin = dict(left=torch.from_numpy(left).pin_memory(), right=torch.from_numpy(right).pin_memory(), depth=torch.empty((H, W), dtype=torch.float32).pin_memory(),
               rgba=torch.empty((H, W, 4), dtype=torch.uint8).pin_memory(), disp=torch.empty((H, W), dtype=torch.int16).pin_memory())
    pp = {k: C.c_void_p(v.data_ptr()) for k, v in pin.items()}
    torch.cuda.synchronize()
    for D in [int(v) for v in args.disparities.split(",")]:
        for P in [int(v) for v in args.paths.split(",")]:
            m = capi.StereoMatcher(eng, W, H, calibration=chain, n_disparities=D, n_paths=P)
            if args.filters:
                m.set_filters(**FILTERS)
            per, per_filter = [], []
            for t in range(args.warmup + args.frames):
                m.compute_dev(left_d, right_d, depth_d, rgba_d, disp_d)
                st = m.last_stats()   # waits for the frame
                if t >= args.warmup:
                    per.append(st)
                    per_filter.append(m.filter_stats() if args.filters else None)
            resident_depth = depth_d.cpu().numpy()
            host_event, host_wall = [], []
            for t in range(args.warmup + args.frames):
                t0 = time.perf_counter()
                eng.check(eng.fn("stereo_compute")(m.h_, pp["left"], pp["right"], pp["depth"], pp["rgba"], pp["disp"]), "stereo_compute")
                m.sync()
                wall = 1e3 * (time.perf_counter() - t0)
                if t >= args.warmup:
                    host_event.append(m.last_stats()["frame_ms"])
                    host_wall.append(wall)
            host_depth = pin["depth"].numpy()
            assert np.array_equal(np.isnan(host_depth), np.isnan(resident_depth)) and np.array_equal(np.nan_to_num(host_depth), np.nan_to_num(resident_depth))
            bytes_ = modelled_bytes(n, D, P, True)
            line = dict(wh=[W, H], n_disparities=D, n_paths=P, warmup=args.warmup, frames=args.frames, valid_pixels=per[-1]["n_valid_pixels"],
                        resident={k: summary([s[k] for s in per]) for k in STAGES}, modelled_bytes={k: int(v) for k, v in bytes_.items()},
                        share_of_copy_rate={k: round(bytes_[k] / COPY_RATE / (1e-3 * statistics.median(s[k] for s in per)), 4) for k in bytes_},
                        host_frame_event_ms=summary(host_event), host_frame_wall_ms=summary(host_wall), budget_ms=50.0)
            if args.filters:
                fbytes = modelled_filter_bytes(n)
                line["filters"] = dict(FILTERS, counts={k: v for k, v in per_filter[-1].items() if k not in FILTER_STAGES})
                line["resident"].update({k: summary([s[k] for s in per_filter]) for k in FILTER_STAGES})
                line["modelled_bytes"].update(fbytes)
                line["share_of_copy_rate"].update({k: round(fbytes[k] / COPY_RATE / (1e-3 * statistics.median(s[k] for s in per_filter)), 4) for k in fbytes})
            if args.cpu_ref:
                t0 = time.perf_counter()
                match = sr.match
                if args.filters:
                    import stereo_filter_ref as fr
                    match = lambda *a, **k: fr.match_filtered(*a, **FILTERS, **k)  # noqa: E731
                want = match(left, right, m.K_rect, np.float32(m.baseline_m), *sr.rectify_maps(chain, W, H)[:2], n_disparities=D, n_paths=P)
                line["reference_one_thread_s"] = round(time.perf_counter() - t0, 2)
                line["equal_to_reference"] = bool(np.array_equal(np.isnan(want["depth"]), np.isnan(host_depth)) and
                                                  np.array_equal(np.nan_to_num(want["depth"]), np.nan_to_num(host_depth)))
            m.close()
            out = json.dumps(line)
            print(out, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(out + "\n")


if __name__ == "__main__":
    main()
