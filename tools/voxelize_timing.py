#!/usr/bin/env python3
"""The voxeliser's steps apart, in one process on one device: the dragon (22866 triangles of a few
columns each) and the 12-triangle box about it (four triangles of a quarter of the grid's columns each) on cubic
grids of --grids voxels a side.  Each leg is device events around --frames enqueues of xrt_voxelize_device with
only that step switched on (xrt_debug_voxelize_stages), after a warm-up; the legs are measured in turn, --rounds
times, so that clock drift shows as spread between the rounds and not as a difference between the legs.

  clear_SCENE_N           clearing the flip volume, u16 [N + 1][N][N]
  scatter_SCENE_N_tT      k_voxel_scatter + k_voxel_tiles with the queue's threshold at T columns (xrt_debug_
                          voxelize_threshold; "lanes": no triangle queued, a lane per triangle alone)
  scan_SCENE_N            k_voxel_scan writing mask, labels and volume
  scan1_SCENE_N           the same with every column's slices in one run (no split of a small grid's slices)
  copy_N                  a plain device copy that moves the bytes the scan moves (it reads 2 (N + 1) N^2 and writes
                          7 N^3), the yardstick of a streaming pass
  all_SCENE_N             the whole call at the default threshold

    python tools/voxelize_timing.py [--grids 128 256 512] [--frames 50] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

THRESHOLDS = [("t4", 4), ("t8", 8), ("t16", 16), ("t32", 32), ("t128", 128), ("t1024", 1024), ("lanes", 0xFFFFFFFF)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import simpleraytracing_amd as xrt
    import voxel_ref
    from scene_kit import box

    dragon = np.ascontiguousarray(xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply")), np.float32).reshape(-1, 9)
    v = dragon.reshape(-1, 3)
    pad = np.float32(0.02) * np.float32((v.max(0) - v.min(0)).max())
    scenes = {"dragon": [dragon], "box": [box(v.min(0) - pad, v.max(0) + pad)]}

    def events(launch, frames):
        for _ in range(min(args.warmup, frames)):
            launch()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(frames):
            launch()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) * 1e3 / frames, 2)

    us, counters, checks = {}, {}, {}
    with xrt.Context(0) as ctx:
        for n in args.grids:
            dims, origin, spacing = voxel_ref.dragon_grid(dragon, n)
            voxels = n ** 3
            mask = torch.empty(voxels, dtype=torch.int16, device="cuda")
            labels = torch.empty(voxels, dtype=torch.uint8, device="cuda")
            volume = torch.empty(voxels, dtype=torch.float32, device="cuda")
            moved = (2 * (n + 1) * n * n + 7 * voxels) // 2
            src = torch.zeros(moved, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)

            def call():
                ctx.voxelize_device(dims, spacing, origin, [0.2], mask.data_ptr(), labels.data_ptr(), volume.data_ptr())

            for name, scene in scenes.items():
                ctx.upload_scene(scene)
                tag = f"{name}_{n}"
                call()
                torch.cuda.synchronize()
                first = mask.cpu().numpy().copy()
                checks[tag] = {"inside_voxels": int(np.count_nonzero(first))}
                same = True
                for _ in range(args.rounds):
                    ctx.voxelize_stages(7)
                    ctx.voxelize_threshold(0)
                    us.setdefault(f"all_{tag}", []).append(events(call, args.frames))
                    ctx.voxelize_stages(2)
                    us.setdefault(f"scan_{tag}", []).append(events(call, args.frames))
                    ctx.voxelize_stages(2 + 8)
                    us.setdefault(f"scan1_{tag}", []).append(events(call, args.frames))
                    us.setdefault(f"copy_{n}", []).append(events(lambda: dst.copy_(src), args.frames))
                    ctx.voxelize_stages(4)
                    us.setdefault(f"clear_{tag}", []).append(events(call, args.frames))
                    ctx.voxelize_stages(1)
                    for label, t in THRESHOLDS:
                        ctx.voxelize_threshold(t)
                        # (a lane that walks a quarter of a 512^2 grid alone takes long: fewer enqueues)
                        frames = max(2, args.frames // 10) if (name == "box" and t > 1024) else args.frames
                        us.setdefault(f"scatter_{tag}_{label}", []).append(events(call, frames))
                    ctx.voxelize_stages(7)
                    for label, t in THRESHOLDS:                  # every schedule gives the first call's volume
                        ctx.voxelize_threshold(t)
                        call()
                        torch.cuda.synchronize()
                        counters[f"{tag}_{label}"] = ctx.voxelize_counters()
                        same = same and bool(np.array_equal(mask.cpu().numpy(), first))
                    ctx.voxelize_threshold(0)
                checks[tag]["every_schedule_equal"] = same
    best = {k: min(vs) for k, vs in us.items()}
    ratios = {}
    for n in args.grids:
        for name in scenes:
            tag = f"{name}_{n}"
            ratios[tag] = {"scan_over_copy": round(best[f"scan_{tag}"] / best[f"copy_{n}"], 3),
                           "scan_GBps": round((2 * (n + 1) * n * n + 7 * n ** 3) / best[f"scan_{tag}"] / 1e3, 1),
                           "scan_one_run_over_scan": round(best[f"scan1_{tag}"] / best[f"scan_{tag}"], 3),
                           "lanes_over_t16": round(best[f"scatter_{tag}_lanes"] / best[f"scatter_{tag}_t16"], 2)}
    result = {"grids": args.grids, "frames": args.frames, "us_per_call": us, "ratios": ratios, "counters": counters,
              "checks": checks, "method": "device events around the enqueues, one step switched on at a time",
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
