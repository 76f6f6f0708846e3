#!/usr/bin/env python3
"""The voxel trace, k_volume_paths, over a 256^3 phantom of concentric shells in one process on one device.
The legs are measured in turn, --rounds times, so that clock drift shows as spread between the rounds and not
as a difference between the legs; each leg is device events around --frames launches on one stream after a
warm-up, divided by the launches.  A leg is named  M<labels>[d]_<side>_<camera>_<shape>:

  M4, M4d, M1, M16   the label count (the kernel's three instantiations), d: with a density per voxel
  1024, 2048         the detector's side in pixels
  base, yaw45        the volume's own camera, and the same turned 45 degrees about the vertical axis through
                     the volume's centre: its rays cross the x-fastest layout diagonally
  tiles, rows        waves of 8 x 8 pixel tiles (what the library runs) or of 64 x 1 row segments
                     (xrt_debug_volume_wave_shape): the A/B the layout rests on

Voxel steps are counted on the host from each ray's entry and exit voxel (|dix| + |diy| + |diz| + 1).

    python tools/volume_timing.py [--sides 1024 2048] [--dim 256] [--frames 200] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shells(n, M):
    """n^3 concentric shells about the centre, label 1 innermost .. M outermost, 0 outside the ball."""
    import numpy as np
    g = (np.arange(n, dtype=np.float32) - (n - 1) / 2.0) ** 2
    r = np.sqrt(g[:, None, None] + g[None, :, None] + g[None, None, :])
    lab = np.floor(r / ((n / 2.0) / M)).astype(np.int32) + 1
    return np.where(lab <= M, lab, 0).astype(np.uint8)


def voxel_steps(c13, W, H, n, lo, s):
    """The voxels every ray of the frame visits, summed: from the slab test's entry and exit points."""
    import numpy as np
    import camera_kit
    d = camera_kit.ray_directions(c13, W, H).astype(np.float64).reshape(-1, 3)
    O = np.asarray(c13[0:3], np.float64)
    hi = lo + n * s
    with np.errstate(all="ignore"):
        t0, t1 = (lo - O) / d, (hi - O) / d
        te = np.maximum(np.nanmax(np.minimum(t0, t1), axis=1), 0.0)
        tx = np.nanmin(np.maximum(t0, t1), axis=1)
    hit = te < tx
    a = np.clip(np.floor((O + te[hit, None] * d[hit] - lo) / s), 0, n - 1)
    b = np.clip(np.floor((O + tx[hit, None] * d[hit] - lo) / s), 0, n - 1)
    return int(np.abs(b - a).sum() + hit.sum()), int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import camera_kit
    import simpleraytracing_amd as xrt

    n = args.dim
    spacing, origin = np.float32(1.0), np.full(3, -n / 2.0, np.float32)
    lo, hi = xrt.volume_bbox((n, n, n), spacing, origin)
    centre = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    cams, steps = {}, {}
    for side in args.sides:
        base = camera_kit.cam13(xrt.camera_from_bbox(lo, hi, side, side))
        for name, c13 in (("base", base), ("yaw45", camera_kit.general_camera(base, centre, side, side, yaw=45.0))):
            cams[(side, name)] = camera_kit.as_camera(c13, side, side)
            steps[f"{side}_{name}"] = voxel_steps(c13, side, side, n, lo.astype(np.float64), float(spacing))
    density = np.random.default_rng(1).uniform(0.5, 2.0, (n, n, n)).astype(np.float32)
    labels = {M: shells(n, M) for M in (1, 4, 16)}
    volumes = [("M4", 4, None), ("M4d", 4, density), ("M1", 1, None), ("M16", 16, None)]
    out = torch.empty(16 * max(args.sides) ** 2, device="cuda")

    def events(launch):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.frames):
            launch()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) * 1e3 / args.frames, 2)

    us = {}
    with xrt.Context(0) as ctx:
        for _ in range(args.rounds):
            for vname, M, den in volumes:
                ctx.upload_volume(labels[M], spacing, origin, den, M)
                for (side, cname), cam in cams.items():
                    for shape in ("tiles", "rows"):
                        ctx.volume_wave_shape(shape == "rows")
                        leg = f"{vname}_{side}_{cname}_{shape}"
                        us.setdefault(leg, []).append(
                            events(lambda: ctx.volume_paths_device(cam, 0, side, M, out.data_ptr())))
        ctx.volume_wave_shape(False)
    gsteps = {leg: round(steps["_".join(leg.split("_")[1:3])][0] / (min(v) * 1e-6) / 1e9, 2) for leg, v in us.items()}
    result = {"dim": n, "frames": args.frames, "us_per_launch": us, "voxel_steps_and_hit_rays": steps,
              "giga_voxel_steps_per_second_best_round": gsteps, "method": "device events around the launches",
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
