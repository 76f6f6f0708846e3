#!/usr/bin/env python3
"""What the detector response costs: k_lsf over one --size plane with (1,1), (9,9),
(41,41) and (129,129) taps, beside a device-to-device copy of the plane (one read and
one write: the memory floor) and k_apply_spectrum with 8 bins over the paths render's
planes of the three-mesh dragon scene (a box around the dragon, the dragon, a box
beside it) -- the kernel that precedes this one in the post-trace chain.  One process,
one device; the legs are measured in turn, --rounds times, so that clock drift shows
as spread between the rounds and not as a difference between the legs.  Every leg:
device events around --frames launches on one stream after a warm-up, divided by the
launches.  The plane the response reads is the scene's own hole-filled image.

    python tools/lsf_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAPS = [(1, 1), (9, 9), (41, 41), (129, 129)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[2048, 2048], metavar=("W", "H"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import simpleraytracing_amd as xrt
    from materials_kit import DRAGON_MU, dragon_scene

    W, H = args.size
    n = W * H
    dragon = xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply"))
    scene = dragon_scene(dragon)
    M = len(scene)
    cam = xrt.camera_for_scene(scene, W, H)
    lb = torch.empty(n, device="cuda")
    image = torch.empty(n, device="cuda")
    out = torch.empty(n, device="cuda")
    out_u8 = torch.empty(n, dtype=torch.uint8, device="cuda")
    paths = torch.empty(M * n, device="cuda")
    opn = torch.empty(n, dtype=torch.int16, device="cuda")

    K = 8                                               # equal weights that sum to 80; DRAGON_MU in bin 0, falling 3% a bin
    w = np.full(K, 80.0 / K, np.float32)
    mu = (np.asarray(DRAGON_MU, np.float64)[:, None] * 0.97 ** np.arange(K)[None, :]).astype(np.float32)

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

    names = ["copy_plane", "apply_spectrum_8_bins"] + [f"detector_response_{nx}x{ny}" for nx, ny in TAPS]
    us = {name: [] for name in names}
    with xrt.Context(0) as ctx:
        ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        ctx.upload_scene(scene)
        ctx.set_paths()
        ctx.render_paths_device(cam, 0, H, M, paths.data_ptr(), opn.data_ptr())
        ctx.apply_spectrum_device(n, paths.data_ptr(), opn.data_ptr(), w, mu, lb.data_ptr())
        ctx.hole_fill_device(W, H, lb.data_ptr(), image.data_ptr(), 0)
        torch.cuda.synchronize()
        ctx.read_stats()
        taps = {(nx, ny): (xrt.lsf_gaussian(nx / 8.0 + 0.3, nx), xrt.lsf_gaussian(ny / 8.0 + 0.3, ny)) for nx, ny in TAPS}
        for _ in range(args.rounds):
            us["copy_plane"].append(events(lambda: out.copy_(image)))
            us["apply_spectrum_8_bins"].append(
                events(lambda: ctx.apply_spectrum_device(n, paths.data_ptr(), opn.data_ptr(), w, mu, lb.data_ptr())))
            for nx, ny in TAPS:
                hx, hy = taps[(nx, ny)]
                us[f"detector_response_{nx}x{ny}"].append(
                    events(lambda: ctx.detector_response_device(W, H, 1, image.data_ptr(), hx, hy, out.data_ptr(),
                                                                out_u8.data_ptr())))
    best = {name: min(v) for name, v in us.items()}
    result = {"size": [W, H], "frames": args.frames, "us_per_launch": us,
              "method": "device events around the launches of one stream, divided by the launches",
              "yardstick": {"detector_response_41x41 <= apply_spectrum_8_bins (same run, best of the rounds)":
                            bool(best["detector_response_41x41"] <= best["apply_spectrum_8_bins"])},
              "us_per_tap_pair_41_over_9": round((best["detector_response_41x41"] - best["detector_response_9x9"]) / 32.0, 3),
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
