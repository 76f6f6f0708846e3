#!/usr/bin/env python3
"""What the line-integral projections cost: k_log_projection over one --size plane -- with a
scalar flat out of place, the same in place, and with flat and dark planes -- and over 8 planes
of half the size in sinogram order, beside a device-to-device copy of the plane (one read and one
write: the memory floor) and the detector response under one tap on each axis, k_lsf (1,1): the
pass that precedes this one in the post-trace chain, with no arithmetic in it.  One process, one
device; the legs are measured in turn, --rounds times, so that clock drift shows as spread
between the rounds and not as a difference between the legs.  Every leg: device events around
--frames launches on one stream after a warm-up, divided by the launches.  The plane is seeded
intensities in (1, 80]; a pointwise pass costs the same on any finite values (no branch of
xrt_logf diverges: the special cases are selects).

    python tools/projection_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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

    W, H = args.size
    n = W * H
    P, SW, SH = 8, W // 2, H // 2                      # the sinogram leg: 8 planes of a quarter of the pixels
    gen = torch.Generator(device="cuda").manual_seed(1)
    image = torch.rand(n, device="cuda", generator=gen) * 79.0 + 1.0
    flat = torch.rand(n, device="cuda", generator=gen) * 10.0 + 80.0
    dark = torch.rand(n, device="cuda", generator=gen) * 0.5
    stack = torch.rand(P * SW * SH, device="cuda", generator=gen) * 79.0 + 1.0
    out = torch.empty(n, device="cuda")
    work = torch.empty(n, device="cuda")
    sino = torch.empty(P * SW * SH, device="cuda")
    out_u8 = torch.empty(n, dtype=torch.uint8, device="cuda")
    one = np.array([1.0], np.float32)

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

    with xrt.Context(0) as ctx:
        def in_place():                                 # (line integrals of line integrals: any finite values cost the same)
            ctx.log_projection_device(W, H, 1, work.data_ptr(), work.data_ptr(), flat_value=80.0, t_min=1e-6)

        legs = [
            ("copy_plane", lambda: out.copy_(image)),
            ("detector_response_1x1", lambda: ctx.detector_response_device(W, H, 1, image.data_ptr(), one, one,
                                                                           out.data_ptr(), out_u8.data_ptr())),
            ("log_projection_scalar_flat", lambda: ctx.log_projection_device(W, H, 1, image.data_ptr(), out.data_ptr(),
                                                                             flat_value=80.0)),
            ("log_projection_in_place", in_place),
            ("log_projection_flat_dark_planes", lambda: ctx.log_projection_device(
                W, H, 1, image.data_ptr(), out.data_ptr(), flat.data_ptr(), dark.data_ptr())),
            (f"log_projection_sinograms_{P}x{SW}x{SH}", lambda: ctx.log_projection_device(
                SW, SH, P, stack.data_ptr(), sino.data_ptr(), flat_value=80.0, sinograms=True)),
        ]
        us = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, launch in legs:
                if name == "log_projection_in_place":
                    work.copy_(image)
                us[name].append(events(launch))
    best = {name: min(v) for name, v in us.items()}
    result = {"size": [W, H], "frames": args.frames, "us_per_launch": us,
              "method": "device events around the launches of one stream, divided by the launches",
              "yardstick": {"log_projection_scalar_flat <= detector_response_1x1 (same run, best of the rounds)":
                            bool(best["log_projection_scalar_flat"] <= best["detector_response_1x1"])},
              "scalar_flat_over_copy": round(best["log_projection_scalar_flat"] / best["copy_plane"], 3),
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
