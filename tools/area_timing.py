#!/usr/bin/env python3
"""What area sampling costs: k_area_integrate over --size written pixels at bin 2 (one source and nine), bin 4
(at half the size: the same input), bin 1 with nine sources and bin 3 (the pixel-by-pixel form), each beside a
device-to-device copy of that leg's own INPUT bytes, and the line integrals, k_log_projection with a scalar flat,
for scale.  The copy reads the input and writes as much again; the pass reads it once and writes 1 / (S bin^2) of
it, so a pass that is bound by memory costs no more than its copy: that is the yardstick of the bin 1, 2 and 4
legs (bin 3 is reported only).  One process, one device; the legs are measured in turn, --rounds times, so that
clock drift shows as spread between the rounds and not as a difference between the legs.  Every leg: device events
around --frames launches on one stream after a warm-up, divided by the launches.  The same buffers are launched
over and over, so whatever of a leg's bytes fits the 256 MiB Infinity Cache may be served from it, for the pass
and for its copy alike: each leg's bytes are reported beside its times.

    python tools/area_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
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
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import simpleraytracing_amd as xrt

    W, H = args.size
    # (name, written W, written H, bin, sources, held to the yardstick)
    passes = [("bin2_S1", W, H, 2, 1, True), ("bin4_S1_half_size", W // 2, H // 2, 4, 1, True),
              ("bin1_S9", W, H, 1, 9, True), ("bin2_S9", W, H, 2, 9, True), ("bin3_S1", W, H, 3, 1, False)]
    most = max(w * h * b * b * s for _, w, h, b, s, _ in passes)
    gen = torch.Generator(device="cuda").manual_seed(1)
    image = torch.rand(most, device="cuda", generator=gen) * 80.0
    twin = torch.empty(most, device="cuda")
    out = torch.empty(W * H, device="cuda")

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
        legs, info = [], {}
        for name, w, h, b, s, held in passes:
            n_in = w * h * b * b * s
            weights = np.ones(s, np.float32)
            legs.append(("copy_input_" + name, lambda n=n_in: twin[:n].copy_(image[:n])))
            legs.append(("area_" + name, lambda w=w, h=h, b=b, wt=weights: ctx.area_integrate_device(
                w, h, 1, image.data_ptr(), out.data_ptr(), 0, b, wt)))
            info[name] = {"written": [w, h], "bin": b, "sources": s, "input_bytes": 4 * n_in, "output_bytes": 4 * w * h,
                          "copy_moves_bytes": 8 * n_in, "pass_moves_bytes": 4 * n_in + 4 * w * h, "yardstick": held}
        legs.append(("log_projection_scalar_flat", lambda: ctx.log_projection_device(W, H, 1, image.data_ptr(),
                                                                                     out.data_ptr(), flat_value=80.0)))
        us = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, launch in legs:
                us[name].append(events(launch))
    best = {name: min(v) for name, v in us.items()}
    for name, leg in info.items():
        leg["pass_over_copy"] = round(best["area_" + name] / best["copy_input_" + name], 3)
        leg["pass_TB_per_s"] = round(leg["pass_moves_bytes"] / best["area_" + name] / 1e6, 2)
        leg["copy_TB_per_s"] = round(leg["copy_moves_bytes"] / best["copy_input_" + name] / 1e6, 2)
        if leg["yardstick"]:
            leg["met"] = bool(best["area_" + name] <= best["copy_input_" + name])
    result = {"size": [W, H], "frames": args.frames, "us_per_launch": us, "legs": info,
              "method": "device events around the launches of one stream, divided by the launches; best of the rounds "
                        "compared; buffers relaunched in place, so bytes within the 256 MiB Infinity Cache may stay there",
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
