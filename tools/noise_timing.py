#!/usr/bin/env python3
"""What the photon noise costs: k_photon_noise over one --size plane at a mean near 10^4 (the normal
branch) and near 10 (the search branch, which diverges: a wave runs as long as its slowest pixel),
out of place and in place, beside a device-to-device copy of the plane (one read and one write: the
memory floor), the detector response under 41 taps on each axis, k_lsf (41,41), and the line
integrals, k_log_projection with a scalar flat: the passes around this one in the post-trace chain.
One process, one device; the legs are measured in turn, --rounds times, so that clock drift shows
as spread between the rounds and not as a difference between the legs.  Every leg: device events
around --frames launches on one stream after a warm-up, divided by the launches.  The planes are
seeded intensities: (40, 80] under a gain of 166 (means of 6640 to 13280) and of 1/6 (6.7 to 13.3).
Also a dark plane -- a mean of 0.01, where the search ends at once -- and one that mixes the
branches lane by lane.

    python tools/noise_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
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

    import torch
    import simpleraytracing_amd as xrt

    W, H = args.size
    n = W * H
    gen = torch.Generator(device="cuda").manual_seed(1)
    image = torch.rand(n, device="cuda", generator=gen) * 40.0 + 40.0
    mixed = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.5, image, image * 1e-3)
    out = torch.empty(n, device="cuda")
    work = torch.empty(n, device="cuda")
    out_u8 = torch.empty(n, dtype=torch.uint8, device="cuda")
    lsf = xrt.lsf_gaussian(6.0, 41)
    HI, LO, DARK = 166.0, 1.0 / 6.0, 1.0 / 6000.0

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
        def noise(src, dst, gain):
            return lambda: ctx.photon_noise_device(W, H, 1, src.data_ptr(), dst.data_ptr(), gain, 7)

        launches = [0]

        def in_place():
            # (a noisy plane's noise: the same means.  A seed per launch: under one seed a pixel meets the same
            # deviate every time and its mean walks off, downwards into the search branch for half of them)
            launches[0] += 1
            ctx.photon_noise_device(W, H, 1, work.data_ptr(), work.data_ptr(), 1.0, launches[0])

        legs = [
            ("copy_plane", lambda: out.copy_(image)),
            ("detector_response_41x41", lambda: ctx.detector_response_device(W, H, 1, image.data_ptr(), lsf, lsf,
                                                                             out.data_ptr(), out_u8.data_ptr())),
            ("log_projection_scalar_flat", lambda: ctx.log_projection_device(W, H, 1, image.data_ptr(), out.data_ptr(),
                                                                             flat_value=80.0)),
            ("photon_noise_mean_1e4", noise(image, out, HI)),
            ("photon_noise_mean_1e4_in_place", in_place),
            ("photon_noise_mean_10", noise(image, out, LO)),
            ("photon_noise_mean_0.01", noise(image, out, DARK)),
            ("photon_noise_mixed_1e4_and_10", noise(mixed, out, HI)),
        ]
        us = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, launch in legs:
                if name.endswith("in_place"):
                    work.copy_(image * HI)
                us[name].append(events(launch))
    best = {name: min(v) for name, v in us.items()}
    result = {"size": [W, H], "frames": args.frames, "us_per_launch": us,
              "method": "device events around the launches of one stream, divided by the launches",
              "yardstick": {"photon_noise_mean_1e4 <= detector_response_41x41 (same run, best of the rounds)":
                            bool(best["photon_noise_mean_1e4"] <= best["detector_response_41x41"])},
              "mean_1e4_over_copy": round(best["photon_noise_mean_1e4"] / best["copy_plane"], 3),
              "mean_10_over_mean_1e4": round(best["photon_noise_mean_10"] / best["photon_noise_mean_1e4"], 3),
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
