#!/usr/bin/env python3
"""The spectral detector beside the parent's kernels it fuses: k_spectral_detector over the paths
render's planes of the three-mesh dragon scene (a box around the dragon, the dragon, a box beside it)
at --size, in one process on one device.  The legs are measured in turn, --rounds times, so that clock
drift shows as spread between the rounds and not as a difference between the legs; each leg is device
events around --frames repetitions on one stream after a warm-up, divided by the repetitions.

  apply_spectrum_K          k_apply_spectrum, K bins (the yardstick of the expected legs)
  detector_expected_c1_K    XRT_DETECT_EXPECTED, one channel of ones
  unfused_noisy_8           k_apply_spectrum with 8 bins and eight k_photon_noise launches over planes
                            of the same per-bin means (the unfused route's launches, without its
                            accumulation passes: the yardstick of detector_noisy_c1_8)
  detector_noisy_*          XRT_DETECT_NOISY: one channel, eight channels, 32 bins, a dark gain (every
                            mean in the search branch), read noise on

    python tools/detector_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    paths = torch.empty(M * n, device="cuda")
    opn = torch.empty(n, dtype=torch.int16, device="cuda")
    out = torch.empty(8 * n, device="cuda")
    means = torch.empty(8 * n, device="cuda")
    GAIN, DARK, SEED = 1000.0, 0.05, 2024

    def table(K):
        """K equal weights that sum to 80; DRAGON_MU in bin 0, falling 3% a bin."""
        w = np.full(K, 80.0 / K, np.float32)
        mu = (np.asarray(DRAGON_MU, np.float64)[:, None] * 0.97 ** np.arange(K)[None, :]).astype(np.float32)
        return w, mu

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

    ones = {K: np.ones((1, K), np.float32) for K in (8, 32)}
    eight = {K: np.tile(np.linspace(20.0, 120.0, K, dtype=np.float32), (8, 1)) for K in (8, 32)}
    us = {}
    with xrt.Context(0) as ctx:
        ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        ctx.upload_scene(scene)
        ctx.set_paths()
        ctx.render_paths_device(cam, 0, H, M, paths.data_ptr(), opn.data_ptr())
        torch.cuda.synchronize()
        st = ctx.read_stats()
        w8, mu8 = table(8)
        for e in range(8):                                  # the unfused route's planes: bin e's mean over gain
            ctx.apply_spectrum_device(n, paths.data_ptr(), opn.data_ptr(), w8[e:e + 1], mu8[:, e:e + 1],
                                      means.data_ptr() + 4 * e * n)
        torch.cuda.synchronize()

        def detect(K, response, noisy, gain=GAIN, read_noise=0.0):
            w, mu = table(K)
            return lambda: ctx.spectral_detector_device(n, paths.data_ptr(), opn.data_ptr(), w, mu, response, out.data_ptr(),
                                                        gain, SEED, noisy, True, read_noise)

        def apply(K):
            w, mu = table(K)
            return lambda: ctx.apply_spectrum_device(n, paths.data_ptr(), opn.data_ptr(), w, mu, lb.data_ptr())

        def unfused():
            apply8()
            for e in range(8):
                ctx.photon_noise_device(W, H, 1, means.data_ptr() + 4 * e * n, out.data_ptr() + 4 * e * n, GAIN, SEED, True,
                                        e * n)

        apply8 = apply(8)
        legs = {
            "apply_spectrum_8": apply8,
            "detector_expected_c1_8": detect(8, ones[8], False, 1.0),
            "apply_spectrum_32": apply(32),
            "detector_expected_c1_32": detect(32, ones[32], False, 1.0),
            "unfused_noisy_8": unfused,
            "detector_noisy_c1_8": detect(8, ones[8], True),
            "detector_expected_c8_8": detect(8, eight[8], False, 1.0),
            "detector_noisy_c8_8": detect(8, eight[8], True),
            "detector_noisy_c1_32": detect(32, ones[32], True),
            "detector_noisy_dark_c1_8": detect(8, ones[8], True, DARK),
            "detector_noisy_read_noise_c1_8": detect(8, ones[8], True, GAIN, 30.0),
        }
        us = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, leg in legs.items():
                us[name].append(events(leg))
    result = {"size": [W, H], "frames": args.frames, "us_per_launch": us, "gain": GAIN, "dark_gain": DARK,
              "method": "device events around the launches",
              "stats": {"hit_rays": st.hit_rays, "open": st.odd_rays}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
