#!/usr/bin/env python3
"""Material decomposition beside the detector it inverts: k_decompose over the expected channels of the
three-mesh dragon scene (a box around the dragon, the dragon, a box beside it) at --size, in one process on
one device.  For each (B, C, K) the first B planes of the paths render are the basis line integrals; the
detector's EXPECTED launch over them at the same C and K is the yardstick, measured beside the
decomposition's legs.  The legs are measured in turn, --rounds times, so that clock drift shows as spread
between the rounds and not as a difference between the legs; each leg is device events around --frames
launches on one stream after a warm-up, divided by the launches.

  detector_expected_B_C_K     spectral_detector_device, XRT_DETECT_EXPECTED (the yardstick)
  decompose_B_C_K_iterN       decompose_device, tol = 0, max_iter = N in 1, 4, 8: every unmasked pixel runs N
                              iterations, so the slope over N is the cost of one iteration of the whole frame
  decompose_B_C_K_tol         tol = 1e-6, max_iter = 32: what leaving early saves on a frame that is mostly
                              background; `iters` holds that launch's histogram of statuses

    python tools/decompose_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [(2, 2, 8), (2, 4, 8), (3, 8, 8), (2, 4, 32)]


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
    import decompose_kit as kit
    from materials_kit import dragon_scene

    W, H = args.size
    n = W * H
    dragon = xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply"))
    scene = dragon_scene(dragon)
    M = len(scene)
    cam = xrt.camera_for_scene(scene, W, H)
    paths = torch.empty(M * n, device="cuda")
    opn = torch.empty(n, dtype=torch.int16, device="cuda")
    channels = torch.empty(8 * n, device="cuda")
    out = torch.empty(3 * n, device="cuda")
    iters = torch.empty(n, dtype=torch.uint8, device="cuda")

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

    us, hist, worst = {}, {}, {}
    with xrt.Context(0) as ctx:
        ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        ctx.upload_scene(scene)
        ctx.set_paths()
        ctx.render_paths_device(cam, 0, H, M, paths.data_ptr(), opn.data_ptr())
        torch.cuda.synchronize()
        st = ctx.read_stats()
        for _ in range(args.rounds):
            for B, C, K in CONFIGS:
                w, mu = kit.table(B, K)
                r = kit.windows(C, K)
                guess = xrt.decompose_guess(w, mu, r)
                tag = f"{B}_{C}_{K}"

                def detect():
                    ctx.spectral_detector_device(n, paths.data_ptr(), opn.data_ptr(), w, mu, r, channels.data_ptr(), 1.0, 0,
                                                 False, True)

                def decompose(max_iter, tol):
                    return lambda: ctx.decompose_device(n, channels.data_ptr(), opn.data_ptr(), w, mu, r, out.data_ptr(),
                                                        iters.data_ptr(), 1.0, True, guess, max_iter, tol)

                us.setdefault(f"detector_expected_{tag}", []).append(events(detect))        # (leaves the channels behind)
                for N in (1, 4, 8):
                    us.setdefault(f"decompose_{tag}_iter{N}", []).append(events(decompose(N, 0.0)))
                us.setdefault(f"decompose_{tag}_tol", []).append(events(decompose(32, 1e-6)))
                torch.cuda.synchronize()
                hist[tag] = {str(k): int(v) for k, v in enumerate(np.bincount(iters.cpu().numpy(), minlength=256)) if v}
                keep = (opn.cpu().numpy() == 0)
                got = out.cpu().numpy()[:B * n].reshape(B, n)[:, keep]
                want = paths.cpu().numpy()[:B * n].reshape(B, n)[:, keep]
                worst[tag] = float(np.max(np.abs(got - want)))
    slopes = {}
    for B, C, K in CONFIGS:
        tag = f"{B}_{C}_{K}"
        lo, hi = min(us[f"decompose_{tag}_iter1"]), min(us[f"decompose_{tag}_iter8"])
        slope = (hi - lo) / 7.0
        slopes[tag] = {"us_per_iteration": round(slope, 2),
                       "over_detector": round(slope / min(us[f"detector_expected_{tag}"]), 3), "one_plus_B": 1 + B}
    result = {"size": [W, H], "frames": args.frames, "us_per_launch": us, "slopes": slopes, "iters": hist,
              "largest_error_against_the_paths": worst, "method": "device events around the launches",
              "stats": {"hit_rays": st.hit_rays, "open": st.odd_rays}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
