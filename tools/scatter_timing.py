#!/usr/bin/env python3
"""What the scatter estimate costs beside the primary it rides on: one --size plane of the
three-mesh dragon scene (a box around the dragon, the dragon, a box beside it, as
tools/paths_timing.py sets it up), K = 8 bins, traced once into paths planes; then, by
device events around --frames launches on one stream after a warm-up, in turn and --rounds
times in one process, so that clock drift shows as spread between the rounds:

  apply_spectrum          k_apply_spectrum, the yardstick
  source_D*_lbuffer       k_scatter_source writing the L-buffer too, D = 8 and 16
  source_D*               ... the source alone
  blurs_D*                the G = 2 blurs of (41, 41) taps over the coarse plane
  add_D*                  k_scatter_add with G = 2, primary in, total out
  copy                    a device copy of the plane

    python tools/scatter_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
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
    K, G, BINS = 8, 2, (8, 16)
    dragon = xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply"))
    scene = dragon_scene(dragon)
    M = len(scene)
    cam = xrt.camera_for_scene(scene, W, H)
    f32 = dict(dtype=torch.float32, device="cuda")
    lb, total, copy = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32)
    paths = torch.empty(M * n, **f32)
    opn = torch.empty(n, dtype=torch.int16, device="cuda")
    w = np.full(K, 80.0 / K, np.float32)
    mu = (np.asarray(DRAGON_MU, np.float64)[:, None] * 0.97 ** np.arange(K)[None, :]).astype(np.float32)
    sg = (0.4 * mu).astype(np.float32)
    amp = np.array([0.2, 0.05], np.float32)
    coarse = {D: ((W + D - 1) // D, (H + D - 1) // D) for D in BINS}
    src = {D: torch.empty(coarse[D][0] * coarse[D][1], **f32) for D in BINS}
    blurred = {D: torch.empty(G * coarse[D][0] * coarse[D][1], **f32) for D in BINS}
    taps = {D: [xrt.scatter_gaussian(5.0 * D * (g + 1), D, 41) for g in range(G)] for D in BINS}

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
        ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        ctx.upload_scene(scene)
        ctx.set_paths()
        ctx.render_paths_device(cam, 0, H, M, paths.data_ptr(), opn.data_ptr())
        st = ctx.read_stats()
        torch.cuda.synchronize()

        def blurs(D):
            wc, hc = coarse[D]
            for g in range(G):
                ctx.detector_response_device(wc, hc, 1, src[D].data_ptr(), taps[D][g], taps[D][g],
                                             blurred[D].data_ptr() + 4 * g * wc * hc)

        legs = [("apply_spectrum", lambda: ctx.apply_spectrum_device(n, paths.data_ptr(), opn.data_ptr(), w, mu, lb.data_ptr()))]
        for D in BINS:
            legs += [
                (f"source_D{D}_lbuffer", lambda D=D: ctx.scatter_source_device(W, H, 1, paths.data_ptr(), opn.data_ptr(), w, mu, sg,
                                                                               D, lb.data_ptr(), src[D].data_ptr())),
                (f"source_D{D}", lambda D=D: ctx.scatter_source_device(W, H, 1, paths.data_ptr(), opn.data_ptr(), w, mu, sg, D, 0,
                                                                       src[D].data_ptr())),
                (f"blurs_D{D}", lambda D=D: blurs(D)),
                (f"add_D{D}", lambda D=D: ctx.scatter_add_device(W, H, 1, D, blurred[D].data_ptr(), amp, lb.data_ptr(),
                                                                 total.data_ptr())),
            ]
        legs.append(("copy", lambda: copy.copy_(lb)))
        for name, _ in legs:
            us[name] = []
        for _ in range(args.rounds):
            for name, launch in legs:
                us[name].append(events(launch))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    estimate = {f"D{D}": round((med[f"source_D{D}_lbuffer"] + med[f"blurs_D{D}"] + med[f"add_D{D}"]) / med["apply_spectrum"], 3)
                for D in BINS}
    out = {"size": [W, H], "frames": args.frames, "bins": K, "meshes": M, "kernels": G, "us_per_launch": us,
           "median_us": med, "estimate_over_apply_spectrum": estimate,
           "note": "estimate = (source with the L-buffer + blurs + add) / apply_spectrum, medians of one run; the source "
                   "with the L-buffer replaces apply_spectrum, so the estimate's extra cost is that ratio minus 1",
           "stats": {"hit_rays": st.hit_rays, "open": st.odd_rays}, "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
