#!/usr/bin/env python3
"""k_render_binned per frame for the materials model and the spectrum model with
1, 8 and 32 energy bins, all on the three-mesh dragon scene (a box around the
dragon, the dragon, a box beside it) at --size, in one process on one device.
The legs are measured in turn, --rounds times, so that clock drift shows as
spread between the rounds and not as a difference between the legs.  Per
measurement: --frames steady L-buffer frames inside xrt_timing_begin/end (the
render kernel's in-kernel span, first wave's start to last wave's end) after a
warm-up.  The one-bin leg against the materials leg is what the finish of the
spectrum model costs; the 8- and 32-bin legs add the f64 exp of every bin.

    python tools/spectrum_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
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
    dragon = xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply"))
    scene = dragon_scene(dragon)
    cam = xrt.camera_for_scene(scene, W, H)
    lb = torch.empty(W * H, device="cuda")

    def table(K):
        """K equal weights that sum to 80; DRAGON_MU in bin 0, falling 3% a bin."""
        w = np.full(K, 80.0 / K, np.float32)
        mu = (np.asarray(DRAGON_MU, np.float64)[:, None] * 0.97 ** np.arange(K)[None, :]).astype(np.float32)
        return w, mu

    cases = [("materials_3_meshes", lambda ctx: ctx.set_materials(DRAGON_MU))]
    for K in (1, 8, 32):
        cases.append((f"spectrum_3_meshes_{K}_bins", lambda ctx, K=K: ctx.set_spectrum(*table(K))))
    us = {name: [] for name, _ in cases}
    stats = {}
    with xrt.Context(0) as ctx:
        ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        ctx.upload_scene(scene)
        for _ in range(args.rounds):
            for name, setup in cases:
                setup(ctx)
                for _ in range(args.warmup):
                    ctx.render_rows_device(cam, 0, H, 0, lb.data_ptr(), 0)
                torch.cuda.synchronize()
                ctx.timing_begin()
                for _ in range(args.frames):
                    ctx.render_rows_device(cam, 0, H, 0, lb.data_ptr(), 0)
                torch.cuda.synchronize()
                ms, n = ctx.timing_end()
                us[name].append(round(ms * 1e3 / max(n, 1), 2))
                st = ctx.read_stats()
                stats[name] = {"hit_rays": st.hit_rays, "hits": st.hits, "flagged": st.odd_rays,
                               "overflow_rays": st.overflow_rays, "max_hits": st.max_hits}
    out = {"size": [W, H], "frames": args.frames, "kernel_us_per_frame": us, "stats": stats,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
