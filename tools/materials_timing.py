#!/usr/bin/env python3
"""k_render_binned per frame for the signed model, the materials model with one
mesh (the same rays and hits, the per-mesh finish) and the materials model on
a three-mesh scene (a box around the dragon, the dragon, a box beside it), on
dragon.ply at --size, in one process on one device.  The three are measured in
turn, --rounds times, so that clock drift shows as spread between the rounds
and not as a difference between the models.  Per measurement: --frames steady
L-buffer frames inside xrt_timing_begin/end (the render kernel's in-kernel
span, first wave's start to last wave's end) after a warm-up.

    python tools/materials_timing.py [--size 2048 2048] [--frames 200] [--rounds 3] [--json FILE]
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

    import torch
    import simpleraytracing_amd as xrt
    from materials_kit import DRAGON_MU, dragon_scene

    W, H = args.size
    dragon = xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply"))
    scene = dragon_scene(dragon)
    lb = torch.empty(W * H, device="cuda")

    def signed(ctx):
        ctx.upload_mesh(dragon)
        ctx.set_model(xrt.XRT_MODEL_SIGNED, 0.1037)
        return xrt.camera_for_mesh(dragon, W, H)

    def materials_one(ctx):
        ctx.upload_scene([dragon])
        ctx.set_materials([0.1037])
        return xrt.camera_for_mesh(dragon, W, H)

    def materials_scene(ctx):
        ctx.upload_scene(scene)
        ctx.set_materials(DRAGON_MU)
        return xrt.camera_for_scene(scene, W, H)

    cases = [("signed", signed), ("materials_1_mesh", materials_one), ("materials_3_meshes", materials_scene)]
    us = {name: [] for name, _ in cases}
    stats = {}
    with xrt.Context(0) as ctx:
        ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        for _ in range(args.rounds):
            for name, setup in cases:
                cam = setup(ctx)
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
