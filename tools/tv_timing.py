#!/usr/bin/env python3
"""What the TV descent costs: k_tv_gradient, the sum of squares and one descent
step over an N^3 volume beside k_volume_update over the same voxels -- the library's streaming
yardstick: three planes read, one written --, and one iteration of xrt_sirt_tv_device with
--steps descent steps beside one of xrt_sirt_device on section 10.12's scan.  The legs are
measured in turn, --rounds times, so that clock drift shows as spread between the rounds and
not as a difference between the legs.  Every leg: device events around its calls on one stream
after a warm-up, divided by the calls.

    python tools/tv_timing.py [--planes 360] [--plane-size 512 512] [--grid 256] [--steps 10] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=360)
    ap.add_argument("--plane-size", type=int, nargs=2, default=[512, 512], metavar=("W", "H"))
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import simpleraytracing_amd as xrt

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import camera_kit
    import fdk_ref

    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1)

    def events(launch, frames, warmup):
        for _ in range(warmup):
            launch()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(frames):
            launch()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) / frames, 4)

    W, H = args.plane_size
    P, N = args.planes, args.grid
    ps = 0.4
    side = 0.9 * ps * min(W, H) * 100.0 / 150.0 / np.sqrt(2.0)             # the whole grid projects inside the planes
    spacing, origin = np.full(3, side / N, np.float32), np.full(3, -side / 2, np.float32)
    cams = [camera_kit.as_camera(fdk_ref.turntable_camera(2 * np.pi * p / P, 100.0, 150.0, ps), W, H) for p in range(P)]
    A_np = np.stack([xrt.backprojection_matrix(c, origin, spacing) for c in cams])
    dims = (N, N, N)
    volume = torch.rand((N, N, N), device=dev, generator=gen)
    meas = torch.rand((P, H, W), device=dev, generator=gen) * 20.0
    grad, corr = torch.empty_like(volume), torch.rand((N, N, N), device=dev, generator=gen)
    norm = torch.rand((N, N, N), device=dev, generator=gen) + 0.5
    x, y = volume.clone(), volume.clone()
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    tv = (args.steps, 0.2, 1.0, 1e-8)

    with xrt.Context(0) as ctx:
        def gradient():
            ctx.tv_gradient_device(volume.data_ptr(), dims, grad.data_ptr(), 1e-8)

        def sumsq():
            ctx.volume_sumsq_device(N ** 3, grad.data_ptr(), 0, total.data_ptr())

        def sumsq_of_a_difference():
            ctx.volume_sumsq_device(N ** 3, grad.data_ptr(), volume.data_ptr(), total.data_ptr())

        def descent_step():
            ctx.tv_descend_device(y.data_ptr(), dims, 1, 0.01, 1e-8)

        def update():
            ctx.volume_update_device(N ** 3, x.data_ptr(), corr.data_ptr(), norm.data_ptr(), 1.0, 0.0, float("inf"))

        def iteration():
            ctx.sirt_device(W, H, P, meas.data_ptr(), A_np, dims, spacing, 1, x.data_ptr())

        def iteration_with_tv():
            ctx.sirt_device(W, H, P, meas.data_ptr(), A_np, dims, spacing, 1, x.data_ptr(), tv=tv)

        # the gradient and the sum agree with torch's to rounding: the legs time what they say
        gradient()
        sumsq()
        torch.cuda.synchronize()
        sum_diff = abs(float(total[0]) - float((grad.double() ** 2).sum())) / float(total[0])

        legs = [
            ("tv_gradient", gradient, 20, 2),
            ("sumsq", sumsq, 20, 2),
            ("sumsq_of_a_difference", sumsq_of_a_difference, 20, 2),
            ("descent_step", descent_step, 20, 2),
            ("volume_update", update, 20, 2),
            ("sirt_set_up_and_one_iteration", iteration, args.frames, args.warmup),
            ("sirt_tv_set_up_and_one_iteration", iteration_with_tv, args.frames, args.warmup),
        ]
        ms = {name: [] for name, *_ in legs}
        for _ in range(args.rounds):
            for name, launch, frames, warmup in legs:
                ms[name].append(events(launch, frames, warmup))
    best = {name: min(v) for name, v in ms.items()}
    voxels = float(N) ** 3
    tv_ms = best["sirt_tv_set_up_and_one_iteration"] - best["sirt_set_up_and_one_iteration"]
    result = {
        "workload": {"planes": P, "plane_size": [W, H], "grid": [N, N, N], "steps": args.steps},
        "ms_per_call": ms,
        "method": "device events around the calls of one stream, divided by the calls; the legs in turn, per round",
        "tv_gradient_over_volume_update": round(best["tv_gradient"] / best["volume_update"], 3),
        "tv_gradient_G_voxels_per_s": round(voxels / (best["tv_gradient"] * 1e-3) / 1e9, 2),
        "tv_gradient_GB_per_s_at_8_bytes_a_voxel": round(8.0 * voxels / (best["tv_gradient"] * 1e-3) / 1e9, 1),
        "volume_update_GB_per_s_at_16_bytes_a_voxel": round(16.0 * voxels / (best["volume_update"] * 1e-3) / 1e9, 1),
        "descent_step_parts_ms": {"gradient": best["tv_gradient"], "sumsq": best["sumsq"],
                                  "step_by_difference": round(best["descent_step"] - best["tv_gradient"] - best["sumsq"], 4)},
        "tv_ms_per_iteration": round(tv_ms, 3),
        "tv_share_of_the_iteration": round(tv_ms / best["sirt_tv_set_up_and_one_iteration"], 4),
        "agreement": {"sumsq_relative_to_torch": sum_diff},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
