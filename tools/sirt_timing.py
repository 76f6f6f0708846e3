#!/usr/bin/env python3
"""What SIRT costs: k_forward_project over --planes planes of --plane-size pixels
through an N^3 grid beside k_volume_paths -- the project's other walker, at one label with a
density, tracing the same grid from the same cameras in the same process, one launch a camera --
and one SIRT iteration at that size split into its three kernels, beside the backprojector that
is FDK's.  The legs are measured in turn, --rounds times, so that clock drift shows as spread
between the rounds and not as a difference between the legs.  Every leg: device events around
its launches on one stream after a warm-up, divided by the launches.  The two walkers must agree
to the f32 rounding of the trace's ray directions; the largest difference is reported, and the
steps a ray takes are counted on the host from the mean chord (steps = voxel boundaries crossed).

    python tools/sirt_timing.py [--planes 360] [--plane-size 512 512] [--grid 256] [--rounds 3] [--json FILE]
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
        return round(t0.elapsed_time(t1) / frames, 3)

    W, H = args.plane_size
    P, N = args.planes, args.grid
    ps = 0.4
    side = 0.9 * ps * min(W, H) * 100.0 / 150.0 / np.sqrt(2.0)             # the whole grid projects inside the planes
    spacing, origin = np.full(3, side / N, np.float32), np.full(3, -side / 2, np.float32)
    cams = [camera_kit.as_camera(fdk_ref.turntable_camera(2 * np.pi * p / P, 100.0, 150.0, ps), W, H) for p in range(P)]
    A_np = np.stack([xrt.backprojection_matrix(c, origin, spacing) for c in cams])
    R_np = np.stack([xrt.ray_matrix(a) for a in A_np])
    A, R = (torch.from_numpy(m.reshape(-1)).to(dev) for m in (A_np, R_np))
    dims = (N, N, N)
    volume = torch.rand((N, N, N), device=dev, generator=gen)
    meas = torch.rand((P, H, W), device=dev, generator=gen) * 20.0
    out = torch.empty((P, H, W), device=dev)
    trace = torch.empty((P, H, W), device=dev)
    corr, norm = torch.empty_like(volume), torch.rand((N, N, N), device=dev, generator=gen) + 0.5
    x = volume.clone()

    with xrt.Context(0) as ctx:
        ctx.upload_volume(np.ones((N, N, N), np.uint8), spacing, origin, density=volume.cpu().numpy())
        plane_bytes = 4 * H * W

        def walk_forward():
            ctx.forward_project_device(W, H, P, volume.data_ptr(), dims, spacing, R.data_ptr(), out.data_ptr())

        def walk_residual():
            ctx.forward_project_device(W, H, P, volume.data_ptr(), dims, spacing, R.data_ptr(), out.data_ptr(),
                                       xrt.XRT_FP_RESIDUAL, meas.data_ptr())

        def walk_trace():
            for p in range(P):
                ctx.volume_paths_device(cams[p], 0, H, 1, trace.data_ptr() + p * plane_bytes)

        def backproject():
            ctx.backproject_device(W, H, P, out.data_ptr(), A.data_ptr(), dims, 0, N, 1.0, False, corr.data_ptr())

        def update():
            ctx.volume_update_device(N ** 3, x.data_ptr(), corr.data_ptr(), norm.data_ptr(), 1.0, 0.0, float("inf"))

        def iteration():
            ctx.sirt_device(W, H, P, meas.data_ptr(), A_np, dims, spacing, 1, x.data_ptr())

        def set_up_and_iteration_of_12_subsets():
            ctx.sirt_device(W, H, P, meas.data_ptr(), A_np, dims, spacing, 1, x.data_ptr(), subsets=12)

        walk_forward()
        walk_trace()
        torch.cuda.synchronize()
        top = float(trace.max())
        walkers_diff = float((out - trace).abs().max()) / top
        # a ray crosses about chord / spacing voxel boundaries on each axis' share: count from the uniform chord
        ctx.forward_project_device(W, H, P, torch.ones_like(volume).data_ptr(), dims, spacing, R.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        mean_chord = float(out.double().mean())

        legs = [
            ("forward_project", walk_forward, args.frames, args.warmup),
            ("forward_residual", walk_residual, args.frames, args.warmup),
            ("volume_paths_one_label_density", walk_trace, args.frames, args.warmup),
            ("backproject", backproject, args.frames, args.warmup),
            ("volume_update", update, 20, 2),
            ("sirt_set_up_and_one_iteration", iteration, args.frames, args.warmup),
            ("os_sart_12_subsets_set_up_and_one_iteration", set_up_and_iteration_of_12_subsets, args.frames, args.warmup),
        ]
        ms = {name: [] for name, *_ in legs}
        for _ in range(args.rounds):
            for name, launch, frames, warmup in legs:
                ms[name].append(events(launch, frames, warmup))
    best = {name: min(v) for name, v in ms.items()}
    # steps: a ray of chord c crosses |dx| + |dy| + |dz| boundaries, between c / s and sqrt(3) c / s; the mean direction
    # of a turn about z lies in the xy plane: about (4 / pi) c / s
    steps = float(P) * H * W * (4.0 / np.pi) * mean_chord / float(spacing[0])
    result = {
        "workload": {"planes": P, "plane_size": [W, H], "grid": [N, N, N], "mean_chord_voxels": round(mean_chord / float(spacing[0]), 1)},
        "ms_per_call": ms,
        "method": "device events around the calls of one stream, divided by the calls; the legs in turn, per round",
        "forward_project_over_volume_paths": round(best["forward_project"] / best["volume_paths_one_label_density"], 3),
        "forward_project_G_steps_per_s": round(steps / (best["forward_project"] * 1e-3) / 1e9, 2),
        "volume_paths_G_steps_per_s": round(steps / (best["volume_paths_one_label_density"] * 1e-3) / 1e9, 2),
        "one_iteration_ms": {"project": best["forward_residual"], "backproject": best["backproject"], "update": best["volume_update"],
                             "sum": round(best["forward_residual"] + best["backproject"] + best["volume_update"], 3)},
        "iteration_over_fdk_backprojection": round((best["forward_residual"] + best["backproject"] + best["volume_update"]) / best["backproject"], 2),
        "yardstick": {"forward_project <= volume_paths (best of the rounds)":
                          bool(best["forward_project"] <= best["volume_paths_one_label_density"])},
        "agreement": {"walkers_max_abs_diff_over_max": walkers_diff},
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
