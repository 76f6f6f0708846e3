#!/usr/bin/env python3
"""What OS-MLTR costs, on tools/sirt_timing.py's workload and by its method:
k_poisson_project beside k_forward_project in residual mode, k_backproject_update beside the
composition it replaces -- two backprojections and the voxel update --, and one MLTR iteration
beside one SIRT iteration at one subset and at twelve.  The legs are measured in turn, --rounds
times, so that clock drift shows as spread between the rounds and not as a difference between
the legs.  Every leg: device events around its launches on one stream after a warm-up, divided
by the launches.  The fused kernel's volume is compared bit for bit with the composition's.

    python tools/mltr_timing.py [--planes 360] [--plane-size 512 512] [--grid 256] [--rounds 3] [--json FILE]
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
    inf = float("inf")
    # a volume whose line integrals stay below 3, so that the expected counts are ordinary numbers
    volume = torch.rand((N, N, N), device=dev, generator=gen) * float(3.0 / (side * np.sqrt(3.0)))
    meas = torch.rand((P, H, W), device=dev, generator=gen) * 20.0
    counts = torch.poisson(torch.rand((P, H, W), device=dev, generator=gen) * 1000.0, generator=gen)
    flat = torch.full((H, W), 1000.0, device=dev)
    background = torch.full((P, H, W), 20.0, device=dev)
    out = torch.empty((P, H, W), device=dev)
    pairs = torch.empty((P, H, W, 2), device=dev)
    corr, norm = torch.empty_like(volume), torch.empty_like(volume)
    x = volume.clone()

    with xrt.Context(0) as ctx:
        def forward_residual():
            ctx.forward_project_device(W, H, P, volume.data_ptr(), dims, spacing, R.data_ptr(), out.data_ptr(),
                                       xrt.XRT_FP_RESIDUAL, meas.data_ptr())

        def poisson_project():
            ctx.poisson_project_device(W, H, P, volume.data_ptr(), dims, spacing, R.data_ptr(), counts.data_ptr(),
                                       flat.data_ptr(), pairs.data_ptr())

        def poisson_project_background():
            ctx.poisson_project_device(W, H, P, volume.data_ptr(), dims, spacing, R.data_ptr(), counts.data_ptr(),
                                       flat.data_ptr(), pairs.data_ptr(), background.data_ptr())

        def backproject():
            ctx.backproject_device(W, H, P, out.data_ptr(), A.data_ptr(), dims, 0, N, 1.0, False, corr.data_ptr())

        def composition(target=x):
            ctx.backproject_device(W, H, P, num.data_ptr(), A.data_ptr(), dims, 0, N, 1.0, False, corr.data_ptr())
            ctx.backproject_device(W, H, P, den.data_ptr(), A.data_ptr(), dims, 0, N, 1.0, False, norm.data_ptr())
            ctx.volume_update_device(N ** 3, target.data_ptr(), corr.data_ptr(), norm.data_ptr(), 1.0, 0.0, inf)

        def backproject_update(target=x):
            ctx.backproject_update_device(W, H, P, pairs.data_ptr(), A.data_ptr(), dims, target.data_ptr(), 1.0, 0.0, inf)

        def mltr(subsets):
            return lambda: ctx.mltr_device(W, H, P, counts.data_ptr(), flat.data_ptr(), A_np, dims, spacing, 1, x.data_ptr(),
                                           subsets=subsets, d_background=background.data_ptr())

        def sirt(subsets):
            return lambda: ctx.sirt_device(W, H, P, meas.data_ptr(), A_np, dims, spacing, 1, x.data_ptr(), subsets=subsets)

        poisson_project_background()
        torch.cuda.synchronize()
        num, den = pairs[..., 0].contiguous(), pairs[..., 1].contiguous()
        a, b = volume.clone(), volume.clone()
        backproject_update(a)
        composition(b)
        torch.cuda.synchronize()
        equal = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        moved = int((a != volume).sum())

        legs = [
            ("forward_residual", forward_residual, args.frames, args.warmup),
            ("poisson_project", poisson_project, args.frames, args.warmup),
            ("poisson_project_with_background", poisson_project_background, args.frames, args.warmup),
            ("backproject", backproject, args.frames, args.warmup),
            ("two_backprojections_and_update", composition, args.frames, args.warmup),
            ("backproject_update", backproject_update, args.frames, args.warmup),
            ("mltr_one_iteration", mltr(1), args.frames, args.warmup),
            ("sirt_set_up_and_one_iteration", sirt(1), args.frames, args.warmup),
            ("mltr_12_subsets_one_iteration", mltr(12), args.frames, args.warmup),
            ("os_sart_12_subsets_set_up_and_one_iteration", sirt(12), args.frames, args.warmup),
        ]
        ms = {name: [] for name, *_ in legs}
        for _ in range(args.rounds):
            for name, launch, frames, warmup in legs:
                ms[name].append(events(launch, frames, warmup))
    best = {name: min(v) for name, v in ms.items()}
    result = {
        "workload": {"planes": P, "plane_size": [W, H], "grid": [N, N, N]},
        "ms_per_call": ms,
        "method": "device events around the calls of one stream, divided by the calls; the legs in turn, per round",
        "poisson_project_over_forward_residual": round(best["poisson_project"] / best["forward_residual"], 3),
        "poisson_project_with_background_over_forward_residual":
            round(best["poisson_project_with_background"] / best["forward_residual"], 3),
        "backproject_update_over_composition": round(best["backproject_update"] / best["two_backprojections_and_update"], 3),
        "backproject_update_over_one_backprojection": round(best["backproject_update"] / best["backproject"], 3),
        "mltr_over_sirt_iteration": {"1 subset": round(best["mltr_one_iteration"] / best["sirt_set_up_and_one_iteration"], 3),
                                     "12 subsets": round(best["mltr_12_subsets_one_iteration"] /
                                                         best["os_sart_12_subsets_set_up_and_one_iteration"], 3)},
        "note": "a SIRT call also backprojects its norm volumes once (its set-up); an MLTR call has none",
        "agreement": {"backproject_update_equals_composition_bit_for_bit": equal, "voxels_moved": moved},
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
