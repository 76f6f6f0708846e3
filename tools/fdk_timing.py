#!/usr/bin/env python3
"""What FDK reconstruction costs: k_fdk_filter over --filter-planes planes of
--filter-size pixels under 2 W - 1 taps, and k_backproject of --planes planes of --plane-size
pixels into an N^3 grid, each beside a plain PyTorch statement of the same contract on the same
device in the same process -- a Toeplitz matmul in f64 for the filter (the weight product and the
two conversions included, the matrix built ahead; its time does not depend on the table, so the
Ram-Lak table's leg and the Hann table's, which has no zeros to leave out, share it), f64 matrix arithmetic and indexed gathers for
the backprojector -- and beside a device-to-device copy of the volume (the memory floor).  The
legs are measured in turn, --rounds times, so that clock drift shows as spread between the rounds
and not as a difference between the legs.  Every leg: device events around its launches on one
stream after a warm-up, divided by the launches.  The two statements must agree with the kernels
(to f32 rounding: PyTorch's matmul reorders the sums); the largest differences are reported.

    python tools/fdk_timing.py [--filter-size 2048 2048] [--filter-planes 16] [--planes 360]
                               [--plane-size 512 512] [--grid 256] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter-size", type=int, nargs=2, default=[2048, 2048], metavar=("W", "H"))
    ap.add_argument("--filter-planes", type=int, default=16)
    ap.add_argument("--planes", type=int, default=360)
    ap.add_argument("--plane-size", type=int, nargs=2, default=[512, 512], metavar=("W", "H"))
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import simpleraytracing_amd as xrt

    sys.path.insert(0, os.path.join(ROOT, "tests"))
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

    # ---- the filter
    FW, FH = args.filter_size
    FP, T = args.filter_planes, 2 * FW - 1
    image = torch.rand((FP, FH, FW), device=dev, generator=gen)
    weight = torch.rand((FH, FW), device=dev, generator=gen) * 0.5 + 0.5
    taps = torch.from_numpy(xrt.ramp_filter(T)).to(dev)                   # Ram-Lak: Context.fdk's default
    hann = torch.from_numpy(xrt.ramp_filter(T, xrt.XRT_RAMP_HANN)).to(dev)   # no zeros: every term runs
    f_out = torch.empty_like(image)
    i = torch.arange(FW, device=dev)
    toeplitz = taps.double()[(i[:, None] - i[None, :]) + (FW - 1)]          # [pixel, output] = taps[pixel - output + r]

    def torch_filter():
        return ((image * weight).double().reshape(-1, FW) @ toeplitz).float().reshape(FP, FH, FW)

    # ---- the backprojector
    W, H = args.plane_size
    P, N = args.planes, args.grid
    proj = torch.rand((P, H, W), device=dev, generator=gen)
    ps = 0.4
    side = 0.9 * ps * min(W, H) * 100.0 / 150.0 / np.sqrt(2.0)             # the whole grid projects inside the planes
    spacing, origin = np.full(3, side / N, np.float32), np.full(3, -side / 2, np.float32)
    import camera_kit
    mats_np = np.stack([xrt.backprojection_matrix(
        camera_kit.as_camera(fdk_ref.turntable_camera(2 * np.pi * p / P, 100.0, 150.0, ps), W, H), origin, spacing)
        for p in range(P)])
    mats = torch.from_numpy(mats_np.reshape(-1)).to(dev)
    volume = torch.empty((N, N, N), device=dev)
    copy = torch.empty_like(volume)
    dims = (N, N, N)

    def torch_backproject():
        idx = torch.arange(N, device=dev, dtype=torch.float64)
        k, j, ii = idx[:, None, None], idx[None, :, None], idx[None, None, :]
        acc = torch.zeros((N, N, N), device=dev, dtype=torch.float64)
        zero = torch.zeros((), device=dev)
        for p in range(P):
            m = [float(v) for v in mats_np[p].reshape(-1)]
            a = m[0] * ii + ((m[1] * j + m[2] * k) + m[3])
            b = m[4] * ii + ((m[5] * j + m[6] * k) + m[7])
            c = m[8] * ii + ((m[9] * j + m[10] * k) + m[11])
            w = 1.0 / c
            col, row = a * w, b * w
            ok = (c > 0) & (col > -1) & (col < W) & (row > -1) & (row < H)
            col, row = torch.where(ok, col, 0.0), torch.where(ok, row, 0.0)
            fc, fr = torch.floor(col), torch.floor(row)
            fx, fy = (col - fc).float(), (row - fr).float()
            x0, y0 = fc.long(), fr.long()
            plane = proj[p]

            def s(y, x):
                inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                return torch.where(inside, plane[y.clamp(0, H - 1), x.clamp(0, W - 1)], zero)
            s00, s01, s10, s11 = s(y0, x0), s(y0, x0 + 1), s(y0 + 1, x0), s(y0 + 1, x0 + 1)
            top = s00 + fx * (s01 - s00)
            bot = s10 + fx * (s11 - s10)
            v = top + fy * (bot - top)
            acc = torch.where(ok, acc + v.double() * (w * w), acc)
        return (acc * 0.5).float()

    with xrt.Context(0) as ctx:
        def hip_filter():
            ctx.fdk_filter_device(FW, FH, FP, image.data_ptr(), taps.data_ptr(), T, f_out.data_ptr(), weight.data_ptr())

        def hip_filter_hann():
            ctx.fdk_filter_device(FW, FH, FP, image.data_ptr(), hann.data_ptr(), T, f_out.data_ptr(), weight.data_ptr())

        def hip_backproject():
            ctx.backproject_device(W, H, P, proj.data_ptr(), mats.data_ptr(), dims, 0, N, 0.5, False, volume.data_ptr())

        # the two statements agree with the kernels
        hip_filter()
        hip_backproject()
        torch.cuda.synchronize()
        ref = torch_filter()
        filter_diff = float((ref - f_out).abs().max() / ref.abs().max())
        del ref
        ref = torch_backproject()
        backproject_bits_equal = bool(torch.equal(ref.view(torch.int32), volume.view(torch.int32)))
        backproject_diff = float((ref - volume).abs().max() / ref.abs().max())
        del ref

        legs = [
            ("filter_hip", hip_filter, args.frames, args.warmup),
            ("filter_hip_hann", hip_filter_hann, args.frames, args.warmup),
            ("filter_torch_toeplitz_f64", torch_filter, args.frames, args.warmup),
            ("backproject_hip", hip_backproject, args.frames, args.warmup),
            ("backproject_torch_f64_gathers", torch_backproject, 1, 0),
            ("copy_volume", lambda: copy.copy_(volume), 50, 5),
        ]
        ms = {name: [] for name, *_ in legs}
        for _ in range(args.rounds):
            for name, launch, frames, warmup in legs:
                ms[name].append(events(launch, frames, warmup))
    best = {name: min(v) for name, v in ms.items()}
    updates = float(P) * N ** 3
    result = {
        "filter": {"planes": FP, "size": [FW, FH], "taps": T},
        "backprojection": {"planes": P, "plane_size": [W, H], "grid": [N, N, N]},
        "ms_per_call": ms,
        "method": "device events around the calls of one stream, divided by the calls; the legs in turn, per round",
        "filter_torch_over_hip": round(best["filter_torch_toeplitz_f64"] / best["filter_hip"], 2),
        "filter_torch_over_hip_hann": round(best["filter_torch_toeplitz_f64"] / best["filter_hip_hann"], 2),
        "backproject_torch_over_hip": round(best["backproject_torch_f64_gathers"] / best["backproject_hip"], 2),
        "backproject_hip_over_copy_volume": round(best["backproject_hip"] / best["copy_volume"], 1),
        "backproject_voxel_updates_per_s": round(updates / (best["backproject_hip"] * 1e-3), -6),
        "filter_multiply_add_pairs_per_s": round(float(FP) * FH * FW * FW / (best["filter_hip"] * 1e-3), -6),
        "yardstick": {"filter_hip < filter_torch (best of the rounds)": bool(best["filter_hip"] < best["filter_torch_toeplitz_f64"]),
                      "filter_hip_hann < filter_torch (best of the rounds)":
                          bool(best["filter_hip_hann"] < best["filter_torch_toeplitz_f64"]),
                      "backproject_hip < backproject_torch (best of the rounds)":
                          bool(best["backproject_hip"] < best["backproject_torch_f64_gathers"])},
        "agreement": {"filter_max_abs_diff_over_max": filter_diff, "backproject_bits_equal": backproject_bits_equal,
                      "backproject_max_abs_diff_over_max": backproject_diff},
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
