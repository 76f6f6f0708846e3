#!/usr/bin/env python3
"""A turntable scan with and without an upload per projection: wall time per
projection of a --projections-step turn, --step degrees a step, materials
model, BINNED, one device, for two scenes -- box + dragon + box at 2048^2 and
the 1.12 M-triangle tiled dragon (one mesh) at 8192^2.  Legs, run in turn
--rounds times in one process so that drift shows as spread between the rounds:

  a  upload   pose_triangles on the host, upload_scene, a device render
  b  pose     set_pose of every mesh, a device render
  c  pose_one set_pose of the dragon only (the one mesh of the tiled scene)
  d  still    the scene at rest, a device render per "projection" (the floor)

Every projection ends with a stream synchronise (a scan reads each projection
back).  k_pose's own span: device events over --launches writings of the whole
posed soup, beside the bytes it moves (72 a triangle) over the HBM rate the
microarchitecture guide measured for a copy (6.29 TB/s).

    python tools/pose_timing.py [--projections 64] [--step 1.0] [--rounds 3] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--projections", type=int, default=64)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--small", action="store_true", help="both scenes at 512^2, the tiled one 3 x 3 (a rehearsal)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import simpleraytracing_amd as xrt
    from simpleraytracing_amd.scenes import tiled_mesh
    from materials_kit import DRAGON_MU, dragon_scene

    dragon = xrt.load_ply(os.path.join(ROOT, "data", "dragon.ply"))
    cases = [("box+dragon+box", dragon_scene(dragon), DRAGON_MU, 512 if args.small else 2048, [1]),
             ("tiled dragon", [tiled_mesh(dragon, 3 if args.small else 7)], [0.1037], 512 if args.small else 8192, [0])]
    out = {"projections": args.projections, "step_degrees": args.step, "rounds": args.rounds, "scenes": {},
           "method": "wall clock around the projections of a leg, each ended by a stream synchronise; "
                     "k_pose by device events", "device": torch.cuda.get_device_name(0)}
    for name, scene, mu, size, turned in cases:
        W = H = size
        cam = xrt.camera_for_scene(scene, W, H)
        lo, hi = xrt.scene_bbox(scene)
        centre = (lo + ((hi - lo).astype(np.float64) / 2.0).astype(np.float32)).astype(np.float32)
        poses = [xrt.pose_rotation((0, 1, 0), args.step * (k + 1), centre) for k in range(args.projections)]
        lb = torch.empty(W * H, device="cuda")
        tris = sum(len(m) for m in scene)
        ms = {leg: [] for leg in ("a_upload", "b_pose", "c_pose_one", "d_still")}
        counters = {}
        with xrt.Context(0) as ctx:
            ctx.set_kernel(xrt.XRT_KERNEL_BINNED)
            ctx.upload_scene(scene)
            ctx.set_materials(mu)

            def frame():
                ctx.render_rows_device(cam, 0, H, 0, lb.data_ptr(), 0)
                torch.cuda.synchronize()

            def leg(prepare):
                ctx.upload_scene(scene)
                for _ in range(3):
                    frame()
                g0 = ctx.geometry_counters()
                t0 = time.perf_counter()
                for q in poses:
                    prepare(q)
                    frame()
                dt = (time.perf_counter() - t0) * 1e3 / len(poses)
                g1 = ctx.geometry_counters()
                return round(dt, 4), {k: g1[k] - g0[k] for k in g1}

            def upload(q):
                ctx.upload_scene([xrt.pose_triangles(m, q) for m in scene])

            def pose_all(q):
                for m in range(len(scene)):
                    ctx.set_pose(m, q)

            def pose_one(q):
                for m in turned:
                    ctx.set_pose(m, q)

            for _ in range(args.rounds):
                for key, prepare in (("a_upload", upload), ("b_pose", pose_all), ("c_pose_one", pose_one),
                                     ("d_still", lambda q: None)):
                    dt, g = leg(prepare)
                    ms[key].append(dt)
                    counters[key] = g
            ctx.upload_scene(scene)
            pose_all(poses[0])
            spans = [round(ctx.pose_span(args.launches), 3) for _ in range(args.rounds)]
        moved = 72 * tris
        out["scenes"][name] = {
            "size": [W, H], "triangles": tris, "meshes": len(scene), "ms_per_projection": ms,
            "geometry_counters_per_leg": counters,
            "k_pose": {"us_per_writing": spans, "launches": args.launches, "bytes_moved": moved,
                       "us_at_hbm_rate": round(moved / (HBM_TBS * 1e6), 3)}}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
