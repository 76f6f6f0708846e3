#!/usr/bin/env python3
"""FDK, SIRT and TV-regularised SIRT of a dragon scan against the scene's voxelised truth (DESIGN 10.12, 10.13,
10.15), through xrt_main: a turntable scan of 120 projections of 192^2, the reconstruction and --voxelize on the
same 96^3 grid in one run each, then the RMS of (reconstruction - mu * inside) over the grid, inside and outside
the truth, with the mean inside, all over the attenuation model's mu per scene unit.

    python tools/voxelize_truth.py [FILE.json]      (default profiles/voxelize/dragon_truth.json)
"""
import json
import os
import subprocess
import sys

import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import simpleraytracing_amd as xrt

EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
out = tempfile.mkdtemp()                                  # (the projections' text files stay off the output directory)
os.makedirs(os.path.join(out, "out"), exist_ok=True)
target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voxelize", "dragon_truth.json")
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
N, W, P = 96, 192, 120
MU = 0.3971 * 0.1                                         # the attenuation model's coefficient per scene unit
result = {"grid": N, "detector": W, "projections": P, "mu": MU}
for name, extra in (("fdk", []), ("sirt", ["--sirt", "30"]), ("tv", ["--sirt", "30", "--tv", "10"])):
    r = subprocess.run([EXE, "-s", str(W), str(W), "-i", os.path.join(ROOT, "data", "dragon.ply"), "-f", f"{name}.txt",
                        "--turntable", f"{P}:z", "--log-projection", "80", "--reconstruct", f"{name}.mhd:{N}",
                        "--voxelize", f"truth_{name}.mhd:{N}"] + extra, capture_output=True, text=True, cwd=out, timeout=500)
    if r.returncode != 0:
        print(r.stderr[-2000:])
        sys.exit(r.returncode if r.returncode > 0 else 1)
    vol, sp, org = xrt.load_volume(os.path.join(out, f"{name}.mhd"))
    lab, tsp, torg = xrt.load_volume(os.path.join(out, f"truth_{name}.mhd"))
    assert np.array_equal(sp, tsp) and np.array_equal(org, torg)
    truth = MU * (lab > 0)
    err = vol.astype(np.float64) - truth
    result[name] = {"rms": float(np.sqrt(np.mean(err ** 2))), "rms_over_mu": float(np.sqrt(np.mean(err ** 2)) / MU),
                    "inside_voxels": int(np.count_nonzero(lab)), "mean_inside": float(vol[lab > 0].mean()),
                    "mean_inside_over_mu": float(vol[lab > 0].mean() / MU), "rms_inside_over_mu": float(np.sqrt(np.mean(err[lab > 0] ** 2)) / MU),
                    "rms_outside_over_mu": float(np.sqrt(np.mean(err[lab == 0] ** 2)) / MU), "spacing": float(sp[0])}
print(json.dumps(result))
with open(target, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
