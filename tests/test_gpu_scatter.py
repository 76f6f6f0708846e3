"""The scatter model on the GPU: k_scatter_source and k_scatter_add through the
host and the _device entries on scatter_kit's cases, bit for bit against tests/scatter_ref.py
(a NaN standing for any NaN); the L-buffer against apply_spectrum_device's own; a traced scene
through Context.scatter against the reference chain; two launches with two tables back to back."""
import os
import subprocess

import numpy as np
import pytest

import scatter_kit as kit
import scatter_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT, bits
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
# (P, M, K): every mesh bound of the kernel, stacks of 1, 3 and 17 planes
STACKED = [(1, 1, 1), (3, 1, 1), (1, 3, 8), (3, 3, 8), (17, 3, 8), (1, 16, 32), (3, 16, 32), (1, 7, 5)]


@pytest.fixture(scope="module")
def sctx():
    """A context of this module's own: the models and scenes set here never reach other tests."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda")


@pytest.mark.parametrize("W,H,D", kit.SHAPES)
def test_source_host_and_device_forms(sctx, W, H, D):
    import torch
    for P, M, K in STACKED:
        p, o, w, mu, sg, src, lb = kit.source_case(W, H, D, P, M, K)
        got_src, got_lb = sctx.scatter_source(p, o, w, mu, sg, D)
        kit.check(got_lb, lb, ("lbuffer", W, H, D, P, M, K))
        kit.check(got_src, src, ("source", W, H, D, P, M, K))
        dp, do = _dev(p), _dev(o.view(np.int16))
        d_lb = torch.zeros(lb.size, dtype=torch.float32, device="cuda")
        d_src = torch.zeros(src.size, dtype=torch.float32, device="cuda")
        d_spec = torch.zeros(lb.size, dtype=torch.float32, device="cuda")
        sctx.scatter_source_device(W, H, P, dp.data_ptr(), do.data_ptr(), w, mu, sg, D, d_lb.data_ptr(), d_src.data_ptr())
        sctx.apply_spectrum_device(lb.size, dp.data_ptr(), do.data_ptr(), w, mu, d_spec.data_ptr())
        torch.cuda.synchronize()
        kit.check(d_lb.cpu().numpy(), lb, ("device lbuffer", W, H, D, P, M, K))
        kit.check(d_src.cpu().numpy(), src, ("device source", W, H, D, P, M, K))
        kit.check(d_lb.cpu().numpy(), d_spec.cpu().numpy(), ("k_apply_spectrum's lbuffer", W, H, D, P, M, K))
        if (P, M, K) == (3, 3, 8):                                               # no masks, no L-buffer
            src2, _ = scatter_ref.source(p, None, w, mu, sg, D)
            d_src.zero_()
            sctx.scatter_source_device(W, H, P, dp.data_ptr(), 0, w, mu, sg, D, 0, d_src.data_ptr())
            torch.cuda.synchronize()
            kit.check(d_src.cpu().numpy(), src2, ("no masks", W, H, D))


@pytest.mark.parametrize("W,H,D", kit.SHAPES)
def test_add_host_and_device_forms(sctx, W, H, D):
    import torch
    for P in (1, 3, 17):
        for G in kit.KERNELS:
            b, a, prim, with_p, without = kit.add_case(W, H, D, P, G)
            shape, n = (P, H, W), P * H * W
            for primary, want in ((prim, with_p), (None, without)):
                out, sc, u8 = sctx.scatter_add(b, a, D, shape, primary)
                kit.check(out, want[0], ("out", W, H, D, P, G))
                kit.check(sc, want[1], ("scatter", W, H, D, P, G))
                assert np.array_equal(u8, want[2])
            db, dprim = _dev(b), _dev(prim)
            d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
            d_sc = torch.zeros(n, dtype=torch.float32, device="cuda")
            d_u8 = torch.zeros(n, dtype=torch.uint8, device="cuda")
            sctx.scatter_add_device(W, H, P, D, db.data_ptr(), a, dprim.data_ptr(), d_out.data_ptr(), d_sc.data_ptr(),
                                    d_u8.data_ptr())
            torch.cuda.synchronize()
            kit.check(d_out.cpu().numpy(), with_p[0], ("device out", W, H, D, P, G))
            kit.check(d_sc.cpu().numpy(), with_p[1], ("device scatter", W, H, D, P, G))
            assert np.array_equal(d_u8.cpu().numpy().reshape(shape), with_p[2])
    # each output alone
    b, a, prim, with_p, _ = kit.add_case(W, H, D, 3, 4)
    for keep in ((True, False, False), (False, True, False), (False, False, True)):
        got = sctx.scatter_add(b, a, D, (3, H, W), prim, *keep)
        for g, k, wnt in zip(got, keep, with_p):
            assert (g is None) == (not k)
            if k:
                kit.check(g, wnt, keep)
    with pytest.raises(xrt.XrtError) as e:
        sctx.scatter_add(b, a, D, (3, H, W), prim, False, False, False)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT


@pytest.mark.parametrize("D", [1, 8, 64])
def test_waves_that_miss_everything(sctx, D):
    """Rows of +0.0 in every plane -- whole waves that miss, which the kernel answers without an exp -- between rows
    that hit, with a flag, a -0.0 and a NaN alone in otherwise empty rows (each makes its wave compute); and planes
    that are empty altogether."""
    W, H, P, M, K = 130, 70, 3, 3, 8
    w, mu, sg = kit.tables(M, K, seed=11)
    p, o = kit.planes(M, P, H, W, seed=11, specials=False)
    p, o = p.copy(), o.copy()
    p[:, :, 10:50] = 0.0
    o[:, 10:50] = 0
    o[:, 20, 5] = 4                                                              # a flag in a wave of misses
    p[1, :, 30, 70] = F(-0.0)
    p[2, :, 40, 129] = F(np.nan)
    for planes, masks in ((p, o), (np.zeros_like(p), None)):
        src, lb = scatter_ref.source(planes, masks, w, mu, sg, D)
        got_src, got_lb = sctx.scatter_source(planes, masks, w, mu, sg, D)
        kit.check(got_lb, lb, ("lbuffer", D))
        kit.check(got_src, src, ("source", D))
    assert (bits(got_src) == 0).all()                                            # empty planes: +0.0, not -0.0


def test_two_tables_back_to_back(sctx):
    """Two launches of each kernel on one stream with different tables and amplitudes, no host wait between
    them: each gives its own reference (the tables travel by value with the launch); an overlap is refused."""
    import torch
    W, H, D, P, M, K = 67, 45, 16, 3, 3, 8
    p, o, w1, mu1, sg1, src1, lb1 = kit.source_case(W, H, D, P, M, K)
    w2, mu2, sg2 = kit.tables(M, K, seed=77)
    src2, lb2 = scatter_ref.source(p, o, w2, mu2, sg2, D)
    assert not np.array_equal(bits(src1), bits(src2))
    dp, do = _dev(p), _dev(o.view(np.int16))
    lbs = [torch.zeros(lb1.size, dtype=torch.float32, device="cuda") for _ in range(2)]
    srcs = [torch.zeros(src1.size, dtype=torch.float32, device="cuda") for _ in range(2)]
    with pytest.raises(xrt.XrtError) as e:
        sctx.scatter_source_device(W, H, P, dp.data_ptr(), do.data_ptr(), w1, mu1, sg1, D, 0, dp.data_ptr() + 4 * (p.size - 1))
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)
    sctx.scatter_source_device(W, H, P, dp.data_ptr(), do.data_ptr(), w1, mu1, sg1, D, lbs[0].data_ptr(), srcs[0].data_ptr())
    sctx.scatter_source_device(W, H, P, dp.data_ptr(), do.data_ptr(), w2, mu2, sg2, D, lbs[1].data_ptr(), srcs[1].data_ptr())
    torch.cuda.synchronize()
    kit.check(srcs[0].cpu().numpy(), src1, "first table")
    kit.check(srcs[1].cpu().numpy(), src2, "second table")
    kit.check(lbs[0].cpu().numpy(), lb1, "first table's lbuffer")
    kit.check(lbs[1].cpu().numpy(), lb2, "second table's lbuffer")
    assert np.array_equal(bits(dp.cpu().numpy()), bits(p))                       # the input is only read

    b, a1, prim, want1, _ = kit.add_case(W, H, D, P, 4)
    a2 = kit.amps(4, seed=9)
    want2 = scatter_ref.add(b, a2, D, (P, H, W), prim)
    db, dprim = _dev(b), _dev(prim)
    outs = [torch.zeros(prim.size, dtype=torch.float32, device="cuda") for _ in range(2)]
    with pytest.raises(xrt.XrtError) as e:
        sctx.scatter_add_device(W, H, P, D, db.data_ptr(), a1, dprim.data_ptr(), dprim.data_ptr())
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)
    sctx.scatter_add_device(W, H, P, D, db.data_ptr(), a1, dprim.data_ptr(), outs[0].data_ptr())
    sctx.scatter_add_device(W, H, P, D, db.data_ptr(), a2, dprim.data_ptr(), outs[1].data_ptr())
    torch.cuda.synchronize()
    kit.check(outs[0].cpu().numpy(), want1[0], "first amplitudes")
    kit.check(outs[1].cpu().numpy(), want2[0], "second amplitudes")


def test_traced_scene_through_the_composition(sctx, dragon):
    """box + dragon + box at 96 x 80 with D = 8: render_paths, then Context.scatter against the reference chain
    over the rendered planes (source -> oracle hole fill -> lsf_ref per kernel -> add)."""
    from oracle import oracle
    from scene_kit import box
    lo, hi = xrt.mesh_bbox(dragon)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    meshes = [box(c - half * F(1.2), c + half * F(1.2)), dragon, box(c - half * F(0.3), c + half * F(0.3))]
    W, H, D = 96, 80, 8
    cam = xrt.camera_for_scene(meshes, W, H)
    sctx.upload_scene(meshes)
    sctx.set_paths()
    paths, open_, _ = sctx.render_paths(cam)
    paths, open_ = np.asarray(paths).reshape(3, H, W), np.asarray(open_).reshape(H, W)
    assert np.count_nonzero(paths) > 1000
    w, mu, sg = kit.tables(3, 8, seed=3)
    kernels = [(0.3, xrt.scatter_gaussian(20.0, D), xrt.scatter_gaussian(20.0, D)),
               (0.05, xrt.scatter_gaussian(60.0, D, 41), xrt.scatter_gaussian(40.0, D, 41))]
    total, sc, primary = sctx.scatter(paths, open_, w, mu, sg, kernels, D, W, H)
    src, lb = scatter_ref.source(paths[:, None], open_[None], w, mu, sg, D)
    prim = oracle.hole_fill(lb[0], W, H).reshape(1, H, W)
    want = scatter_ref.estimate(src, kernels, D, (1, H, W), prim)
    kit.check(primary, prim[0], "primary")
    kit.check(sc, want[1][0], "scatter")
    kit.check(total, want[0][0], "total")
    assert sc.max() > 0 and not np.isnan(sc).any()
    m_total, m_sc, m_prim = xrt.scatter(paths, open_, w, mu, sg, kernels, D, W, H)   # the module-level form
    assert np.array_equal(bits(m_total), bits(total)) and np.array_equal(bits(m_sc), bits(sc))
    assert np.array_equal(bits(m_prim), bits(primary))


def _read_text(path, W, H):
    return np.array([[float(v) for v in line.split("\t")] for line in open(path).read().split("\n")], np.float64).reshape(H, W)


def test_cli_scatter_on_a_turntable(tmp_path):
    """xrt_main --paths --spectrum --scatter on a traced box, --turntable 8:z, 64 x 64, D = 8: every projection's
    total, scatter and plane files exist; NAME.EXT without --scatter is the primary, and total - primary is the
    scatter file -- within the files' six digits: each of the three values is off by at most 5e-6 of itself, the
    total by half an f32 ulp more --; the scatter is positive and differs between projections; under
    --log-projection --reconstruct the scan with scatter reconstructs, lower than the scan without; the option's
    refusals hold."""
    from scene_kit import box
    W = H = 64
    P = 8
    _write_obj(tmp_path / "box.obj", box(np.array([-20, -12, -8], F), np.array([20, 12, 8], F)))
    (tmp_path / "out").mkdir()
    (tmp_path / "beam.txt").write_text("50 30\n0.3 0.2\n")
    (tmp_path / "scatter.txt").write_text("# D, the box's scattering part, two kernels\n8\n0.12 0.1\n0.3 20\n0.05 40:21\n")
    scan = ["--spectrum", "beam.txt", "-i", "box.obj", "-s", str(W), str(H), "--turntable", f"{P}:z"]
    common = ["--paths"] + scan           # (the primary alone is the spectrum model's scan: --turntable takes no bare --paths)

    def run(*args, ok=True):
        res = subprocess.run([EXE, *args], capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert (res.returncode == 0) == ok, res.stderr
        return res

    out = tmp_path / "out"
    run(*scan, "-f", "p.txt")
    run(*common, "-f", "t.txt", "--scatter", "scatter.txt", "--u8", "t.pgm")
    planes = []
    for k in range(P):
        for name in (f"t.p{k:03d}.txt", f"t.p{k:03d}.scatter.txt", f"t.p{k:03d}.m0.txt", f"t.p{k:03d}.open.txt", f"p.p{k:03d}.txt"):
            assert (out / name).exists(), name
        assert not (out / f"p.p{k:03d}.scatter.txt").exists()
        total, prim, sc = (_read_text(out / f"{n}.txt", W, H) for n in (f"t.p{k:03d}", f"p.p{k:03d}", f"t.p{k:03d}.scatter"))
        bound = 5e-6 * (np.abs(total) + np.abs(prim) + np.abs(sc)) + 2.0 ** -24 * np.abs(total)
        assert (np.abs(total - prim - sc) <= bound).all(), (k, np.abs(total - prim - sc).max())
        assert sc.min() > 0.0 and sc.max() < prim.max()
        planes.append(sc)
    assert np.abs(planes[0] - planes[1]).max() > 1e-3 * planes[0].max()          # a projection's own source
    assert len(list(tmp_path.rglob("t.p*.pgm"))) == P                            # --u8: the total's 8-bit image, a projection each
    # the stage comes before --lsf and --log-projection, and feeds --reconstruct
    vols = {}
    for name, model, extra in (("r0", scan, []), ("r1", common, ["--scatter", "scatter.txt"])):
        run(*model, "-f", f"{name}.txt", *extra, "--lsf-gaussian", "0.8", "--log-projection", "80", "--reconstruct", f"{name}.mhd:16")
        raw = [f for f in list(out.iterdir()) + list(tmp_path.iterdir()) if f.name == f"{name}.raw"]
        assert raw, name
        vols[name] = np.fromfile(raw[0], np.float32)
    inside = vols["r0"] > 0.5 * vols["r0"].max()
    assert vols["r0"].size == 16 ** 3 and vols["r1"][inside].mean() < vols["r0"][inside].mean()     # scatter lowers the object
    line = _read_text(out / "r1.p000.txt", W, H)
    assert line.max() > 0.1 and (out / "r1.p000.scatter.txt").exists()
    # refusals, each before a device is opened
    still = ["--paths", "--spectrum", "beam.txt", "-i", "box.obj", "-s", str(W), str(H), "-f", "x.txt", "--scatter", "scatter.txt"]
    (tmp_path / "det.txt").write_text("1 1\n")
    for extra, word in ((["--detector", "det.txt"], "--detector"), (["--supersample", "2"], "--supersample"),
                        (["--focal-spot", "1x1:2x2"], "--focal-spot"), (["-g", "2"], "-g"), (["--rows", "0:4"], "--rows"),
                        (["--batch", "2"], "--batch")):
        res = run(*still, *extra, ok=False)
        assert res.stderr.startswith("ERROR:") and "--scatter" in res.stderr and word in res.stderr, res.stderr
    res = run("--spectrum", "beam.txt", "-i", "box.obj", "-s", str(W), str(H), "-f", "x.txt", "--scatter", "scatter.txt", ok=False)
    assert "--scatter needs --paths --spectrum" in res.stderr
