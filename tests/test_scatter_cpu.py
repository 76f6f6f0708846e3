"""The scatter model without a GPU: the kernels' arithmetic, host-compiled
(xrt_host_scatter_source, xrt_host_scatter_add), against tests/scatter_ref.py bit for bit;
every argument error of both entry pairs through a NULL context; the contract's identities;
what binning costs; whether the estimate cups a reconstruction; the kernels' code-object
metadata and a stand-alone sanitizer build of the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lsf_ref
import scatter_kit as kit
import scatter_ref
import simpleraytracing_amd as xrt
import spectrum_ref
from simpleraytracing_amd import _abi
from conftest import ROOT, bits
from test_materials_cpu import _render_kernel_metadata
from test_pose_cpu import _sanitizer_runtime

F = np.float32


# --------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("M,K", kit.TABLES)
@pytest.mark.parametrize("P", kit.STACKS)
@pytest.mark.parametrize("W,H,D", kit.SHAPES)
def test_source_equals_the_reference(W, H, D, P, M, K):
    p, o, w, mu, sg, src, lb = kit.source_case(W, H, D, P, M, K)
    got_src, got_lb = xrt.host_scatter_source(p, o, w, mu, sg, D)
    kit.check(got_lb, lb, ("lbuffer", W, H, D, P, M, K))
    kit.check(got_src, src, ("source", W, H, D, P, M, K))
    # the L-buffer is the spectrum model's own, flags and all
    d = np.moveaxis(p.reshape(M, -1), 0, 1)
    want = spectrum_ref.integrate(d, np.repeat((o.reshape(-1) != 0)[:, None], M, 1), w, mu)
    kit.check(got_lb.reshape(-1), want, ("spectrum_ref", W, H, D, P, M, K))
    assert (got_lb[o != 0] == F(-1.0)).all()
    only_src, none = xrt.host_scatter_source(p, o, w, mu, sg, D, lbuffer=False)        # lbuffer NULL
    assert none is None
    kit.check(only_src, src, "source alone")
    if H * W > 40:
        assert np.isnan(src).any() and np.isnan(lb).any()        # the special values reached the planes


@pytest.mark.parametrize("G", kit.KERNELS)
@pytest.mark.parametrize("P", kit.STACKS)
@pytest.mark.parametrize("W,H,D", kit.SHAPES)
def test_add_equals_the_reference(W, H, D, P, G):
    b, a, prim, with_p, without = kit.add_case(W, H, D, P, G)
    shape = (P, H, W)
    for primary, want in ((prim, with_p), (None, without)):
        out, sc, u8 = xrt.host_scatter_add(b, a, D, shape, primary)
        kit.check(out, want[0], ("out", W, H, D, P, G, primary is None))
        kit.check(sc, want[1], ("scatter", W, H, D, P, G))
        assert np.array_equal(u8, want[2])
    assert np.array_equal(bits(without[0]), bits(without[1]))                    # no primary: out is the scatter
    # each output NULL in turn, and each alone
    for keep in ((False, True, True), (True, False, True), (True, True, False), (True, False, False),
                 (False, True, False), (False, False, True)):
        got = xrt.host_scatter_add(b, a, D, shape, prim, *keep)
        for g, k, wnt in zip(got, keep, with_p):
            assert (g is None) == (not k)
            if k:
                kit.check(g, wnt, keep)


def test_bin_one_is_spectrum_then_lsf_then_a_product():
    """D = 1, written out without scatter_ref: q from spectrum_ref's pieces, the blur from lsf_ref,
    one product and one sum a kernel."""
    from oracle import oracle
    M, K, P, H, W = 3, 8, 2, 19, 23
    w, mu, sg = kit.tables(M, K, seed=5)
    p, _ = kit.planes(M, P, H, W, seed=5, specials=False)
    d = [p[m].astype(np.float64) * 0.1 for m in range(M)]
    Q = np.zeros((P, H, W))
    for e in range(K):
        xe, se = np.zeros((P, H, W)), np.zeros((P, H, W))
        for m in range(M):
            xe = xe + np.float64(mu[m, e]) * d[m]
            se = se + np.float64(sg[m, e]) * d[m]
        Q = Q + (np.float64(w[e]) * oracle.exp(-xe).reshape(xe.shape)) * se
    lb = spectrum_ref.integrate(np.moveaxis(p.reshape(M, -1), 0, 1), None, w, mu).reshape(P, H, W)
    src, got_lb = xrt.host_scatter_source(p, None, w, mu, sg, 1)
    assert np.array_equal(bits(src), bits(Q.astype(F))) and np.array_equal(bits(got_lb), bits(lb))
    hx, hy = lsf_ref.taps(3, 9), lsf_ref.taps(4, 5)
    amp = np.array([0.25, 0.0625], F)
    blurred = np.stack([xrt.host_lsf(src, hx, hy, u8=False)[0], xrt.host_lsf(src, hy, hx, u8=False)[0]])
    ref_blur = [lsf_ref.apply(Q.astype(F), hx, hy)[0], lsf_ref.apply(Q.astype(F), hy, hx)[0]]
    S = np.float64(amp[0]) * ref_blur[0].astype(np.float64)
    S = S + np.float64(amp[1]) * ref_blur[1].astype(np.float64)
    out, sc, _ = xrt.host_scatter_add(blurred, amp, 1, (P, H, W), lb)
    assert np.array_equal(bits(sc), bits(S.astype(F)))
    assert np.array_equal(bits(out), bits((lb.astype(np.float64) + S).astype(F)))


@pytest.mark.parametrize("D", kit.BINS)
def test_empty_planes_give_a_positive_zero(D):
    M, K, P, H, W = 3, 8, 2, 37, 45
    w, mu, sg = kit.tables(M, K)
    src, lb = xrt.host_scatter_source(np.zeros((M, P, H, W), F), None, w, mu, sg, D)
    assert (bits(src) == 0).all()                                                # +0.0, not -0.0
    assert (bits(lb) == bits(np.full(1, spectrum_ref.miss_value(w)))[0]).all()
    blurred = np.stack([xrt.host_lsf(src, lsf_ref.gaussian(1.5, 9)[1], u8=False)[0]] * 2)
    prim = lsf_ref.plane(D, W, H, P)                                             # -0.0, denormals and spikes among them
    out, sc, _ = xrt.host_scatter_add(blurred, [0.5, 2.0], D, (P, H, W), prim)
    assert (bits(sc) == 0).all()
    keep = bits(prim) != 0x80000000
    assert np.array_equal(bits(out)[keep], bits(prim)[keep]) and (bits(out)[~keep] == 0).all() and (~keep).any()


@pytest.mark.parametrize("D", kit.BINS)
def test_a_constant_coarse_plane_comes_back_exactly(D):
    P, H, W = 2, 45, 67
    Hc, Wc = scatter_ref.coarse_size(H, D), scatter_ref.coarse_size(W, D)
    for c in (F(0.1), F(1e-41), F(3.3e7), F(-0.0)):
        b = np.full((1, P, Hc, Wc), c, F)
        _, sc, _ = xrt.host_scatter_add(b, [1.0], D, (P, H, W))
        want = bits(np.full(1, F(np.float64(0.0) + np.float64(1.0) * np.float64(c))))[0]
        assert (bits(sc) == want).all(), (D, c)


def test_bin_one_ignores_the_neighbour():
    b = np.array([[[[1.0, np.inf], [np.nan, -np.inf]]]], F)
    _, sc, _ = xrt.host_scatter_add(b, [1.0], 1, (1, 2, 2))
    kit.check(sc, b[0], "D = 1")


def test_scatter_gaussian():
    assert np.array_equal(bits(xrt.scatter_gaussian(14.0, 8)), bits(xrt.lsf_gaussian(1.75, 15)))
    assert np.array_equal(bits(xrt.scatter_gaussian(14.0, 4, 9)), bits(xrt.lsf_gaussian(3.5, 9)))
    assert xrt.scatter_gaussian(16.0, 1).size == 129
    for args in ((17.0, 1), (100.0, 4), (0.0, 4), (np.nan, 4), (10.0, 4, 131), (10.0, 4, 4)):
        with pytest.raises(xrt.XrtError) as e:
            xrt.scatter_gaussian(*args)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT


# --------------------------------------------------------------------------- the refusals
def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _dev(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _source(lib, entry, w, h, p, m, paths, open, weight, mu, sigma, k, d, lb, src):
    fp, u16 = _abi._fp, _abi._u16p
    tabs = (_ptr(weight, fp), _ptr(mu, fp), _ptr(sigma, fp), k, d)
    if entry == "device":
        return lib.xrt_scatter_source_device(None, w, h, p, m, _dev(paths), _dev(open), *tabs, _dev(lb), _dev(src), None)
    if entry == "host":
        return lib.xrt_scatter_source(None, w, h, p, m, _ptr(paths, fp), _ptr(open, u16), *tabs, _ptr(lb, fp), _ptr(src, fp))
    return lib.xrt_host_scatter_source(w, h, p, m, _ptr(paths, fp), _ptr(open, u16), *tabs, _ptr(lb, fp), _ptr(src, fp))


def _add(lib, entry, w, h, p, d, blurred, g, amp, primary, out, sc, u8):
    fp, u8p = _abi._fp, _abi._u8p
    if entry == "device":
        return lib.xrt_scatter_add_device(None, w, h, p, d, _dev(blurred), g, _ptr(amp, fp), _dev(primary), _dev(out),
                                          _dev(sc), _dev(u8), None)
    args = (w, h, p, d, _ptr(blurred, fp), g, _ptr(amp, fp), _ptr(primary, fp), _ptr(out, fp), _ptr(sc, fp), _ptr(u8, u8p))
    return lib.xrt_scatter_add(None, *args) if entry == "host" else lib.xrt_host_scatter_add(*args)


def _refused(lib, entry, rc, word, what):
    assert rc == _abi.XRT_ERR_ARGUMENT, (word, what)
    if entry != "hook":
        assert word.encode() in lib.xrt_last_error(None), (word, what, lib.xrt_last_error(None))


@pytest.mark.parametrize("entry", ["host", "device", "hook"])
def test_source_argument_errors_without_a_device(entry):
    """Every check comes before the context is looked at: with a NULL context each is
    XRT_ERR_ARGUMENT with its own message (the entries), or XRT_ERR_ARGUMENT (the hook)."""
    lib = _abi.load()
    W, H, P, M, K, D = 6, 4, 2, 2, 3, 4
    paths = np.zeros(M * P * H * W + 8, F)
    open_ = np.zeros(P * H * W, np.uint16)
    lb = np.zeros(P * H * W, F)
    src = np.zeros(P * 1 * 2, F)
    w = np.ones(K, F)
    mu = np.full(M * K, 0.1, F)
    sg = np.full(M * K, 0.05, F)

    def bad(a, at, v):
        b = a.copy()
        b[at] = v
        return b
    ok = dict(w=W, h=H, p=P, m=M, paths=paths, open=open_, weight=w, mu=mu, sigma=sg, k=K, d=D, lb=lb, src=src)
    cases = [
        (dict(paths=None), "paths is NULL"), (dict(sigma=None), "sigma is NULL"), (dict(src=None), "source is NULL"),
        (dict(weight=None), "weight is NULL"), (dict(mu=None), "mu is NULL"),
        (dict(m=0), "XRT_MAX_MESHES"), (dict(m=17), "XRT_MAX_MESHES"), (dict(k=0), "XRT_MAX_BINS"), (dict(k=33), "XRT_MAX_BINS"),
        (dict(weight=bad(w, 1, 0.0)), "weight"), (dict(weight=bad(w, 0, np.nan)), "weight"),
        (dict(mu=bad(mu, 5, -0.5)), "coefficient"), (dict(mu=bad(mu, 0, np.inf)), "coefficient"),
        (dict(sigma=bad(sg, 5, -0.5)), "sigma"), (dict(sigma=bad(sg, 0, np.nan)), "sigma"), (dict(sigma=bad(sg, 2, np.inf)), "sigma"),
        (dict(d=0), "bin"), (dict(d=3), "bin"), (dict(d=128), "bin"), (dict(d=6), "bin"),
        (dict(w=0), "is 0"), (dict(h=0), "is 0"), (dict(p=0), "is 0"),
        (dict(w=0x80000000), "2^31"), (dict(h=0x80000000), "2^31"), (dict(p=65536, w=1, h=1), "65535"),
        (dict(h=4 * 65535 + 1, w=1, p=1), "65535"),
        (dict(src=paths[4:]), "overlaps"), (dict(lb=paths[M * P * H * W - 1:]), "overlaps"),
        (dict(src=open_.view(F)[2:]), "overlaps"), (dict(lb=open_.view(F)), "overlaps"), (dict(src=lb[44:]), "overlaps"),
    ]
    for change, word in cases:
        _refused(lib, entry, _source(lib, entry, **{**ok, **change}), word, change.keys())
    for good in (ok, {**ok, "open": None}, {**ok, "lb": None}, {**ok, "src": paths[M * P * H * W:]}, {**ok, "d": 64}):
        rc = _source(lib, entry, **good)
        if entry == "hook":
            assert rc == _abi.XRT_OK
        else:
            assert rc == _abi.XRT_ERR_ARGUMENT and b"context is NULL" in lib.xrt_last_error(None)


@pytest.mark.parametrize("entry", ["host", "device", "hook"])
def test_add_argument_errors_without_a_device(entry):
    lib = _abi.load()
    W, H, P, D, G = 6, 4, 2, 4, 2
    n = P * H * W
    blurred = np.zeros(G * P * 1 * 2 + 4, F)
    prim = np.zeros(n, F)
    out, sc = np.zeros(n + 4, F), np.zeros(n, F)
    u8 = np.zeros(n, np.uint8)
    amp = np.array([0.5, 0.0], F)
    ok = dict(w=W, h=H, p=P, d=D, blurred=blurred, g=G, amp=amp, primary=prim, out=out, sc=sc, u8=u8)
    cases = [
        (dict(blurred=None), "blurred is NULL"), (dict(amp=None), "amp is NULL"),
        (dict(out=None, sc=None, u8=None), "all NULL"),
        (dict(g=0), "num_kernels"), (dict(g=5), "num_kernels"),
        (dict(amp=np.array([0.5, -1.0], F)), "amp"), (dict(amp=np.array([np.nan, 1.0], F)), "amp"),
        (dict(amp=np.array([np.inf, 1.0], F)), "amp"),
        (dict(d=0), "bin"), (dict(d=3), "bin"), (dict(d=128), "bin"),
        (dict(w=0), "is 0"), (dict(h=0), "is 0"), (dict(p=0), "is 0"),
        (dict(w=0x80000000), "2^31"), (dict(p=65536, w=1, h=1), "65535"), (dict(h=64 * 65535 + 1, w=1, p=1), "65535"),
        (dict(out=prim), "overlaps"), (dict(sc=prim[n - 1:]), "overlaps"), (dict(u8=prim.view(np.uint8)[4 * n - 1:]), "overlaps"),
        (dict(out=blurred), "overlaps"), (dict(sc=blurred[7:]), "overlaps"), (dict(u8=blurred.view(np.uint8)), "overlaps"),
    ]
    for change, word in cases:
        _refused(lib, entry, _add(lib, entry, **{**ok, **change}), word, change.keys())
    for good in (ok, {**ok, "primary": None}, {**ok, "out": None}, {**ok, "sc": None, "u8": None}):
        rc = _add(lib, entry, **good)
        if entry == "hook":
            assert rc == _abi.XRT_OK
        else:
            assert rc == _abi.XRT_ERR_ARGUMENT and b"context is NULL" in lib.xrt_last_error(None)


def test_python_shape_errors():
    w, mu, sg = kit.tables(3, 8)
    with pytest.raises(ValueError):
        xrt.host_scatter_source(np.zeros((2, 4, 4), F), None, w, mu, sg, 2)
    with pytest.raises(ValueError):
        xrt.host_scatter_source(np.zeros((3, 4, 4), F), np.zeros((4, 5), np.uint16), w, mu, sg, 2)
    with pytest.raises(ValueError):
        xrt.host_scatter_source(np.zeros((3, 4, 4), F), None, w, mu, sg[:2], 2)
    with pytest.raises(ValueError):
        xrt.host_scatter_add(np.zeros((1, 2, 3), F), [1.0], 2, (4, 4))


# --------------------------------------------------------------------------- the CLI's refusals
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
GOOD = "8\n0.12 0.1\n0.3 20\n"


def test_cli_help_lists_the_option():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--scatter FILE" in r.stderr


@pytest.mark.parametrize("text,args,word", [
    (GOOD, ["--detector", "det.txt"], "--detector"), (GOOD, ["--supersample", "2"], "--supersample"),
    (GOOD, ["--focal-spot", "1x1:2x2"], "--focal-spot"), (GOOD, ["--volume", "v.mhd"], "--volume"), (GOOD, ["-g", "2"], "-g"),
    (GOOD, ["--rows", "0:4"], "--rows"), (GOOD, ["--batch", "2"], "--batch"),
    (GOOD, "no --paths", "--paths --spectrum"), (GOOD, "no --spectrum", "--paths --spectrum"),
    ("# nothing\n\n", [], "binning factor"), ("3\n0.12 0.1\n0.3 20\n", [], "power of two"), ("128\n0.12 0.1\n0.3 20\n", [], "power of two"),
    ("8 1\n0.12 0.1\n0.3 20\n", [], "binning factor"), ("8\n0.12 0.1\n", [], "kernels"), ("8\n0.3 20\n", [], "kernels"),
    ("8\n0.12 0.1\n" + "0.3 20\n" * 5, [], "kernels"), ("8\n0.12 0.1 0.2\n0.3 20\n", [], "bins"), ("8\n0.12 -0.1\n0.3 20\n", [], "coefficient"),
    ("8\n0.12 nan\n0.3 20\n", [], "coefficient"), ("8\n0.12 0.1\n-0.3 20\n", [], "amplitude"), ("8\n0.12 0.1\n0.3 0\n", [], "SIGMA"),
    ("8\n0.12 0.1\n0.3 20:4\n", [], "taps"), ("8\n0.12 0.1\n0.3 20:131\n", [], "taps"), ("1\n0.12 0.1\n0.3 20\n", [], "taps"),
    ("8\n0.12 0.1\n0.3 20:5:1\n", [], "AMP SIGMA"), ("8\n0.12 0.1\n0.3 20 7\n", [], "AMP SIGMA"), (None, [], "cannot read"),
])
def test_cli_errors(tmp_path, text, args, word):
    """Each is an error before any device is opened: exit 1, stderr 'ERROR: ...' naming --scatter and the fault."""
    if text is not None:
        (tmp_path / "scatter.txt").write_text(text)
    (tmp_path / "beam.txt").write_text("50 30\n0.3 0.2\n")
    (tmp_path / "det.txt").write_text("1 1\n")
    model = ["--paths", "--spectrum", "beam.txt"]
    if args == "no --paths":
        model, args = ["--spectrum", "beam.txt"], []
    elif args == "no --spectrum":
        model, args = ["--paths"], []
    from conftest import DRAGON
    r = subprocess.run([EXE, "-s", "16", "16", "-i", DRAGON, *model, "--scatter", "scatter.txt"] + args, capture_output=True,
                       text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("ERROR:") and "--scatter" in r.stderr and word in r.stderr and "xrt_create" not in r.stderr, r.stderr


# --------------------------------------------------------------------------- the studies
# DESIGN 10.16's table, measured in scatter_ref.binning_deviation: a ball of R = 60 on 192 x 192, two bins, one
# Gaussian of sigma = 14 pixels.  Each bound is twice the measured value: the margin is for a change of the
# phantom's position, the reference being deterministic.
BINNING = {2: 0.000616, 4: 0.00305, 8: 0.0126, 16: 0.0494}


@pytest.mark.parametrize("D", sorted(BINNING))
def test_binning_deviation(D):
    dev = scatter_ref.binning_deviation(D)
    print(f"D = {D}, sigma / D = {14.0 / D}: largest deviation {dev:.6f} of the scatter plane's maximum")
    assert dev <= 2.0 * BINNING[D], (D, dev)
    if D > 2:
        assert dev > BINNING[D // 2]                                             # coarser bins cost more


def test_binning_deviation_of_the_library():
    """The same study through the code users get (the host hooks of both kernels and of the blur) at D = 8: the
    bound holds for it, and its planes are the reference's bit for bit."""
    w, mu, sg = scatter_ref.BALL_TABLE
    size, s = 192, 14.0
    paths = scatter_ref.ball_chords(size, size, 60.0)[None, None]
    planes = {}
    for d in (1, 8):
        h = xrt.scatter_gaussian(s, d)
        src, _ = xrt.host_scatter_source(paths, None, w, mu, sg, d, lbuffer=False)
        blurred = xrt.host_lsf(src, h, h, u8=False)[0][None]
        planes[d] = xrt.host_scatter_add(blurred, [1.0], d, (1, size, size), out=False, u8=False)[1].astype(np.float64)
        ref_src, _ = scatter_ref.source(paths, None, w, mu, sg, d)
        want = scatter_ref.estimate(ref_src, [(1.0, h, h)], d, (1, size, size))[1]
        assert np.array_equal(bits(planes[d].astype(F)), bits(want)), d
    dev = float(np.abs(planes[8] - planes[1]).max() / planes[1].max())
    print("the library, D = 8:", dev)
    assert dev <= 2.0 * BINNING[8]


def test_binning_deviation_with_the_ball_off_centre():
    """What the margin is for: the ball a third of a block off the grid stays inside the bound."""
    w, mu, sg = scatter_ref.BALL_TABLE
    size, D, s = 192, 8, 14.0
    paths = scatter_ref.ball_chords(size, size, 60.0, 95.5 + 2.7, 95.5 - 1.3)[None, None]
    planes = {}
    for d in (1, D):
        h = lsf_ref.gaussian(s / d, 2 * int(np.ceil(4.0 * s / d)) + 1)[1]
        src, _ = scatter_ref.source(paths, None, w, mu, sg, d)
        planes[d] = scatter_ref.estimate(src, [(1.0, h, h)], d, (1, size, size))[1].astype(np.float64)
    dev = float(np.abs(planes[D] - planes[1]).max() / planes[1].max())
    print("off centre, D = 8:", dev)
    assert dev <= 2.0 * BINNING[D]


def test_scatter_cups_the_reconstruction():
    """DESIGN 10.11's ball scan through -ln and fdk_ref, the primary alone and with the estimate added: scatter
    lowers the interior and deepens the drop from the rim to the centre.  Only the two orderings are asserted."""
    (c0, r0), (c1, r1) = scatter_ref.cupping_study()
    print(f"without scatter: centre {c0:.5f}, rim {r0:.5f}, drop {r0 - c0:.5f}; "
          f"with: centre {c1:.5f}, rim {r1:.5f}, drop {r1 - c1:.5f}")
    assert c1 < c0
    assert r1 - c1 > r0 - c0


# --------------------------------------------------------------------------- the code object, the sanitizers
def test_kernel_metadata():
    """k_scatter_source (four mesh bounds) and k_scatter_add in the gfx950 code object: no scratch, no spills,
    the tables by value."""
    meta = _render_kernel_metadata()
    src = {k: v for k, v in meta.items() if "k_scatter_source" in k}
    add = {k: v for k, v in meta.items() if "k_scatter_add" in k}
    assert len(src) == 4 and len(add) == 1, sorted(meta)
    for name, f in {**src, **add}.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
    for f in src.values():
        assert f["kernarg_segment_size"] >= 4 * 8 + 4 * 4 + (32 + 1 + 2 * 512) * 4, f
        assert 0 < f["group_segment_fixed_size"] <= 16384, f


def test_host_code_under_sanitizers(tmp_path):
    """tools/scatter_san.cpp: a stand-alone program over csrc/xrt_scatter_host.inc (the checks and both host
    restatements on exact-size heap buffers) with AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "scatter_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "scatter_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "scatter_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
