"""Tables and scenes of the spectrum model's tests, and their references (each
scene's per-mesh sums computed once and shared; a table only reruns the final loop)."""
import functools

import numpy as np

import materials_kit as kit
import spectrum_ref
from oracle import oracle
from scene_kit import box

F = np.float32
NAN_NEG = np.array([0xFFC00000], np.uint32).view(F)[0]


def table(M, K, seed=0, first_bin=None):
    """(weights (K,), mu (M, K)): falling weights, coefficients that fall with the bin's
    energy at a rate of the mesh's own, a zero here and there; bin 0 = first_bin if given."""
    rng = np.random.default_rng(1000 * M + K + seed)
    w = (rng.uniform(0.5, 1.5, K) * 80.0 / K).astype(F)
    base = rng.uniform(0.02, 0.6, (M, 1))
    mu = (base * np.exp(-rng.uniform(0.0, 0.15, (M, 1)) * np.arange(K)[None, :])).astype(F)
    mu[rng.integers(0, M), rng.integers(0, K)] = 0.0
    if first_bin is not None:
        mu[:, 0] = np.asarray(first_bin, F)
    return w, np.ascontiguousarray(mu)


def phantom_table(K):
    """The phantom's table of K bins: the materials tests' coefficients are bin 0."""
    return table(5, K, first_bin=kit.PHANTOM_MU)


ONE_BIN = (np.array([80.0], F), np.asarray(kit.PHANTOM_MU, F).reshape(5, 1))


@functools.lru_cache(maxsize=None)
def phantom_sums(W, H):
    meshes = kit.phantom()
    return spectrum_ref.sums(meshes, kit.cam13_of(meshes, W, H), W, H)


def phantom_ref(W, H, K):
    w, mu = ONE_BIN if K == 1 else phantom_table(K)
    return spectrum_ref.from_sums(phantom_sums(W, H), w, mu)


def check_exercised(ref, materials, floor):
    """The spectrum reference of the phantom walks every path: the counts that
    materials_kit.check_exercised asks of the materials reference, taken from this one,
    each at least `floor` -- and the same rays flagged, the same hits per mesh."""
    assert np.array_equal(ref.flagged_by >= 0, materials.flagged_by >= 0)
    assert np.array_equal(ref.mesh_hits, materials.mesh_hits)
    over = ref.nhits > 12
    flagged = ref.lbuffer == F(-1.0)
    assert np.array_equal(flagged, ref.flagged_by >= 0)
    in_meshes = (ref.mesh_hits > 0).sum(1)
    counts = {
        "hit rays": np.count_nonzero(ref.nhits),
        "rays with more than 12 hits": np.count_nonzero(over),
        "... unflagged": np.count_nonzero(over & ~flagged),
        "flagged rays": np.count_nonzero(flagged),
        "rays in >= 2 meshes": np.count_nonzero(in_meshes >= 2),
        "rays in >= 3 meshes": np.count_nonzero(in_meshes >= 3),
        "rays that miss": np.count_nonzero(ref.nhits == 0),
    }
    print(counts)
    for name, v in counts.items():
        assert v >= floor, (name, v)
    assert np.count_nonzero(ref.sign_sum[:, 3] != 0) > 0 and np.count_nonzero(ref.sign_sum[:, 4] != 0) > 0


def sixteen_boxes():
    """Sixteen boxes, nested and overlapping: shrinking shells whose centres wander, so
    that each cuts through its neighbours' faces and a central ray crosses all sixteen."""
    out = []
    for k in range(16):
        r = F(40 - 2.2 * k)
        c = np.array([60 + (k % 3 - 1) * 2.5, (k % 4 - 1.5) * 2.0, ((k * 7) % 5 - 2) * 1.5], F)
        half = np.array([r, r * F(0.8), r * F(0.7)], F)
        out.append(box(c - half, c + half))
    return out


@functools.lru_cache(maxsize=None)
def boxes_sums(W, H):
    meshes = sixteen_boxes()
    return spectrum_ref.sums(meshes, kit.cam13_of(meshes, W, H), W, H)


_dragon = {}


def dragon_sums(dragon, W, H):
    if (W, H) not in _dragon:
        meshes = kit.dragon_scene(dragon)
        _dragon[(W, H)] = spectrum_ref.sums(meshes, kit.cam13_of(meshes, W, H), W, H)
    return _dragon[(W, H)]


def crafted_rows():
    """(distance (n, 3), sign_sum (n, 3), weights (2,), mu (3, 2)) -- the model's edge
    cases, M = 3, K = 2; mesh 2 has mu = 0 in bin 1 only."""
    inf = F(np.inf)
    d = np.array([
        [0.0, 0.0, 0.0],             # 0: the weight chain
        [0.0, 2.0, 0.0],             # 1: a zero distance beside others
        [-3.0, -2.5, -1.0],          # 2: negative sums
        [1.0, 2.0, 3.0],             # 3: flagged by the first mesh
        [1.0, 2.0, 3.0],             # 4: ... the middle one
        [1.0, 2.0, 3.0],             # 5: ... the last
        [inf, 1.0, 2.0],             # 6: +inf with mu > 0: both bins contribute weight * 0
        [1.0, -inf, 2.0],            # 7: -inf with mu > 0: +inf
        [1.0, 2.0, inf],             # 8: infinite with mu = 0 in bin 1 only: 0 * inf there
        [1.0, 2.0, -inf],            # 9: the same, -inf
        [NAN_NEG, 1.0, 2.0],         # 10: x86's default NaN as a distance
        [inf, -inf, 1.0],            # 11: +inf and -inf meet in x
        [-inf, 1.0, inf],            # 12: ... in bin 0 only (mesh 2's mu is 0 in bin 1)
        [700.0, -650.0, 20.0],       # 13: large finite exponents either way
        [NAN_NEG, 2.0, 3.0],         # 14: a NaN distance in a flagged ray
    ], F)
    s = np.zeros(d.shape, np.int32)
    s[3, 0] = 1
    s[4, 1] = -2
    s[5, 2] = 1
    s[14, 1] = 2
    w = np.array([50.0, 30.0], F)
    mu = np.array([[0.1037, 0.08], [0.3971, 0.25], [0.2, 0.0]], F)
    return d, s, w, mu


def lut(img):
    return oracle.lut_u8_array(img)
