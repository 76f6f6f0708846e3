"""Scenes of the materials model's tests, and their references (computed once)."""
import functools

import numpy as np

import materials_ref
from oracle import oracle
from scene_kit import box, plane_stack, second_mesh_for, striped_sheets

F = np.float32

PHANTOM_MU = [0.1037, 0.3971, 0.5, 0.2059, 0.05]
DRAGON_MU = [0.1037, 0.3971, 0.2]


def phantom():
    """Tissue around bone, an empty mesh, a deep stack of alternately wound planes
    (more hits than the hit list holds, signs cancelling) and open quads (flags)."""
    stack = plane_stack(16, alternate=True).reshape(-1, 3)
    stack = (stack * np.array([50, 18, 16], F) + np.array([72, -28, -22], F)).astype(F).reshape(-1, 9)
    return [box((40, -30, -25), (90, 30, 25)), box((55, -12, -10), (70, 8, 14)), np.zeros((0, 9), F),
            np.ascontiguousarray(stack), np.ascontiguousarray(striped_sheets(seed=5, n=12)[12:])]


def dragon_scene(dragon):
    p = dragon.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    r = hi - lo
    return [box(lo - F(0.1) * r, hi + F(0.1) * r), dragon, second_mesh_for(dragon)]


def cam13_of(meshes, W, H):
    return oracle.camera_for_scene(meshes, W, H)


@functools.lru_cache(maxsize=None)
def phantom_ref(W, H):
    meshes = phantom()
    return materials_ref.render(meshes, PHANTOM_MU, cam13_of(meshes, W, H), W, H)


@functools.lru_cache(maxsize=None)
def mesh0_only_ref(W, H):
    """The phantom with the fork's mesh filter: what the scene gave before this model."""
    meshes = phantom()
    return materials_ref.render(meshes, PHANTOM_MU, cam13_of(meshes, W, H), W, H, mesh0_only=True)


def check_exercised(ref, mesh0_ref, floor):
    """The phantom's reference exercises the model: each count is at least `floor`."""
    over = ref.nhits > 12
    flagged = ref.flagged_by >= 0
    in_meshes = (ref.mesh_hits > 0).sum(1)
    counts = {
        "hit rays": np.count_nonzero(ref.nhits),
        "rays with more than 12 hits": np.count_nonzero(over),
        "... unflagged": np.count_nonzero(over & ~flagged),
        "flagged rays": np.count_nonzero(flagged),
        "rays in >= 2 meshes": np.count_nonzero(in_meshes >= 2),
        "rays in >= 3 meshes": np.count_nonzero(in_meshes >= 3),
        "pixels that differ from mesh 0 only": np.count_nonzero(
            ref.lbuffer.view(np.uint32) != mesh0_ref.lbuffer.view(np.uint32)),
    }
    print(counts, "flagged by mesh:", np.bincount(ref.flagged_by[flagged], minlength=5), "max hits", ref.nhits.max())
    for name, v in counts.items():
        assert v >= floor, (name, v)
    assert ref.nhits.max() > 12
    assert np.count_nonzero(ref.flagged_by == 3) > 0 and np.count_nonzero(ref.flagged_by == 4) > 0


_dragon_ref = {}


def dragon_ref(dragon, W=128, H=112):
    if (W, H) not in _dragon_ref:
        meshes = dragon_scene(dragon)
        _dragon_ref[(W, H)] = materials_ref.render(meshes, DRAGON_MU, cam13_of(meshes, W, H), W, H)
    return _dragon_ref[(W, H)]


def lut(img):
    return oracle.lut_u8_array(img)
