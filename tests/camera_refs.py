"""The scenes of the general-camera GPU suites and the oracle's frame of each
(scene, case), computed once per session and shared between the modules."""
import camera_kit as ck
from oracle import oracle
from scene_kit import corner_soup, synthetic_soup

SCENES = ["dragon", "soup", "corner", "inside"]
_frames = {}


def scene(name, dragon):
    """(triangles, W, H, base camera, centre of the turn)."""
    if name == "dragon":
        tris, W, H = dragon, 67, 45
    elif name == "soup":
        tris, W, H = synthetic_soup(seed=9, n=2000), 80, 72
    elif name == "corner":
        tris, W, H = corner_soup(), 33, 31
    else:                                       # the source inside the soup
        tris, W, H = synthetic_soup(), 64, 48
        return tris, W, H, ck.inside_source_camera(tris, W, H), ck.scene_centre([tris[:200]])
    return tris, W, H, oracle.camera_for_mesh(tris, W, H), ck.scene_centre([tris])


def reference(name, case, dragon):
    """(triangles, W, H, the 13 camera floats, the oracle's frame), read-only."""
    if (name, case) not in _frames:
        tris, W, H, base, centre = scene(name, dragon)
        c13 = ck.general_camera(base, centre, W, H, **ck.CASES[case])
        ref = oracle.render_rows(tris, c13, W, H)
        for a in (c13,) + tuple(ref[:4]):
            a.setflags(write=False)
        _frames[name, case] = (tris, W, H, c13, ref)
    return _frames[name, case]
