"""Scenes and grids for the voxeliser's tests (test-only), shared by the CPU and GPU suites.
A case is a dict: meshes (a list of (T, 9) float32 soups, as posed), dims (nx, ny, nz), origin and spacing
(x, y, z) float32, value (one float32 per mesh).  `reference(name)` is voxel_ref's definition -- every triangle
against every column -- computed once and shared read-only; the cases named in FAST are too large for it and
take voxel_ref.voxelize_fast, which test_voxelize_cpu.py checks against the definition on every other case."""
import functools
import os

import numpy as np

import scene_kit
import simpleraytracing_amd as xrt
import voxel_ref

F = np.float32
DRAGON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "dragon.ply")


def _case(meshes, dims, origin, spacing, value=None):
    meshes = [np.ascontiguousarray(m, F).reshape(-1, 9) for m in meshes]
    value = np.arange(1, len(meshes) + 1, dtype=F) * F(0.375) if value is None else np.asarray(value, F)
    return dict(meshes=meshes, dims=tuple(int(n) for n in dims), origin=np.asarray(origin, F),
                spacing=np.broadcast_to(np.asarray(spacing, F), (3,)).copy(), value=value)


@functools.lru_cache(maxsize=None)
def dragon():
    return np.ascontiguousarray(xrt.load_ply(DRAGON), F).reshape(-1, 9)


def turned_box():
    """A box turned 33 degrees about (1, 2, 3): no face is parallel to an axis."""
    pose = xrt.pose_rotation((1.0, 2.0, 3.0), 33.0, (0.25, -0.5, 0.125))
    return scene_kit.box((-1.0, -1.5, -0.75), (1.25, 0.5, 1.0)), pose


def single_triangle():
    return np.array([[0.1, 0.2, 0.3, 2.3, 0.4, 1.1, 0.9, 2.6, 1.9]], F)


def degenerate_soup():
    """Zero-area triangles (a point, a doubled vertex, three collinear vertices) and triangles seen edge-on from
    +z (n.z == 0, some with a non-zero area), in front of one ordinary triangle."""
    return np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1],
                     [0.5, 0.5, 0.5, 2.5, 2.5, 1.5, 2.5, 2.5, 1.5],
                     [0.25, 0.25, 0.25, 1.25, 1.25, 1.25, 2.25, 2.25, 2.25],
                     [0.5, 1.0, 0.0, 2.5, 1.0, 0.0, 1.5, 1.0, 3.0],          # in the plane y = 1
                     [1.0, 0.5, 0.0, 1.0, 2.5, 0.0, 1.0, 1.5, 3.0],          # in the plane x = 1
                     [0.5, 0.5, 0.0, 2.5, 2.5, 0.0, 1.5, 1.5, 3.0],          # in the plane x = y
                     [0.2, 0.3, 1.0, 2.7, 0.4, 1.2, 1.1, 2.8, 1.4]], F)


def sixteen_meshes():
    """Sixteen overlapping boxes: mesh m is a box shifted by m steps along the diagonal, so that up to six overlap
    in a voxel, bit 15 and label 16 occur and the value sums have several terms."""
    step = np.array([0.4, 0.3, 0.35], F)
    return [scene_kit.box(F(m) * step, F(m) * step + np.array([2.1, 1.7, 1.9], F)) for m in range(16)]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "box32":
        return _case([scene_kit.box((-1.0, -1.0, -1.0), (1.0, 1.5, 2.0))], (32, 32, 32), (-2.0, -2.0, -2.5), 0.15)
    if name == "exact":
        # centres at odd multiples of 0.125 on every axis, and so are the box's corners: its faces lie on slice
        # centres (z == c_z(k)), its edges on column centres (w == 0 and a.y == py)
        return _case([scene_kit.box((0.375, 0.625, 0.375), (2.125, 1.875, 2.625))], (12, 10, 12), (0.0, 0.0, 0.0), 0.25)
    if name == "cut":
        # the grid holds a corner of the box only: crossings below slice 0 and past the last slice (plane nz),
        # and most of the box's columns outside the grid
        return _case([scene_kit.box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))], (9, 14, 6), (0.13, -1.6, -0.41), (0.21, 0.17, 0.13))
    if name == "aniso":
        box, pose = turned_box()
        return _case([xrt.pose_triangles(box, pose)], (37, 29, 23), (-2.3, -2.9, -1.7), (0.13, 0.17, 0.19))
    if name == "sixteen":
        v = (F(1.0) / np.arange(3, 19, dtype=F)).astype(F)                   # no two sums alike, none exact
        v[5] = F(-0.0)
        return _case(sixteen_meshes(), (21, 17, 19), (-0.3, -0.2, -0.4), (0.41, 0.37, 0.39), v)
    if name == "posed":
        box, pose = turned_box()
        return _case([scene_kit.box((-2.5, -2.5, -2.5), (2.5, 2.5, 2.5)), xrt.pose_triangles(box, pose)], (24, 20, 28),
                     (-3.0, -2.0, -3.5), (0.25, 0.2, 0.25))
    if name == "sheets":
        # striped_sheets' open quads face +x: with the axes rolled (x, y, z) -> (y, z, x) they face the columns
        s = scene_kit.striped_sheets().reshape(-1, 3, 3)[:, :, [1, 2, 0]].reshape(-1, 9)
        return _case([s], (40, 20, 24), (-32.0, -27.0, 40.0), (1.6, 2.7, 1.3))
    if name == "sheets_edge_on":
        # as they come the quads lie in planes x = const, edge-on to the columns: n.z == 0 with an area
        return _case([scene_kit.striped_sheets()], (24, 40, 20), (40.0, -32.0, -27.0), (1.3, 1.6, 2.7))
    if name == "triangle":
        return _case([single_triangle()], (16, 16, 8), (0.0, 0.0, 0.0), (0.2, 0.2, 0.3))
    if name == "degenerate":
        return _case([degenerate_soup()], (12, 12, 8), (0.0, 0.0, 0.0), (0.25, 0.25, 0.5))
    if name == "soup":
        # open random triangles, collinear and duplicate ones among them, two meshes
        s = scene_kit.synthetic_soup(n=600)
        return _case([s[:350], s[350:]], (20, 24, 16), (-60.0, -58.0, -55.0), (6.0, 5.0, 7.0))
    if name == "dragon48":
        d = dragon()
        dims, origin, spacing = voxel_ref.dragon_grid(d, 48)
        return _case([d], dims, origin, spacing)
    if name == "dragon_in_box":
        # both regimes of the scatter at once: at 14^3 the dragon's triangles cover 12 columns at most, under the
        # queue's threshold of 16, and the four triangles of the box's faces across the columns 84 each
        d = dragon()
        dims, origin, spacing = voxel_ref.dragon_grid(d, 14)
        v = d.reshape(-1, 3)
        pad = F(0.02) * F((v.max(0) - v.min(0)).max())
        return _case([scene_kit.box(v.min(0) - pad, v.max(0) + pad), d], dims, origin, spacing, (0.02, 0.2))
    raise KeyError(name)


SMALL = ["box32", "exact", "cut", "aniso", "sixteen", "posed", "sheets", "sheets_edge_on", "triangle", "degenerate", "soup"]
FAST = ["dragon48", "dragon_in_box"]
OPEN = ["sheets", "triangle", "soup"]


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    fn = voxel_ref.voxelize_fast if name in FAST else voxel_ref.voxelize
    ref = fn(c["meshes"], c["dims"], c["origin"], c["spacing"], c["value"])
    for a in ref.values():
        a.setflags(write=False)
    return ref


def assert_equal(got, ref, what):
    """Every output of `got` equals the reference's bit for bit."""
    for key in ("mask", "labels", "odd_columns"):
        assert np.array_equal(got[key], ref[key]), f"{what}: {key} differs"
    assert np.array_equal(got["volume"].view(np.uint32), ref["volume"].view(np.uint32)), f"{what}: volume differs"
