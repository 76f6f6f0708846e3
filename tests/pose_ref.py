"""Mesh poses in numpy f32: the reference of xrt_pose_triangles and k_pose.

A pose is 12 f32, row-major 3x4 [R | t].  For a vertex (x, y, z) of the rest soup

    p_i  = (r_i0 * x + r_i1 * y) + r_i2 * z
    v'_i = p_i + t_i   if some t_j is not +-0, else p_i

every product and sum rounded to f32 on its own (numpy f32 arrays do exactly
that).  A pose whose 12 values are bitwise the identity returns its input bits.
"""
import numpy as np

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def is_identity(pose):
    return np.array_equal(np.asarray(pose, F).reshape(12).view(np.uint32), IDENTITY.view(np.uint32))


def apply_pose(tris, pose):
    """A (T, 9) soup under one pose (None: the identity)."""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    if pose is None or is_identity(pose):
        return tris.copy()
    q = np.asarray(pose, F).reshape(3, 4)
    v = tris.reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = (q[i, 0] * x + q[i, 1] * y) + q[i, 2] * z
        if np.any(q[:, 3] != 0):                   # (-0.0 == 0: a translation of mixed +-0 adds nothing)
            for i in range(3):
                out[:, i] = out[:, i] + q[i, 3]
    return out.reshape(-1, 9)


def apply(meshes, poses):
    """The scene's meshes, each under its pose: poses is a list (None entries: rest) or a dict by mesh."""
    if isinstance(poses, dict):
        poses = [poses.get(m) for m in range(len(meshes))]
    return [apply_pose(m, q) for m, q in zip(meshes, poses)]


def rotation(axis, degrees, centre=(0.0, 0.0, 0.0)):
    """xrt_pose_rotation restated in f64: Rodrigues about the normalised axis, t = c - R c, rounded once."""
    a = np.asarray(axis, F).astype(np.float64)
    c = np.asarray(centre, F).astype(np.float64)
    u = a / np.sqrt((a * a).sum())
    th = np.float64(degrees) * (np.pi / 180.0)
    co, si = np.cos(th), np.sin(th)
    k = 1.0 - co
    R = np.array([[co + u[0] * u[0] * k, u[0] * u[1] * k - u[2] * si, u[0] * u[2] * k + u[1] * si],
                  [u[1] * u[0] * k + u[2] * si, co + u[1] * u[1] * k, u[1] * u[2] * k - u[0] * si],
                  [u[2] * u[0] * k - u[1] * si, u[2] * u[1] * k + u[0] * si, co + u[2] * u[2] * k]])
    t = c - ((R[:, 0] * c[0] + R[:, 1] * c[1]) + R[:, 2] * c[2])
    return np.concatenate([R, t[:, None]], 1), np.concatenate([R, t[:, None]], 1).astype(F).reshape(12)


def translation(t):
    q = IDENTITY.copy()
    q[3], q[7], q[11] = t
    return q
