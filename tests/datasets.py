"""Deterministic inputs shared by the tests, smoke() and bench.py."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# tst/point2point.cpp:93-101 — Rx(0.3) * Ry(0.4) * Rz(0.5), t = (10.5, 10.2, 0.1)
FIXTURE_T = np.array([10.5, 10.2, 0.1])
# (t, log R) of that pose: where LM must arrive from x0 = 0
FIXTURE_X = np.array([10.5, 10.2, 0.1, 0.38994502377414, 0.31542006718654, 0.54962215934141])
X_ZERO = np.zeros(6)
X_GENERIC = np.array([0.5, -0.3, 0.2, 0.1, -0.2, 0.3])


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def fixture_rotation():
    return _rot(0, 0.3) @ _rot(1, 0.4) @ _rot(2, 0.5)


def apply_fixture_transform(src):
    """tgt = T * [p; 1] with the association of a 4x4 matrix-vector product
    (tst/point2point.cpp:109-123)."""
    R = fixture_rotation()
    t = FIXTURE_T
    out = np.empty_like(src)
    for r in range(3):
        out[:, r] = ((R[r, 0] * src[:, 0] + R[r, 1] * src[:, 1]) + R[r, 2] * src[:, 2]) + t[r]
    return out


def facade_pair():
    q = np.load(os.path.join(GOLDEN, "fachada_xyz_1e8.npz"))["xyz_1e8"]
    src = q.astype(np.float64) / 1e8
    return src, apply_fixture_transform(src)


def synthetic_pair(n, seed=42, noise=0.0, dtype=np.float64):
    """src ~ U[0,10]^3 (the shape of tst/parallel.cpp:39-47); tgt = R src + t with the fixture
    pose, optionally + N(0, noise^2)."""
    rng = np.random.default_rng(seed)
    src = rng.random((n, 3)) * 10.0
    tgt = apply_fixture_transform(src)
    if noise > 0:
        tgt = tgt + rng.normal(0.0, noise, size=tgt.shape)
    return src.astype(dtype), tgt.astype(dtype)


# Scenes at the scales registration is run at (tests/test_gpu_scene_scale.py): where the source cloud
# lies (offset added to a unit box scaled by `box`), where the pose under test sends it (`shift` of the
# target's centroid against the source's), the target's noise and the translation error of the pose
# under test, which with SCENE_ROTATION_ERROR keeps the residuals at a tenth of the cloud's size or so.
SCENES = {
    # the shape every other test uses: the control
    "sensor": dict(box=(10, 10, 10), offset=(0, 0, 0), shift=(0, 0, 0), noise=0.01, dt=(0.3, -0.2, 0.25)),
    # a site frame, a map frame: source and target in the same far frame
    "site": dict(box=(10, 10, 10), offset=(1e3, 7e2, 10), shift=(0, 0, 0), noise=0.01, dt=(0.3, -0.2, 0.25)),
    "map": dict(box=(10, 10, 10), offset=(1e5, 7e4, 1e3), shift=(0, 0, 0), noise=0.01, dt=(0.3, -0.2, 0.25)),
    # a map-frame (UTM) scan registered to a target in a local frame: t ~ -R c
    "utm_to_local": dict(box=(10, 10, 10), offset=(1e6, 7e5, 1e4), shift=(-1e6, -7e5, -1e4), noise=0.01,
                         dt=(0.3, -0.2, 0.25)),
    "utm_to_local_7e6": dict(box=(10, 10, 10), offset=(7e6, 4.9e6, 7e4), shift=(-7e6, -4.9e6, -7e4),
                             noise=0.01, dt=(0.3, -0.2, 0.25)),
    # ... and the other way round: a far translation
    "local_to_map": dict(box=(10, 10, 10), offset=(0, 0, 0), shift=(1e6, 7e5, 1e4), noise=0.01,
                         dt=(0.3, -0.2, 0.25)),
    # a millimetre-sized object, a flat wall
    "mm": dict(box=(1e-2, 1e-2, 1e-2), offset=(0, 0, 0), shift=(0, 0, 0), noise=1e-5, dt=(3e-4, -2e-4, 2.5e-4)),
    "wall": dict(box=(100, 1, 0.01), offset=(0, 0, 0), shift=(0, 0, 0), noise=0.01, dt=(0.3, -0.2, 0.25)),
}
SCENE_ROTATION_ERROR = np.array([0.01, -0.02, 0.015])
SCENE_SIZES = (4097, 513)  # eight fp64 tiles + 1; one + 1
_SCENE_SEEDS = {name: 1000 + 17 * k for k, name in enumerate(SCENES)}


def _exp_so3(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    a = np.asarray(w) / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene_pair(name, n, dtype=np.float64, rot=None, about_origin=False):
    """(src, tgt, x) of a scene of SCENES: src ~ U[0, box] + offset; tgt = the source turned by the
    fixture rotation about its centroid, moved by `shift`, + N(0, noise^2); x the pose under test —
    rotation vector `rot` (default: the fixture's + SCENE_ROTATION_ERROR), translation such that the
    source's centroid lands `dt` from the target's.  about_origin: the same-frame pose with a small
    translation instead — tgt = Exp(rot) src + noise, a turn about the frame's origin, and
    x = (dt, rot), so that |t| stays a fraction of a metre however far the cloud lies.  Fixed seed per
    scene, everything rounded to `dtype` at the end."""
    sc = SCENES[name]
    rng = np.random.default_rng(_SCENE_SEEDS[name] + n)
    src = rng.random((n, 3)) * np.array(sc["box"], dtype=np.float64) + np.array(sc["offset"], dtype=np.float64)
    if about_origin:
        w = np.zeros(3) if rot is None else np.asarray(rot, dtype=np.float64)
        R = _exp_so3(w).astype(np.longdouble)
        tgt = np.asarray(src.astype(np.longdouble) @ R.T, dtype=np.float64)
        tgt = tgt + rng.normal(0.0, sc["noise"], size=src.shape)
        x = np.concatenate([np.array(sc["dt"], dtype=np.float64), w])
        return src.astype(dtype), tgt.astype(dtype), x.astype(dtype)
    c = src.mean(axis=0)
    c_tgt = c + np.array(sc["shift"], dtype=np.float64)
    tgt = (src - c) @ fixture_rotation().T + c_tgt + rng.normal(0.0, sc["noise"], size=src.shape)
    w = FIXTURE_X[3:] + SCENE_ROTATION_ERROR if rot is None else np.asarray(rot, dtype=np.float64)
    # t = c_tgt - R_x c + dt, the product in long double: at a 1e7 offset its fp64 rounding is 1e-9
    Rc = (_exp_so3(w).astype(np.longdouble) @ c.astype(np.longdouble))
    t = np.asarray(c_tgt.astype(np.longdouble) - Rc, dtype=np.float64) + np.array(sc["dt"])
    x = np.concatenate([t, w])
    return src.astype(dtype), tgt.astype(dtype), x.astype(dtype)


def synthetic_camera(n, seed=7, x_true=(-0.01, 0.02, -0.058, 0.018, -0.0013, 0.027)):
    """Points in front of the camera of tst/camera_calibration.cpp and the rounded pixels their
    projection under x_true lands on."""
    rng = np.random.default_rng(seed)
    pts = np.empty((n, 4))
    pts[:, 0] = rng.uniform(1.5, 4.0, n)     # depth along the laser x axis
    pts[:, 1] = rng.uniform(-1.0, 1.0, n)
    pts[:, 2] = rng.uniform(-0.5, 0.8, n)
    pts[:, 3] = 1.0
    K = np.array([[586.122314453125, 0, 638.8477694496105, 0],
                  [0, 722.3973388671875, 323.031267074588, 0], [0, 0, 1, 0]])
    C = np.eye(4)
    C[:3, :3] = _rot(0, np.pi / 2) @ _rot(2, np.pi / 2)
    x = np.asarray(x_true, dtype=np.float64)
    th = np.linalg.norm(x[3:])
    a = x[3:] / th
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = x[:3]
    o = (K @ T @ C @ pts.T).T
    pix = np.rint(o[:, :2] / o[:, 2:3]).astype(np.int32)
    return pts, pix
