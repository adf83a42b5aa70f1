"""mopt_cloud_voxel_downsample on the GPU against the numpy restatement (tests/voxel_reference.py).

Membership (the number of voxels and every population, in ascending voxel id) must be exact: the kernel
evaluates the header's fp64 expression.  A centroid coordinate of a voxel of k points may differ by
(k + 1) * eps_S * max |that coordinate in the voxel|: any order of k additions, the division and the one
rounding to the scalar type S (voxel_reference.centroid_bound) — derived, not measured.  The shapes are the
ones at which the segmented reduction changes path: a wave (64), a workgroup's tile (2048 = the sort's
tile), several tiles in a carry chain, voxels open on both edges of a tile."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import datasets as ds
from tests import voxel_reference as vr

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]


def _check(mo, pts, leaf):
    out, counts = mo.voxel_downsample(pts, leaf, return_counts=True)
    ids, want, want_counts, largest = vr.voxel_reference(pts, leaf)
    assert out.dtype == pts.dtype and counts.dtype == np.int32
    assert len(out) == len(want), (len(out), len(want))
    assert np.array_equal(counts, want_counts)
    assert (np.diff(ids) > 0).all()
    err = np.abs(out.astype(np.float64) - want.astype(np.float64))
    bound = vr.centroid_bound(want_counts, largest, pts.dtype)
    assert (err <= bound).all(), (err.max(), (err - bound).max())
    return out, counts


def _uniform(n, dtype, seed=11):
    return np.random.default_rng(seed).uniform(-5.0, 5.0, (n, 3)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 2048, 2049, 3 * 2048 + 1])
def test_all_points_in_one_voxel(hip_lib, dtype, n):
    pts = np.random.default_rng(n).uniform(0.1, 0.4, (n, 3)).astype(dtype)
    out, counts = _check(hip_lib, pts, 0.5)
    assert len(out) == 1 and counts[0] == n


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_point_its_own_voxel_in_ascending_id(hip_lib, dtype):
    i, j, k = np.meshgrid(np.arange(20), np.arange(25), np.arange(10), indexing="ij")
    lattice = (np.column_stack([i.ravel(), j.ravel(), k.ravel()]) + 0.5) * 0.5  # exact in fp32 too
    pts = lattice[np.random.default_rng(5).permutation(len(lattice))].astype(dtype)
    out, counts = _check(hip_lib, pts, 0.5)
    order = np.lexsort((lattice[:, 0], lattice[:, 1], lattice[:, 2]))  # x fastest, then y, then z
    assert np.array_equal(out, lattice[order].astype(dtype)) and (counts == 1).all()


# The head flags' scan (exclusiveScan, csrc/cell_order.hpp) runs over kept + 1 entries in tiles of 1024, and
# its middle step has one thread per tile total up to 256 tiles, several totals per thread beyond: kept + 1
# on both sides of one tile (1024) and of 256 tiles (262 144).  The dims multiply to `kept`.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(3, 11, 31), (8, 8, 16), (57, 63, 73), (64, 64, 64)])
def test_every_point_its_own_voxel_across_the_scan_regimes(hip_lib, dtype, dims):
    kept = dims[0] * dims[1] * dims[2]
    assert kept + 1 in (1024, 1025, 262144, 262145)
    i, j, k = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    lattice = (np.column_stack([i.ravel(), j.ravel(), k.ravel()]) + 0.5) * 0.5  # exact in fp32 too
    pts = lattice[np.random.default_rng(kept).permutation(kept)].astype(dtype)
    out, counts = _check(hip_lib, pts, 0.5)
    order = np.lexsort((lattice[:, 0], lattice[:, 1], lattice[:, 2]))  # x fastest, then y, then z
    assert np.array_equal(out, lattice[order].astype(dtype)) and (counts == 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_giant_voxels_on_both_edges_of_the_tiles(hip_lib, dtype):
    rng = np.random.default_rng(8)
    first = rng.uniform(0.05, 0.45, (5000, 3))
    singles = rng.uniform(0.05, 0.45, (300, 3)) + np.array([1.0, 0, 0]) + 0.5 * np.arange(300)[:, None] * [1, 0, 0]
    last = rng.uniform(0.05, 0.45, (5000, 3)) + np.array([160.0, 0, 0])
    pts = np.vstack([first, singles, last])
    for shuffled in (False, True):
        cloud = (pts[rng.permutation(len(pts))] if shuffled else pts).astype(dtype)
        out, counts = _check(hip_lib, cloud, 0.5)
        assert list(counts) == [5000] + [1] * 300 + [5000]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("leaf", [0.5, 3.0])
def test_uniform_volume_with_negative_coordinates(hip_lib, dtype, leaf):
    pts = _uniform(20_000, dtype)
    out, _ = _check(hip_lib, pts, leaf)
    again = hip_lib.voxel_downsample(pts, leaf)
    assert out.tobytes() == again.tobytes()  # the same bits from call to call


@pytest.mark.parametrize("dtype", DTYPES)
def test_points_exactly_on_voxel_faces(hip_lib, dtype):
    pts = (np.random.default_rng(3).integers(-12, 13, (4000, 3)) * 0.25).astype(dtype)
    _check(hip_lib, pts, 0.5)  # (multiples of 0.25: every key and every sum is exact)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cloud_far_from_the_origin(hip_lib, dtype):
    pts = (1.0e6 + np.random.default_rng(9).uniform(0.0, 10.0, (5000, 3))).astype(dtype)
    _check(hip_lib, pts, 0.5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows_are_dropped(hip_lib, dtype):
    mo = hip_lib
    clean = _uniform(3000, dtype, seed=21)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, 900.0, -900.0],
                    [700.0, np.nan, np.inf]], dtype=dtype)
    rows = np.vstack([clean, np.tile(bad, (40, 1))])
    where = np.random.default_rng(2).permutation(len(rows))
    mixed = np.empty_like(rows)
    mixed[where] = rows  # (interleaved, and the clean rows in another order than in `clean`)
    out, counts = _check(mo, mixed, 0.5)
    out_clean, counts_clean = _check(mo, clean, 0.5)
    assert np.array_equal(counts, counts_clean) and counts.sum() == len(clean)
    assert np.abs(out.astype(np.float64) - out_clean.astype(np.float64)).max() <= \
        2 * (counts.max() + 1) * np.finfo(dtype).eps * 5.0  # two summation orders of the same voxels
    none, no_counts = mo.voxel_downsample(np.tile(bad, (30, 1)), 0.5, return_counts=True)
    assert none.shape == (0, 3) and no_counts.shape == (0,)
    empty = mo.voxel_downsample(np.zeros((0, 3), dtype=dtype), 0.5)
    assert empty.shape == (0, 3)


def _raw(lib, pts, leaf, out, counts, capacity, flags=0):
    n_out = ctypes.c_int64(-1)
    rc = lib.mopt_cloud_voxel_downsample(
        0, pts.itemsize, pts.ctypes.data_as(ctypes.c_void_p), len(pts), leaf, flags,
        None if out is None else out.ctypes.data_as(ctypes.c_void_p),
        None if counts is None else counts.ctypes.data_as(ctypes.c_void_p), capacity, ctypes.byref(n_out))
    return rc, n_out.value


@pytest.mark.parametrize("dtype", DTYPES)
def test_capacity_and_count_only_calls_write_nothing(hip_lib, dtype):
    lib = hip_lib.capi.load()
    pts = _uniform(20_000, dtype)
    want = len(vr.voxel_reference(pts, 0.5)[0])
    assert _raw(lib, pts, 0.5, None, None, 0) == (0, want)
    out = np.full((want, 3), -77.0, dtype=dtype)
    counts = np.full(want, -77, dtype=np.int32)
    assert _raw(lib, pts, 0.5, out, counts, want - 1) == (0, want)
    assert (out == -77.0).all() and (counts == -77).all()
    assert _raw(lib, pts, 0.5, None, counts, want) == (0, want) and (counts == -77).all()
    # points without populations
    assert _raw(lib, pts, 0.5, out, None, want) == (0, want)
    assert np.array_equal(out, hip_lib.voxel_downsample(pts, 0.5))


@pytest.mark.parametrize("dtype", DTYPES)
def test_too_many_cells_is_refused_with_a_leaf_that_fits(hip_lib, dtype):
    lib = hip_lib.capi.load()
    pts = np.array([[0, 0, 0], [1.0e6, 1.0e6, 1.0e6]], dtype=dtype)
    rc, n_out = _raw(lib, pts, 1e-4, None, None, 0)
    message = lib.mopt_last_error().decode()
    assert rc == 1 and n_out == 0 and "leaf" in message and "1e+06" in message, (rc, message)
    # the leaf it names does fit
    fits = float(message.rsplit(" ", 1)[1])
    assert 1e-4 < fits < 1e4 and _raw(lib, pts, fits, None, None, 0) == (0, 2)


def _surface_pair(dtype):
    """A scanned relief with four returns per patch (20 000 points) and its rigidly moved copy; the pose of
    test_gpu_device_lm.test_icp_* (tgt = R src + t)."""
    rng = np.random.default_rng(4)
    xy = np.repeat(rng.random((5000, 2)) * 20.0, 4, axis=0) + rng.normal(0.0, 0.004, (20_000, 2))
    z = 1.5 * np.sin(0.6 * xy[:, 0]) * np.cos(0.5 * xy[:, 1]) + 0.4 * np.sin(1.7 * xy[:, 0] + 0.9 * xy[:, 1])
    tgt = np.column_stack([xy, z])
    x_true = np.array([0.15, -0.1, 0.2, 0.02, -0.03, 0.025])
    th = np.linalg.norm(x_true[3:])
    a = x_true[3:] / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    src = (tgt - x_true[:3]) @ R
    return src.astype(dtype), tgt.astype(dtype), x_true


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_in_device_out_feeds_the_icp_create_call(hip_lib, dtype):
    mo = hip_lib
    import torch
    src, tgt, x_true = _surface_pair(dtype)
    thin = {}
    for name, cloud in (("src", src), ("tgt", tgt)):
        host, host_counts = _check(mo, cloud, 0.1)
        dev, dev_counts = mo.voxel_downsample(torch.from_numpy(cloud).cuda(), 0.1, return_counts=True)
        assert dev.is_cuda and dev.dtype == torch.from_numpy(cloud).dtype and dev_counts.dtype == torch.int32
        assert dev.cpu().numpy().tobytes() == host.tobytes()  # bit for bit the host path's result
        assert np.array_equal(dev_counts.cpu().numpy(), host_counts)
        assert len(host) < 0.35 * len(cloud)  # (it thins: four returns per patch become one point)
        thin[name] = dev
    # the thinned clouds never leave the device: mopt_icp_create_from(MOPT_INPUT_DEVICE), then the solve
    # of test_gpu_device_lm.test_icp_*: 60 iterations, the pose to 2e-3
    cost = mo.IcpCost(thin["src"], thin["tgt"], max_distance=0.6)
    xd, rep = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], np.zeros(6), max_iterations=60)
    cost.close()
    assert np.abs(xd - x_true).max() < 2e-3, (xd - x_true, rep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpp_wrapper_matches_the_restatement(hip_lib, dtype, tmp_path):
    exe = str(tmp_path / "cloud_filter")
    lib_dir = os.path.join(ds.ROOT, "moptimizer_0_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ds.ROOT, "include"), "-o", exe,
                           os.path.join(ds.ROOT, "tests", "cpp", "cloud_filter.cpp"),
                           "-L", lib_dir, "-lmoptimizer_hip", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    refused = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert refused.returncode == 0 and "refused 2 of 2" in refused.stdout, refused.stdout + refused.stderr
    pts = _uniform(5000, dtype, seed=31)
    paths = [str(tmp_path / name) for name in ("in.bin", "out.bin", "counts.bin")]
    pts.tofile(paths[0])
    ran = subprocess.run([exe, "f64" if dtype == np.float64 else "f32", "0.75"] + paths, capture_output=True,
                         text=True, timeout=120)
    assert ran.returncode == 0 and "FAIL" not in ran.stdout, ran.stdout + ran.stderr
    out = np.fromfile(paths[1], dtype=dtype).reshape(-1, 3)
    counts = np.fromfile(paths[2], dtype=np.int32)
    _, want, want_counts, largest = vr.voxel_reference(pts, 0.75)
    assert np.array_equal(counts, want_counts) and len(out) == len(want)
    assert (np.abs(out.astype(np.float64) - want.astype(np.float64)) <=
            vr.centroid_bound(want_counts, largest, dtype)).all()
