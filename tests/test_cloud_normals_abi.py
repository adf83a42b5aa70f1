"""mopt_cloud_estimate_normals at the C ABI without a device: the symbol is exported, every up-front
refusal comes back as MOPT_ERR_INVALID_ARGUMENT with a message that names the argument, the header stays
plain C, the C++ wrapper (include/moptimizer_amd/cloud_filter.hpp) compiles warning-free, the numpy
restatement the GPU tests check against (tests/normals_reference.py) gives a hand-worked case, and the
kernel's per-point arithmetic (csrc/normals_device.hpp), run on the CPU, stays within the bound the GPU
tests hold the kernel to."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import datasets as ds
from tests import normals_reference as nr

INVALID, NO_DEVICE = 1, 3
INC = os.path.join(ds.ROOT, "include")
CSRC = os.path.join(ds.ROOT, "moptimizer_0_amd", "csrc")


def _call(lib, xyz, count, radius=0.5, min_neighbors=3, viewpoint=None, scalar_bytes=8, flags=0,
          with_normals=True):
    out = np.full((max(count, 1), 3), -7.0)
    view = None if viewpoint is None else (ctypes.c_double * 3)(*viewpoint)
    rc = lib.mopt_cloud_estimate_normals(
        0, scalar_bytes, None if xyz is None else xyz.ctypes.data_as(ctypes.c_void_p), count, radius,
        min_neighbors, view, flags, out.ctypes.data_as(ctypes.c_void_p) if with_normals else None, None, None)
    return rc, lib.mopt_last_error().decode(), out


def test_symbol_is_exported_and_the_python_wrapper_with_it():
    import moptimizer_0_amd as mo
    lib = mo.capi.load()
    assert hasattr(lib, "mopt_cloud_estimate_normals")
    assert mo.estimate_normals is mo.capi.estimate_normals
    normals, curvature, counts = mo.estimate_normals(np.zeros((0, 3), dtype=np.float32), 0.5,
                                                     return_curvature=True, return_counts=True)
    assert normals.shape == (0, 3) and normals.dtype == np.float32
    assert curvature.shape == (0,) and counts.shape == (0,) and counts.dtype == np.int32
    assert mo.estimate_normals(np.zeros((0, 3)), 0.5).shape == (0, 3)


def test_invalid_arguments_are_refused_before_a_device_is_looked_for():
    import moptimizer_0_amd as mo
    lib = mo.capi.load()
    pts = np.zeros((4, 3))
    inf, nan = float("inf"), float("nan")
    cases = {
        "out_normals": dict(xyz=pts, count=4, with_normals=False),
        "scalar_bytes": dict(xyz=pts, count=4, scalar_bytes=2),
        "scalar_bytes ": dict(xyz=pts, count=4, scalar_bytes=16),
        "flags": dict(xyz=pts, count=4, flags=4),
        "flags ": dict(xyz=pts, count=4, flags=1 | 8),
        "count": dict(xyz=pts, count=-1),
        "count ": dict(xyz=pts, count=2 ** 31),
        "radius": dict(xyz=pts, count=4, radius=0.0),
        "radius ": dict(xyz=pts, count=4, radius=-1.0),
        "radius  ": dict(xyz=pts, count=4, radius=nan),
        "radius   ": dict(xyz=pts, count=4, radius=inf),
        "min_neighbors": dict(xyz=pts, count=4, min_neighbors=-1),
        "xyz": dict(xyz=None, count=4),
        "viewpoint": dict(xyz=pts, count=4, viewpoint=(0.0, nan, 0.0)),
        "viewpoint ": dict(xyz=pts, count=4, viewpoint=(0.0, 0.0, -inf)),
    }
    for what, kw in cases.items():
        rc, message, out = _call(lib, **kw)
        assert rc == INVALID and what.strip() in message, (what, rc, message)
        assert (out == -7.0).all()
    # an empty cloud is no error, needs no device and writes nothing
    rc, _, out = _call(lib, None, 0)
    assert rc == 0 and (out == -7.0).all()
    rc, _, _ = _call(lib, None, 0, with_normals=False)
    assert rc == 0


def test_valid_call_without_a_device_says_so():
    import moptimizer_0_amd as mo
    rc, message, out = _call(mo.capi.load(), nr.lattice_plane(16), 16, viewpoint=(0.0, 0.0, 10.0))
    if mo.capi.device_count() > 0:  # (where there is one the call goes through: test_gpu_cloud_normals.py)
        assert rc == 0 and np.array_equal(out, np.tile([0.0, 0.0, 1.0], (16, 1))), (rc, message)
    else:
        assert rc == NO_DEVICE and "device" in message and (out == -7.0).all(), (rc, message)


def test_header_with_the_normals_entry_is_plain_c(tmp_path):
    src = tmp_path / "use_normals.c"
    src.write_text('#include "moptimizer_hip.h"\n'
                   "int main(void) {\n"
                   "  double xyz[3] = {0, 0, 0}, view[3] = {0, 0, 1}, normals[3], curvature[1];\n"
                   "  int32_t counts[1];\n"
                   "  return mopt_cloud_estimate_normals(0, 8, xyz, 1, 0.5, 3, view, MOPT_CLOUD_INPUT_DEVICE,\n"
                   "                                     normals, curvature, counts);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC,
                           "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, "-x", "c++",
                           "-fsyntax-only", str(src)])


def test_cpp_wrapper_header_compiles_without_warnings(tmp_path):
    src = tmp_path / "use_filter.cpp"
    src.write_text('#include "moptimizer_amd/cloud_filter.hpp"\n'
                   "int main() {\n"
                   "  std::vector<double> d(6, 0.0), curvature;\n"
                   "  std::vector<float> f(6, 0.f);\n"
                   "  std::vector<int32_t> counts;\n"
                   "  const double view[3] = {0, 0, 1};\n"
                   "  const auto a = moptimizer::io::estimateNormals(d, 0.5, 3, view, 0, &curvature, &counts);\n"
                   "  const auto b = moptimizer::io::estimateNormals<float>(f, 0.5);\n"
                   "  return int(a.size() + b.size() + counts.size());\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, "-fsyntax-only",
                           str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, "-fsyntax-only",
                           os.path.join(ds.ROOT, "tests", "cpp", "cloud_normals.cpp")])


def test_restatement_on_the_plane_lattice():
    """A 9 x 9 patch of the plane z = 0.75 on multiples of 0.25, radius 0.5: the offsets with i^2 + j^2 <= 4 are
    neighbours (those at exactly the radius included) — 13 for an interior point, 6 at a corner — and the
    normal is (0, 0, 1) towards a viewpoint above the plane, (0, 0, -1) towards one below."""
    pts = nr.lattice_plane(81)
    ref = nr.normals_reference(pts, 0.5, viewpoint=(0.0, 0.0, 10.0))
    ix, iy = np.rint(pts[:, 0] / 0.25).astype(int) + 3, np.rint(pts[:, 1] / 0.25).astype(int) + 2
    interior = (ix >= 2) & (ix <= 6) & (iy >= 2) & (iy <= 6)
    corner = ((ix == 0) | (ix == 8)) & ((iy == 0) | (iy == 8))
    assert interior.sum() == 25 and (ref["counts"][interior] == 13).all() and (ref["counts"][corner] == 6).all()
    assert ref["counts"].dtype == np.int32
    assert np.array_equal(ref["normals"], np.tile([0.0, 0.0, 1.0], (81, 1)))
    assert (ref["curvature"] == 0.0).all() and (ref["eigenvalues"][:, 0] == 0.0).all()
    below = nr.normals_reference(pts, 0.5, viewpoint=(0.0, 0.0, -10.0))
    assert np.array_equal(below["normals"], np.tile([0.0, 0.0, -1.0], (81, 1)))
    # too few neighbours, a non-finite row, min_neighbors
    two = nr.normals_reference(np.vstack([pts[:2], [[np.nan, 0.0, 0.0]]]).astype(np.float32), 0.5)
    assert list(two["counts"][2:]) == [0] and np.isnan(two["normals"]).all() and np.isnan(two["curvature"]).all()
    many = nr.normals_reference(pts, 0.5, min_neighbors=13)
    assert np.array_equal(np.isnan(many["normals"][:, 0]), ref["counts"] < 13)
    assert np.isinf(nr.normal_bound([5], 0.5, [[0.0, 0.0, 1.0]], np.float64)).all()


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    """tests/cpp/normals_solver.cpp: the kernel's per-point arithmetic compiled for the CPU, every operation
    rounded on its own."""
    exe = str(tmp_path_factory.mktemp("normals") / "normals_solver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas", "-I", CSRC, "-o", exe,
                           os.path.join(ds.ROOT, "tests", "cpp", "normals_solver.cpp")])

    def run(pts, radius, viewpoint, min_neighbors=3):
        work = os.path.dirname(exe)
        paths = [os.path.join(work, name) for name in ("in.bin", "normals.bin", "curvature.bin", "counts.bin")]
        np.ascontiguousarray(pts, dtype=np.float64).tofile(paths[0])
        subprocess.check_call([exe, paths[0], repr(float(radius)), str(min_neighbors)] +
                              [repr(float(v)) for v in viewpoint] + paths[1:], timeout=120)
        return (np.fromfile(paths[1]).reshape(-1, 3), np.fromfile(paths[2]),
                np.fromfile(paths[3], dtype=np.int32))
    return run


@pytest.mark.parametrize("name", ["lattice", "noisy_plane", "sphere", "plane_at_1e6", "volume"])
def test_kernel_arithmetic_on_the_cpu_is_within_the_bound(solver, name):
    """One pass about the query point and the fixed-sweep Jacobi against two passes in long double and
    LAPACK: counts exact, unit length, sin of the angle within normal_bound and the curvature within
    curvature_bound on every row the GPU tests check; and the share of rows those tests may leave out
    (bound > 1e-6) stays under their 2 % cap on the restatement alone."""
    pts, radius, view = {
        "lattice": (nr.lattice_plane(257), 0.5, (0.0, 0.0, 10.0)),
        "noisy_plane": (nr.noisy_plane(), 0.5, (2.0, 2.0, 5.0)),
        "sphere": (nr.sphere(), 0.5, (0.0, 0.0, 0.0)),
        "plane_at_1e6": (nr.noisy_plane(offset=1.0e6), 0.5, (1.0e6 + 2.0, 1.0e6 + 2.0, 1.0e6 + 5.0)),
        "volume": (nr.uniform_volume(), 0.4, (0.0, 0.0, 0.0)),
    }[name]
    ref = nr.normals_reference(pts, radius, viewpoint=view)
    normals, curvature, counts = solver(pts, radius, view)
    assert np.array_equal(counts, ref["counts"])
    valid = counts >= 3
    assert np.array_equal(np.isnan(normals[:, 0]), ~valid) and np.array_equal(np.isnan(curvature), ~valid)
    assert np.abs(np.linalg.norm(normals[valid], axis=1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    bound = nr.normal_bound(counts, radius, ref["eigenvalues"], np.float64)
    checked = valid & (bound <= 1e-6)
    considered = valid & (counts >= 10) if name == "volume" else valid
    left_out = (considered & ~checked).sum() / max(considered.sum(), 1)
    assert left_out < 0.02 if name == "volume" else left_out == 0.0, left_out
    sin = nr.sin_angle(normals[checked], ref["normals"][checked])
    assert (sin <= bound[checked]).all(), (sin / bound[checked]).max()
    if name == "lattice":
        assert np.array_equal(normals[valid], np.tile([0.0, 0.0, 1.0], (valid.sum(), 1)))
        assert (curvature[valid] == 0.0).all()
    resolved = checked & (ref["eigenvalues"].sum(axis=1) > 0.0)
    cerr = np.abs(curvature[resolved] - ref["curvature"][resolved])
    assert (cerr <= nr.curvature_bound(counts, radius, ref["eigenvalues"], np.float64)[resolved]).all()
    to_view = view - pts
    clear = checked & (np.abs(np.einsum("ij,ij->i", ref["normals"], to_view)) >
                       1e-6 * np.linalg.norm(to_view, axis=1))
    assert (np.einsum("ij,ij->i", normals[clear], ref["normals"][clear]) > 0.0).all()
