"""mopt_cloud_voxel_downsample at the C ABI without a device: every up-front refusal comes back as
MOPT_ERR_INVALID_ARGUMENT with a message that names the argument, the header stays plain C with the new
enum, the C++ wrapper (include/moptimizer_amd/cloud_filter.hpp) compiles warning-free, and the numpy
restatement the GPU tests check against (tests/voxel_reference.py) gives a hand-worked case."""
import ctypes
import os
import subprocess

import numpy as np

from tests import datasets as ds
from tests import voxel_reference as vr

INVALID = 1
INC = os.path.join(ds.ROOT, "include")


def _call(lib, xyz, count, leaf=0.5, scalar_bytes=8, flags=0, with_out_count=True):
    n_out = ctypes.c_int64(-7)
    rc = lib.mopt_cloud_voxel_downsample(
        0, scalar_bytes, None if xyz is None else xyz.ctypes.data_as(ctypes.c_void_p), count, leaf, flags,
        None, None, 0, ctypes.byref(n_out) if with_out_count else None)
    return rc, lib.mopt_last_error().decode(), n_out.value


def test_invalid_arguments_are_refused_before_a_device_is_looked_for():
    import moptimizer_0_amd as mo
    lib = mo.capi.load()
    pts = np.zeros((4, 3))
    cases = {
        "out_count": dict(xyz=pts, count=4, with_out_count=False),
        "scalar_bytes": dict(xyz=pts, count=4, scalar_bytes=2),
        "scalar_bytes ": dict(xyz=pts, count=4, scalar_bytes=16),
        "flags": dict(xyz=pts, count=4, flags=4),
        "flags ": dict(xyz=pts, count=4, flags=1 | 8),
        "count": dict(xyz=pts, count=-1),
        "leaf": dict(xyz=pts, count=4, leaf=0.0),
        "leaf ": dict(xyz=pts, count=4, leaf=-1.0),
        "leaf  ": dict(xyz=pts, count=4, leaf=float("nan")),
        "leaf   ": dict(xyz=pts, count=4, leaf=float("inf")),
        "xyz": dict(xyz=None, count=4),
    }
    for what, kw in cases.items():
        rc, message, _ = _call(lib, **kw)
        assert rc == INVALID and what.strip() in message, (what, rc, message)
    # an empty cloud is no error and needs no device either
    rc, _, n_out = _call(lib, None, 0)
    assert rc == 0 and n_out == 0


def test_python_wrapper_is_exported():
    import moptimizer_0_amd as mo
    assert mo.voxel_downsample is mo.capi.voxel_downsample
    out, counts = mo.voxel_downsample(np.zeros((0, 3)), 0.5, return_counts=True)
    assert out.shape == (0, 3) and counts.shape == (0,)


def test_header_with_the_cloud_entry_is_plain_c(tmp_path):
    src = tmp_path / "use_cloud.c"
    src.write_text('#include "moptimizer_hip.h"\n'
                   "int main(void) {\n"
                   "  double xyz[3] = {0, 0, 0}, out[3];\n"
                   "  int32_t counts[1];\n"
                   "  int64_t n = 0;\n"
                   "  unsigned flags = MOPT_CLOUD_INPUT_DEVICE | MOPT_CLOUD_OUTPUT_DEVICE;\n"
                   "  (void)flags;\n"
                   "  return mopt_cloud_voxel_downsample(0, 8, xyz, 1, 0.5, 0u, out, counts, 1, &n);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC,
                           "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, "-x", "c++",
                           "-fsyntax-only", str(src)])


def test_cpp_wrapper_header_compiles_without_warnings(tmp_path):
    src = tmp_path / "use_filter.cpp"
    src.write_text('#include "moptimizer_amd/cloud_filter.hpp"\n'
                   "int main() {\n"
                   "  std::vector<double> d(6, 0.0);\n"
                   "  std::vector<float> f(6, 0.f);\n"
                   "  std::vector<int32_t> counts;\n"
                   "  const auto a = moptimizer::io::voxelDownsample(d, 0.5);\n"
                   "  const auto b = moptimizer::io::voxelDownsample<float>(f, 0.5, 0, &counts);\n"
                   "  return int(a.size() + b.size() + counts.size());\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, "-fsyntax-only",
                           str(src)])


def test_restatement_on_a_hand_worked_case():
    """5 points, leaf 0.5.  lo = (-0.6, 0.1, 0), hi = (0.3, 0.4, 0.2): origin = (-1, 0, 0), dims = (3, 1, 1).
    Cells along x: -0.6 -> 0, -0.55 -> 0, 0.1 -> 2, 0.3 -> 2, 0.25 -> 2: voxels 0 (2 points) and 2 (3)."""
    pts = np.array([[0.1, 0.1, 0.0], [-0.6, 0.2, 0.1], [0.3, 0.4, 0.2], [-0.55, 0.3, 0.0], [0.25, 0.1, 0.1]])
    kept, ids, dims = vr.voxel_ids(pts, 0.5)
    assert kept.all() and list(dims) == [3, 1, 1] and list(ids) == [2, 0, 2, 0, 2]
    uniq, cent, counts, largest = vr.voxel_reference(pts, 0.5)
    assert list(uniq) == [0, 2] and list(counts) == [2, 3] and counts.dtype == np.int32
    want = np.array([[(-0.6 - 0.55) / 2, 0.25, 0.05], [(0.1 + 0.3 + 0.25) / 3, 0.2, 0.1]])
    assert np.abs(cent - want).max() < 1e-15
    assert np.array_equal(largest, [[0.6, 0.3, 0.1], [0.3, 0.4, 0.2]])
    # a non-finite row is in no voxel and shapes no box; fp32 input is widened, the result is fp32
    with_nan = np.vstack([pts, [[np.nan, 100.0, 100.0]], [[0.0, np.inf, 0.0]]]).astype(np.float32)
    uniq32, cent32, counts32, _ = vr.voxel_reference(with_nan, 0.5)
    assert list(uniq32) == [0, 2] and list(counts32) == [2, 3] and cent32.dtype == np.float32
    bound = vr.centroid_bound(counts, largest, np.float32)
    assert (np.abs(cent32.astype(np.float64) - want) <= bound).all()
