"""numpy restatement of mopt_cloud_voxel_downsample (include/moptimizer_hip.h): the checker of
test_cloud_voxel_abi.py and test_gpu_cloud_voxel.py.  The reference project has no voxel filter to
compare against; this follows the header's formulas in fp64 and sums in np.longdouble."""
import numpy as np


def voxel_ids(xyz, leaf):
    """(kept mask, id of every kept point, dims): fp64 arithmetic on the widened input."""
    v = np.asarray(xyz).reshape(-1, 3).astype(np.float64)
    kept = np.isfinite(v).all(axis=1)
    v = v[kept]
    if len(v) == 0:
        return kept, np.zeros(0, dtype=np.int64), np.ones(3, dtype=np.int64)
    leaf = np.float64(leaf)
    lo, hi = v.min(axis=0), v.max(axis=0)
    origin = np.floor(lo / leaf) * leaf
    dims = np.floor((hi - origin) / leaf).astype(np.int64) + 1
    cell = np.clip(np.floor((v - origin) / leaf), 0, dims - 1).astype(np.int64)
    return kept, cell[:, 0] + dims[0] * (cell[:, 1] + dims[1] * cell[:, 2]), dims


def voxel_reference(xyz, leaf):
    """One row per occupied voxel in ascending id: (ids, centroids in xyz's dtype, counts int32,
    per-axis max |coordinate| of the voxel's points as fp64 — what the tests' error bound is made of)."""
    pts = np.asarray(xyz).reshape(-1, 3)
    dtype = pts.dtype
    kept, ids, _ = voxel_ids(pts, leaf)
    v = pts[kept].astype(np.float64)
    if len(v) == 0:
        return (np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=dtype), np.zeros(0, dtype=np.int32),
                np.zeros((0, 3)))
    order = np.argsort(ids, kind="stable")
    uniq, start, counts = np.unique(ids[order], return_index=True, return_counts=True)
    sums = np.add.reduceat(v[order].astype(np.longdouble), start, axis=0)
    centroids = (sums / counts[:, None].astype(np.longdouble)).astype(dtype)
    largest = np.maximum.reduceat(np.abs(v[order]), start, axis=0)
    return uniq, centroids, counts.astype(np.int32), largest


def centroid_bound(counts, largest, dtype):
    """(k + 1) * eps * max |coordinate in the voxel|, per voxel and axis: any order of k additions in
    fp64 or wider, the division, and the one rounding to the scalar type."""
    return (counts[:, None].astype(np.float64) + 1.0) * np.finfo(dtype).eps * largest
