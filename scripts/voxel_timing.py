#!/usr/bin/env python3
"""Device time of mopt_cloud_voxel_downsample per stage (events on the call's stream:
mopt_cloud_voxel_profile), beside two yardsticks: the same thinning in numpy on the host (np.unique +
np.add.reduceat) and the call's own sort stage (one sortByCell at that size).

  python scripts/voxel_timing.py --out profiles/voxel_timing.json [--sizes 1000000,10000000] [--reps 5]

1 M and 10 M points, fp64 and fp32, a surface scan and a uniform volume, leaves for about 1, 10 and 1000
points per voxel and one voxel, host input and device input (device input also writes device output).
Per configuration: two warm-up calls, then the median over --reps calls of every stage."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import moptimizer_0_amd as mo  # noqa: E402

EXTENT = 100.0


def cloud(shape, n, seed=1):
    rng = np.random.default_rng(seed)
    if shape == "volume":
        return rng.random((n, 3)) * EXTENT
    xy = rng.random((n, 2)) * EXTENT  # a relief over the plane: a scanned surface
    # (a flat relief: at 10 M points and one point per voxel the lattice over the bounding box must stay
    # below 2^31 cells — 100 x 100 x 10 at leaf 0.032 is 3.2e9 and is refused)
    z = np.sin(0.11 * xy[:, 0]) * np.cos(0.07 * xy[:, 1]) + 50.0
    return np.column_stack([xy, z])


def leaf_for(shape, n, per_voxel):
    if per_voxel is None:
        return 10.0 * EXTENT  # one voxel
    return EXTENT * (per_voxel / n) ** (1.0 / 3.0 if shape == "volume" else 0.5)


def numpy_thinning(pts, leaf):
    t0 = time.perf_counter()
    v = pts.astype(np.float64, copy=False)
    origin = np.floor(v.min(axis=0) / leaf) * leaf
    dims = np.floor((v.max(axis=0) - origin) / leaf).astype(np.int64) + 1
    cell = np.floor((v - origin) / leaf).astype(np.int64)
    ids = cell[:, 0] + dims[0] * (cell[:, 1] + dims[1] * cell[:, 2])
    order = np.argsort(ids, kind="stable")
    _, start, counts = np.unique(ids[order], return_index=True, return_counts=True)
    out = np.add.reduceat(v[order], start, axis=0) / counts[:, None]
    return (time.perf_counter() - t0) * 1e3, len(out)


def device_stages(lib, size, src_ptr, n, leaf, flags, out_ptr, counts_ptr, capacity, reps):
    n_out = ctypes.c_int64(0)
    stage = (ctypes.c_double * len(mo.capi.CLOUD_VOXEL_STAGES))()
    rows, walls = [], []
    mo.capi.check(lib.mopt_cloud_voxel_profile(1, None))
    for r in range(2 + reps):
        t0 = time.perf_counter()
        mo.capi.check(lib.mopt_cloud_voxel_downsample(0, size, src_ptr, n, leaf, flags, out_ptr, counts_ptr,
                                                      capacity, ctypes.byref(n_out)))
        wall = (time.perf_counter() - t0) * 1e3
        mo.capi.check(lib.mopt_cloud_voxel_profile(1, stage))
        if r >= 2:
            rows.append(list(stage))
            walls.append(wall)
    mo.capi.check(lib.mopt_cloud_voxel_profile(0, None))
    return np.median(np.array(rows), axis=0), float(np.median(walls)), n_out.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    lib = mo.capi.load()
    results = []
    for n in [int(s) for s in args.sizes.split(",")]:
        for shape in ("surface", "volume"):
            base = cloud(shape, n)
            for per_voxel in (1, 10, 1000, None):
                leaf = leaf_for(shape, n, per_voxel)
                numpy_ms, numpy_voxels = numpy_thinning(base, leaf)
                for dtype in (np.float64, np.float32):
                    pts = np.ascontiguousarray(base.astype(dtype))
                    sized = ctypes.c_int64(0)  # (rounding to fp32 moves a few points across faces)
                    mo.capi.check(lib.mopt_cloud_voxel_downsample(0, pts.itemsize, ctypes.c_void_p(pts.ctypes.data),
                                                                  n, leaf, 0, None, None, 0, ctypes.byref(sized)))
                    voxels = sized.value
                    out = np.zeros((voxels, 3), dtype=dtype)
                    counts = np.zeros(voxels, dtype=np.int32)
                    d_pts = torch.from_numpy(pts).cuda()
                    d_out = torch.empty((voxels, 3), dtype=d_pts.dtype, device="cuda")
                    d_counts = torch.empty((voxels,), dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    for path, call in (
                            ("host", (ctypes.c_void_p(pts.ctypes.data), 0, ctypes.c_void_p(out.ctypes.data),
                                      ctypes.c_void_p(counts.ctypes.data))),
                            ("device", (ctypes.c_void_p(d_pts.data_ptr()), 3, ctypes.c_void_p(d_out.data_ptr()),
                                        ctypes.c_void_p(d_counts.data_ptr())))):
                        stages, wall, got = device_stages(lib, pts.itemsize, call[0], n, leaf, call[1], call[2],
                                                          call[3], voxels, args.reps)
                        total = float(stages.sum())
                        after_sort = float(stages[3] + stages[4])
                        row = dict(points=n, shape=shape, dtype=np.dtype(dtype).name, path=path, leaf=leaf,
                                   per_voxel_wanted=per_voxel or n, voxels=got, voxels_numpy_fp64=numpy_voxels,
                                   stage_ms=dict(zip(mo.capi.CLOUD_VOXEL_STAGES, [float(s) for s in stages])),
                                   device_ms=total, wall_ms=wall, numpy_ms=numpy_ms,
                                   numpy_over_device=numpy_ms / total, numpy_over_wall=numpy_ms / wall,
                                   reduction_over_sort=after_sort / float(stages[2]))
                        results.append(row)
                        print(json.dumps(row), flush=True)
                    del d_pts, d_out, d_counts
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=2, results=results), f,
                  indent=1)


if __name__ == "__main__":
    main()
