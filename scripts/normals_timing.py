#!/usr/bin/env python3
"""Wall time of mopt_cloud_estimate_normals with device input and device output (a host clock around the
blocking call), beside a host baseline: scipy.spatial.cKDTree neighbourhoods + numpy PCA where scipy is
importable, a numpy cell-grid search + numpy PCA otherwise (on a subsample, scaled to the whole cloud).

  python scripts/normals_timing.py --out profiles/normals_timing.json [--points 1000000] [--reps 5]

1 M points, a surface scan and a uniform volume, radii for about 10, 30 and 100 neighbours, fp64 and fp32.
Per configuration: two warm-up calls, then the median over --reps calls."""
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
BASELINE_SAMPLE = 20_000  # query points of the host baseline


def cloud(shape, n, seed=1):
    rng = np.random.default_rng(seed)
    if shape == "volume":
        return rng.random((n, 3)) * EXTENT
    xy = rng.random((n, 2)) * EXTENT  # a relief over the plane: a scanned surface
    z = np.sin(0.11 * xy[:, 0]) * np.cos(0.07 * xy[:, 1]) + 50.0
    return np.column_stack([xy, z])


def radius_for(shape, n, neighbours):
    if shape == "volume":
        return (neighbours * EXTENT ** 3 / n / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)
    return (neighbours * EXTENT ** 2 / n / np.pi) ** 0.5


def pca_normals(pts, neighbour_lists):
    out = np.full((len(neighbour_lists), 3), np.nan)
    for i, idx in enumerate(neighbour_lists):
        if len(idx) >= 3:
            q = pts[idx]
            out[i] = np.linalg.eigh(np.cov(q.T, bias=True))[1][:, 0]
    return out


def host_baseline(pts, radius):
    """(name, milliseconds for the whole cloud, mean neighbours): the search structure over all points, the
    queries and the PCA over BASELINE_SAMPLE of them, scaled."""
    n = len(pts)
    sample = np.random.default_rng(0).choice(n, min(n, BASELINE_SAMPLE), replace=False)
    t0 = time.perf_counter()
    try:
        from scipy.spatial import cKDTree
        name = "scipy.cKDTree + numpy"
        tree = cKDTree(pts)
        built = time.perf_counter()
        lists = tree.query_ball_point(pts[sample], radius)
    except ImportError:
        name = "numpy cell grid + numpy"
        cell = np.floor((pts - pts.min(axis=0)) / radius).astype(np.int64)
        dims = cell.max(axis=0) + 3
        key = (cell[:, 0] + 1) + dims[0] * ((cell[:, 1] + 1) + dims[1] * (cell[:, 2] + 1))
        order = np.argsort(key, kind="stable")
        sorted_key = key[order]
        offsets = np.array([dx + dims[0] * (dy + dims[1] * dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1)
                            for dx in (-1, 0, 1)])
        built = time.perf_counter()
        lists = []
        for i in sample:
            lo = np.searchsorted(sorted_key, key[i] + offsets, side="left")
            hi = np.searchsorted(sorted_key, key[i] + offsets, side="right")
            cand = np.concatenate([order[a:b] for a, b in zip(lo, hi)])
            d = pts[cand] - pts[i]
            lists.append(cand[(d * d).sum(axis=1) <= radius * radius])
    pca_normals(pts, lists)
    # the structure is built once for the whole cloud; the queries and the PCA go with the number of points
    ms = ((built - t0) + (time.perf_counter() - built) * (n / len(sample))) * 1e3
    return name, ms, float(np.mean([len(idx) for idx in lists]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    lib = mo.capi.load()
    n = args.points
    results = []
    for shape in ("surface", "volume"):
        base = cloud(shape, n)
        for wanted in (10, 30, 100):
            radius = radius_for(shape, n, wanted)
            baseline, baseline_ms, baseline_k = host_baseline(base, radius)
            for dtype in (np.float64, np.float32):
                d_pts = torch.from_numpy(np.ascontiguousarray(base.astype(dtype))).cuda()
                d_normals = torch.empty((n, 3), dtype=d_pts.dtype, device="cuda")
                d_curv = torch.empty((n,), dtype=d_pts.dtype, device="cuda")
                d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                walls = []
                for r in range(2 + args.reps):
                    t0 = time.perf_counter()
                    mo.capi.check(lib.mopt_cloud_estimate_normals(
                        0, d_pts.element_size(), ctypes.c_void_p(d_pts.data_ptr()), n, radius, 3, None, 3,
                        ctypes.c_void_p(d_normals.data_ptr()), ctypes.c_void_p(d_curv.data_ptr()),
                        ctypes.c_void_p(d_counts.data_ptr())))  # (blocks: the stream is synchronised inside)
                    if r >= 2:
                        walls.append((time.perf_counter() - t0) * 1e3)
                counts = d_counts.cpu().numpy()
                row = dict(points=n, shape=shape, dtype=np.dtype(dtype).name, radius=radius,
                           neighbours_wanted=wanted, neighbours_mean=float(counts.mean()),
                           neighbours_max=int(counts.max()), nan_rows=int((counts < 3).sum()),
                           wall_ms=float(np.median(walls)), wall_ms_min=float(min(walls)),
                           wall_ms_max=float(max(walls)), baseline=baseline, baseline_ms_scaled=baseline_ms,
                           baseline_sample=min(n, BASELINE_SAMPLE), baseline_neighbours_mean=baseline_k,
                           baseline_over_wall=baseline_ms / float(np.median(walls)))
                results.append(row)
                print(json.dumps(row), flush=True)
                del d_pts, d_normals, d_curv, d_counts
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=2, results=results), f,
                  indent=1)


if __name__ == "__main__":
    main()
