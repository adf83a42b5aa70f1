"""numpy restatement of mopt_cloud_estimate_normals (include/moptimizer_hip.h): the checker of
test_cloud_normals_abi.py and test_gpu_cloud_normals.py.  The reference project has no normal estimation
to compare against.  Three parts: brute-force neighbourhoods with d2 in the header's exact fp64
expression, the moments about the neighbourhood's mean in np.longdouble (two passes), np.linalg.eigh.

The brute force compares every finite point with every finite point of a slab: the points are sorted
along x, and a block of consecutive ones is tested against those whose x lies within radius * (1 + 1e-6)
of the block's extent — no pair that the expression accepts has |dx| > radius * (1 + 2^-52), so the slab
drops none."""
import numpy as np

PAIRS_PER_BLOCK = 3_000_000


def _blocks(x_sorted, radius):
    """(first row, last row + 1, first column, last column + 1) of blocks of rows of the x-sorted cloud."""
    n, reach = len(x_sorted), radius * (1.0 + 1e-6)
    start = 0
    while start < n:
        lo = np.searchsorted(x_sorted, x_sorted[start] - reach, side="left")
        rows = n
        while True:  # as many rows as keep the block near PAIRS_PER_BLOCK
            stop = min(n, start + rows)
            hi = np.searchsorted(x_sorted, x_sorted[stop - 1] + reach, side="right")
            if rows <= 64 or (stop - start) * (hi - lo) <= PAIRS_PER_BLOCK:
                break
            rows //= 2
        yield start, stop, lo, hi
        start = stop


def normals_reference(xyz, radius, min_neighbors=3, viewpoint=None):
    """dict(counts int32 [n], normals fp64 [n, 3], curvature fp64 [n], eigenvalues fp64 [n, 3] ascending) in
    the caller's order; NaN rows where k < max(min_neighbors, 3) or the point is not finite (count 0 there).
    Nothing is rounded to the input's scalar type: the tests' bounds carry that rounding."""
    pts = np.asarray(xyz).reshape(-1, 3).astype(np.float64)
    n = len(pts)
    view = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, dtype=np.float64).reshape(3)
    r2 = np.float64(radius) * np.float64(radius)
    counts = np.zeros(n, dtype=np.int32)
    normals = np.full((n, 3), np.nan)
    curvature = np.full(n, np.nan)
    eigenvalues = np.full((n, 3), np.nan)
    finite = np.flatnonzero(np.isfinite(pts).all(axis=1) & (np.abs(pts) <= 1e300).all(axis=1))
    order = finite[np.argsort(pts[finite, 0], kind="stable")]
    v = pts[order]
    wide = v.astype(np.longdouble)
    cov = np.zeros((len(v), 3, 3))
    k_sorted = np.zeros(len(v), dtype=np.int64)
    for r0, r1, c0, c1 in _blocks(v[:, 0], float(radius)):
        d = v[None, c0:c1, :] - v[r0:r1, None, :]  # d = q - p
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        rows, cols = np.nonzero(d2 <= r2)  # (sorted by row; every row holds itself)
        del d, d2
        first = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        k = np.diff(np.r_[first, len(rows)])
        q = wide[c0 + cols]
        mean = np.add.reduceat(q, first, axis=0) / k[:, None].astype(np.longdouble)
        dev = q - np.repeat(mean, k, axis=0)
        for a in range(3):
            for b in range(a, 3):
                c = np.add.reduceat(dev[:, a] * dev[:, b], first) / k.astype(np.longdouble)
                cov[r0:r1, a, b] = cov[r0:r1, b, a] = c.astype(np.float64)
        k_sorted[r0:r1] = k
    counts[order] = k_sorted
    enough = k_sorted >= max(int(min_neighbors), 3)
    lam, vec = np.linalg.eigh(cov[enough])
    nrm = vec[:, :, 0]
    towards = np.einsum("ij,ij->i", nrm, view - v[enough])
    nrm = np.where(towards[:, None] < 0.0, -nrm, nrm)
    trace = lam.sum(axis=1)
    rows = order[enough]
    normals[rows] = nrm
    eigenvalues[rows] = lam
    curvature[rows] = np.where(trace == 0.0, 0.0, lam[:, 0] / np.where(trace == 0.0, 1.0, trace))
    return dict(counts=counts, normals=normals, curvature=curvature, eigenvalues=eigenvalues)


def normal_bound(k, radius, eigenvalues, dtype):
    """sin of the angle between the library's normal and the restatement's, at most
        2 * 3 (k + 40) eps64 radius^2 / (l1 - l0) + 2 eps_S:
    Davis-Kahan (sin <= 2 ||E||_2 / gap, ||E||_2 <= 3 max |E_ij|) with every entry of C off by at most
    (k + 40) eps64 radius^2 — k additions of terms bounded by radius^2, the division, the subtraction and
    the solver's backward error — and the rounding of the three components to the scalar type S.  Derived,
    not measured.  inf where the gap is 0 or the row is NaN."""
    k = np.asarray(k, dtype=np.float64)
    lam = np.asarray(eigenvalues, dtype=np.float64).reshape(-1, 3)
    gap = lam[:, 1] - lam[:, 0]
    eps64 = np.finfo(np.float64).eps
    with np.errstate(divide="ignore", invalid="ignore"):
        first = 2.0 * 3.0 * (k + 40.0) * eps64 * float(radius) ** 2 / gap
    return np.where(gap > 0.0, first, np.inf) + 2.0 * np.finfo(dtype).eps


def curvature_bound(k, radius, eigenvalues, dtype):
    """|curvature - restatement's| <= 3 (k + 40) eps64 radius^2 / trace + 2 eps_S (the same entry error,
    Weyl's inequality for l0, over the trace)."""
    k = np.asarray(k, dtype=np.float64)
    trace = np.asarray(eigenvalues, dtype=np.float64).reshape(-1, 3).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        first = 3.0 * (k + 40.0) * np.finfo(np.float64).eps * float(radius) ** 2 / trace
    return np.where(trace > 0.0, first, np.inf) + 2.0 * np.finfo(dtype).eps


def lattice_plane(n, seed=3):
    """n points of the plane z = 0.75 on multiples of 0.25, a square patch filled row by row, shuffled: with
    radius 0.5 every offset (i, j) with i^2 + j^2 <= 4 is a neighbour, 13 for an interior point, and every
    sum is exact."""
    width = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    pts = np.column_stack([(i % width - 3) * 0.25, (i // width - 2) * 0.25, np.full(n, 0.75)])
    return pts[np.random.default_rng(seed).permutation(n)]


def noisy_plane(n=1500, offset=0.0, seed=5):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0.0, 4.0, (n, 2)), rng.normal(0.0, 0.01, n)]) + offset


def sphere(n=3000, seed=6):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return 2.0 * v / np.linalg.norm(v, axis=1, keepdims=True)


def dense_ball(n=3 * 2048 + 1, seed=7):
    """n points in the ball of radius 0.2 about (0.25, 0.25, 0.25): one cell, every point everyone's neighbour."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (0.2 * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return v + 0.25


def uniform_volume(n=20_000, seed=11):
    return np.random.default_rng(seed).uniform(-5.0, 5.0, (n, 3))


def flat_spread(n=4096, seed=12):
    """Pairs of points up to 0.3 apart per axis, spread over 1e4 x 1e4 and 0.1 thick: at radius 0.5 the
    lattice over the bounding box would have 4e8 cells, so the cell edge is doubled."""
    rng = np.random.default_rng(seed)
    base = np.column_stack([rng.uniform(0.0, 1.0e4, (n // 2, 2)), rng.uniform(0.0, 0.1, n // 2)])
    mate = base + np.column_stack([rng.uniform(-0.3, 0.3, (n // 2, 2)), np.zeros(n // 2)])
    return np.vstack([base, mate])[rng.permutation(n)]


def sin_angle(a, b):
    """sin of the angle between the rows of a and b (unit vectors, either sign), in fp64."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(np.cross(a, b), axis=1)
