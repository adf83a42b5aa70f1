"""Long-double references, seeded system generators and the runner for tests/cpp/device_units.hip:
the device functions of the LM step (csrc/lm_device.hpp) tested one call at a time.

Everything here is plain numpy in np.longdouble on inputs already rounded to the type under test,
so a reference carries none of that type's rounding.  tests/test_device_units_reference.py keeps
this module honest on the CPU and measures the two constants the GPU tests' bounds are built on.
"""
import functools
import os
import subprocess

import numpy as np

from tests import datasets as ds
from tests import highprec as hp

LD = hp.LD
EXE = os.path.join(ds.ROOT, "tests", "cpp", "_build", "device_units")
DTYPES = (np.float64, np.float32)
SPD_CONDS = {np.float64: (1.0, 1e3, 1e6, 1e9), np.float32: (1.0, 1e2, 1e4)}

# max |x - x_ld|_inf / (|x_ld|_inf eps cond_2(A)) of the unpivoted LDL^T restated in numpy in the type
# itself (unpivoted_ldlt below: separate multiplies and subtractions, true divisions) against the
# long-double solve, over the SPD family n in {2, 4, 6} x SPD_CONDS x 40 draws, lambda = 1e-4, seed 20240.
# Measured by test_device_units_reference.test_unpivoted_restatement_constant, which asserts that it
# stays <= 1.5 and that these figures cover it:
#   fp64  1.133 (n = 6, cond 1); 1.051 (n = 4, cond 1); 0.955 (n = 2, cond 1); <= 0.34 at cond >= 1e3
#   fp32  0.597 (n = 2, cond 1); 0.567 (n = 4, cond 1); 0.513 (n = 6, cond 1); <= 0.43 at cond >= 1e2
# (cond_2 overestimates what a random right-hand side feels of an ill-conditioned matrix.)
C_REF = {np.float64: 1.14, np.float32: 0.60}

# worst |w - w_ld|_inf / se3_unit of the host so3.hpp se3Plus / se3PlusRight (mo.capi.se3_plus,
# se3_plus_right) against se3_plus_ld over se3_grid.  Measured by
# test_device_units_reference.test_host_se3_updates_constant, which asserts these figures cover it:
#   fp64  left 18.49, right 18.69      fp32  left 33.41, right 29.07
# (the unit carries one power of 1 / sin theta; towards pi - 0.1 the theta / sin theta Log loses about
# two, which is where these worst cases sit).  The translation part of the same runs is within 1.4 eps
# (|x_t|_inf + |delta_t|_inf) on the left and 0.5 on the right, of the 4 allowed.
C_SE3_REF = {np.float64: 18.7, np.float32: 33.5}


def eps_of(dtype):
    return LD(np.finfo(dtype).eps)


def pivot_floor(dtype):
    """kPivotFloor of solveDampedPositive: S(1e-10) in fp64, 64 eps in fp32."""
    return LD(np.float64(1e-10)) if np.dtype(dtype) == np.float64 else LD(64) * eps_of(dtype)


def damped_ld(H, lam):
    """tril(H) mirrored + lam diag(H) in long double: the matrix both device solvers factor."""
    H = np.asarray(H).astype(LD)
    return np.tril(H) + np.tril(H, -1).T + LD(lam) * np.diag(np.diag(H))


def solve_ld(H, b, lam):
    """delta = (H + lam diag H)^-1 (-b) by Gaussian elimination with partial pivoting in long double
    (a zero row and column keeps delta_i = 0)."""
    return hp._solve_sym(damped_ld(H, lam), -np.asarray(b).astype(LD))


def cond2(H, lam):
    """cond_2 of the damped matrix over its live rows (the zero rows of a zero-row system left out)."""
    A = damped_ld(H, lam).astype(np.float64)
    live = [i for i in range(A.shape[0]) if A[i, i] != 0]
    return float(np.linalg.cond(A[np.ix_(live, live)])) if live else 1.0


def positive_predicate_ld(H, lam, dtype):
    """What solveDampedPositive decides, in long double: the unpivoted recurrence in the given order
    over the lower triangle, every d_k > floor (1 + lam) H_kk.  Returns (flag, ratios) with
    ratios[k] = d_k / (floor a_kk) (-inf where a_kk is not positive, NaN where NaN reaches d_k)."""
    H = np.asarray(H).astype(LD)
    n = H.shape[0]
    floor = pivot_floor(dtype)
    L = np.zeros((n, n), dtype=LD)
    d = np.zeros(n, dtype=LD)
    flag, ratios = True, []
    with np.errstate(all="ignore"):
        for k in range(n):
            akk = (LD(1) + LD(lam)) * H[k, k]
            u = [L[k, j] * d[j] for j in range(k)]
            dk = akk - sum((L[k, j] * u[j] for j in range(k)), LD(0))
            flag = flag and bool(dk > floor * akk)
            ratios.append(dk / (floor * akk) if akk > 0 or np.isnan(dk) else LD(-np.inf))
            d[k] = dk
            for i in range(k + 1, n):
                L[i, k] = (H[i, k] - sum((L[i, j] * u[j] for j in range(k)), LD(0))) / dk
    return flag, np.array(ratios, dtype=LD)


def unpivoted_ldlt(H, b, lam, dtype):
    """The unpivoted LDL^T solve of the damped system restated in `dtype` itself, operation by
    operation (no fused multiply-add, true divisions): what C_REF is measured on."""
    S = np.dtype(dtype).type
    H = np.asarray(H, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    n = H.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    d = np.zeros(n, dtype=dtype)
    for k in range(n):
        dk = H[k, k] + S(lam) * H[k, k]
        u = [L[k, j] * d[j] for j in range(k)]
        for j in range(k):
            dk = dk - L[k, j] * u[j]
        d[k] = dk
        for i in range(k + 1, n):
            v = H[i, k]
            for j in range(k):
                v = v - L[i, j] * u[j]
            L[i, k] = v / dk
    y = np.zeros(n, dtype=dtype)
    for i in range(n):
        v = -b[i]
        for j in range(i):
            v = v - L[i, j] * y[j]
        y[i] = v
    y = y / d
    for i in range(n - 1, -1, -1):
        v = y[i]
        for j in range(i + 1, n):
            v = v - L[j, i] * y[j]
        y[i] = v
    assert y.dtype == np.dtype(dtype)
    return y


def pivot_trace_ld(A):
    """The diagonal-pivoted LDL^T of the long-double matrix A: (exchanges, gap) — the (k, piv) pairs
    with piv != k, first largest |diagonal| winning as in solveDamped, and the smallest factor by
    which a chosen pivot exceeded the runner-up (inf where there was none)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    exchanges, gap = [], LD(np.inf)
    for k in range(n):
        diag = np.abs(np.diag(A)[k:])
        piv = k + int(np.argmax(diag))
        rest = np.delete(diag, piv - k)
        if rest.size and rest.max() > 0:
            gap = min(gap, diag[piv - k] / rest.max())
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            A[:, [k, piv]] = A[:, [piv, k]]
            exchanges.append((k, piv))
        if A[k, k] != 0:
            col = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(col, A[k, k + 1:])
    return exchanges, gap


# ---- system generators (every one returns H, b already rounded to dtype) -------------------------------
def _orthogonal(n, rng):
    return np.linalg.qr(rng.normal(size=(n, n)))[0].astype(LD)


def _round(H, b, dtype):
    H = ((H + H.T) / LD(2)).astype(dtype)
    return H, np.asarray(b).astype(dtype)


def spd_system(n, cond, dtype, rng):
    """H = Q diag(s) Q^T, symmetrised, s from 1 down to 1 / cond in equal ratios."""
    Q = _orthogonal(n, rng)
    s = LD(10) ** (-np.log10(LD(cond)) * np.arange(n, dtype=LD) / max(n - 1, 1))
    return _round((Q * s) @ Q.T, rng.normal(size=n), dtype)


def spd_system_clear_of_floor(n, cond, dtype, rng, lambdas):
    """spd_system whose every unpivoted pivot is, in long double, at least a factor 2 above the
    fallback floor at each lambda of `lambdas` (the well-posed case solveDampedPositive is for: at
    the largest condition numbers one draw in a few comes within reach of the floor and is redrawn)."""
    for _ in range(200):
        H, b = spd_system(n, cond, dtype, rng)
        if all(positive_predicate_ld(H, lam, dtype)[1].min() >= 2 for lam in lambdas):
            return H, b
    raise AssertionError("no SPD draw clear of the floor: n=%d cond=%g %s" % (n, cond, np.dtype(dtype)))


def exchanged_system(n, dtype, rng, lam=0.0):
    """An SPD system D C D whose pivot search must exchange at every step: C = Q diag(s) Q^T with
    s in [1, 1.25] (diagonal within a factor 1.25, Schur updates below 2 %), D^2 = 2^-rank with the
    ranks laid out as one n-cycle — selection by largest diagonal then exchanges at each of its
    n - 1 steps.  Asserted in long double on the rounded, damped matrix, with the chosen pivot at
    least 10 % ahead of the runner-up so that rounding cannot reorder it."""
    rank = list(range(n))
    for i in range(n - 1, 0, -1):  # Sattolo: a uniformly random n-cycle
        j = int(rng.integers(0, i))
        rank[i], rank[j] = rank[j], rank[i]
    Q = _orthogonal(n, rng)
    s = LD(1) + LD(0.25) * np.arange(n, dtype=LD) / max(n - 1, 1)
    D = LD(2) ** (-np.array(rank, dtype=LD) / 2)
    H, b = _round(((Q * s) @ Q.T) * np.outer(D, D), rng.normal(size=n), dtype)
    exchanges, gap = pivot_trace_ld(damped_ld(H, lam))
    assert len(exchanges) >= n - 1 and gap >= 1.1, (n, rank, exchanges, gap)
    assert n == 1 or [k for k, _ in exchanges] == list(range(n - 1)), exchanges
    return H, b


def indefinite_system(n, dtype, rng):
    """Symmetric indefinite and non-singular: D (Sigma + E) D with Sigma = diag(+-1) of both signs
    (n >= 2), |E_ij| <= 0.5 / n off the diagonal and D^2 over three decades.  Sigma + E is strictly
    diagonally dominant, and stays so under symmetric permutation and in every Schur complement:
    LDL^T with 1 x 1 diagonal pivots — which an indefinite matrix does not admit stably in general —
    has no element growth on this family, so the eps cond_2 bound applies to it."""
    sign = np.where(rng.permutation(n) % 2 == 0, -1.0, 1.0).astype(LD)
    E = rng.uniform(-0.5 / n, 0.5 / n, size=(n, n)).astype(LD)
    E = np.tril(E, -1) + np.tril(E, -1).T
    D = LD(10) ** (rng.uniform(-0.75, 0.75, size=n).astype(LD))
    H, b = _round((np.diag(sign) + E) * np.outer(D, D), rng.normal(size=n), dtype)
    assert n == 1 or (np.diag(H).min() < 0 < np.diag(H).max())
    return H, b


def zero_row_system(n, z, dtype, rng):
    """An SPD system (cond 100) with row and column z exactly zero; b_z is not."""
    H, b = spd_system(n, 100.0, dtype, rng)
    H[z, :] = 0
    H[:, z] = 0
    return H, b


def zero_system(n, dtype, rng):
    return np.zeros((n, n), dtype=dtype), rng.normal(size=n).astype(dtype)


def tie_system(n, dtype, rng, coupled):
    """Diagonal entries of one magnitude d, signs mixed (+d and -d); `coupled` adds the off-diagonal E
    of indefinite_system (every first pivot search is then an n-way tie: the first index must win),
    without it the matrix is diagonal and every search is a tie."""
    sign = np.where(rng.permutation(n) % 2 == 0, 1.0, -1.0).astype(LD)
    d = LD(0.75) * LD(2) ** int(rng.integers(-3, 4))
    E = np.zeros((n, n), dtype=LD)
    if coupled:
        E = rng.uniform(-0.5 / n, 0.5 / n, size=(n, n)).astype(LD)
        E = np.tril(E, -1) + np.tril(E, -1).T
    H, b = _round(d * (np.diag(sign) + E), rng.normal(size=n), dtype)
    assert np.all(np.abs(np.diag(H)) == np.abs(H[0, 0]))
    return H, b


def threshold_system(n, k, above, dtype, rng):
    """An SPD-shaped system L D L^T (lambda = 0) whose k-th unpivoted pivot sits a factor 4 above
    (`above`) or below the fallback floor, d_k = r f a_kk with r = 4 or 1 / 4, every other pivot being
    of the order of its diagonal entry.  Built in long double, rounded once; asserted in long double
    on the rounded matrix: pivot k still a factor 2 clear of the floor on its side, the others a
    factor 2 above it.  Returns (H, b, expected flag)."""
    assert 1 <= k < n
    f = pivot_floor(dtype)
    r = LD(4) if above else LD(1) / LD(4)
    L = np.tril((rng.choice([-1.0, 1.0], size=(n, n)) * rng.uniform(0.2, 0.5, size=(n, n))).astype(LD), -1)
    d = rng.uniform(0.5, 2.0, size=n).astype(LD)
    s = (L[k, :k] ** 2 * d[:k]).sum()
    d[k] = r * f * s / (LD(1) - r * f)
    L = L + np.eye(n, dtype=LD)
    H, b = _round((L * d) @ L.T, rng.normal(size=n), dtype)
    flag, ratios = positive_predicate_ld(H, 0.0, dtype)
    others = np.delete(ratios, k)
    assert others.min() >= 2, (n, k, above, ratios)
    assert (ratios[k] >= 2) if above else (ratios[k] <= 0.5), (n, k, above, ratios)
    assert flag == above
    return H, b, above


# ---- SE(3) -------------------------------------------------------------------------------------------
def exp_ld(w, dtype):
    """so3.hpp expSO3 in long double; identity at |w| <= 10 eps of `dtype`.  Returns (R, theta)."""
    w = np.asarray(w).astype(LD)
    th = np.sqrt((w * w).sum())
    if not th > LD(10) * eps_of(dtype):
        return np.eye(3, dtype=LD), th
    ax, ay, az = w / th
    s, c1 = np.sin(th), LD(1) - np.cos(th)
    xx, yy, zz = ax * ax, ay * ay, az * az
    R = np.array([[1 + c1 * (-(yy + zz)), s * (-az) + c1 * (ax * ay), s * ay + c1 * (ax * az)],
                  [s * az + c1 * (ax * ay), 1 + c1 * (-(xx + zz)), s * (-ax) + c1 * (ay * az)],
                  [s * (-ay) + c1 * (ax * az), s * ax + c1 * (ay * az), 1 + c1 * (-(xx + yy))]], dtype=LD)
    return R, th


def se3_plus_ld(x, delta, dtype, right=False, check_margins=True):
    """so3.hpp se3Plus (se3PlusRight) in long double on inputs rounded to dtype, branch rules
    included: Exp is the identity at |w| <= 10 eps; Log takes theta = 0 for trace > S(3) - S(1e-6) and
    w = K / 2 for |theta| < S(1e-3).  Returns (out, info): info["theta"] is the composite angle,
    info["acos"] whether Log took the acos branch.  With check_margins every branch point is asserted
    a factor 2 away (|w| against 10 eps, 3 - trace against 1e-6, theta against 1e-3), so that an
    evaluation in dtype takes the same branches, and theta <= pi - 0.1."""
    S = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype).astype(LD)
    delta = np.asarray(delta, dtype=dtype).astype(LD)
    R, thx = exp_ld(x[3:], dtype)
    D, thd = exp_ld(delta[3:], dtype)
    out = np.zeros(6, dtype=LD)
    if right:
        RR = R @ D
        out[:3] = x[:3] + delta[:3]
    else:
        RR = D @ R
        out[:3] = D @ x[:3] + delta[:3]
    trace = RR[0, 0] + RR[1, 1] + RR[2, 2]
    K = np.array([RR[2, 1] - RR[1, 2], RR[0, 2] - RR[2, 0], RR[1, 0] - RR[0, 1]], dtype=LD)
    composite = np.arctan2(np.sqrt((K * K).sum()) / 2, (trace - 1) / 2)
    theta = LD(0) if trace > LD(S(3.0) - S(1e-6)) else np.arccos(LD(0.5) * (trace - LD(1)))
    small = abs(theta) < LD(S(0.001))
    k = LD(0.5) if small else LD(0.5) * theta / np.sin(theta)
    out[3:] = k * K
    info = dict(theta=composite, acos=not small, theta_x=thx, theta_d=thd, trace=trace)
    if check_margins:
        assert se3_case_is_clear(info, dtype), info
    return out, info


def se3_case_is_clear(info, dtype):
    e10 = LD(10) * eps_of(dtype)
    for th in (info["theta_x"], info["theta_d"]):
        if not (th <= e10 / 2 or th >= e10 * 2):
            return False
    gap = LD(3) - info["trace"]
    if not (gap <= LD(0.5e-6) or gap >= LD(2e-6)):
        return False
    th = info["theta"]
    if not (th <= LD(0.5e-3) or th >= LD(2e-3)) or th > LD(np.pi) - LD(0.1):
        return False
    return info["acos"] == bool(th >= LD(2e-3))


def se3_unit(info, dtype):
    """The unit the rotation part's error is counted in: eps (1 + 1 / |sin theta|), theta the composite
    angle — 1 / sin theta is the conditioning of the theta / sin theta Log.  Where Log does not take
    that branch (theta < 1e-3: w = K / 2, no acos, no division) the unit is the factor's least value,
    2 eps, not the 1 / theta the formula would allow there."""
    if not info["acos"]:
        return LD(2) * eps_of(dtype)
    return eps_of(dtype) * (LD(1) + LD(1) / abs(np.sin(info["theta"])))


X_DECADES = (1e-9, 1e-6, 1e-4, 1e-2, 0.1, 0.7, 3.0)          # as tests/test_so3_bitwise._grid
DELTA_DECADES = (1e-12, 1e-9, 1e-6, 1e-3, 1e-2, 0.1, 1.0)


def x_grid(dtype, per_decade=12, seed=7):
    """Poses at the |x_j| decades of test_so3_bitwise._grid, pure-axis rotations, and rotation vectors
    on both sides of the 10 eps switch — none within a factor 2 of it."""
    rng = np.random.default_rng(seed)
    e10 = 10 * float(np.finfo(dtype).eps)
    xs = [ds.X_ZERO, ds.X_GENERIC]
    for scale in X_DECADES:
        xs += list(rng.normal(0.0, scale, size=(per_decade, 6)))
    for a in (0.4 * e10, 2.5 * e10, 1e-8, 0.3, 1.5, 3.0):
        for k in range(3):
            x = np.zeros(6)
            x[3 + k] = a
            xs.append(x)
    for a in (0.4 * e10, 2.5 * e10):  # generic directions at the switch, with a translation
        u = rng.normal(size=3)
        xs.append(np.concatenate([rng.normal(0, 1, 3), a * u / np.linalg.norm(u)]))
    keep = []
    for x in xs:
        x = np.asarray(x, dtype=dtype)
        th = float(np.linalg.norm(x[3:].astype(np.float64)))
        if th <= e10 / 2 or th >= e10 * 2:
            keep.append(x)
    return keep


@functools.lru_cache(maxsize=None)
def se3_grid(dtype, right=False, seed=11):
    """(x, delta, reference, info) for se3Plus / se3PlusRight: x_grid x delta at decades 1e-12 .. 1, pure-axis
    pairs, both sides of the 10 eps switch in x and in delta, composite angles on both sides of 1e-3
    (small rotations adding up; large ones cancelling) and up to pi - 0.1.  Pairs within a factor 2 of
    a branch point, or composing to more than pi - 0.1, are left out (se3_case_is_clear); reference and
    info are se3_plus_ld's, computed once and shared (leave them unchanged)."""
    rng = np.random.default_rng(seed)
    e10 = 10 * float(np.finfo(dtype).eps)
    pairs = []
    for x in x_grid(dtype, per_decade=6):
        for scale in DELTA_DECADES:
            pairs.append((x, rng.normal(0.0, scale, size=6)))
    for a in (1e-8, 0.3, 1.5, 3.0):
        for b in (0.4 * e10, 2.5 * e10, 1e-10, 1e-4, 0.2):
            for k in range(3):
                for m in range(3):
                    x, d = np.zeros(6), np.zeros(6)
                    x[3 + k], d[3 + m] = a, b
                    pairs.append((x, d))
    for _ in range(24):  # one axis: the composite angle is the sum of the two
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        t, dt = rng.normal(0, 1, 3), rng.normal(0, 0.1, 3)
        for a, b in ((3e-4, 1e-4), (2e-4, -1e-4), (1.5e-3, 1e-3), (3e-3, -5e-4), (0.5, -0.5 + 3e-4),
                     (0.5, -0.5 - 2.5e-3), (-1.2, 1.2 + 4e-4), (2.0, np.pi - 0.12 - 2.0), (1.0, 1.9),
                     (0.0, 3e-4), (4e-4, 0.0), (0.0, 2.5e-3)):
            pairs.append((np.concatenate([t, a * u]), np.concatenate([dt, b * u])))
    for a in (0.0, 0.4 * e10):  # both rotations below the switch: the identity composed with itself
        for k in range(3):
            x, d = rng.normal(0, 1, 6), rng.normal(0, 0.1, 6)
            x[3:], d[3:] = 0.0, 0.0
            x[3 + k], d[3 + (k + 1) % 3] = a, 0.4 * e10
            pairs.append((x, d))
    keep = []
    for x, d in pairs:
        x, d = np.asarray(x, dtype=dtype), np.asarray(d, dtype=dtype)
        ref, info = se3_plus_ld(x, d, dtype, right=right, check_margins=False)
        if se3_case_is_clear(info, dtype):
            keep.append((x, d, ref, info))
    return keep


# ---- the program ---------------------------------------------------------------------------------------
def pack_systems(systems, dtype, sentinel):
    """[(H, b, lam), ...] of one n -> the `positive` / `pivoted*` input records."""
    rec = [np.concatenate([np.asarray(H, dtype=dtype).ravel(order="F"), np.asarray(b, dtype=dtype),
                           np.array([lam, sentinel], dtype=dtype)]) for H, b, lam in systems]
    return np.stack(rec)


def run(op, dtype, n, records, tmp_dir, out_width):
    """One fresh child process of tests/cpp/device_units: `records` (count, width) in, (count, out_width)
    out, both in dtype."""
    assert os.path.exists(EXE), "build it with `make cpptests`"
    records = np.ascontiguousarray(records, dtype=np.dtype(dtype).newbyteorder("<"))
    count = records.shape[0]
    tag = "%s_%d_%d" % (op, np.dtype(dtype).itemsize, n)
    path_in, path_out = os.path.join(tmp_dir, tag + ".in"), os.path.join(tmp_dir, tag + ".out")
    records.tofile(path_in)
    done = subprocess.run([EXE, op, str(np.dtype(dtype).itemsize), str(n), str(count), path_in, path_out],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (op, done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    out = np.fromfile(path_out, dtype=np.dtype(dtype).newbyteorder("<")).astype(dtype)
    assert out.size == count * out_width, (op, out.size, count, out_width)
    return out.reshape(count, out_width)
