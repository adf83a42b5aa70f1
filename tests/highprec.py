"""An extended-precision statement of the point2point linearization, and the metric the
scene-scale tests judge by.

The CPU oracle restates the reference's loops in the scalar type under test, so its sums carry
fp64 (or fp32) rounding of their own: at map coordinates that rounding is no longer far below the
1e-6 bar, and a kernel cannot be asked to be closer to the oracle than the oracle is to the truth.
Here the per-point residual and Jacobian and the three sums are taken in 80-bit long double, from
inputs rounded to the type under test, written from the model's definition and independently of
oracle/test_models.hpp.

The pose enters as the matrix the product and the oracle both build from x (they agree bit for bit,
tests/test_so3_bitwise.py): the same Rodrigues form evaluated in the type under test, then widened.
It is an input of the sums, not part of what is checked here.
"""
import numpy as np

LD = np.longdouble
# 64-bit significand or better; a host whose long double is a plain double must fail, not skip
assert np.finfo(LD).eps <= 1.1e-19, (
    "tests/highprec.py needs an 80-bit (or wider) long double, this host has eps = %g"
    % np.finfo(LD).eps)


def transform_from_x(x, dtype=np.float64):
    """(R, t) of x = (t, omega) in `dtype` arithmetic, by the oracle's form
    R = (I + sin(th) K) + (1 - cos(th)) (K K), K = skew(omega / th); identity below 10 eps."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    w = x[3:]
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    R = np.eye(3, dtype=dtype)
    if th > dt(10.0) * np.finfo(dtype).eps:
        a = w / th
        z = dt(0)
        K = np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], dtype=dtype)
        s, c1 = np.sin(th), dt(1) - np.cos(th)
        KK = np.zeros((3, 3), dtype=dtype)
        for k in range(3):
            KK = KK + np.outer(K[:, k], K[k, :])
        R = (np.eye(3, dtype=dtype) + s * K) + c1 * KK
    assert R.dtype == np.dtype(dtype)
    return R.astype(LD), x[:3].astype(LD)


def _neg_skew(v):
    """-skew(v) per point: rows (0, z, -y), (-z, 0, x), (y, -x, 0); v is (n, 3)."""
    n = v.shape[0]
    M = np.zeros((n, 3, 3), dtype=LD)
    M[:, 0, 1], M[:, 0, 2] = v[:, 2], -v[:, 1]
    M[:, 1, 0], M[:, 1, 2] = -v[:, 2], v[:, 0]
    M[:, 2, 0], M[:, 2, 1] = v[:, 1], -v[:, 0]
    return M


def _prepare(src, tgt, x, dtype):
    src = np.asarray(src).astype(dtype).astype(LD).reshape(-1, 3)
    tgt = np.asarray(tgt).astype(dtype).astype(LD).reshape(-1, 3)
    R, t = transform_from_x(x, dtype)
    warped = src @ R.T + t
    return src, R, warped, warped - tgt


def p2p_linearize_ld(src, tgt, x, jac_mode, cov=None, loss=None, dtype=np.float64):
    """(H, b, cost) in long double: H = sum w J^T S J, b = sum w J^T S r, cost = sum r.r with
    r = R p + t - q and w = rho^2 / (r.r + rho)^2 (`loss` = rho, None: w = 1).  jac_mode 0:
    J = [I | -skew(p)]; 1: that matrix written column-major into the buffer the sums read
    row-major; 3: [I | -skew(R p + t)]; 4: [I | -R skew(p)]."""
    src, R, warped, r = _prepare(src, tgt, x, dtype)
    n = src.shape[0]
    J = np.zeros((n, 3, 6), dtype=LD)
    J[:, :, :3] = np.eye(3, dtype=LD)
    if jac_mode in (0, 1):
        J[:, :, 3:] = _neg_skew(src)
        if jac_mode == 1:
            J = np.ascontiguousarray(J.transpose(0, 2, 1)).reshape(n, 3, 6)
    elif jac_mode == 3:
        J[:, :, 3:] = _neg_skew(warped)
    elif jac_mode == 4:
        J[:, :, 3:] = np.einsum("rm,nmc->nrc", R, _neg_skew(src))
    else:
        raise ValueError("analytic Jacobian modes only (0, 1, 3, 4), got %r" % (jac_mode,))
    rr = (r * r).sum(axis=1)
    if loss is None:
        w = np.ones(n, dtype=LD)
    else:
        rho = LD(np.dtype(dtype).type(loss))
        w = (rho * rho) / ((rr + rho) * (rr + rho))
    S = np.eye(3, dtype=LD) if cov is None else np.asarray(cov).astype(dtype).astype(LD)
    SJ = np.einsum("ab,nbj->naj", S, J)
    Sr = np.einsum("ab,nb->na", S, r)
    wJ = J * w[:, None, None]
    H = np.einsum("nai,naj->ij", wJ, SJ)
    b = np.einsum("nai,na->i", wJ, Sr)
    return H, b, rr.sum()


def p2p_cost_ld(src, tgt, x, dtype=np.float64):
    """sum r.r of the cost-only sweep, in long double."""
    _, _, _, r = _prepare(src, tgt, x, dtype)
    return (r * r).sum()


def lm_scaled_err(got, ref):
    """(eH, eb, ec) of got = (H, b, cost) against ref, in the coordinates Levenberg-Marquardt
    solves in: H + lambda diag(H) is invariant under x_i -> x_i / d_i with d = sqrt(diag H), where
    H has a unit diagonal and every entry at most 1.
      eH = max_ij |dH_ij| / (d_i d_j)
      eb = max_i (|db_i| / d_i) / max_i (|b_i| / d_i)
      ec = |dcost| / |cost|
    A row or column without a positive diagonal entry (jac_mode 1 scrambles the columns and can
    leave one empty) takes the norm-wise scale d_i = sqrt(max|H|); zeros of a scale count as 1."""
    H, b, s = got
    Hr, br, sr = (np.asarray(ref[0], dtype=LD), np.asarray(ref[1], dtype=LD), LD(ref[2]))
    diag = np.diag(Hr).copy()
    whole = np.abs(Hr).max() if Hr.size else LD(0)
    fallback = np.sqrt(whole) if whole > 0 else LD(1)
    d = np.where(diag > 0, np.sqrt(np.where(diag > 0, diag, LD(1))), fallback)
    dH = np.abs(np.asarray(H).astype(LD) - Hr)
    db = np.abs(np.asarray(b).astype(LD) - br)
    eH = (dH / np.outer(d, d)).max()
    b_scale = (np.abs(br) / d).max()
    eb = (db / d).max() / (b_scale if b_scale > 0 else LD(1))
    ec = abs(LD(s) - sr) / (abs(sr) if sr != 0 else LD(1))
    return float(eH), float(eb), float(ec)
