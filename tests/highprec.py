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
    M = np.zeros((n, 3, 3), dtype=v.dtype)
    M[:, 0, 1], M[:, 0, 2] = v[:, 2], -v[:, 1]
    M[:, 1, 0], M[:, 1, 2] = -v[:, 2], v[:, 0]
    M[:, 2, 0], M[:, 2, 1] = v[:, 1], -v[:, 0]
    return M


def _prepare(src, tgt, x, dtype, work=LD):
    src = np.asarray(src).astype(dtype).astype(work).reshape(-1, 3)
    tgt = np.asarray(tgt).astype(dtype).astype(work).reshape(-1, 3)
    R, t = transform_from_x(x, dtype)
    R, t = R.astype(work), t.astype(work)
    warped = src @ R.T + t
    return src, R, warped, warped - tgt


def p2p_linearize_ld(src, tgt, x, jac_mode, cov=None, loss=None, dtype=np.float64, work=LD):
    """(H, b, cost) in long double: H = sum w J^T S J, b = sum w J^T S r, cost = sum r.r with
    r = R p + t - q and w = rho^2 / (r.r + rho)^2 (`loss` = rho, None: w = 1).  jac_mode 2: forward
    differences of r with the reference's steps; 0:
    J = [I | -skew(p)]; 1: that matrix written column-major into the buffer the sums read
    row-major; 3: [I | -skew(R p + t)]; 4: [I | -R skew(p)].  `work`: the type the sums are taken in
    (long double; np.float64 only to measure what that rounding does to a loop, lm_minimize_ld)."""
    W = work
    src, R, warped, r = _prepare(src, tgt, x, dtype, work)
    n = src.shape[0]
    J = np.zeros((n, 3, 6), dtype=W)
    J[:, :, :3] = np.eye(3, dtype=W)
    if jac_mode in (0, 1):
        J[:, :, 3:] = _neg_skew(src)
        if jac_mode == 1:
            J = np.ascontiguousarray(J.transpose(0, 2, 1)).reshape(n, 3, 6)
    elif jac_mode == 3:
        J[:, :, 3:] = _neg_skew(warped)
    elif jac_mode == 4:
        J[:, :, 3:] = np.einsum("rm,nmc->nrc", R, _neg_skew(src))
    elif jac_mode == 2:
        # forward differences (linearization.h:78-105): h_j = sqrt(eps) |x_j|, sqrt(eps) at x_j = 0, the
        # perturbed x and its pose formed in `dtype` as the product forms them, the quotient in `work`
        xs = np.asarray(x, dtype=dtype)
        root = np.sqrt(np.finfo(dtype).eps).astype(dtype)
        for j in range(6):
            h = root * abs(xs[j]) if xs[j] != 0 else root
            xp = xs.copy()
            xp[j] = xs[j] + h
            J[:, :, j] = (_prepare(src, tgt, xp, dtype, work)[3] - r) / W(h)
    else:
        raise ValueError("Jacobian modes 0 - 4, got %r" % (jac_mode,))
    rr = (r * r).sum(axis=1)
    if loss is None:
        w = np.ones(n, dtype=W)
    else:
        rho = W(np.dtype(dtype).type(loss))
        w = (rho * rho) / ((rr + rho) * (rr + rho))
    S = np.eye(3, dtype=W) if cov is None else np.asarray(cov).astype(dtype).astype(W)
    SJ = np.einsum("ab,nbj->naj", S, J)
    Sr = np.einsum("ab,nb->na", S, r)
    wJ = J * w[:, None, None]
    H = np.einsum("nai,naj->ij", wJ, SJ)
    b = np.einsum("nai,na->i", wJ, Sr)
    return H, b, rr.sum()


def p2p_cost_ld(src, tgt, x, dtype=np.float64, work=LD):
    """sum r.r of the cost-only sweep, in long double."""
    _, _, _, r = _prepare(src, tgt, x, dtype, work)
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


# ---- the Levenberg-Marquardt loop over those sums, with a trace ----------------------------------------
CONVERGED, MAX_ITERATIONS, SMALL_DELTA, NUMERIC_ERROR = 0, 1, 2, 3


def _solve_sym(A, rhs):
    """A z = rhs by Gaussian elimination with partial pivoting in A's own type (numpy's solvers stop at
    double).  A row and column that are exactly zero — a parameter no residual depends on — keep z_i = 0,
    as the pivoted LDL^T of the loop leaves it."""
    n = A.shape[0]
    live = [i for i in range(n) if A[i, i] != 0]
    z = np.zeros(n, dtype=A.dtype)
    if not live:
        return z
    M = A[np.ix_(live, live)].copy()
    v = rhs[live].astype(A.dtype).copy()
    m = len(live)
    for c in range(m):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
            v[[c, p]] = v[[p, c]]
        for r in range(c + 1, m):
            f = M[r, c] / M[c, c]
            M[r, c:] = M[r, c:] - f * M[c, c:]
            v[r] = v[r] - f * v[c]
    out = np.zeros(m, dtype=A.dtype)
    for r in range(m - 1, -1, -1):
        out[r] = (v[r] - (M[r, r + 1:] * out[r + 1:]).sum(dtype=A.dtype)) / M[r, r]
    z[live] = out
    return z


def lm_minimize_ld(src, tgt, x0, jac_mode, max_iter=15, lm_iter=3, cov=None, loss=None, manifold=0,
                   dtype=np.float64, work=LD):
    """LevenbergMarquadtDynamic::minimize (levenberg_marquadt_dyn.cpp:34-119) over p2p_linearize_ld /
    p2p_cost_ld, every scalar of the loop in `work` (long double); x itself is held in `dtype`, the type
    the product holds it in, and the stopping tests use that type's epsilon.  The step is that of tril(H)
    mirrored + lambda diag(H) (the reference's LDLT reads the lower triangle).  Euclidean update only.

    Returns (x, status, iterations, trace, states):
      trace   one dict per trial: it (outer iteration, from 0), k (inner, from 0), lam and nu the trial was
              taken with, y0, yi, rho, max_delta, outcome — "accepted", "rejected" (another trial of the same
              outer iteration follows), "exhausted" (rejected, and the inner loop's last) or "stopped"
              (rho < 0 with a small delta: the loop returns)
      states  states[j] = dict(x, lam, trials, exhausted) after j completed outer iterations (states[0] is the
              start: lam = -1); a run limited to k <= len(states) - 1 iterations returns states[k]["x"],
              MAX_ITERATIONS, k (truncate())."""
    if manifold:
        raise NotImplementedError("lm_minimize_ld takes the Euclidean update only")
    W = work
    dt = np.dtype(dtype).type
    eps = W(np.finfo(dtype).eps)
    small_cost, small_delta = W(8) * eps, np.sqrt(eps)
    x = np.asarray(x0, dtype=dtype).copy()
    lam = W(-1)
    trace, states = [], [dict(x=x.copy(), lam=lam, trials=0, exhausted=False)]

    def done(status, it):
        return x, status, it, trace, states

    for it in range(max_iter):
        H, b, y0 = p2p_linearize_ld(src, tgt, x, jac_mode, cov=cov, loss=loss, dtype=dtype, work=W)
        if abs(y0) < small_cost:
            return done(CONVERGED, it)
        if lam < 0:
            lam = W(dt(1e-9)) * np.abs(np.diag(H)).max()
        nu = W(2)
        Hl = np.tril(H) + np.tril(H, -1).T
        accepted = False
        for k in range(lm_iter):
            A = Hl + lam * np.diag(np.diag(H))
            delta = _solve_sym(A, -b)
            xi = (x.astype(W) + delta).astype(dtype)
            yi = p2p_cost_ld(src, tgt, xi, dtype=dtype, work=W)
            if np.isnan(yi):
                return done(NUMERIC_ERROR, it)
            rho = (y0 - yi) / (delta * (lam * delta - b)).sum(dtype=W)
            rec = dict(it=it, k=k, lam=lam, nu=nu, y0=y0, yi=yi, rho=rho, max_delta=np.abs(delta).max())
            trace.append(rec)
            if rho < 0:
                if rec["max_delta"] < small_delta:
                    rec["outcome"] = "stopped"
                    return done(CONVERGED if abs(yi) < small_cost else SMALL_DELTA, it)
                rec["outcome"] = "exhausted" if k == lm_iter - 1 else "rejected"
                lam = nu * lam
                nu = W(2) * nu
                continue
            rec["outcome"] = "accepted"
            x = xi
            lam = lam * max(W(1) / W(3), W(1) - (W(2) * rho - W(1)) ** 3)
            accepted = True
            break
        states.append(dict(x=x.copy(), lam=lam, trials=len(trace), exhausted=lm_iter > 0 and not accepted))
    return done(MAX_ITERATIONS, max_iter)


def truncate(result, k):
    """What lm_minimize_ld(max_iter=k) returns, read from a longer run `result`: (x, status, iterations,
    lam, trials)."""
    x, status, iterations, trace, states = result
    if k < len(states):
        s = states[k]
        return s["x"], MAX_ITERATIONS, k, s["lam"], s["trials"]
    # a loop that returned from inside an outer iteration holds the lambda its last trial was taken with
    stopped = trace and trace[-1]["outcome"] == "stopped"
    return x, status, iterations, trace[-1]["lam"] if stopped else states[-1]["lam"], len(trace)


def exhausted_iterations(result):
    """the outer iterations (counted from 1, as the number of iterations a run limited to them reports)
    that left x where it was"""
    return [j for j, s in enumerate(result[4]) if s["exhausted"]]


def decision_margins(trace, dtype=np.float64):
    """How far every decision of a trace is from falling the other way under rounding:
      rho       min |rho| over the trials
      delta     min over the rejected trials of the factor between max|delta| and sqrt(eps)
      cost      min over the trials' y0 and yi of the factor between them and 8 eps"""
    eps = LD(np.finfo(dtype).eps)
    factor = lambda a, b: max(LD(a) / b, b / LD(a)) if a > 0 else LD(np.inf)
    rho = min((abs(LD(t["rho"])) for t in trace), default=LD(np.inf))
    delta = min((factor(t["max_delta"], np.sqrt(eps)) for t in trace if t["rho"] < 0), default=LD(np.inf))
    cost = min((factor(abs(y), 8 * eps) for t in trace for y in (t["y0"], t["yi"])), default=LD(np.inf))
    return dict(rho=float(rho), delta=float(delta), cost=float(cost))


def assert_decision_margins(trace, dtype=np.float64, what=None):
    """|rho| >= 1e-3 at every trial; max|delta| of a rejected trial and every y0, yi a factor 10 away from
    their thresholds: a device that adds its sums in another order takes the same decisions."""
    m = decision_margins(trace, dtype)
    assert m["rho"] >= 1e-3 and m["delta"] >= 10 and m["cost"] >= 10, (what, m)
    return m
