"""mopt_batch — B independent small point2point problems minimised by ONE launch of B workgroups
(finalize_kernels.hip p2pSolveBatchKernel) — against the lone one-launch solve of each problem
(mopt_lm_minimize on a Point2PointCost of the same data: p2pSolveSmallKernel, unchanged), whose device
function it shares.

Bar.  The two kernels run one inlined device function over the same sums in the same order: equal status,
iterations and sweeps, and x and cost equal BIT FOR BIT, for every Jacobian mode, manifold update,
covariance form, the robust loss and both scalar types.  Against the CPU loop: the one-launch solve's own
bar (same status and count, x within 1e-9 max(1, |x|))."""
import numpy as np
import pytest

from tests import datasets as ds
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

UNSUPPORTED = "error 5"
COV_SYM = np.array([[2.0, 0.3, -0.1], [0.3, 0.5, 0.2], [-0.1, 0.2, 1.5]])
COV_GENERAL = np.array([[2.0, 0.7, -0.1], [0.3, 0.5, 0.9], [-0.4, 0.2, 1.5]])


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_same_solve(got_x, got_rep, lone_x, lone_rep, what):
    """the batch's problem against its lone solve: status, iterations, sweeps, and x and cost bit for bit"""
    print("batch vs lone", what, "max |dx|", np.abs(np.asarray(got_x, dtype=np.float64) - lone_x).max(),
          "cost", got_rep["cost"], lone_rep["cost"])
    assert (got_rep["status"], got_rep["iterations"], got_rep["sweeps"]) == \
        (lone_rep["status"], lone_rep["iterations"], lone_rep["sweeps"]), (what, got_rep, lone_rep)
    assert bits(got_x) == bits(lone_x), (what, got_x, lone_x)
    assert bits(np.float64(got_rep["cost"])) == bits(np.float64(lone_rep["cost"])), (what, got_rep, lone_rep)


def lone_solves(mo, costs, x0s, jac, **kw):
    return [mo.capi.lm_minimize([c], [jac], x0, **kw) for c, x0 in zip(costs, x0s)]


def start_poses(count, dtype, seed=3):
    rng = np.random.default_rng(seed)
    x0s = rng.uniform(-0.3, 0.3, size=(count, 6))
    x0s[0] = 0.0  # one problem starts where the reference's test does
    return x0s.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_problem_takes_the_lone_solves_iterates(hip_lib, dtype):
    mo = hip_lib
    per_tile = 512 if dtype == np.float64 else 1024
    sizes = (3, 7, per_tile - 1, per_tile, per_tile + 1, 1000, 4 * per_tile - 1, 4 * per_tile)
    pairs = [ds.synthetic_pair(n, seed=60 + i, noise=0.01, dtype=dtype) for i, n in enumerate(sizes)]
    x0s = start_poses(len(sizes), dtype)
    batch = mo.Point2PointBatch([p[0] for p in pairs], [p[1] for p in pairs], dtype=dtype)
    assert batch.info() == dict(num_problems=len(sizes), total_count=sum(sizes), scalar_bytes=np.dtype(dtype).itemsize)
    costs = [mo.Point2PointCost(s, t, dtype=dtype) for s, t in pairs]
    # the cases of test_small_problems_in_one_launch_take_the_same_iterates (tests/test_gpu_device_lm.py)
    cases = [(mo.JAC_ANALYTIC, 0, None, 0), (mo.JAC_NUMERIC, 0, None, 0), (mo.JAC_ANALYTIC_TST_LAYOUT, 0, None, 0),
             (mo.JAC_ANALYTIC_LEFT, 1, None, 0), (mo.JAC_ANALYTIC_RIGHT, 2, None, 0),
             (mo.JAC_ANALYTIC, 0, COV_SYM, 1), (mo.JAC_NUMERIC, 0, np.diag([0.5, 2.0, 3.0]), 1)]
    compared = 0
    for jac, manifold, cov, loss in cases:
        batch.set_covariance(cov)
        batch.set_loss(loss, 100.0)
        for c in costs:
            c.set_covariance(cov)
            c.set_loss(loss, 100.0)
        for k in (1, 3, 15):
            xs, reps = batch.minimize(x0s, jac, max_iterations=k, manifold=manifold)
            lone = lone_solves(mo, costs, x0s, jac, max_iterations=k, manifold=manifold)
            for i, (xl, rl) in enumerate(lone):
                assert_same_solve(xs[i], reps[i], xl, rl, (sizes[i], jac, manifold, cov is not None, loss, k))
                compared += 1
    assert compared == 7 * 3 * len(sizes)
    batch.close()
    for c in costs:
        c.close()


def test_more_workgroups_than_compute_units_and_one(hip_lib):
    mo = hip_lib
    # B = 1
    src, tgt = ds.synthetic_pair(1000, seed=5, noise=0.01)
    one = mo.Point2PointBatch([src], [tgt])
    cost = mo.Point2PointCost(src, tgt)
    xs, reps = one.minimize(np.zeros((1, 6)), mo.JAC_ANALYTIC)
    xl, rl = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], np.zeros(6))
    assert xs.shape == (1, 6) and len(reps) == 1
    assert_same_solve(xs[0], reps[0], xl, rl, "B = 1")
    one.close()
    cost.close()
    # B = 600: more workgroups than the device has compute units
    rng = np.random.default_rng(77)
    sizes = rng.integers(64, 201, size=600)
    pairs = [ds.synthetic_pair(int(n), seed=1000 + i, noise=0.01) for i, n in enumerate(sizes)]
    x0s = start_poses(600, np.float64, seed=9)
    batch = mo.Point2PointBatch([p[0] for p in pairs], [p[1] for p in pairs])
    xs, reps = batch.minimize(x0s, mo.JAC_ANALYTIC, max_iterations=15)
    assert len(reps) == 600 and np.isfinite(xs).all()
    assert all(r["sweeps"] >= 1 and r["status"] in (0, 1, 2) and np.isfinite(r["cost"]) for r in reps)
    for i in rng.choice(600, size=16, replace=False):
        cost = mo.Point2PointCost(*pairs[i])
        xl, rl = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], x0s[i], max_iterations=15)
        assert_same_solve(xs[i], reps[i], xl, rl, ("B = 600", int(i), int(sizes[i])))
        cost.close()
    batch.close()


def test_problems_do_not_see_each_other(hip_lib):
    mo = hip_lib
    sizes = (100, 513, 9, 1500, 64)
    pairs = [ds.synthetic_pair(n, seed=200 + i, noise=0.01) for i, n in enumerate(sizes)]
    x0s = start_poses(len(sizes), np.float64, seed=4)
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    forward = mo.Point2PointBatch(srcs, tgts)
    backward = mo.Point2PointBatch(srcs[::-1], tgts[::-1])
    for jac in (mo.JAC_ANALYTIC, mo.JAC_NUMERIC):
        xf, rf = forward.minimize(x0s, jac)
        xb, rb = backward.minimize(x0s[::-1], jac)
        assert bits(xf) == bits(xb[::-1]), (jac, xf - xb[::-1])
        for a, b in zip(rf, rb[::-1]):
            assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["sweeps"] == b["sweeps"]
            assert bits(np.float64(a["cost"])) == bits(np.float64(b["cost"])) and \
                bits(np.float64(a["lambda_"])) == bits(np.float64(b["lambda_"]))
    backward.close()
    # a problem whose targets are all NaN (every index rejected) and one of 2 correspondences (singular
    # normal equations) next to the well-posed ones
    nan_src, nan_tgt = ds.synthetic_pair(300, seed=301)
    nan_tgt = np.full_like(nan_tgt, np.nan)
    two_src, two_tgt = ds.synthetic_pair(2, seed=302, noise=0.01)
    mixed = mo.Point2PointBatch([srcs[0], nan_src, srcs[1], srcs[2], two_src, srcs[3], srcs[4]],
                                [tgts[0], nan_tgt, tgts[1], tgts[2], two_tgt, tgts[3], tgts[4]])
    x0_mixed = np.vstack([x0s[0], np.zeros(6), x0s[1], x0s[2], np.zeros(6), x0s[3], x0s[4]])
    xm, rm = mixed.minimize(x0_mixed, mo.JAC_ANALYTIC)
    xf, rf = forward.minimize(x0s, mo.JAC_ANALYTIC)
    for good, at in enumerate((0, 2, 3, 5, 6)):
        assert bits(xm[at]) == bits(xf[good]) and rm[at] == rf[good], (good, at, rm[at], rf[good])
    for at, (s, t) in ((1, (nan_src, nan_tgt)), (4, (two_src, two_tgt))):
        cost = mo.Point2PointCost(s, t)
        _, rl = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], np.zeros(6))
        assert rm[at]["status"] == rl["status"], (at, rm[at], rl)
        cost.close()
    mixed.close()
    forward.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_forward_differences_are_chosen_per_problem(hip_lib, oracle, dtype):
    mo = hip_lib
    rng = np.random.default_rng(21)
    # nearly aligned clouds, started near the pose: every point literal
    # (test_one_launch_solve_holds_both_forward_difference_forms) ...
    x_small = np.array([0.02, -0.03, 0.01, 0.004, -0.006, 0.005])
    # ... and from 0 towards a pose whose components are all >= 0.2: moments after the fixed first step
    x_large = np.array([0.5, -0.3, 0.2, 0.25, -0.2, 0.3])
    pairs, x0s = [], []
    for n, x_true, x0 in ((700, x_small, 0.5 * x_small), (900, x_large, np.zeros(6)),
                          (1300, x_small, 0.5 * x_small), (2048, x_large, np.zeros(6))):
        src = rng.random((n, 3)) * 10.0
        T = oracle.se3_from_x(x_true)
        tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, (n, 3))
        pairs.append((src.astype(dtype), tgt.astype(dtype)))
        x0s.append(x0)
    x0s = np.array(x0s, dtype=dtype)
    batch = mo.Point2PointBatch([p[0] for p in pairs], [p[1] for p in pairs], dtype=dtype)
    costs = [mo.Point2PointCost(s, t, dtype=dtype) for s, t in pairs]
    for cov in (None, COV_SYM, COV_GENERAL):
        batch.set_covariance(cov)
        for c in costs:
            c.set_covariance(cov)
        before = [c.lm_choice_stats() for c in costs]
        points0, literal0 = batch.lm_choice_stats()
        xs, reps = batch.minimize(x0s, mo.JAC_NUMERIC)
        lone = lone_solves(mo, costs, x0s, mo.JAC_NUMERIC)
        for i, (xl, rl) in enumerate(lone):
            assert_same_solve(xs[i], reps[i], xl, rl, ("numeric", i, cov is not None))
        after = [c.lm_choice_stats() for c in costs]
        points, literal = batch.lm_choice_stats()
        points, literal = points - points0, literal - literal0
        assert points == sum(a[0] - b[0] for a, b in zip(after, before)) == sum(r["sweeps"] for r in reps)
        assert literal == sum(a[1] - b[1] for a, b in zip(after, before))
        assert 0 < literal < points, (points, literal)
    batch.close()
    for c in costs:
        c.close()


def test_against_the_cpu_loop(hip_lib, oracle):
    mo = hip_lib
    pairs = [ds.synthetic_pair(1000, seed=5 + i, noise=0.01) for i in range(3)]
    batch = mo.Point2PointBatch([p[0] for p in pairs], [p[1] for p in pairs])
    for k in (1, 2, 3, 5, 15):
        xs, reps = batch.minimize(np.zeros((3, 6)), mo.JAC_ANALYTIC, max_iterations=k)
        for i, (src, tgt) in enumerate(pairs):
            xr, status, iters = oracle.p2p_minimize(src, tgt, np.zeros(6), cost_class=ob.ANALYTIC_DYN,
                                                    layout=ob.LAYOUT_ROW_MAJOR, max_iter=k)
            assert (reps[i]["status"], reps[i]["iterations"]) == (status, iters), (k, i, reps[i], status, iters)
            assert np.abs(xs[i] - xr).max() < 1e-9 * max(1.0, np.abs(xr).max()), (k, i, xs[i], xr)
    batch.close()


def test_refusals_on_the_device(hip_lib):
    mo = hip_lib
    for dtype, per_tile in ((np.float64, 512), (np.float32, 1024)):
        small = ds.synthetic_pair(50, seed=1, dtype=dtype)
        large = ds.synthetic_pair(4 * per_tile + 1, seed=2, dtype=dtype)
        with pytest.raises(mo.MoptError) as e:
            mo.Point2PointBatch([small[0], large[0]], [small[1], large[1]], dtype=dtype)
        assert UNSUPPORTED in str(e.value) and "problem 1" in str(e.value) and str(4 * per_tile + 1) in str(e.value)
    # a cloud far from its frame's origin: |c0|^2 = 1.5e6 > 1e3 r^2 = 750
    rng = np.random.default_rng(8)
    far_src = rng.random((400, 3)) + np.array([1e3, 7e2, 10.0])
    far_tgt = far_src + np.array([0.05, -0.02, 0.03]) + rng.normal(0, 0.001, far_src.shape)
    near = ds.synthetic_pair(400, seed=3, noise=0.01)
    batch = mo.Point2PointBatch([near[0], far_src], [near[1], far_tgt])
    x0s = np.zeros((2, 6))
    with pytest.raises(mo.MoptError) as e:
        batch.minimize(x0s, mo.JAC_ANALYTIC_LEFT, manifold=1)
    assert UNSUPPORTED in str(e.value) and "problem 1" in str(e.value)
    # the same batch under the Euclidean-parameter Jacobian is solved — and still solves after the refusal
    xs, reps = batch.minimize(x0s, mo.JAC_ANALYTIC)
    for i, (s, t) in enumerate(((near[0], near[1]), (far_src, far_tgt))):
        cost = mo.Point2PointCost(s, t)
        xl, rl = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], np.zeros(6))
        assert_same_solve(xs[i], reps[i], xl, rl, ("after a refusal", i))
        cost.close()
    batch.close()


def test_streams_and_pool_memory_are_returned(hip_lib):
    mo = hip_lib
    src, tgt = ds.synthetic_pair(3000, seed=11, noise=0.01)
    cost = mo.Point2PointCost(src, tgt)
    H0, b0, s0 = cost.linearize(ds.X_GENERIC, mo.JAC_ANALYTIC)
    pairs = [ds.synthetic_pair(100 + 10 * i, seed=400 + i, noise=0.01) for i in range(8)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    first = None
    for _ in range(50):
        batch = mo.Point2PointBatch(srcs, tgts)
        xs, reps = batch.minimize(np.zeros((8, 6)), mo.JAC_ANALYTIC)
        batch.close()
        first = xs if first is None else first
        assert bits(xs) == bits(first) and all(r["status"] in (0, 1, 2) for r in reps)
    cost.linearize(ds.X_ZERO, mo.JAC_ANALYTIC)  # (another x in between: the next call sweeps, it is not answered from the cost's cache)
    H1, b1, s1 = cost.linearize(ds.X_GENERIC, mo.JAC_ANALYTIC)
    assert bits(H1) == bits(H0) and bits(b1) == bits(b0) and s1 == s0
    cost.close()
