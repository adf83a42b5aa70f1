"""The Levenberg-Marquardt state machine on the device where trials are REJECTED: several rejections in a row,
inner loops that run out (lm_device.hpp: the next outer iteration starts from the stored H | b | y0 without a
sweep and keeps the grown lambda), lm_max_iterations other than 3 and 0, and the batch's limits — in its three
forms: the launch-per-point loop (lmStepBody), the one-launch solve (p2pSolveSmallKernel) and a workgroup of
the batch (p2pSolveBatchKernel).

Reference.  tests/highprec.lm_minimize_ld: the loop of levenberg_marquadt_dyn.cpp:34-119 in 80-bit long double
over the 80-bit sums, with a trace of every trial; it shares no code with oracle/ and is pinned against the
oracle on the CPU (tests/test_highprec_reference.py).  One run yields every truncation k.

Cases (tests/lm_rejection_cases.py; ds.synthetic_pair(300, seed=11, noise=0.01) unless said; analytic Jacobian;
"exhausted": the outer iterations, counted from 1, that leave x where it was; runs of 15):

  row          x0                        lm_iter: exhausted
  ROLL         [0,0,0,3.1,0,0]           1: 2...15 (all)   2: 2...6   3: 2, 3   5: 2
  TUMBLE       [0,0,0,2.5,-2,3]          1: 3...14   2: 3...6   3: 3, 4   5: 3
  PITCH        [0,0,0,0,3.0,0]           2: 2...6 and 8
  FAR          [50,-40,30,1.5,1.5,-1.5]  1, 2, 3: 12...15, at the optimum.  lm_iter 5 is left out of the GPU rows:
                                         it ends in SMALL_DELTA at 14 on a trial whose max|delta| = 7.2e-9 is
                                         within a factor 2.1 of sqrt(eps) (the CPU pin keeps it)
  GM_OUTLIERS  0, every third target     3: 2...6; Geman-McClure (1.0)
               + N(0, 30^2) (seed 1)
  SMALL_DELTA  0, the same with seed 8   8: 3, then SMALL_DELTA in iteration 4 (runs of 6).  lm_iter 8 because
                                         consecutive trials shrink delta by nu = 2, 4, 8, ...: only from nu = 128
                                         on does one step jump from 10 sqrt(eps) to sqrt(eps) / 10; with lm_iter
                                         3 or 5 every SMALL_DELTA found (seeds 0...11, the starts above) stops
                                         within a factor 3 of sqrt(eps)
  GENERAL_COV  TUMBLE's x0, COV_GENERAL  1: 1...12   2: 1...4   3: 1, 2   5: 1.  (ROLL's x0 under this covariance
                                         has a trial with |rho| = 5.7e-4: no margin)
  SEVEN        ROLL's x0, n = 7          1: 2...15   3: 2, 3
  ROLL_5_TILES / TUMBLE_5_TILES  n = 2100: 1: 2...14, 3: 2, 3 / 1: 3...11
  ROLL_TWO_COSTS  synthetic_pair(1025, seed 31 and 32, noise 0.02) as two costs: 1: 2...14, 3: 2, 3
  WELL         0, synthetic_pair(1000, seed=5): 1: 8...15, 3: 8...11 (the batch's well-behaved problem)
  NAN_ROWS     0, synthetic_pair(n, seed=70 + n) for n = 700, 2048 without the rows whose target is NaN: 3: none
               exhausted, every trial accepted; runs of 5 (analytic), the first 3 iterations under forward differences
No truncation is left out as too sensitive: the two CPU loops agree to 5e-14 at every k of every row (bar 1e-10).
fp32 rows: ROLL and TUMBLE, lm_iter 1 and 3 — the float oracle and the long-double loop over float inputs take
the same decisions at every k, so both keep their fp32 leg.  In the fp32 batch WELL and the SMALL_DELTA cloud
are judged against their traces up to k = 6 (4 under Geman-McClure): beyond, float's sqrt(eps) = 3.5e-4 is
within a factor 6 of a rejected delta.

Margins (asserted on the trace before the device is looked at; measured on the CPU, worst over the fp64 rows and
their lm_iter): |rho| >= 1e-3 — 3.2e-3 (SEVEN, lm_iter 1 and 3), then 8.4e-3 (ROLL, lm_iter 2, 3, 5) and 9.3e-3
(PITCH); max|delta| of a rejected trial a factor >= 10 from sqrt(eps) — 10.6 (SMALL_DELTA), 68 (WELL, lm_iter
3), 3.9e3 (WELL, lm_iter 1), 5.1e3 (FAR), every other row >= 1.5e5; y0, yi a factor >= 10 from 8 eps — 5.1e13 (FAR).

lambda_.  The project had no bar for it.  Measured on the CPU: the largest relative difference of lambda between
lm_minimize_ld in long double and the same function in np.float64, over every state of every row above, is
2.56e-8 (WELL: the accepted steps' factor 1 - (2 rho - 1)^3 amplifies the rounding of rho; the rejection rows
stay below 2e-9) — LAMBDA_MEASURED = 2.6e-8, bound LAMBDA_RTOL = 10 x that = 2.6e-7.  Under forward differences
(NAN_ROWS, the first 3 iterations) the same measurement gives 2.69e-9 — the quotients' own rounding in max diag H,
which the first lambda is taken from — LAMBDA_MEASURED_FD = 2.7e-9, bound LAMBDA_RTOL_FD = 2.7e-8.  Both
constants live in tests/lm_rejection_cases.py and tests/test_highprec_reference.py re-measures them; lambda_ is
asserted on every fp64 solve that is compared with a trace, under either Jacobian."""
import numpy as np
import pytest

from tests import datasets as ds
from tests import highprec as hp
from tests import lm_rejection_cases as lc
from tests import oracle_binding as ob
from tests.test_gpu_batch_solve import assert_same_solve, bits
from tests.test_gpu_device_lm import FD_ITERATE_TOL

pytestmark = pytest.mark.gpu

LAMBDA_RTOL, LAMBDA_RTOL_FD = lc.LAMBDA_RTOL, lc.LAMBDA_RTOL_FD
CONVERGED, MAX_ITERATIONS, SMALL_DELTA = 0, 1, 2
ONE_LAUNCH = "MOPT_LM_ONE_LAUNCH_TILES"
EPS_F = float(np.finfo(np.float32).eps)


def configure(mo, obj, case):
    obj.set_covariance(case.cov)
    obj.set_loss(mo.LOSS_NONE if case.loss is None else mo.LOSS_GEMAN_MCCLURE, case.loss or 0.0)


def against_trace(x, rep, case, lm_iter, k, what, dtype=np.float64, jac_mode=0, data=None):
    """one device solve limited to k iterations against the long-double loop of its row"""
    res = case.reference(lm_iter, dtype=dtype, jac_mode=jac_mode)
    xr, status, iters, lam, trials = hp.truncate(res, k)
    src, tgt = data if data is not None else case.data(dtype)
    xr = np.asarray(xr, dtype=np.float64)
    err = np.abs(np.asarray(x, dtype=np.float64) - xr).max() / max(1.0, np.abs(xr).max())
    cost_ref = float(hp.p2p_cost_ld(src, tgt, x, dtype=dtype))
    lam_err = abs(hp.LD(rep["lambda_"]) - lam) / lam
    print(what, "k", k, rep, "x err %.2e cost rel %.2e lambda rel %.2e" %
          (err, abs(rep["cost"] - cost_ref) / cost_ref, float(lam_err)))
    if dtype == np.float32:
        assert err <= 2e-3, (what, k, x, xr)
        return
    assert (rep["status"], rep["iterations"]) == (status, iters), (what, k, rep, status, iters)
    assert rep["sweeps"] == 1 + trials, (what, k, rep, trials)
    assert err <= (FD_ITERATE_TOL if jac_mode == 2 else 1e-9), (what, k, x, xr)
    assert abs(rep["cost"] - cost_ref) <= 1e-9 * cost_ref, (what, k, rep["cost"], cost_ref)
    assert lam_err <= (LAMBDA_RTOL_FD if jac_mode == 2 else LAMBDA_RTOL), (what, k, rep["lambda_"], float(lam))


def exhausted_steps_are_exact(solves, case, lm_iter, what, dtype=np.float64):
    """On the device's own reports: an exhausted iteration multiplies lambda by nu = 2, 4, ... 2^lm_iter —
    powers of two, so exactly — and leaves x bit for bit.  solves: {k: (x, rep)}."""
    res = case.reference(lm_iter, dtype=dtype)
    factor = 2.0 ** (lm_iter * (lm_iter + 1) // 2)
    checked = 0
    for k in hp.exhausted_iterations(res):
        if k - 1 in solves and k in solves and k >= 2:
            (xa, ra), (xb, rb) = solves[k - 1], solves[k]
            assert ra["lambda_"] > 0 and rb["lambda_"] == factor * ra["lambda_"], (what, k, ra, rb)
            assert bits(xa) == bits(xb), (what, k, xa, xb)
            checked += 1
    return checked


def run_forms(mo, case, lm_iter, dtype, monkeypatch, forms=("per point", "one launch", "batch")):
    """{form: {k: (x, rep)}} of the row at every truncation"""
    src, tgt = case.data(dtype)
    cost = mo.Point2PointCost(src, tgt, dtype=dtype)
    batch = mo.Point2PointBatch([src], [tgt], dtype=dtype) if "batch" in forms else None
    configure(mo, cost, case)
    if batch is not None:
        configure(mo, batch, case)
    x0 = case.x0.astype(dtype)
    out = {form: {} for form in forms}
    for k in range(1, case.kmax + 1):
        for form in forms:
            if form == "batch":
                xs, reps = batch.minimize(x0[None, :], mo.JAC_ANALYTIC, max_iterations=k, lm_max_iterations=lm_iter)
                out[form][k] = (xs[0], reps[0])
                continue
            if form == "per point":
                monkeypatch.setenv(ONE_LAUNCH, "0")
            else:
                monkeypatch.delenv(ONE_LAUNCH, raising=False)
            out[form][k] = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], x0, max_iterations=k,
                                               lm_max_iterations=lm_iter)
    monkeypatch.delenv(ONE_LAUNCH, raising=False)
    cost.close()
    if batch is not None:
        batch.close()
    return out


@pytest.mark.parametrize("row", range(len(lc.CASES)), ids=[c.name for c in lc.CASES])
def test_rejected_trials_and_exhausted_loops_in_the_three_device_forms(hip_lib, monkeypatch, row):
    case = lc.CASES[row]
    for lm_iter in case.lm_iters:
        res = case.reference(lm_iter)
        hp.assert_decision_margins(res[3], what=(case.name, lm_iter))
        assert hp.exhausted_iterations(res), (case.name, lm_iter)
        solves = run_forms(hip_lib, case, lm_iter, np.float64, monkeypatch)
        for form, by_k in solves.items():
            for k, (x, rep) in by_k.items():
                against_trace(x, rep, case, lm_iter, k, (case.name, lm_iter, form))
            checked = exhausted_steps_are_exact(by_k, case, lm_iter, (case.name, lm_iter, form))
            assert checked >= len([k for k in hp.exhausted_iterations(res) if k >= 2]) - 1
        # the batch's workgroup and the lone one-launch solve share their device function: bit for bit
        for k in solves["batch"]:
            assert_same_solve(*solves["batch"][k], *solves["one launch"][k], (case.name, lm_iter, k))
    if case is lc.ROLL:  # all exhausted: x never moves after the first iterate, in any form
        for form, by_k in run_forms(hip_lib, case, 1, np.float64, monkeypatch).items():
            assert len({bits(x) for x, _ in by_k.values()}) == 1, form
            assert [by_k[k][1]["iterations"] for k in sorted(by_k)] == list(range(1, 16)), form


@pytest.mark.parametrize("case", [lc.ROLL_5_TILES, lc.TUMBLE_5_TILES], ids=lambda c: c.name)
def test_launch_per_point_loop_at_five_tiles(hip_lib, monkeypatch, case):
    """2 100 fp64 correspondences: past the one-launch solve's four tiles, so the launch-per-point loop runs at
    the size it is there for, with the environment untouched."""
    monkeypatch.delenv(ONE_LAUNCH, raising=False)
    mo = hip_lib
    src, tgt = case.data()
    cost = mo.Point2PointCost(src, tgt)
    for lm_iter in case.lm_iters:
        res = case.reference(lm_iter)
        hp.assert_decision_margins(res[3], what=(case.name, lm_iter))
        by_k = {k: mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], case.x0, max_iterations=k, lm_max_iterations=lm_iter)
                for k in range(1, 16)}
        for k, (x, rep) in by_k.items():
            against_trace(x, rep, case, lm_iter, k, (case.name, lm_iter), data=(src, tgt))
        assert exhausted_steps_are_exact(by_k, case, lm_iter, (case.name, lm_iter)) >= 1
    cost.close()


@pytest.mark.parametrize("case", [lc.ROLL, lc.TUMBLE], ids=lambda c: c.name)
def test_float_rejections_and_exhausted_loops(hip_lib, oracle, monkeypatch, case):
    mo = hip_lib
    src, tgt = case.data(np.float32)
    for lm_iter in (1, 3):
        res = case.reference(lm_iter, dtype=np.float32)
        hp.assert_decision_margins(res[3], np.float32, what=(case.name, lm_iter))
        solves = run_forms(mo, case, lm_iter, np.float32, monkeypatch)
        for k in range(1, 16):
            _, status, iters = oracle.p2p_minimize(src, tgt, case.x0, cost_class=ob.ANALYTIC_DYN,
                                                   layout=ob.LAYOUT_ROW_MAJOR, max_iter=k, lm_iter=lm_iter,
                                                   dtype=np.float32)
            assert hp.truncate(res, k)[1:3] == (status, iters), (case.name, lm_iter, k)  # the fp32 leg has margin
            for form, by_k in solves.items():
                x, rep = by_k[k]
                assert (rep["status"], rep["iterations"]) == (status, iters), (case.name, lm_iter, form, k, rep)
                against_trace(x, rep, case, lm_iter, k, (case.name, lm_iter, form, "fp32"), dtype=np.float32,
                              data=(src, tgt))
        for form, by_k in solves.items():
            assert exhausted_steps_are_exact(by_k, case, lm_iter, (case.name, lm_iter, form), np.float32) >= 1


def test_two_costs_reduced_by_one_finalize_then_an_exhausted_step(hip_lib):
    """Two Point2PointCosts of 1025 + 1025 correspondences against the loop over the concatenated clouds."""
    mo = hip_lib
    case = lc.ROLL_TWO_COSTS
    src, tgt = case.data()
    costs = [mo.Point2PointCost(src[:1025], tgt[:1025]), mo.Point2PointCost(src[1025:], tgt[1025:])]
    for lm_iter in case.lm_iters:
        res = case.reference(lm_iter)
        hp.assert_decision_margins(res[3], what=(case.name, lm_iter))
        by_k = {k: mo.capi.lm_minimize(costs, [mo.JAC_ANALYTIC] * 2, case.x0, max_iterations=k,
                                       lm_max_iterations=lm_iter) for k in range(1, 16)}
        for k, (x, rep) in by_k.items():
            against_trace(x, rep, case, lm_iter, k, (case.name, lm_iter), data=(src, tgt))
        assert exhausted_steps_are_exact(by_k, case, lm_iter, (case.name, lm_iter)) >= 1
    for c in costs:
        c.close()


# the batch's problems: (clouds, x0, largest k judged against the trace per scalar type and loss)
BATCH_PROBLEMS = (
    ("well", dict(n=1000, seed=5), np.zeros(6), {("float64", False): 15, ("float64", True): 6, ("float32", False): 6, ("float32", True): 6}),
    ("roll", dict(), lc.X_ROLL, {("float64", False): 15, ("float64", True): 6, ("float32", False): 15, ("float32", True): 6}),
    ("tumble", dict(), lc.X_TUMBLE, {("float64", False): 15, ("float64", True): 6, ("float32", False): 15, ("float32", True): 6}),
    ("small delta", dict(outliers=8), np.zeros(6), {("float64", False): 15, ("float64", True): 6, ("float32", False): 6, ("float32", True): 4}),
)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_whose_workgroups_leave_the_loop_at_different_trip_counts(hip_lib, oracle, dtype):
    """Four clouds side by side and in reverse, each against its own trace and bit for bit its lone solve.
    lm_max_iterations is one value per call, so the regimes cannot all meet in one launch; three rounds:
      lm_iter 1          WELL accepts seven trials in a row, ROLL exhausts every loop from iteration 2, TUMBLE from 3;
                         the outlier cloud ("small delta") under no loss accepts everything
      lm_iter 3          WELL accepts, ROLL exhausts 2 and 3, TUMBLE 3 and 4, the outlier cloud accepts
      Geman-McClure, 8   the outlier cloud exhausts iteration 3 and stops on SMALL_DELTA in iteration 4 while the
                         others run to the limit (runs of 6)
    With lm_iter 1 every iteration costs one point whether it accepts or exhausts, so there the workgroups differ in
    what they do, not in how long they stay; with lm_iter 3 they leave after different numbers of points (asserted
    on the reports' sweeps at k = 5, both scalar types), and in the third round at different iterations with
    different statuses (asserted in fp64; in fp32 that cloud has no margin past k = 4)."""
    mo = hip_lib
    name = np.dtype(dtype).name
    for loss, lm_iter, kmax in ((None, 1, 15), (None, 3, 15), (lc.GM, 8, 6)):
        rows = [lc.Case(label, x0, (lm_iter,), loss=loss, kmax=limits[(name, loss is not None)], **kw)
                for label, kw, x0, limits in BATCH_PROBLEMS]
        for case in rows:
            hp.assert_decision_margins(case.reference(lm_iter, dtype=dtype)[3], dtype, what=(case.name, loss, lm_iter))
        pairs = [case.data(dtype) for case in rows]
        x0s = np.array([case.x0 for case in rows], dtype=dtype)
        costs = [mo.Point2PointCost(s, t, dtype=dtype) for s, t in pairs]
        for c, case in zip(costs, rows):
            configure(mo, c, case)
        for order in (slice(None), slice(None, None, -1)):
            batch = mo.Point2PointBatch([p[0] for p in pairs][order], [p[1] for p in pairs][order], dtype=dtype)
            configure(mo, batch, rows[0])
            statuses = set()
            for k in range(1, kmax + 1):
                xs, reps = batch.minimize(x0s[order], mo.JAC_ANALYTIC, max_iterations=k, lm_max_iterations=lm_iter)
                xs, reps = xs[order], reps[order]
                for i, case in enumerate(rows):
                    what = (name, loss, lm_iter, case.name)
                    xl, rl = mo.capi.lm_minimize([costs[i]], [mo.JAC_ANALYTIC], x0s[i], max_iterations=k,
                                                 lm_max_iterations=lm_iter)
                    assert_same_solve(xs[i], reps[i], xl, rl, what + (k,))
                    assert reps[i]["lambda_"] == rl["lambda_"], (what, k, reps[i], rl)
                    if k > case.kmax:
                        continue
                    statuses.add((reps[i]["status"], reps[i]["iterations"] == k))
                    if dtype == np.float32:
                        _, status, iters = oracle.p2p_minimize(
                            pairs[i][0], pairs[i][1], case.x0, cost_class=ob.ANALYTIC_DYN, layout=ob.LAYOUT_ROW_MAJOR,
                            max_iter=k, lm_iter=lm_iter, loss_kind=0 if loss is None else 1, loss_param=loss or 0.0,
                            dtype=np.float32)
                        assert (reps[i]["status"], reps[i]["iterations"]) == (status, iters), (what, k, reps[i])
                    against_trace(xs[i], reps[i], case, lm_iter, k, what, dtype=dtype, data=pairs[i])
                if loss is None and k == 5:
                    # the points each workgroup evaluates in this one launch, from the traces: WELL accepts five
                    # trials (6 points); with lm_iter 3 ROLL and TUMBLE spend three on each exhausted iteration
                    want = [1 + hp.truncate(case.reference(lm_iter, dtype=dtype), 5)[4] for case in rows]
                    assert want[0] == 6 and (lm_iter == 1 or (want[1] > want[2] > want[0])), want
                    assert [r["sweeps"] for r in reps] == want, (reps, want)
            if loss is not None and dtype == np.float64:
                assert (SMALL_DELTA, False) in statuses and (MAX_ITERATIONS, True) in statuses, statuses
            batch.close()
        for c in costs:
            c.close()


def exact_pair(n, seed, dtype):
    """targets that ARE the sources under ds.FIXTURE_X as the type under test forms that pose, rounded to the
    type: the residuals are the targets' rounding, and sum r.r is far below 8 eps"""
    src, _ = ds.synthetic_pair(n, seed=seed, dtype=dtype)
    R, t = hp.transform_from_x(ds.FIXTURE_X.astype(dtype), dtype)
    tgt = np.asarray(src.astype(hp.LD) @ R.T + t).astype(dtype)
    return src, tgt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lm_max_iterations_zero(hip_lib, dtype):
    """No trial point is ever formed: every outer iteration linearizes at x0 and the loop runs into its limit,
    unless the cost at x0 is below 8 eps.  The lone call at a one-launch size and at five tiles, and a batch."""
    mo = hip_lib
    eps = float(np.finfo(dtype).eps)
    per_tile = 512 if dtype == np.float64 else 1024
    x_noisy = ds.X_GENERIC.astype(dtype)
    x_exact = ds.FIXTURE_X.astype(dtype)

    def expect(x, rep, x0, src, tgt, exact, what):
        want = float(hp.p2p_cost_ld(src, tgt, x0, dtype=dtype))
        print(what, rep, "reference cost", want)
        assert bits(x) == bits(x0) and rep["sweeps"] == 1, (what, x, rep)
        if exact:
            assert want < 8 * eps / 10, (what, want)  # the fixture: the reference value itself is below 8 eps
            assert (rep["status"], rep["iterations"]) == (CONVERGED, 0) and abs(rep["cost"]) < 8 * eps, (what, rep)
        else:
            assert (rep["status"], rep["iterations"]) == (MAX_ITERATIONS, 7), (what, rep)
            rtol = 1e-12 if dtype == np.float64 else 64 * EPS_F * len(src)
            assert abs(rep["cost"] - want) <= rtol * want, (what, rep["cost"], want)

    for n in (300, 4 * per_tile + 52):
        for exact in (False, True):
            src, tgt = exact_pair(n, 21, dtype) if exact else ds.synthetic_pair(n, seed=22, noise=0.01, dtype=dtype)
            x0 = x_exact if exact else x_noisy
            cost = mo.Point2PointCost(src, tgt, dtype=dtype)
            for jac in (mo.JAC_ANALYTIC, mo.JAC_NUMERIC):
                x, rep = mo.capi.lm_minimize([cost], [jac], x0, max_iterations=7, lm_max_iterations=0)
                expect(x, rep, x0, src, tgt, exact, ("lone", n, exact, jac))
            cost.close()
    # the batch: noisy, exact and all-NaN-target problems side by side
    noisy = [ds.synthetic_pair(n, seed=23 + n, noise=0.01, dtype=dtype) for n in (300, per_tile + 1)]
    exacts = [exact_pair(n, 24 + n, dtype) for n in (7, 700)]
    nan_src, nan_tgt = ds.synthetic_pair(300, seed=301, dtype=dtype)
    nan_tgt = np.full_like(nan_tgt, np.nan)
    problems = [(noisy[0], x_noisy, False), (exacts[0], x_exact, True), ((nan_src, nan_tgt), x_noisy, None),
                (noisy[1], x_noisy, False), (exacts[1], x_exact, True)]
    batch = mo.Point2PointBatch([p[0][0] for p in problems], [p[0][1] for p in problems], dtype=dtype)
    x0s = np.array([p[1] for p in problems], dtype=dtype)
    for jac in (mo.JAC_ANALYTIC, mo.JAC_NUMERIC):
        xs, reps = batch.minimize(x0s, jac, max_iterations=7, lm_max_iterations=0)
        for i, ((src, tgt), x0, exact) in enumerate(problems):
            if exact is None:  # every index rejected: cost 0
                assert bits(xs[i]) == bits(x0) and reps[i]["sweeps"] == 1 and reps[i]["cost"] == 0.0, reps[i]
                assert (reps[i]["status"], reps[i]["iterations"]) == (CONVERGED, 0), reps[i]
            else:
                expect(xs[i], reps[i], x0, src, tgt, exact, ("batch", i, jac))
    # max_iterations = 0: the loop body never runs — blank reports, x untouched
    xs, reps = batch.minimize(x0s, mo.JAC_ANALYTIC, max_iterations=0)
    assert bits(xs) == bits(x0s)
    for rep in reps:
        assert rep == dict(status=MAX_ITERATIONS, iterations=0, sweeps=0, cost=0.0, lambda_=0.0), rep
    batch.close()


def test_batch_refuses_more_than_4096_points_and_the_lone_call_runs(hip_lib):
    mo = hip_lib
    case = lc.Case("well behaved, 300", np.zeros(6), (3,), seed=5, kmax=40)
    src, tgt = case.data()
    batch = mo.Point2PointBatch([src], [tgt])
    with pytest.raises(mo.MoptError) as e:
        batch.minimize(np.zeros((1, 6)), mo.JAC_ANALYTIC, max_iterations=2000, lm_max_iterations=3)
    assert "error 5" in str(e.value) and "4096 points" in str(e.value), str(e.value)
    # 1 + 1365 * 3 = 4096 points are still a batch's
    xs, reps = batch.minimize(np.zeros((1, 6)), mo.JAC_ANALYTIC, max_iterations=1365, lm_max_iterations=3)
    # the lone call with the refused options runs, launch per point (6001 points are past the one launch's bound)
    cost = mo.Point2PointCost(src, tgt)
    x, rep = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], np.zeros(6), max_iterations=2000, lm_max_iterations=3)
    xl, rl = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC], np.zeros(6), max_iterations=1365, lm_max_iterations=3)
    assert_same_solve(xs[0], reps[0], xl, rl, "after the refusal")
    res = case.reference(3)
    xr = np.asarray(res[0], dtype=np.float64)
    print("lone, 2000 iterations allowed:", rep, "reference", res[1], res[2], hp.decision_margins(res[3]))
    assert res[1] == SMALL_DELTA and res[2] < 40  # the data converges within a few iterations
    assert rep["status"] == SMALL_DELTA and rep["sweeps"] < 200, rep
    assert np.abs(x - xr).max() <= 1e-9 * max(1.0, np.abs(xr).max()), (x, xr)
    assert reps[0]["status"] == SMALL_DELTA and np.abs(xs[0] - xr).max() <= 1e-9 * max(1.0, np.abs(xr).max())
    cost.close()
    batch.close()


def test_each_workgroup_chooses_with_its_own_source_bound(hip_lib, oracle):
    """forwardStepThreshold = 0.08 max(1, rho / 30) with rho = |source bound| + |t|: a 10-box at the origin
    (rho ~ 17) takes the literal forward differences only where some 0 < |x_j| < 0.08, the same box at
    (3000, 4000, 0) (rho ~ 5000, threshold 13) at every point.  A workgroup reading a neighbour's bound would
    take the other form somewhere: another count, other bits."""
    mo = hip_lib
    rng = np.random.default_rng(41)
    poses = ([0.5, -0.3, 0.05, 0.25, -0.2, 0.3], [0.4, 0.6, -0.03, 0.3, 0.2, -0.5],
             [-0.3, 0.2, 0.06, 0.2, 0.35, 0.25], [0.2, -0.5, 0.04, -0.4, 0.2, 0.3])
    pairs = []
    for i, (n, x_true) in enumerate(zip((700, 900, 1300, 2048), poses)):
        src = rng.random((n, 3)) * 10.0 + (np.array([3000.0, 4000.0, 0.0]) if i % 2 else 0.0)
        T = oracle.se3_from_x(np.array(x_true))
        pairs.append((src, src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, (n, 3))))
    x0s = np.zeros((4, 6))
    costs = [mo.Point2PointCost(s, t) for s, t in pairs]
    before = [c.lm_choice_stats() for c in costs]
    lone = [mo.capi.lm_minimize([c], [mo.JAC_NUMERIC], x0) for c, x0 in zip(costs, x0s)]
    delta = [(a[0] - b[0], a[1] - b[1]) for a, b in zip([c.lm_choice_stats() for c in costs], before)]
    print("points, literal points per lone cost:", delta, [r for _, r in lone])
    for i, (points, literal) in enumerate(delta):  # the fixture discriminates
        assert points == lone[i][1]["sweeps"] > 1
        assert (literal == points) if i % 2 else (0 < literal < points), (i, points, literal)
    for order in (slice(None), slice(None, None, -1)):
        batch = mo.Point2PointBatch([p[0] for p in pairs][order], [p[1] for p in pairs][order])
        points0, literal0 = batch.lm_choice_stats()
        xs, reps = batch.minimize(x0s[order], mo.JAC_NUMERIC)
        points, literal = batch.lm_choice_stats()
        xs, reps = xs[order], reps[order]
        for i, (xl, rl) in enumerate(lone):
            assert_same_solve(xs[i], reps[i], xl, rl, ("source bound", i))
            assert reps[i]["status"] in (CONVERGED, MAX_ITERATIONS, SMALL_DELTA), reps[i]
        assert points - points0 == sum(d[0] for d in delta) and literal - literal0 == sum(d[1] for d in delta)
        batch.close()
    for c in costs:
        c.close()


def test_some_nan_targets_in_the_registers_held_solve(hip_lib, monkeypatch):
    """Every fifth target NaN and a NaN run across the first tile boundary (510...515): the rejected indices lie
    between valid ones.  Against the long-double loop over the cloud without those rows (lc.NAN_ROWS), under the
    analytic Jacobian and under forward differences, three legs:
      lone one-launch   a Point2PointCost under its default variant (MOPT_KERNEL_AUTO): p2pSolveSmallKernel, the
                        correspondences held in registers; under forward differences the step chooses the form per
                        point (moments at the fixed first step from 0, FD_ITERATE_TOL bar)
      batch             the same cloud as a problem of a Point2PointBatch, which has no variant of its own and
                        runs as AUTO does.  That the lone leg IS the one-launch form is asserted through it: the
                        two share their device function and must agree bit for bit, which the launch-per-point
                        loop (other sums order) does not
      lone literal      the cost under MOPT_KERNEL_LITERAL, forward differences: a literal cost takes the
                        launch-per-point loop whatever its size — the variant the FD_ITERATE_TOL bar was stated for
    Forward differences up to k = 3 (lc.FD_KMAX): from the fourth iteration on the cost is stationary to twelve
    digits and y0 - yi of a trial is rounding noise of the quotients — the double oracle and the long-double loop
    already stop at different iterations there (n = 2048)."""
    mo = hip_lib
    monkeypatch.delenv(ONE_LAUNCH, raising=False)
    clouds = [lc.nan_clouds(n) for n in lc.NAN_SIZES]
    for (src, tgt), n in zip(clouds, lc.NAN_SIZES):  # the fixture: NaN rows between valid ones, across the boundary
        bad = np.isnan(tgt).any(axis=1)
        assert bad[505] and not bad[509] and bad[510:516].all() and not bad[516] and bad[n - n % 5 - 5] and not bad[-1]
    batch = mo.Point2PointBatch([c[0] for c in clouds], [c[1] for c in clouds])
    costs = [mo.Point2PointCost(s, t) for s, t in clouds]
    x0 = np.zeros(6)
    for jac in (mo.JAC_ANALYTIC, mo.JAC_NUMERIC):
        for k in ((1, 2, 3, 5) if jac == mo.JAC_ANALYTIC else range(1, lc.FD_KMAX + 1)):
            xs, reps = batch.minimize(np.zeros((2, 6)), jac, max_iterations=k)
            for i, case in enumerate(lc.NAN_ROWS):
                res = case.reference(3, jac_mode=jac)
                hp.assert_decision_margins([t for t in res[3] if t["it"] < k], what=(case.name, jac, k))
                costs[i].set_kernel_variant(mo.KERNEL_AUTO)
                xl, rl = mo.capi.lm_minimize([costs[i]], [jac], x0, max_iterations=k)
                against_trace(xl, rl, case, 3, k, (case.name, "lone one-launch", jac), jac_mode=jac)
                against_trace(xs[i], reps[i], case, 3, k, (case.name, "batch", jac), jac_mode=jac)
                assert_same_solve(xs[i], reps[i], xl, rl, (case.name, "batch against lone one-launch", jac, k))
                assert reps[i]["lambda_"] == rl["lambda_"], (case.name, jac, k, reps[i], rl)
                if jac == mo.JAC_NUMERIC:
                    costs[i].set_kernel_variant(mo.KERNEL_LITERAL)
                    xp, rp = mo.capi.lm_minimize([costs[i]], [jac], x0, max_iterations=k)
                    against_trace(xp, rp, case, 3, k, (case.name, "lone literal, launch per point", jac), jac_mode=jac)
                    # (another kernel, other sums: were this bit-equal too, the equality above would tell nothing)
                    assert bits(xp) != bits(xl), (case.name, k)
    batch.close()
    for c in costs:
        c.close()
