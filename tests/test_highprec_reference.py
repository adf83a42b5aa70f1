"""Guards the two references the scene-scale GPU tests judge by (tests/test_gpu_scene_scale.py):
the 80-bit statement of tests/highprec.py and the CPU oracle are written independently, so on the
control scene they must agree to fp64 summation rounding; on every other scene the oracle's own
distance from the 80-bit sums — which the GPU tests take as the kernel's allowance, times 8 — is
pinned, so that allowance cannot grow unnoticed.  No GPU."""
import numpy as np
import pytest

from tests import datasets as ds
from tests import highprec as hp
from tests import lm_rejection_cases as lc
from tests import oracle_binding as ob

COV_GENERAL = np.array([[2.0, 0.7, -0.1], [0.3, 0.5, 0.9], [-0.4, 0.2, 1.5]])
LAYOUT = {0: ob.LAYOUT_ROW_MAJOR, 1: ob.LAYOUT_TST, 3: ob.LAYOUT_LEFT, 4: ob.LAYOUT_RIGHT}
N = ds.SCENE_SIZES[0]

# The oracle's literal fp64 sums against the 80-bit ones, measured on these scenes at n = 4097 (worst
# over modes, covariances and losses; the pose is shared bit for bit, so this is summation and residual
# rounding only): b and the cost within 2e-14 near the origin, and growing with the coordinates as
# eps |R p + t| / |r| must.  Pinned at 4 x the measurement; the emulation the scenes were laid out with
# quoted 2.1e-7 for b at the 1e6 offsets (its pose was rounded separately), which these stay far inside.
EB_MEASURED = {"site": 2.1e-14, "map": 7.1e-13, "utm_to_local": 4.0e-12, "utm_to_local_7e6": 2.1e-11,
               "local_to_map": 3.5e-12, "mm": 3.5e-15, "wall": 3.3e-15}
EC_MEASURED = {"site": 5.3e-15, "map": 3.3e-13, "utm_to_local": 2.5e-12, "utm_to_local_7e6": 6.1e-12,
               "local_to_map": 3.1e-12, "mm": 1.7e-15, "wall": 6e-16}


def losses_of(scene):
    return (None, 1e-6, 1.0) if scene == "mm" else (None, 0.5)


def oracle_analytic(oracle, src, tgt, x, jac_mode, cov, loss, dtype=np.float64):
    H, b, s = oracle.p2p_linearize(src, tgt, x, cost_class=ob.ANALYTIC_DYN, layout=LAYOUT[jac_mode],
                                   cov=cov, loss_kind=0 if loss is None else 1,
                                   loss_param=0.0 if loss is None else loss, dtype=dtype)
    return np.asarray(H, dtype=np.float64), np.asarray(b, dtype=np.float64), float(s)


@pytest.mark.parametrize("jac_mode", [0, 1, 3, 4])
def test_sensor_scene_two_restatements_agree(oracle, jac_mode):
    src, tgt, x = ds.scene_pair("sensor", N)
    for cov in (None, COV_GENERAL):
        for loss in losses_of("sensor"):
            ref = hp.p2p_linearize_ld(src, tgt, x, jac_mode, cov=cov, loss=loss)
            got = oracle_analytic(oracle, src, tgt, x, jac_mode, cov, loss)
            eH, eb, ec = hp.lm_scaled_err(got, ref)
            assert eH <= 1e-12 and eb <= 1e-12 and ec <= 1e-12, (cov is not None, loss, eH, eb, ec)
            # ... and norm-wise, the metric of tests/test_gpu_parity.py
            H, b, _ = (np.asarray(v, dtype=np.float64) for v in ref)
            assert np.abs(got[0] - H).max() <= 1e-12 * np.abs(H).max()
            assert np.abs(got[1] - b).max() <= 1e-12 * np.abs(b).max()
    c = hp.p2p_cost_ld(src, tgt, x)
    assert abs(oracle.p2p_cost(src, tgt, x) - float(c)) <= 1e-12 * float(c)


@pytest.mark.parametrize("scene", [s for s in ds.SCENES if s != "sensor"])
def test_oracle_distance_from_extended_precision_is_pinned(oracle, scene):
    src, tgt, x = ds.scene_pair(scene, N)
    eb_bound, ec_bound = 4 * EB_MEASURED[scene], 4 * EC_MEASURED[scene]
    assert eb_bound <= 4 * 2.1e-7 and (scene in ("utm_to_local", "utm_to_local_7e6", "local_to_map") or
                                       eb_bound <= 4 * 6e-12)  # never looser than the quoted figures
    for jac_mode in (0, 1, 3, 4):
        for cov in (None, COV_GENERAL):
            for loss in losses_of(scene):
                ref = hp.p2p_linearize_ld(src, tgt, x, jac_mode, cov=cov, loss=loss)
                eH, eb, ec = hp.lm_scaled_err(oracle_analytic(oracle, src, tgt, x, jac_mode, cov, loss), ref)
                print(scene, jac_mode, cov is not None, loss, "eH %.2e eb %.2e ec %.2e" % (eH, eb, ec))
                assert eH <= 1e-10, (jac_mode, cov is not None, loss, eH)
                assert eb <= eb_bound, (jac_mode, cov is not None, loss, eb, eb_bound)
                assert ec <= ec_bound, (jac_mode, cov is not None, loss, ec, ec_bound)


def test_scene_residuals_are_a_fraction_of_the_cloud():
    """The scenes are what the table says: residual size, where the pose sends the cloud."""
    for scene, sc in ds.SCENES.items():
        src, tgt, x = ds.scene_pair(scene, 513)
        R, t = hp.transform_from_x(x)
        r = np.asarray(src.astype(np.longdouble) @ R.T + t - tgt, dtype=np.float64)
        size = max(sc["box"])
        rms = np.sqrt((r * r).sum(axis=1).mean())
        assert 0.01 * size <= rms <= 0.2 * size or 0.1 <= rms <= 1.5, (scene, rms)
    src, tgt, x = ds.scene_pair("utm_to_local", 513)
    assert np.abs(tgt).max() < 20 and np.abs(x[:3]).max() > 5e5
    src, tgt, x = ds.scene_pair("local_to_map", 513)
    assert np.abs(src).max() <= 10 and np.abs(x[:3] - np.array([1e6, 7e5, 1e4])).max() < 20


def test_lm_scaled_err_reads_what_the_norm_wise_metric_misses():
    """A translation block wrong by 100 % under a 1e4 m offset: 1e-8 norm-wise, 1 in LM's scale."""
    src, tgt, x = ds.scene_pair("map", 513)
    H, b, s = (np.asarray(v, dtype=np.float64) for v in hp.p2p_linearize_ld(src, tgt, x, 0))
    bad = H.copy()
    bad[0, 0] *= 2.0
    assert np.abs(bad - H).max() / np.abs(H).max() < 1e-6
    eH, eb, ec = hp.lm_scaled_err((bad, b, s), (H, b, s))
    assert eH == pytest.approx(1.0) and eb == 0.0 and ec == 0.0


# ---- the long-double Levenberg-Marquardt loop (highprec.lm_minimize_ld) --------------------------------
def oracle_minimize(oracle, case, src, tgt, lm_iter, k, dtype=np.float64):
    return oracle.p2p_minimize(src, tgt, case.x0, cost_class=ob.ANALYTIC_DYN, layout=ob.LAYOUT_ROW_MAJOR,
                               max_iter=k, lm_iter=lm_iter, cov=case.cov, loss_kind=0 if case.loss is None else 1,
                               loss_param=case.loss or 0.0, dtype=dtype)


@pytest.mark.parametrize("row", range(len(lc.ISSUE_TABLE)))
def test_long_double_lm_loop_takes_the_oracles_decisions(oracle, row):
    """Two statements of levenberg_marquadt_dyn.cpp:34-119 that share no code — the oracle's in double, the
    trace-keeping one in long double — on the starts where trials are rejected and inner loops run out: the
    same status, count and exhausted iterations at every truncation, x within 1e-9 (measured: 5e-14, so no
    truncation is left out as too sensitive: the bar for that is 1e-10)."""
    case, exhausted = lc.ISSUE_TABLE[row]
    src, tgt = case.data()
    for lm_iter in (1, 2, 3, 5):
        res = hp.lm_minimize_ld(src, tgt, case.x0, 0, max_iter=15, lm_iter=lm_iter)
        if lm_iter in exhausted:
            assert hp.exhausted_iterations(res) == exhausted[lm_iter], (case.name, lm_iter)
        previous, unchanged = case.x0, []
        for k in range(1, 16):
            xr, status, iters = oracle_minimize(oracle, case, src, tgt, lm_iter, k)
            x, s, i, _, _ = hp.truncate(res, k)
            assert (s, i) == (status, iters), (case.name, lm_iter, k, s, i, status, iters)
            err = np.abs(x - xr).max() / max(1.0, np.abs(xr).max())
            assert err <= 1e-10, (case.name, lm_iter, k, err)  # (1e-9 is the bar; 1e-10: fit to judge a GPU by)
            if iters == k and np.array_equal(xr, previous):
                unchanged.append(k)
            previous = xr
        # the oracle's own exhausted iterations: those that left its x where it was
        assert unchanged == [k for k in hp.exhausted_iterations(res)], (case.name, lm_iter, unchanged)


def test_every_case_of_the_rejection_table_has_its_margins_and_the_oracles_decisions(oracle):
    """What tests/test_gpu_lm_rejections.py judges the device by: every row's long-double trace keeps |rho| >=
    1e-3, and max|delta| of rejected trials and all costs a factor 10 from their thresholds; the oracle (with
    the row's covariance and loss) decides the same; and the rows the GPU tests need are there."""
    rows = lc.CASES + (lc.WELL, lc.ROLL_5_TILES, lc.TUMBLE_5_TILES, lc.ROLL_TWO_COSTS) + lc.NAN_ROWS
    for case in rows:
        src, tgt = case.data()
        for lm_iter in case.lm_iters:
            res = case.reference(lm_iter)
            m = hp.assert_decision_margins(res[3], what=(case.name, lm_iter))
            print(case.name, lm_iter, "status", res[1], res[2], "exhausted", hp.exhausted_iterations(res), m)
            for k in range(1, case.kmax + 1):
                xr, status, iters = oracle_minimize(oracle, case, src, tgt, lm_iter, k)
                x, s, i, _, _ = hp.truncate(res, k)
                assert (s, i) == (status, iters), (case.name, lm_iter, k)
                assert np.abs(x - xr).max() <= 1e-10 * max(1.0, np.abs(xr).max()), (case.name, lm_iter, k)
    ex = lambda case, lm_iter: hp.exhausted_iterations(case.reference(lm_iter))
    assert ex(lc.ROLL, 1) == list(range(2, 16))                                  # all exhausted
    assert ex(lc.TUMBLE, 3) == [3, 4] and ex(lc.ROLL, 3) == [2, 3]               # two, then accepted steps
    assert lc.SMALL_DELTA.reference(8)[1] == hp.SMALL_DELTA and ex(lc.SMALL_DELTA, 8) == [3]
    assert lc.GM_OUTLIERS.loss and len(ex(lc.GM_OUTLIERS, 3)) >= 2
    assert lc.GENERAL_COV.cov is not None and ex(lc.GENERAL_COV, 3) == [1, 2]
    # the sizes the launch-per-point loop and the two-cost finalize run at keep the pattern
    assert ex(lc.ROLL_5_TILES, 1) == list(range(2, 15)) and ex(lc.ROLL_5_TILES, 3) == [2, 3]
    assert ex(lc.TUMBLE_5_TILES, 1) == list(range(3, 12))
    assert ex(lc.ROLL_TWO_COSTS, 1) == list(range(2, 15)) and ex(lc.ROLL_TWO_COSTS, 3) == [2, 3]
    # fp32: the float oracle and the long-double loop over float inputs decide alike on the two fp32 rows
    for case in (lc.ROLL, lc.TUMBLE):
        src, tgt = case.data(np.float32)
        for lm_iter in (1, 3):
            res = case.reference(lm_iter, dtype=np.float32)
            hp.assert_decision_margins(res[3], np.float32, what=(case.name, lm_iter, "fp32"))
            for k in range(1, 16):
                _, status, iters = oracle_minimize(oracle, case, src, tgt, lm_iter, k, dtype=np.float32)
                assert hp.truncate(res, k)[1:3] == (status, iters), (case.name, lm_iter, k)


def lambda_rounding(cases, jac_mode=0, states=None):
    """the largest relative difference of lambda, over every state (or the first `states`) of every row, between
    the loop in long double and the same loop in double"""
    worst = 0.0
    for case in cases:
        for lm_iter in case.lm_iters:
            ld = case.reference(lm_iter, jac_mode=jac_mode)
            dbl = case.reference(lm_iter, jac_mode=jac_mode, work=np.float64)
            last = len(ld[4]) - 1 if states is None else states
            if states is None:
                assert len(ld[4]) == len(dbl[4]) and ld[1:3] == dbl[1:3], (case.name, lm_iter)
            for a, b in zip(ld[4][1:last + 1], dbl[4][1:last + 1]):
                worst = max(worst, float(abs(a["lam"] - hp.LD(b["lam"])) / a["lam"]))
    return worst


def test_lambda_bounds_are_ten_times_what_double_rounding_does_to_the_loop():
    rows = lc.CASES + (lc.WELL, lc.ROLL_5_TILES, lc.TUMBLE_5_TILES, lc.ROLL_TWO_COSTS) + lc.NAN_ROWS
    worst = lambda_rounding(rows)
    worst_fd = lambda_rounding(lc.NAN_ROWS, jac_mode=2, states=lc.FD_KMAX)
    print("lambda: long double against double, worst relative difference %.3e, forward differences %.3e"
          % (worst, worst_fd))
    assert worst <= lc.LAMBDA_MEASURED and lc.LAMBDA_RTOL == max(10 * lc.LAMBDA_MEASURED, 1e-12)
    assert worst_fd <= lc.LAMBDA_MEASURED_FD and lc.LAMBDA_RTOL_FD == max(10 * lc.LAMBDA_MEASURED_FD, 1e-12)
    for case in lc.NAN_ROWS:  # the truncations the forward-difference legs are judged at have their margins
        trace = [t for t in case.reference(3, jac_mode=2)[3] if t["it"] < lc.FD_KMAX]
        hp.assert_decision_margins(trace, what=(case.name, "forward differences"))
