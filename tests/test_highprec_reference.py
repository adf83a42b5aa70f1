"""Guards the two references the scene-scale GPU tests judge by (tests/test_gpu_scene_scale.py):
the 80-bit statement of tests/highprec.py and the CPU oracle are written independently, so on the
control scene they must agree to fp64 summation rounding; on every other scene the oracle's own
distance from the 80-bit sums — which the GPU tests take as the kernel's allowance, times 8 — is
pinned, so that allowance cannot grow unnoticed.  No GPU."""
import numpy as np
import pytest

from tests import datasets as ds
from tests import highprec as hp
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
