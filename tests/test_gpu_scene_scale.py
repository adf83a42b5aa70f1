"""Point2point sweeps at the scales registration is run at, judged in the coordinates LM solves in.

Every other parity test draws src ~ U[0,10]^3 under the fixture pose and compares norm-wise
(max|dH| / max|H|).  Neither shows what a reduction kernel gets wrong on real scenes: with the cloud
1e4 m from the origin max|H| is 1e8 x the translation block, so the norm-wise 1e-6 lets H_tt be wrong
by 100 %; and the moments evaluation (AUTO's default) contracts raw moments with a basis whose terms
grow with the coordinates and can cancel.  Here the scenes of tests/datasets.py SCENES (site, map and
UTM frames, a source and a target in different frames, a millimetre object, a flat wall) are swept in
every evaluation, and compared with the 80-bit sums of tests/highprec.py under lm_scaled_err — the
error of H after the Jacobi scaling under which H + lambda diag(H) is invariant, where max|H| = 1
and the project's 1e-6 bar means what it says.

Bounds.  eH <= 1e-6.  For b and the cost max(1e-6, 8 x e_oracle), e_oracle being the same error of
the CPU oracle's fp64 sums on the same inputs, computed here: r = R p + t - q is itself only known
to eps |R p + t| / |r|, so at a 1e6 offset no fp64 evaluation can be asked for more, and the kernel
may be 8 x further from the truth than the reference's own arithmetic is, no more
(tests/test_highprec_reference.py pins e_oracle).  Each case is a few thousand points.
"""
import functools

import numpy as np
import pytest

from tests import datasets as ds
from tests import highprec as hp
from tests import oracle_binding as ob
from tests.test_gpu_parity import REL, check, fd_tolerance, oracle_ref

pytestmark = pytest.mark.gpu

AUTO, LITERAL, MOMENTS, MOMENTS_ALWAYS = 0, 1, 2, 3
COV_GENERAL = np.array([[2.0, 0.7, -0.1], [0.3, 0.5, 0.9], [-0.4, 0.2, 1.5]])  # test_p2p_loss_and_covariance
LAYOUT = {0: ob.LAYOUT_ROW_MAJOR, 1: ob.LAYOUT_TST, 3: ob.LAYOUT_LEFT, 4: ob.LAYOUT_RIGHT}
F32_BAR = 2e-4  # test_p2p_float32


def losses_of(scene):
    return (None, 1e-6, 1.0) if scene == "mm" else (None, 0.5)


def covs():
    return (None, COV_GENERAL)


@functools.lru_cache(maxsize=None)
def scene(name, n, dtype=np.float64, rot=None, about_origin=False):
    return ds.scene_pair(name, n, dtype=dtype, rot=rot, about_origin=about_origin)


@functools.lru_cache(maxsize=None)
def reference(name, n, jac_mode, general_cov, loss, dtype=np.float64):
    """(80-bit H, b, cost; the oracle's own lm_scaled_err against them), once per case."""
    src, tgt, x = scene(name, n, dtype)
    cov = COV_GENERAL if general_cov else None
    ref = hp.p2p_linearize_ld(src, tgt, x, jac_mode, cov=cov, loss=loss, dtype=dtype)
    H, b, s = ob.load().p2p_linearize(src, tgt, x, cost_class=ob.ANALYTIC_DYN, layout=LAYOUT[jac_mode], cov=cov,
                                      loss_kind=0 if loss is None else 1,
                                      loss_param=0.0 if loss is None else loss, dtype=dtype)
    return ref, hp.lm_scaled_err((H, b, s), ref)


@functools.lru_cache(maxsize=None)
def cost_reference(name, n, dtype=np.float64):
    src, tgt, x = scene(name, n, dtype)
    ref = hp.p2p_cost_ld(src, tgt, x, dtype=dtype)
    got = ob.load().p2p_cost(src, tgt, x, dtype=dtype)
    return ref, float(abs(np.longdouble(got) - ref) / ref)


def set_case(mo, cost, cov, loss):
    cost.set_covariance(cov)
    cost.set_loss(mo.LOSS_NONE if loss is None else mo.LOSS_GEMAN_MCCLURE, 0.0 if loss is None else loss)


@pytest.mark.parametrize("variant", [AUTO, LITERAL, MOMENTS])
@pytest.mark.parametrize("jac_mode", [0, 1, 3, 4])
@pytest.mark.parametrize("n", ds.SCENE_SIZES)
@pytest.mark.parametrize("name", list(ds.SCENES))
def test_analytic_modes_at_scene_scale(hip_lib, oracle, name, n, jac_mode, variant):
    mo = hip_lib
    src, tgt, x = scene(name, n)
    cost = mo.Point2PointCost(src, tgt)
    cost.set_kernel_variant(variant)
    failures = []
    for cov in covs():
        for loss in losses_of(name):
            set_case(mo, cost, cov, loss)
            ref, (oH, ob_, oc) = reference(name, n, jac_mode, cov is not None, loss)
            eH, eb, ec = hp.lm_scaled_err(cost.linearize(x, jac_mode), ref)
            print("%s n=%d mode %d variant %d cov %d loss %s: eH %.2e eb %.2e ec %.2e (oracle %.1e %.1e %.1e)"
                  % (name, n, jac_mode, variant, cov is not None, loss, eH, eb, ec, oH, ob_, oc))
            if not (eH <= REL and eb <= max(REL, 8 * ob_) and ec <= max(REL, 8 * oc)):
                failures.append((cov is not None, loss, eH, eb, ec, ob_, oc))
            # the cost-only sweep right after (answered from the linearization sweep where the cost
            # speculates, by its own sweep otherwise)
            cref, coracle = cost_reference(name, n)
            c = cost.compute_cost(x)
            ecost = float(abs(np.longdouble(c) - cref) / cref)
            if not ecost <= max(REL, 8 * coracle):
                failures.append(("cost", cov is not None, loss, ecost, coracle))
    cost.set_speculation(False)
    cref, coracle = cost_reference(name, n)
    ecost = float(abs(np.longdouble(cost.compute_cost(x)) - cref) / cref)
    cost.close()
    assert ecost <= max(REL, 8 * coracle), ("cost sweep", ecost, coracle)
    assert not failures, failures


@pytest.mark.parametrize("variant", [AUTO, LITERAL])
@pytest.mark.parametrize("jac_mode", [0, 3, 4])
@pytest.mark.parametrize("n", ds.SCENE_SIZES)
@pytest.mark.parametrize("name", ["sensor", "site", "mm", "wall"])
def test_float32_at_scene_scale(hip_lib, oracle, name, n, jac_mode, variant):
    """The fp32 instantiation on the scenes fp32 can hold, against the 80-bit sums over the
    fp32-rounded inputs.  Bound on all three errors: max(2e-4, 8 x e_float_oracle) — 2e-4 is the
    fp32 bar of test_p2p_float32, e_float_oracle the oracle run in float on the same inputs."""
    mo = hip_lib
    f32 = np.float32
    src, tgt, x = scene(name, n, f32)
    cost = mo.Point2PointCost(src, tgt, dtype=f32)
    cost.set_kernel_variant(variant)
    failures = []
    for cov in covs():
        for loss in losses_of(name):
            set_case(mo, cost, None if cov is None else cov.astype(f32), loss)
            ref, oracle_err = reference(name, n, jac_mode, cov is not None, loss, f32)
            err = hp.lm_scaled_err(cost.linearize(x, jac_mode), ref)
            print("f32 %s n=%d mode %d variant %d cov %d loss %s: eH %.2e eb %.2e ec %.2e (oracle %.1e %.1e %.1e)"
                  % ((name, n, jac_mode, variant, cov is not None, loss) + err + oracle_err))
            if not all(e <= max(F32_BAR, 8 * o) for e, o in zip(err, oracle_err)):
                failures.append((cov is not None, loss, err, oracle_err))
    cref, coracle = cost_reference(name, n, f32)
    ecost = float(abs(np.longdouble(cost.compute_cost(x)) - cref) / cref)
    cost.close()
    assert ecost <= max(F32_BAR, 8 * coracle), ("cost sweep", ecost, coracle)
    assert not failures, failures


FD_CASES = [(name, a, False) for name in ("sensor", "site", "map", "local_to_map") for a in (0.02, 0.3, 1.0)] + \
           [(name, a, True) for name in ("sensor", "site", "map") for a in (0.0, 0.02, 0.3, 1.0)]


@pytest.mark.parametrize("variant", [LITERAL, AUTO, MOMENTS, MOMENTS_ALWAYS])
@pytest.mark.parametrize("name,a,small_t", FD_CASES)
def test_forward_differences_at_scene_scale(hip_lib, oracle, name, a, small_t, variant):
    """Forward differences: the reference's arithmetic is the definition, so the oracle's numeric
    cost class stays the comparand, under the existing check at REL and under lm_scaled_err at REL;
    rotation components of the pose +-a.  Two poses per scene: the one that maps the source's centroid
    onto the target's (in a far frame its translation (I - R) c is as large as the frame's offset, and so
    are its steps), and, small_t, a turn about the frame's origin with a translation of a fraction of a
    metre — the far same-frame case, where the steps are small and rho is not; a = 0 there is the fixed
    step sqrt(eps) on every rotation component.

    The literal sweep repeats the reference's per-point quotient.  The moments form leaves out the
    reference's cancellation error eps |R p + t| / h_j, h_j = sqrt(eps) |x_j|: that distance was
    measured as 2e-8 / |x_j| on clouds with |R p + t| = 10..30 (fd_tolerance) and is linear in
    |R p + t|, so AUTO and MOMENTS have to evaluate literally below a threshold that grows with the
    scene, and MOMENTS_ALWAYS (a measurement switch) keeps fd_tolerance's bound x rho / 30,
    rho = max |R p + t| of the scene.  On the small_t poses that cell is held only to the worst case
    derived below (2.8e-4 on site, 5e-3 and more on map, 2-6 x what it measures): it says that the
    moments differ from the reference by no more than the reference's own noise, not that they are at
    parity — parity on those poses is what the LITERAL, AUTO and MOMENTS cells assert, at REL.
    Measured figures: profiles/NOTES.md "Scene scale"."""
    mo = hip_lib
    n = ds.SCENE_SIZES[0]
    src, tgt, x = scene(name, n, np.float64, (a, -a, a), small_t)
    tol = REL
    if variant == MOMENTS_ALWAYS:
        R, t = hp.transform_from_x(x)
        rho = float(np.sqrt(((src.astype(np.longdouble) @ R.T + t) ** 2).sum(axis=1)).max())
        tol = max(REL, fd_tolerance(x, variant) * rho / 30.0)
        if small_t:
            # fd_tolerance's figure was measured on rotation columns, which grow with |p| as the noise
            # does.  With a small translation far from the origin the unit translation columns carry it:
            # R p + t is three roundings at magnitude rho, 1.5 eps rho per evaluation, two evaluations
            # over h_j = sqrt(eps) |x_j| (x_j = 0: |x_j| = 1) against a column of 1 — the reference's
            # own noise, which the moments lack, is at most 3 sqrt(eps) rho / min |x_j|.
            ax = np.abs(x)
            tol = max(tol, 3.0 * np.sqrt(np.finfo(np.float64).eps) * rho / np.where(ax > 0, ax, 1.0).min())
    cost = mo.Point2PointCost(src, tgt)
    cost.set_kernel_variant(variant)
    for cov, loss in ((None, None), (COV_GENERAL, 0.5)):
        set_case(mo, cost, cov, loss)
        want = oracle_ref(oracle, src, tgt, x, 2, cov=cov, loss_kind=0 if loss is None else 1,
                          loss_param=0.0 if loss is None else loss)
        got = cost.linearize(x, 2)
        err = hp.lm_scaled_err(got, want)
        print("fd %s a=%g small_t %d variant %d cov %d: eH %.2e eb %.2e ec %.2e (tol %.1e)"
              % ((name, a, small_t, variant, cov is not None) + err + (tol,)))
        check(got, want, tol=tol)
        assert max(err) <= tol, (cov is not None, err, tol)
    cost.close()


def host_lm_left(mo, cost, x0, max_iter=15, lm_iter=3):
    """The reference's loop with x (+) delta composed on the left (mopt_se3_plus), over the
    blocking calls of one HIP cost in MOPT_JAC_ANALYTIC_LEFT."""
    x = np.array(x0, dtype=np.float64)
    lam, eps = -1.0, np.finfo(np.float64).eps
    for it in range(max_iter):
        H, b, y0 = cost.linearize(x, mo.JAC_ANALYTIC_LEFT)
        if abs(y0) < 8 * eps:
            return x, 0
        if lam < 0:
            lam = 1e-9 * np.abs(np.diag(H)).max()
        nu = 2.0
        for _ in range(lm_iter):
            Hl = np.tril(H) + np.tril(H, -1).T
            delta = np.linalg.solve(Hl + lam * np.diag(np.diag(H)), -b)
            xi = mo.capi.se3_plus(x, delta)
            yi = cost.compute_cost(xi)
            if np.isnan(yi):
                return x, 3
            rho = (y0 - yi) / delta.dot(lam * delta - b)
            if rho < 0:
                if np.abs(delta).max() < np.sqrt(eps):
                    return x, (0 if abs(yi) < 8 * eps else 2)
                lam *= nu
                nu *= 2
                continue
            x = xi
            lam *= max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3)
            break
    return x, 1


def test_device_resident_solve_utm_to_local(hip_lib):
    """The device-resident loop builds its basis itself (lm_device.hpp): a LEFT-mode solve with the
    manifold update on the UTM scan, default evaluation, against the host loop over the same cost's
    literal sweeps."""
    mo = hip_lib
    src, tgt, x0 = scene("utm_to_local", ds.SCENE_SIZES[0])
    cost = mo.Point2PointCost(src, tgt)
    x, rep = mo.capi.lm_minimize([cost], [mo.JAC_ANALYTIC_LEFT], x0, manifold=True)
    cost.set_kernel_variant(mo.KERNEL_LITERAL)
    cost.set_speculation(False)
    xh, status = host_lm_left(mo, cost, x0)
    cost.close()
    cost_host = float(hp.p2p_cost_ld(src, tgt, xh))
    cost_device = float(hp.p2p_cost_ld(src, tgt, x))
    print("device", x, rep, "host", xh, status, "dx", np.abs(x - xh).max(), "costs", cost_device, cost_host)
    assert rep["status"] == status, (rep, status)
    assert np.abs(x - xh).max() <= 1e-9 * max(1.0, np.abs(xh).max()), (x, xh)
    # that bound is 1e-3 on a translation of 1e6: the rotation, which is O(1), and the minimum reached
    # (80-bit sums at both end points) say whether the device's H was the host's
    assert np.abs(x[3:] - xh[3:]).max() <= 1e-9, (x[3:], xh[3:])
    assert abs(cost_device - cost_host) <= 1e-9 * cost_host, (cost_device, cost_host)
