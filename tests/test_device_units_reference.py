"""Keeps tests/device_units_reference.py honest, without a GPU: the long-double references and the
system generators the GPU tests of the LM step's device functions (tests/test_gpu_device_units.py)
judge by, and the two constants their bounds are built on, measured here and written down there."""
import numpy as np
import pytest

from tests import device_units_reference as du

LD = du.LD


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_unpivoted_restatement_constant(dtype):
    """Unpivoted LDL^T restated in numpy in the type itself against the long-double solve over the SPD
    family: max |x - x_ld|_inf / (|x_ld|_inf eps cond_2(A)) stays <= 1.5, and C_REF covers it."""
    rng = np.random.default_rng(20240)
    eps, lam = du.eps_of(dtype), 1e-4
    worst = {}
    for n in (2, 4, 6):
        for cond in du.SPD_CONDS[dtype]:
            w = 0.0
            for _ in range(40):
                H, b = du.spd_system(n, cond, dtype, rng)
                ref = du.solve_ld(H, b, lam)
                got = du.unpivoted_ldlt(H, b, lam, dtype).astype(LD)
                w = max(w, float(np.abs(got - ref).max() / (np.abs(ref).max() * eps * du.cond2(H, lam))))
            worst[n, cond] = w
    print(np.dtype(dtype), {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.5, worst
    assert max(worst.values()) <= du.C_REF[dtype] <= 1.5, (worst, du.C_REF[dtype])


def _pivoted_families(n, dtype, rng):
    """(name, H, b, lam) of the families the pivoted solve is run on, for one n."""
    out = []
    for i in range(4):
        lam = (0.0, 1e-4)[i % 2]
        out.append(("exchanged", *du.exchanged_system(n, dtype, rng, lam), lam))
        out.append(("indefinite", *du.indefinite_system(n, dtype, rng), lam))
    return out


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_host_pivoted_ldlt_meets_the_bound(dtype, tmp_path):
    """dense::PivotedLDLT (the host half of tests/cpp/device_units, which needs no device) against the
    long-double solve on the exchanged and indefinite families, at the bound the device is held to:
    8 max(C_REF, 1) eps cond_2 |x_ld|_inf."""
    rng = np.random.default_rng(31)
    eps, worst = du.eps_of(dtype), 0.0
    for n in (1, 2, 3, 4, 6, 7, 8, 9, 12, 15, 16):
        fam = _pivoted_families(n, dtype, rng)
        rec = du.pack_systems([(H, b, lam) for _, H, b, lam in fam], dtype, 0.0)
        got = du.run("host_pivoted", dtype, n, rec, str(tmp_path), n)
        for (name, H, b, lam), x in zip(fam, got):
            ref = du.solve_ld(H, b, lam)
            ratio = float(np.abs(x.astype(LD) - ref).max() / (np.abs(ref).max() * eps * du.cond2(H, lam)))
            worst = max(worst, ratio)
            assert ratio <= 8 * max(du.C_REF[dtype], 1.0), (name, n, ratio)
    print(np.dtype(dtype), "host PivotedLDLT worst ratio", worst)


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_host_se3_updates_constant(dtype):
    """mo.capi.se3_plus / se3_plus_right (host so3.hpp) against se3_plus_ld over se3_grid: the worst
    rotation error in units of se3_unit is what C_SE3_REF records; the translation stays within
    4 eps (|x_t|_inf + |delta_t|_inf)."""
    import moptimizer_0_amd as mo
    eps = du.eps_of(dtype)
    for right, host in ((False, mo.capi.se3_plus), (True, mo.capi.se3_plus_right)):
        grid = du.se3_grid(dtype, right=right)
        assert 65 <= len(grid) <= 4000, len(grid)
        worst_w = worst_t = 0.0
        branches = set()
        for x, d, ref, info in grid:
            assert du.se3_case_is_clear(info, dtype), (x, d, info)
            got = host(x, d, dtype=dtype).astype(LD)
            branches.add((bool(info["theta_x"] > 10 * eps), bool(info["theta_d"] > 10 * eps), info["acos"]))
            worst_w = max(worst_w, float(np.abs(got[3:] - ref[3:]).max() / du.se3_unit(info, dtype)))
            scale = np.abs(x[:3]).max().astype(LD) + np.abs(d[:3]).max().astype(LD)
            if scale > 0:
                worst_t = max(worst_t, float(np.abs(got[:3] - ref[:3]).max() / (eps * scale)))
        print(np.dtype(dtype), "right" if right else "left", len(grid), "rotation", worst_w, "translation", worst_t)
        # every combination of the three branch points but the impossible one (two identities composing
        # to an angle above 1e-3) is met
        assert len(branches) == 7 and (False, False, True) not in branches, branches
        assert worst_w <= du.C_SE3_REF[dtype], (worst_w, du.C_SE3_REF[dtype])
        assert worst_t <= 4.0, worst_t


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_generators_meet_their_own_conditions(dtype):
    """The threshold, exchange and SPD generators under the seeds the GPU tests use: they assert
    their conditions themselves; here also that the threshold rows land on both sides for every k."""
    from tests import test_gpu_device_units as gpu
    for n in (2, 4, 6):
        fam = gpu.positive_families(dtype, n)
        flags = [(k, above) for k, above in fam["threshold_cases"]]
        assert set(flags) == {(k, a) for k in range(1, n) for a in (False, True)}
        assert len(fam["systems"]) >= 65
    for nmax, n in gpu.PIVOTED_CELLS:
        assert len(gpu.pivoted_families(dtype, nmax, n)["systems"]) >= 65


def test_predicate_refuses_what_the_device_must_refuse():
    """The long-double predicate on the refusal rows: zero row / column, negative diagonal, NaN."""
    rng = np.random.default_rng(5)
    for dtype in du.DTYPES:
        H, b = du.spd_system(4, 10.0, dtype, rng)
        assert du.positive_predicate_ld(H, 1e-4, dtype)[0]
        for z in range(4):
            Hz = H.copy()
            Hz[z, :] = 0
            Hz[:, z] = 0
            assert not du.positive_predicate_ld(Hz, 1e-4, dtype)[0]
            Hn = H.copy()
            Hn[z, z] = -Hn[z, z]
            assert not du.positive_predicate_ld(Hn, 1e-4, dtype)[0]
        for i in range(4):
            for j in range(i + 1):
                Hq = H.copy()
                Hq[i, j] = np.nan
                assert not du.positive_predicate_ld(Hq, 1e-4, dtype)[0], (i, j)
        Hu = H.copy()
        Hu[np.triu_indices(4, 1)] = np.nan  # the strict upper triangle is never read
        assert du.positive_predicate_ld(Hu, 1e-4, dtype)[0]
