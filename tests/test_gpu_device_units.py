"""The arithmetic under the device-resident LM step, one call at a time: solveDampedPositive,
solveDamped, se3Plus, se3PlusRight, rigidFrom6DOF, forwardStep and fastReciprocal of
csrc/lm_device.hpp, called unchanged by the thin kernels of tests/cpp/device_units.hip (a fresh
child process per op) and judged against the long-double references of
tests/device_units_reference.py.  An end-to-end LM solve is a weak detector for these: a slightly
wrong step is usually still a descent step.

Every bound below is written from the reference's own measured constant (C_REF, C_SE3_REF) and the
precision of the type; the worst ratios seen on an MI355X are recorded in the docstrings."""
import functools
import tempfile

import numpy as np
import pytest

from tests import device_units_reference as du
from tests import highprec as hp

pytestmark = pytest.mark.gpu

LD = du.LD
SENTINEL = -12345.6875  # exact in both types; nothing any system here solves to
LAMBDAS = (0.0, 1e-4, 2.0, 2.0 ** 10, 2.0 ** 40)  # the loop grows lambda by powers of two
PIVOTED_CELLS = [(8, n) for n in (1, 2, 3, 4, 6, 7, 8)] + [(16, n) for n in (9, 12, 15, 16)] + [(16, 6)]


def _seed(dtype, *key):
    return [20250, np.dtype(dtype).itemsize, *key]


def _nan_upper(H):
    H = H.copy()
    H[np.triu_indices(H.shape[0], 1)] = np.nan
    return H


def _bound(dtype):
    return 8 * max(du.C_REF[dtype], 1.0)


def _ratio(got, ref, H, lam, dtype):
    """|got - ref|_inf / (eps cond_2(A) |ref|_inf)"""
    return float(np.abs(got.astype(LD) - ref).max() / (du.eps_of(dtype) * du.cond2(H, lam) * np.abs(ref).max()))


# ---- solveDampedPositive -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def positive_families(dtype, n):
    """Every system solveDampedPositive<dtype, n> is run on, in one launch of more than one wave:
    kinds[i] names the family of systems[i]; expected[i] is the long-double predicate."""
    rng = np.random.default_rng(_seed(dtype, n))
    lams = [float(np.dtype(dtype).type(l)) for l in LAMBDAS]
    systems, kinds, threshold_cases = [], [], []
    for cond in du.SPD_CONDS[dtype]:
        for _ in range(3):
            H, b = du.spd_system_clear_of_floor(n, cond, dtype, rng, lams)
            for lam in lams:
                systems.append((H, b, lam))
                kinds.append("spd")
    for H, b, lam in [s for s, k in zip(systems, kinds) if k == "spd"]:
        systems.append((_nan_upper(H), b, lam))
        kinds.append("spd_nan_upper")
    for k in range(1, n):
        for above in (False, True):
            for _ in range(3):
                H, b, _ = du.threshold_system(n, k, above, dtype, rng)
                systems.append((H, b, 0.0))
                kinds.append("threshold")
                threshold_cases.append((k, above))
    H0, b0 = du.spd_system(n, 10.0, dtype, rng)
    for z in range(n):
        H = H0.copy()
        H[z, :] = 0
        H[:, z] = 0
        systems.append((H, b0, lams[1]))
        kinds.append("zero_row")
        H = H0.copy()
        H[z, z] = -H[z, z]
        systems.append((H, b0, lams[1]))
        kinds.append("negative_diagonal")
    for i in range(n):
        for j in range(i + 1):
            H = H0.copy()
            H[i, j] = np.nan
            systems.append((H, b0, lams[1]))
            kinds.append("nan")
    expected = [du.positive_predicate_ld(H, lam, dtype)[0] for H, b, lam in systems]
    return dict(systems=systems, kinds=kinds, threshold_cases=threshold_cases, expected=expected)


@functools.lru_cache(maxsize=None)
def _run_positive(dtype, n):
    fam = positive_families(dtype, n)
    with tempfile.TemporaryDirectory() as tmp:
        out = du.run("positive", dtype, n, du.pack_systems(fam["systems"], dtype, SENTINEL), tmp, n + 1)
    return fam, out[:, :n], out[:, n]


def _rows(fam, kind):
    return [i for i, k in enumerate(fam["kinds"]) if k == kind]


@pytest.mark.parametrize("n", (2, 4, 6))
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_positive_solve_on_the_spd_family(hip_lib, dtype, n):
    """flag true and |delta - x_ld|_inf <= 8 max(C_REF, 1) eps cond_2(A) |x_ld|_inf at every lambda.
    Worst ratio on an MI355X, of the 8 max(C_REF, 1) = 9.1 (fp64) / 8 (fp32) allowed:
    fp64 n=2 0.89, n=4 0.58, n=6 0.85; fp32 n=2 0.60, n=4 0.51, n=6 0.51 — the fused multiply-adds and
    reciprocals cost nothing measurable against the numpy restatement (C_REF: 1.13 / 0.60)."""
    fam, delta, flag = _run_positive(dtype, n)
    worst = 0.0
    for i in _rows(fam, "spd"):
        H, b, lam = fam["systems"][i]
        assert fam["expected"][i] and flag[i] == 1, (i, lam)
        worst = max(worst, _ratio(delta[i], du.solve_ld(H, b, lam), H, lam, dtype))
    print("positive spd", np.dtype(dtype), n, "worst ratio", worst)
    assert worst <= _bound(dtype), worst


@pytest.mark.parametrize("n", (2, 4, 6))
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_positive_solve_fallback_threshold(hip_lib, dtype, n):
    """The k-th pivot a factor 4 above or below kPivotFloor a_kk, k = 1 .. n - 1: the flag is the
    long-double predicate on every system, and a refusal leaves delta alone."""
    fam, delta, flag = _run_positive(dtype, n)
    rows = _rows(fam, "threshold")
    assert len(rows) == 6 * (n - 1)
    for i, (k, above) in zip(rows, fam["threshold_cases"]):
        assert fam["expected"][i] == above
        assert flag[i] == (1 if above else 0), (k, above, flag[i])


@pytest.mark.parametrize("n", (2, 4, 6))
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_positive_solve_refusals_and_sentinel(hip_lib, dtype, n):
    """A zero row / column at every index, a negative diagonal entry at every index and NaN at every
    position of the lower triangle are refused; wherever the flag is false — these and the
    threshold rows below the floor — all n entries of delta are the sentinel, bit for bit."""
    fam, delta, flag = _run_positive(dtype, n)
    for kind, count in (("zero_row", n), ("negative_diagonal", n), ("nan", n * (n + 1) // 2)):
        rows = _rows(fam, kind)
        assert len(rows) == count
        for i in rows:
            assert not fam["expected"][i] and flag[i] == 0, (kind, i)
    sentinel = np.full(n, SENTINEL, dtype=dtype).tobytes()
    refused = [i for i in range(len(flag)) if flag[i] == 0]
    # zero rows, negative diagonals, NaN positions, and the threshold rows below the floor
    assert len(refused) == n + n + n * (n + 1) // 2 + 3 * (n - 1)
    for i in range(len(flag)):
        assert flag[i] in (0, 1)
        assert (delta[i].tobytes() == sentinel) == (flag[i] == 0), (fam["kinds"][i], i, delta[i])
        assert bool(flag[i]) == fam["expected"][i], (fam["kinds"][i], i)


@pytest.mark.parametrize("n", (2, 4, 6))
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_positive_solve_reads_the_lower_triangle_only(hip_lib, dtype, n):
    """Each SPD system again with NaN over its strict upper triangle: the same flag, the same bits."""
    fam, delta, flag = _run_positive(dtype, n)
    plain, nan_upper = _rows(fam, "spd"), _rows(fam, "spd_nan_upper")
    assert len(plain) == len(nan_upper) >= 45
    for i, j in zip(plain, nan_upper):
        assert flag[i] == flag[j] == 1
        assert delta[i].tobytes() == delta[j].tobytes(), (i, delta[i], delta[j])


# ---- solveDamped ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pivoted_families(dtype, nmax, n):
    rng = np.random.default_rng(_seed(dtype, nmax, n))
    lam4 = float(np.dtype(dtype).type(1e-4))
    systems, kinds = [], []

    def add(kind, H, b, lam):
        systems.append((H, b, lam))
        kinds.append(kind)

    for i in range(14):
        lam = (0.0, lam4)[i % 2]
        add("exchanged", *du.exchanged_system(n, dtype, rng, lam), lam)
        add("indefinite", *du.indefinite_system(n, dtype, rng), lam)
    for i in range(12):
        add("ties", *du.tie_system(n, dtype, rng, coupled=i % 2 == 1), (0.0, lam4)[(i // 2) % 2])
    for H, b, lam in [s for s, k in zip(systems, kinds) if k in ("exchanged", "indefinite")]:
        add("nan_upper", _nan_upper(H), b, lam)
    for z in range(n):
        add("zero_row", *du.zero_row_system(n, z, dtype, rng), lam4)
    for _ in range(2):
        add("zero", *du.zero_system(n, dtype, rng), lam4)
    if nmax == 8 and n in (2, 4, 6):  # the systems of the unpivoted solve, for the comparison of the two
        fam = positive_families(dtype, n)
        for i in _rows(fam, "spd"):
            add("spd", *fam["systems"][i])
    return dict(systems=systems, kinds=kinds)


@functools.lru_cache(maxsize=None)
def _run_pivoted(dtype, nmax, n):
    fam = pivoted_families(dtype, nmax, n)
    with tempfile.TemporaryDirectory() as tmp:
        out = du.run("pivoted%d" % nmax, dtype, n, du.pack_systems(fam["systems"], dtype, SENTINEL), tmp, 2 * n)
    return fam, out[:, :n], out[:, n:]


@pytest.mark.parametrize("nmax,n", PIVOTED_CELLS)
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_pivoted_solve_is_the_host_statement_bit_for_bit(hip_lib, dtype, nmax, n):
    """solveDamped<S, NMAX> against dense::PivotedLDLT<S> run by the same program on the same damped
    matrix, over every family (exchanges at every step, indefinite, zero row, all zero, ties, NaN in
    the unread triangle): lm_device.hpp's claim "operation for operation the host statement"."""
    fam, device, host = _run_pivoted(dtype, nmax, n)
    assert len(fam["systems"]) >= 65
    for i, kind in enumerate(fam["kinds"]):
        assert device[i].tobytes() == host[i].tobytes(), (kind, i, device[i], host[i])
    plain = [i for i, k in enumerate(fam["kinds"]) if k in ("exchanged", "indefinite")]
    for i, j in zip(plain, _rows(fam, "nan_upper")):
        assert device[i].tobytes() == device[j].tobytes(), i


@pytest.mark.parametrize("nmax,n", PIVOTED_CELLS)
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_pivoted_solve_against_long_double(hip_lib, dtype, nmax, n):
    """8 max(C_REF, 1) eps cond_2 |x_ld|_inf on the non-singular families; a zero row's component is
    exactly 0 (the others meet the bound over the live rows); the zero matrix gives a zero delta.
    Worst ratio on an MI355X, of the 9.1 (fp64) / 8 (fp32) allowed: fp64 1.89 (n = 15), 1.63 (n = 6 under
    kMaxWideParams), <= 1.35 elsewhere; fp32 1.42 (n = 12, n = 15), <= 1.13 elsewhere."""
    fam, device, _ = _run_pivoted(dtype, nmax, n)
    worst = 0.0
    for i, kind in enumerate(fam["kinds"]):
        H, b, lam = fam["systems"][i]
        if kind in ("exchanged", "indefinite", "ties"):
            worst = max(worst, _ratio(device[i], du.solve_ld(H, b, lam), H, lam, dtype))
        elif kind == "zero_row":
            z = [k for k in range(n) if H[k, k] == 0]
            assert len(z) == 1 and device[i][z[0]] == 0, (i, device[i])
            if n > 1:
                worst = max(worst, _ratio(device[i], du.solve_ld(H, b, lam), H, lam, dtype))
        elif kind == "zero":
            assert np.all(device[i] == 0), device[i]
    print("pivoted", np.dtype(dtype), nmax, n, "worst ratio", worst)
    assert worst <= _bound(dtype), worst


@pytest.mark.parametrize("n", (2, 4, 6))
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_pivoted_and_unpivoted_solves_agree(hip_lib, dtype, n):
    """"The same pose, not the same bits": on the SPD family the two device solves differ by at most
    twice the bound either is held to."""
    fam_p, delta_p, flag = _run_positive(dtype, n)
    fam, device, _ = _run_pivoted(dtype, 8, n)
    rows_p, rows = _rows(fam_p, "spd"), _rows(fam, "spd")
    assert len(rows_p) == len(rows) >= 45
    worst = 0.0
    for i, j in zip(rows_p, rows):
        H, b, lam = fam["systems"][j]
        ref = du.solve_ld(H, b, lam)
        worst = max(worst, float(np.abs(delta_p[i].astype(LD) - device[j].astype(LD)).max() /
                                 (du.eps_of(dtype) * du.cond2(H, lam) * np.abs(ref).max())))
    print("pivoted vs unpivoted", np.dtype(dtype), n, "worst ratio", worst)
    assert worst <= 2 * _bound(dtype), worst


# ---- SE(3) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_se3_updates(hip_lib, dtype, right):
    """se3Plus / se3PlusRight over se3_grid (every case a factor 2 clear of each branch point):
    translation within 4 eps (|x_t|_inf + |delta_t|_inf), rotation vector within
    4 max(C_SE3_REF, 1) se3_unit.  Worst on an MI355X, in those units: rotation fp64 18.49
    (left) / 18.69 (right), fp32 33.41 / 29.07 — the host's own figures to every digit (C_SE3_REF: both
    worst cases sit at theta = pi - 0.12, where the error is that of the Log's conditioning, not of
    sincos / acos), of the 74.8 / 134 allowed; translation 1.30 / 0.47 (fp64), 1.37 / 0.45 (fp32) of 4."""
    grid = du.se3_grid(dtype, right=right)
    assert 65 <= len(grid) <= 4000
    with tempfile.TemporaryDirectory() as tmp:
        out = du.run("se3plusright" if right else "se3plus", dtype, 6,
                     np.stack([np.concatenate([x, d]) for x, d, _, _ in grid]), tmp, 6)
    eps = du.eps_of(dtype)
    worst_w = worst_t = 0.0
    for (x, d, ref, info), got in zip(grid, out):
        assert du.se3_case_is_clear(info, dtype), (x, d, info)
        got = got.astype(LD)
        err_t = np.abs(got[:3] - ref[:3]).max()
        scale = np.abs(x[:3]).max().astype(LD) + np.abs(d[:3]).max().astype(LD)
        assert err_t <= 4 * eps * scale, (x, d, err_t)
        if scale > 0:
            worst_t = max(worst_t, float(err_t / (eps * scale)))
        worst_w = max(worst_w, float(np.abs(got[3:] - ref[3:]).max() / du.se3_unit(info, dtype)))
    print("se3", np.dtype(dtype), "right" if right else "left", len(grid), "rotation", worst_w,
          "translation", worst_t)
    assert worst_w <= 4 * max(du.C_SE3_REF[dtype], 1.0), worst_w


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_rigid_from_6dof(hip_lib, dtype):
    """[Exp(w) | t] against highprec.transform_from_x (the same Rodrigues form in the same type) to
    8 eps entrywise; the translation column is x_t itself.  Worst on an MI355X: 0.5 eps (fp64),
    1 eps (fp32)."""
    xs = du.x_grid(dtype)
    assert len(xs) >= 65
    with tempfile.TemporaryDirectory() as tmp:
        out = du.run("rigid", dtype, 6, np.stack(xs), tmp, 12)
    worst = 0.0
    for x, T in zip(xs, out):
        R, t = hp.transform_from_x(x, dtype)
        T = T.reshape(3, 4)
        assert T[:, 3].tobytes() == np.asarray(x[:3], dtype=dtype).tobytes()
        worst = max(worst, float(np.abs(T[:, :3].astype(LD) - R).max() / du.eps_of(dtype)))
    print("rigid", np.dtype(dtype), "worst / eps", worst)
    assert worst <= 8.0, worst


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_forward_step_is_the_host_step_bit_for_bit(hip_lib, dtype):
    xs = du.x_grid(dtype) + [np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=dtype)]
    with tempfile.TemporaryDirectory() as tmp:
        out = du.run("fstep", dtype, 1, np.concatenate(xs).reshape(-1, 1), tmp, 1).reshape(-1, 6)
    for x, h in zip(xs, out):
        host = hip_lib.capi.se3_from_params(x, with_steps=True, dtype=dtype)[2]
        assert h.tobytes() == np.asarray(host, dtype=dtype).tobytes(), (x, h, host)


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_fast_reciprocal(hip_lib, dtype):
    """|r d - 1| <= 2 eps for d = +-m 2^e, e over -100 .. 100 (fp64) or -60 .. 60 (fp32), m over
    [1, 2) with both ends.  Worst on an MI355X: 0.5 eps in both types."""
    rng = np.random.default_rng(_seed(dtype, 99))
    top = 100 if np.dtype(dtype) == np.float64 else 60
    eps = float(np.finfo(dtype).eps)
    d = []
    for e in range(-top, top + 1):
        for m in [1.0, 2.0 - eps, *rng.uniform(1.0, 2.0, size=3)]:
            d += [m * 2.0 ** e, -m * 2.0 ** e]
    d = np.array(d, dtype=dtype)
    with tempfile.TemporaryDirectory() as tmp:
        r = du.run("rcp", dtype, 1, d.reshape(-1, 1), tmp, 1).ravel()
    err = np.abs(r.astype(LD) * d.astype(LD) - LD(1)) / du.eps_of(dtype)
    print("rcp", np.dtype(dtype), "worst / eps", float(err.max()))
    assert err.max() <= 2.0, (float(err.max()), d[int(np.argmax(err))])
