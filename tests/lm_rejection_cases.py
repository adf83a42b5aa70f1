"""The inputs on which the Levenberg-Marquardt loop rejects trials and exhausts its inner loop, shared by the
CPU pin of tests/highprec.lm_minimize_ld (tests/test_highprec_reference.py) and the GPU tests
(tests/test_gpu_lm_rejections.py, whose docstring holds the table with what was measured on them)."""
import numpy as np

from tests import datasets as ds
from tests import highprec as hp

COV_GENERAL = np.array([[2.0, 0.7, -0.1], [0.3, 0.5, 0.9], [-0.4, 0.2, 1.5]])  # tests/test_gpu_batch_solve.py
GM = 1.0  # the Geman-McClure parameter of the cases with outliers

X_ROLL = np.array([0.0, 0.0, 0.0, 3.1, 0.0, 0.0])
X_TUMBLE = np.array([0.0, 0.0, 0.0, 2.5, -2.0, 3.0])
X_PITCH = np.array([0.0, 0.0, 0.0, 0.0, 3.0, 0.0])
X_FAR = np.array([50.0, -40.0, 30.0, 1.5, 1.5, -1.5])


def pair(n=300, seed=11, outliers=None, dtype=np.float64):
    """ds.synthetic_pair(n, seed, noise=0.01); outliers: every third target moved by N(0, 30^2) drawn with
    that seed."""
    src, tgt = ds.synthetic_pair(n, seed=seed, noise=0.01)
    if outliers is not None:
        rng = np.random.default_rng(outliers)
        tgt = tgt.copy()
        tgt[::3] += rng.normal(0.0, 30.0, tgt[::3].shape)
    return src.astype(dtype), tgt.astype(dtype)


class Case:
    """One row: the clouds, x0, covariance and loss, and per lm_max_iterations the largest truncation
    `kmax` judged (the long-double trace of max_iter = kmax has every decision margin)."""

    def __init__(self, name, x0, lm_iters, n=300, seed=11, outliers=None, cov=None, loss=None, kmax=15,
                 clouds=None):
        self.name, self.x0, self.lm_iters, self.kmax = name, np.asarray(x0, dtype=np.float64), tuple(lm_iters), kmax
        self.n, self.seed, self.outliers, self.cov, self.loss, self.clouds = n, seed, outliers, cov, loss, clouds
        self._runs = {}

    def data(self, dtype=np.float64):
        if self.clouds is not None:
            src, tgt = self.clouds()
            return src.astype(dtype), tgt.astype(dtype)
        return pair(self.n, self.seed, self.outliers, dtype)

    def reference(self, lm_iter, dtype=np.float64, jac_mode=0, work=hp.LD):
        """lm_minimize_ld(max_iter = kmax) of this row, computed once per argument set and left unchanged"""
        key = (lm_iter, np.dtype(dtype).name, jac_mode, np.dtype(work).name)
        if key not in self._runs:
            src, tgt = self.data(dtype)
            self._runs[key] = hp.lm_minimize_ld(src, tgt, self.x0, jac_mode, max_iter=self.kmax, lm_iter=lm_iter,
                                                cov=self.cov, loss=self.loss, dtype=dtype, work=work)
        return self._runs[key]

    def with_size(self, n, lm_iters):
        return Case("%s, n = %d" % (self.name, n), self.x0, lm_iters, n=n, seed=self.seed, outliers=self.outliers,
                    cov=self.cov, loss=self.loss, kmax=self.kmax)


def two_clouds():
    a, b = ds.synthetic_pair(1025, seed=31, noise=0.02), ds.synthetic_pair(1025, seed=32, noise=0.02)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


# name: what the row is kept for
ROLL = Case("roll 3.1", X_ROLL, (1, 2, 3, 5))              # lm_iter 1: every iteration from 2 exhausted
TUMBLE = Case("tumble", X_TUMBLE, (1, 2, 3, 5))            # lm_iter 3: 3, 4 exhausted, then accepted steps
PITCH = Case("pitch 3.0", X_PITCH, (2,))                   # 2...6 and 8
FAR = Case("far start", X_FAR, (1, 2, 3))                  # 12...15, at the optimum (lm_iter 5: no delta margin)
GM_OUTLIERS = Case("Geman-McClure, outliers", np.zeros(6), (3,), outliers=1, loss=GM)
SMALL_DELTA = Case("SMALL_DELTA after an exhausted loop", np.zeros(6), (8,), outliers=8, loss=GM, kmax=6)
GENERAL_COV = Case("general covariance", X_TUMBLE, (1, 2, 3, 5), cov=COV_GENERAL)
SEVEN = Case("roll 3.1, n = 7", X_ROLL, (1, 3), n=7)
WELL = Case("well behaved", np.zeros(6), (1, 3), n=1000, seed=5)
CASES = (ROLL, TUMBLE, PITCH, FAR, GM_OUTLIERS, SMALL_DELTA, GENERAL_COV, SEVEN)
# at five fp64 tiles (the launch-per-point loop at its own size), and as two costs of 1025 + 1025
ROLL_5_TILES = ROLL.with_size(2100, (1, 3))
TUMBLE_5_TILES = TUMBLE.with_size(2100, (1,))
ROLL_TWO_COSTS = Case("roll 3.1, two costs", X_ROLL, (1, 3), clouds=two_clouds)
# the issue's table, for the CPU pin: x0 and the exhausted iterations of each lm_iter (runs of 15)
ISSUE_TABLE = (
    (ROLL, {1: list(range(2, 16)), 2: [2, 3, 4, 5, 6], 3: [2, 3], 5: [2]}),
    (TUMBLE, {1: list(range(3, 15)), 2: [3, 4, 5, 6], 3: [3, 4], 5: [3]}),
    (PITCH, {2: [2, 3, 4, 5, 6, 8]}),
    (FAR, {3: [12, 13, 14, 15]}),
)


def nan_clouds(n):
    """synthetic_pair(n, seed=70 + n, noise=0.01) with every fifth target NaN and a NaN run across the first
    fp64 tile boundary (510...515): rejected indices between valid ones"""
    src, tgt = ds.synthetic_pair(n, seed=70 + n, noise=0.01)
    tgt = tgt.copy()
    tgt[::5] = np.nan
    tgt[510:516] = np.nan
    return src, tgt


def nan_row(n):
    """the same cloud without its NaN rows: what the loop over the valid correspondences sees.  Runs of 5 under
    the analytic Jacobian; under forward differences only the first 3 iterations are judged (FD_KMAX)"""
    src, tgt = nan_clouds(n)
    valid = ~np.isnan(tgt).any(axis=1)
    return Case("n = %d without its NaN rows" % n, np.zeros(6), (3,), kmax=5,
                clouds=lambda s=src[valid], t=tgt[valid]: (s, t))


NAN_SIZES = (700, 2048)
NAN_ROWS = tuple(nan_row(n) for n in NAN_SIZES)
FD_KMAX = 3

# lambda_ had no bar.  Measured on the CPU (tests/test_highprec_reference.py re-measures both): the largest
# relative difference of lambda between lm_minimize_ld in long double and the same function in np.float64, over
# every state of every row above under the analytic Jacobian, and over the first FD_KMAX states of NAN_ROWS
# under forward differences (there it is the quotients' rounding, eps |R p + t| / sqrt(eps), in max diag H of
# the first lambda).  Bound: ten times the measurement, floored at 1e-12.
LAMBDA_MEASURED = 2.6e-8
LAMBDA_RTOL = max(10 * LAMBDA_MEASURED, 1e-12)
LAMBDA_MEASURED_FD = 2.7e-9
LAMBDA_RTOL_FD = max(10 * LAMBDA_MEASURED_FD, 1e-12)
