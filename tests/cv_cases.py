"""Inputs shared by tests/test_cv_host.py and tests/test_gpu_cv.py (no test in here).

planted(): the planted-rank input of the rank-choice checks.  A = W0 H0 + noise, 80 x 60, rank 3, 15 % held out, every member started
from its own U(0, 1) factors, 60 outer iterations without a stopping rule.  The noise is sparse: 5 % of the entries carry a spike of up
to 0.5 (the entries of W0 H0 are ~0.75).  With iid noise of any level the oracle's held-out error at ranks 3 and 4 stays within 10 % of
each other at this size (an extra component adds 140 parameters to 4080 training entries); a component that latches onto spikes
reconstructs their rows and columns badly, which is what a held-out set is there to catch.  SEED was chosen on the CPU oracle alone
(test_cv_host.py asserts the margin); nothing here was tuned on the library under test."""
import numpy as np

SEED = 2
NOISE = 0.1
N, M, RANK, FRACTION = 80, 60, 3, 0.15
ITERS, TRACE = 60, 5


def pattern_cols(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def with_nan(A, ptr, idx):
    An = np.array(A, dtype=np.float64, copy=True)
    An[idx, pattern_cols(ptr)] = np.nan
    return An


def assert_trainable(A, ptr, idx, kmax):
    """Every row and column keeps at least kmax + 1 observed entries (below that the result is decided by rounding)."""
    n, m = A.shape
    rows = m - np.bincount(idx, minlength=n)
    cols = n - np.diff(ptr)
    assert rows.min() >= kmax + 1 and cols.min() >= kmax + 1, (int(rows.min()), int(cols.min()), kmax)


def planted(ks):
    """(A, inits [(W, H)] for the ranks ks): the inits are drawn rank after rank, so a longer ks extends a shorter one's."""
    g = np.random.default_rng(SEED)
    A = g.random((N, RANK)) @ g.random((RANK, M)) + NOISE * ((g.random((N, M)) < 0.05) * 5.0 * g.random((N, M)))
    inits = [(g.random((N, k)), g.random((k, M))) for k in ks]
    return A, inits


def numpy_holdout_errors(A, ptr, idx, W, H):
    """mean (a - wh)^2 and mean (a + eps) log((a + eps) / (wh + eps)) - a + wh over the pattern (api.mse_mkl's definition)."""
    cols = pattern_cols(ptr)
    a, p = A[idx, cols], np.einsum("eq,qe->e", W[idx, :], H[:, cols])
    return float(np.mean((a - p) ** 2)), float(np.mean((a + 1e-16) * np.log((a + 1e-16) / (p + 1e-16)) - a + p))
