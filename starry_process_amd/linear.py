"""Host builders of regressor matrices for ``StarryProcess.log_likelihood_linear`` and
``log_likelihood_linear_ensemble``: per-segment offsets (Kepler quarters, TESS sectors) and slow per-segment trends.
Each returns a ``(K, q)`` float64 array, one regressor per column; ``stack_bases`` puts them side by side.
``offset_basis_at`` and ``polynomial_basis_at`` evaluate the same columns at other times (``predict_ensemble``'s
``basis_sample``)."""
import numpy as np

__all__ = ["offset_basis", "polynomial_basis", "offset_basis_at", "polynomial_basis_at", "stack_bases"]

MAX_REGRESSORS = 32   # regressors per star: SP_LIN_QMAX of csrc/sp_linq.h


def check_regressors(basis, basis_var, S, K):
    """``basis`` (K, q) shared or (S, K, q) and ``basis_var`` scalar, (q,) or (S, q) as the ensemble calls with
    regressors take them (``log_likelihood_linear_ensemble``, ``grad.EnsembleGradient``): returns (U (S, K, q),
    lam (S, q) contiguous) in float64; ValueError for another shape, q outside 1 .. 32, a non-finite basis or a variance
    that is negative or not finite.  Host work only."""
    U = np.asarray(basis, dtype=np.float64)
    if U.ndim == 2 and U.shape[0] == K:
        U = np.broadcast_to(U, (S,) + U.shape)
    if U.ndim != 3 or U.shape[0] != S or U.shape[1] != K:
        raise ValueError("`basis` must be (K, q) or (S, K, q) with S = %d, K = %d, not %s"
                         % (S, K, np.shape(basis)))
    q = U.shape[2]
    if not 1 <= q <= MAX_REGRESSORS:
        raise ValueError("1 to %d regressors are served, not %d" % (MAX_REGRESSORS, q))
    if not np.all(np.isfinite(U)):
        raise ValueError("`basis` must be finite")
    return U, check_regressor_variances(basis_var, S, q)


def _regressor_args(basis, basis_var, S, K, need_var="`basis` needs a `basis_var`", required=False):
    """The ``basis=``, ``basis_var=`` pair of an ensemble call: (U, Ut, lam) as ``check_regressors`` checks them, Ut
    [S, q, K] the contiguous copy with a regressor along a row (what the device takes).  Where the pair is optional:
    (None, None, None) without a basis, and ValueError for one of the pair without the other (``need_var``: the
    caller's words for a basis without variances).  ``required``: both go to ``check_regressors`` as they are."""
    if not required:
        if basis is None:
            if basis_var is not None:
                raise ValueError("`basis_var` needs a `basis`")
            return None, None, None
        if basis_var is None:
            raise ValueError(need_var)
    U, lam = check_regressors(basis, basis_var, S, K)
    return U, np.ascontiguousarray(np.swapaxes(U, 1, 2)), lam


def check_regressor_variances(basis_var, S, q):
    """``basis_var`` scalar, (q,) or (S, q), finite and >= 0 -> (S, q) contiguous float64; ValueError otherwise."""
    lam = np.asarray(basis_var, dtype=np.float64)
    if lam.ndim == 0 or lam.shape == (q,) or lam.shape == (S, q):
        lam = np.ascontiguousarray(np.broadcast_to(lam, (S, q)))
    else:
        raise ValueError("`basis_var` must be a scalar, (q,) or (S, q) with S = %d, q = %d, not %s"
                         % (S, q, lam.shape))
    if not np.all(np.isfinite(lam)) or np.any(lam < 0):
        raise ValueError("`basis_var` must be finite and >= 0")
    return lam


def _segment_edges(edges, K):
    """``edges`` as an int64 array 0 = e_0 < e_1 < ... < e_n = K (None: one segment)."""
    if edges is None:
        return np.array([0, K], dtype=np.int64)
    raw = np.asarray(edges)
    if raw.ndim != 1 or raw.size < 2 or not np.all(np.isfinite(raw)) or not np.all(raw == np.floor(raw)):
        raise ValueError("`edges` must be a 1-D array of at least two integer segment edges")
    ed = raw.astype(np.int64)
    if ed[0] != 0 or ed[-1] != K or np.any(np.diff(ed) < 1):
        raise ValueError("`edges` must run 0 = e_0 < e_1 < ... < e_n = K = %d, not %s" % (K, ed.tolist()))
    return ed


def offset_basis(K, edges):
    """One indicator column per segment: column j is 1 on the cadences edges[j] .. edges[j + 1] - 1 and 0 elsewhere.
    ``edges``: 0 = e_0 < e_1 < ... < e_n = K.  Returns (K, n)."""
    K = int(K)
    if K < 1:
        raise ValueError("`K` must be at least 1")
    ed = _segment_edges(edges, K)
    U = np.zeros((K, ed.size - 1))
    for j in range(ed.size - 1):
        U[ed[j]:ed[j + 1], j] = 1.0
    return U


def polynomial_basis(t, degree, edges=None):
    """Legendre columns P_1 .. P_degree in each segment's own time, rescaled to [-1, 1] over the segment
    (x = 2 (t - t_first) / (t_last - t_first) - 1), zero outside the segment.  No constant column: the offsets are
    ``offset_basis``'s.  A segment of one cadence, or of constant time, gets zero columns.  ``edges`` as
    ``offset_basis`` (None: one segment).  Returns (K, n degree), the columns of segment 0 first."""
    t = np.asarray(t, dtype=np.float64)
    degree = int(degree)
    if t.ndim != 1 or t.size < 1 or not np.all(np.isfinite(t)):
        raise ValueError("`t` must be a finite 1-D array")
    if degree < 1:
        raise ValueError("`degree` must be at least 1")
    K = t.size
    ed = _segment_edges(edges, K)
    n = ed.size - 1
    U = np.zeros((K, n * degree))
    for j in range(n):
        ts = t[ed[j]:ed[j + 1]]
        span = ts.max() - ts.min()
        if not span > 0:
            continue
        x = 2.0 * (ts - ts.min()) / span - 1.0
        V = np.polynomial.legendre.legvander(x, degree)
        U[ed[j]:ed[j + 1], j * degree:(j + 1) * degree] = V[:, 1:]
    return U


def _segment_of(t_sample, t, edges):
    """(ts, t, ed, seg): the sample times (1-D float64), the cadences (strictly increasing), the checked edges and the
    segment of every sample time: j when t[e_j] <= ts < t[e_j+1]; before the first cadence the first segment, after
    the last cadence the last."""
    t = np.asarray(t, dtype=np.float64)
    ts = np.asarray(t_sample, dtype=np.float64)
    if t.ndim != 1 or t.size < 1 or not np.all(np.isfinite(t)):
        raise ValueError("`t` must be a finite 1-D array")
    if np.any(np.diff(t) <= 0):
        raise ValueError("`t` must be strictly increasing")
    if ts.ndim != 1 or ts.size < 1 or not np.all(np.isfinite(ts)):
        raise ValueError("`t_sample` must be a finite 1-D array")
    ed = _segment_edges(edges, t.size)
    seg = np.clip(np.searchsorted(t[ed[:-1]], ts, side="right") - 1, 0, ed.size - 2)
    return ts, t, ed, seg


def offset_basis_at(t_sample, t, edges):
    """The columns of ``offset_basis(len(t), edges)`` at the times ``t_sample``: column j is 1 where the sample time
    belongs to segment j -- t[e_j] <= t_sample < t[e_j+1]; times before the first cadence belong to the first segment,
    times after the last cadence to the last.  ``t``: the strictly increasing cadences the edges index.  Returns
    (Ks, n); ``offset_basis_at(t, t, edges)`` is ``offset_basis(len(t), edges)`` bit for bit."""
    ts, t, ed, seg = _segment_of(t_sample, t, edges)
    U = np.zeros((ts.size, ed.size - 1))
    U[np.arange(ts.size), seg] = 1.0
    return U


def polynomial_basis_at(t_sample, t, degree, edges=None):
    """The columns of ``polynomial_basis(t, degree, edges)`` at the times ``t_sample``: the Legendre columns of the
    segment a sample time belongs to (``offset_basis_at``'s rule) in that segment's own rescaled time -- outside the
    segment's cadences the polynomials are extrapolated -- and zeros in the other segments' columns.  A segment of
    one cadence has zero columns, as in ``polynomial_basis``.  Returns (Ks, n degree);
    ``polynomial_basis_at(t, t, degree, edges)`` is ``polynomial_basis(t, degree, edges)`` bit for bit."""
    degree = int(degree)
    if degree < 1:
        raise ValueError("`degree` must be at least 1")
    ts, t, ed, seg = _segment_of(t_sample, t, edges)
    n = ed.size - 1
    U = np.zeros((ts.size, n * degree))
    for j in range(n):
        tj = t[ed[j]:ed[j + 1]]
        span = tj.max() - tj.min()
        if not span > 0:
            continue
        own = seg == j
        x = 2.0 * (ts[own] - tj.min()) / span - 1.0
        V = np.polynomial.legendre.legvander(x, degree)
        U[own, j * degree:(j + 1) * degree] = V[:, 1:]
    return U


def stack_bases(*bases):
    """The given (K, q_i) bases side by side: (K, sum q_i)."""
    if not bases:
        raise ValueError("at least one basis is needed")
    mats = [np.asarray(b, dtype=np.float64) for b in bases]
    if any(m.ndim != 2 for m in mats) or len({m.shape[0] for m in mats}) != 1:
        raise ValueError("every basis must be (K, q_i) with the same K")
    return np.ascontiguousarray(np.concatenate(mats, axis=1))
