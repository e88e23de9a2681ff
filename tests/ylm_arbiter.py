"""
Arbiter of the surface-map posterior (reference sp.py:601-636) and the inputs of its layout-edge sweep.  A helper
module of tests/test_ylm_arbiter_host.py (CPU) and tests/test_gpu_ylm_conditional_edges.py (GPU), not a conftest.

The arbiter evaluates the reference's dense formulas in np.longdouble (80-bit here, u = 2^-64):

    C = diag(d) + b 1 1^T (or a full matrix),   C = L L^T,
    W = Sigma^-1 + A^T C^-1 A,   ycov = W^-1,   ymu = ycov (Sigma^-1 mu + A^T C^-1 r),   ycho = chol(ycov)

with no Sherman-Morrison step, so it shares no algorithm with csrc/sp_ylm.hip beyond the Cholesky idea.  The
factorisation goes column by column and the triangular solves row by row, each step one long-double matrix-vector
product.

The sweep's inputs take the prior precision as a free argument (the engine entry points do): a well-conditioned
Sigma^-1 of the data term's own scale keeps cond_2(W) <= COND_CAP, so the posterior can be checked to rounding, not to
the 1e-6 sd that cond(W) ~ 1e9 of the real moments allows.

Three evaluations of the same posterior live here:
  arbiter       long double, dense                                  -- the truth
  restatement   float64 SciPy cho_factor / cho_solve, dense C and W -- the yardstick: what float64 can do at all
  kernel_form   float64 NumPy in the kernel's Sherman-Morrison form -- carries the mutations of the sensitivity test
"""
import numpy as np
import scipy.linalg

LD = np.longdouble
U = np.finfo(np.float64).eps / 2          # unit roundoff of float64
COND_CAP = 1e3                            # every case of the sweep: cond_2(W) <= COND_CAP

# ---- the sweep -----------------------------------------------------------------------------------------------------
# The degrees stand for the layout classes of N = (ydeg + 1)^2 (ylm_prep_kernel pads N to 64, ylm_epilogue_kernel
# works on 32 x 32 tiles), the K for those of the cadence axis (padded to 32, walked in steps of 64).
K_EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257]
SWEEP = {
    5: K_EDGES,                           # N = 36: ragged, two epilogue tiles per side
    7: K_EDGES,                           # N = 64: exactly one 64-tile
    1: [1, 33, 64, 65, 129],              # N = 4: below one tile
    2: [1, 33, 64, 65, 129],              # N = 9: below one tile
    15: [1, 33, 64, 65, 129, 257],        # N = 256: exact; K < N and K > N
    20: [1, 65, 129],                     # N = 441: ragged, Np = 448, 14 epilogue tiles per side
}
NOISE = ["scalar", "vector"]
S = 3
PERIOD = np.array([0.9, 1.3, 0.7])
INC_DEG = np.array([60.0, 35.0, 80.0])
LIMB = np.array([0.3, 0.1])
BASELINE_MEAN = np.array([0.0, 2e-4, -1e-4])
BASELINE_VAR = np.array([0.0, 1e-6, 3e-6])     # star 0 runs with c = 0
DATA_VAR = 2e-6 * np.array([1.0, 1.5, 0.7])

# YARDSTICK[ydeg]: the largest error of `restatement` against `arbiter` over SWEEP[ydeg] x NOISE x the three stars, in
# the metrics of `errors` (posterior standard deviations), on the oracle's design matrices.  Produced by
#     python tests/ylm_arbiter.py
# (x86-64, 80-bit long double, NumPy 2 / SciPy with OpenBLAS), rounded up to two digits.  The GPU test's bound is
# BOUND_FACTOR x this: ten times the reference's own error, the convention of tests/test_gpu_incl_grad.py.
YARDSTICK = {
    1: 1.1e-14,
    2: 6.9e-15,
    5: 3.6e-14,
    7: 2.5e-14,
    15: 3.2e-14,
    20: 3.0e-14,
}
BOUND_FACTOR = 10.0


def bound(ydeg):
    return BOUND_FACTOR * YARDSTICK[ydeg]


def star_bound(ydeg, K, cw):
    """What one star of a case is held to: bound(ydeg), and never more than the rounding model 32 (K + N) u cond_2(W)
    of a K-term Gram sum and an N x N solve at the star's own cond_2(W) = cw.  The model is the smaller only at the
    smallest shapes (ydeg 1, K = 1: 7e-14 against 1.1e-13)."""
    return min(bound(ydeg), 32 * (K + (ydeg + 1) ** 2) * U * cw)


# ---- long-double linear algebra ------------------------------------------------------------------------------------
def ld(a):
    return np.asarray(a, dtype=LD)


def cholesky(M):
    """Lower Cholesky factor of the symmetric positive definite M, in long double, column by column, each column one
    matrix-vector product: L[j:, j] = (M[j:, j] - L[j:, :j] L[j, :j]) / L[j, j]."""
    M = ld(M)
    n = M.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = M[j:, j] - L[j:, :j].dot(L[j, :j])
        if not col[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at %d" % j)
        L[j:, j] = col / np.sqrt(col[0])
    return L


def solve_lower(L, B):
    """X with L X = B (L lower triangular), row by row in long double."""
    B = ld(B)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i].dot(X[:i])) / L[i, i]
    return X


def solve_upper_t(L, B):
    """X with L^T X = B (L lower triangular), row by row from the last."""
    B = ld(B)
    X = np.zeros_like(B)
    Lt = np.ascontiguousarray(L.T)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (B[i] - Lt[i, i + 1:].dot(X[i + 1:])) / Lt[i, i]
    return X


def spd_inverse(M):
    """(M^-1, L^-1) of the symmetric positive definite M = L L^T in long double: M^-1 = L^-T L^-1, symmetric by
    construction."""
    L = cholesky(M)
    Linv = solve_lower(L, np.eye(M.shape[0], dtype=LD))
    return Linv.T.dot(Linv), Linv


def data_cov(d, b, K):
    """The dense C = diag(d) + b 1 1^T in long double (d scalar or (K,))."""
    return np.diag(np.broadcast_to(ld(d), (K,)).copy()) + LD(b)


def arbiter(A, r, C, sinv, sinvmu):
    """The posterior in long double from dense inputs: A [K, N], r [K] = flux - baseline_mean, C [K, K] (None: the
    identity, the whitened form), sinv [N, N], sinvmu [N].  Returns a dict of long-double arrays W, ycov, ymu, ycho, sd
    (posterior standard deviations) and `selfcheck` = ||W ycov - I||_inf."""
    A, r, sinv, sinvmu = ld(A), ld(r), ld(sinv), ld(sinvmu)
    if C is None:
        Aw, rw = A, r
    else:
        Lc = cholesky(C)
        Aw, rw = solve_lower(Lc, A), solve_lower(Lc, r)
    W = sinv + Aw.T.dot(Aw)
    W = 0.5 * (W + W.T)
    ycov, _ = spd_inverse(W)
    ymu = ycov.dot(sinvmu + Aw.T.dot(rw))
    ycho = cholesky(ycov)
    N = W.shape[0]
    selfcheck = np.max(np.sum(np.abs(W.dot(ycov) - np.eye(N, dtype=LD)), axis=1))
    return dict(W=W, ycov=ycov, ymu=ymu, ycho=ycho, sd=np.sqrt(np.diag(ycov)), selfcheck=selfcheck)


def cond2(W):
    """cond_2 of the symmetric positive definite W (float64 eigenvalues: enough below COND_CAP)."""
    ev = np.linalg.eigvalsh(np.asarray(W, dtype=np.float64))
    return float(ev[-1] / ev[0])


# ---- the float64 evaluations ---------------------------------------------------------------------------------------
def restatement(A, r, C, sinv, sinvmu):
    """The reference's formulas as it evaluates them (sp.py:601-636): float64, cho_factor / cho_solve on the dense C
    and on W.  C None: whitened input.  Returns (ymu, ycov, ycho)."""
    A, r = np.asarray(A, dtype=np.float64), np.asarray(r, dtype=np.float64)
    if C is None:
        CinvA, Cinvr = A, r
    else:
        cho_C = scipy.linalg.cho_factor(np.asarray(C, dtype=np.float64), lower=True)
        CinvA, Cinvr = scipy.linalg.cho_solve(cho_C, A), scipy.linalg.cho_solve(cho_C, r)
    W = np.asarray(sinv, dtype=np.float64) + A.T.dot(CinvA)
    cho_W = scipy.linalg.cho_factor(W, lower=True)
    ycov = scipy.linalg.cho_solve(cho_W, np.eye(W.shape[0]))
    ymu = scipy.linalg.cho_solve(cho_W, np.asarray(sinvmu, dtype=np.float64) + A.T.dot(Cinvr))
    return ymu, ycov, np.linalg.cholesky(ycov)


MUTATIONS = ["drop_last_cadence", "drop_beyond_64", "no_rank1", "hv_no_rank1", "tile_mirror", "row_scale"]


def mutation_applies(name, K, N, b):
    """Whether the mutation changes anything at this shape (b: the star's baseline variance)."""
    if name == "drop_beyond_64":
        return K % 64 != 0 and K > 64
    if name in ("no_rank1", "hv_no_rank1"):
        return b > 0
    if name == "tile_mirror":
        return N > 32
    return True


def kernel_form(A, r, d, b, sinv, sinvmu, mutation=None):
    """The posterior in the kernel's own form (csrc/sp_ylm.hip), float64 NumPy: Bt = (D^-1/2 A)^T, G = Bt Bt^T,
    g = A^T D^-1 1, hv = A^T D^-1 r, s, q, c = b / (1 + b s), W = G + Sigma^-1 - c g g^T mirrored from its lower
    triangle, rhs = Sigma^-1 mu + hv - c g q; then cho_factor / cho_solve.  `mutation`: one of MUTATIONS, a subtly
    wrong kernel.  Returns (ymu, ycov, ycho)."""
    A, r = np.array(A, dtype=np.float64), np.asarray(r, dtype=np.float64)
    K, N = A.shape
    dinv = 1.0 / np.broadcast_to(np.asarray(d, dtype=np.float64), (K,))
    keep = K
    if mutation == "drop_last_cadence":
        keep = K - 1
    elif mutation == "drop_beyond_64":
        keep = (K // 64) * 64
    elif mutation == "row_scale":
        A[K // 2] *= 1.0 + 1e-9
    Bt = (A[:keep] * np.sqrt(dinv[:keep])[:, None]).T
    G = Bt.dot(Bt.T)
    g = A[:keep].T.dot(dinv[:keep])
    hv = A[:keep].T.dot(dinv[:keep] * r[:keep])
    s, q = np.sum(dinv[:keep]), np.sum(dinv[:keep] * r[:keep])
    c = b / (1.0 + b * s)
    low = G + np.asarray(sinv, dtype=np.float64)
    if mutation != "no_rank1":
        low = low - c * np.outer(g, g)
    if mutation == "tile_mirror":
        # the tile (row block 1, column block 0) is stored transposed within itself (its leading square at ragged N)
        n = min(32, N - 32)
        low[32:32 + n, :n] = low[32:32 + n, :n].T.copy()
    W = np.tril(low) + np.tril(low, -1).T
    rhs = np.asarray(sinvmu, dtype=np.float64) + hv
    if mutation != "hv_no_rank1":
        rhs = rhs - c * g * q
    cho_W = scipy.linalg.cho_factor(W, lower=True)
    ycov = scipy.linalg.cho_solve(cho_W, np.eye(N))
    ymu = scipy.linalg.cho_solve(cho_W, rhs)
    return ymu, ycov, np.linalg.cholesky(ycov)


def errors(x, ymu, ycov, ycho=None):
    """The sweep's metrics of a float64 result against the arbiter's dict x, in posterior standard deviations:
    (max |ymu - ymu_x| / sd, max |ycov - ycov_x| / (sd sd^T), max |ycho ycho^T - ycov_x| / (sd sd^T) or 0.0)."""
    sd = x["sd"]
    ss = np.outer(sd, sd)
    e_mu = float(np.max(np.abs(ld(ymu) - x["ymu"]) / sd))
    e_cov = float(np.max(np.abs(ld(ycov) - x["ycov"]) / ss))
    e_cho = 0.0
    if ycho is not None:
        Lc = ld(ycho)
        e_cho = float(np.max(np.abs(Lc.dot(Lc.T) - x["ycov"]) / ss))
    return e_mu, e_cov, e_cho


# ---- inputs --------------------------------------------------------------------------------------------------------
def case_inputs(ydeg, K, noise):
    """The seeded light curves of one case of the sweep: t [S, K] sorted uniform on (0, 3), flux [S, K] = 1e-3 randn,
    d [S, K] the per-cadence variances (`scalar`: DATA_VAR broadcast, `vector`: 1e-6 (1 + rand))."""
    rng = np.random.RandomState(10000 * ydeg + K)
    t = np.sort(rng.uniform(0.0, 3.0, size=(S, K)), axis=1)
    flux = 1e-3 * rng.randn(S, K)
    dvec = 1e-6 * (1.0 + rng.rand(S, K))
    d = np.broadcast_to(DATA_VAR[:, None], (S, K)).copy() if noise == "scalar" else dvec
    return t, flux, d


def prior_precision(A, dinv, seed):
    """A well-conditioned prior precision on the data term's own scale: sinv = Q diag(linspace(1, 10, N)) Q^T
    tr(A^T D^-1 A) / N, symmetrised, Q from a seeded QR; sinvmu = sinv (1e-3 randn).  A [K, N], dinv [K] (ones for the
    whitened form)."""
    K, N = A.shape
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(N, N))
    scale = float(np.sum(A * A * np.asarray(dinv)[:, None])) / N
    sinv = (Q * np.linspace(1.0, 10.0, N)[None, :]).dot(Q.T) * scale
    sinv = 0.5 * (sinv + sinv.T)
    sinvmu = sinv.dot(1e-3 * rng.randn(N))
    return sinv, sinvmu


def prior_seed(ydeg, K, s):
    return 100000 * ydeg + 10 * K + s


def oracle_design(ydeg, t):
    """The oracle's design matrices [S, K, N] of the sweep's three stars at times t [S, K]."""
    from oracle import sp_oracle as orc

    rta1 = orc.rTA1L(ydeg, 2, LIMB)
    return np.array([orc.design_matrix(ydeg, rta1, t[s], INC_DEG[s] * np.pi / 180, PERIOD[s]) for s in range(S)])


def correlated_cov(t, rng):
    """A full data covariance of golden case c's form: per-cadence variances plus 2e-7 exp(-dt^2 / (2 0.05^2))."""
    K = t.shape[0]
    return np.diag(1e-6 * (1.0 + rng.rand(K))) + 2e-7 * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.05 ** 2)


def whiten(C, A, r):
    """(B, r_w) = (L^-1 A, L^-1 r) for C = L L^T, formed in long double and rounded to float64."""
    Lc = cholesky(C)
    return (np.asarray(solve_lower(Lc, A), dtype=np.float64), np.asarray(solve_lower(Lc, r), dtype=np.float64))


# ---- the prior precision of the real moments (Engine.ylm_precision, sp.py:267-271) ---------------------------------
PRECISION_SETS = [("default", 5), ("default", 15), ("default", 20), ("hilat", 15), ("spread", 15)]

# PRECISION_YARDSTICK[(set, ydeg)]: (sinv, sinvmu) errors of `precision_restatement` against `precision_arbiter` in the
# metrics of `precision_errors`, measured by tests/test_ylm_arbiter_host.py::test_precision_yardstick (same machine as
# YARDSTICK), rounded up to two digits.  cond(Sigma_y) is about 1e9 and more, hence their size.
PRECISION_YARDSTICK = {
    ("default", 5): (1.3e-13, 6.6e-17),
    ("default", 15): (2.0e-9, 8.4e-12),
    ("default", 20): (4.0e-9, 6.1e-12),
    ("hilat", 15): (3.4e-8, 7.2e-9),
    ("spread", 15): (4.9e-8, 1.7e-9),
}


def precision_arbiter(mu, Sig):
    """(Sigma^-1, Sigma^-1 mu) in long double."""
    sinv, _ = spd_inverse(Sig)
    return sinv, sinv.dot(ld(mu))


def precision_restatement(mu, Sig):
    """The reference's form (sp.py:267-271): cho_factor, then cho_solve against I and mu, float64."""
    cho = scipy.linalg.cho_factor(np.asarray(Sig, dtype=np.float64), lower=True)
    return scipy.linalg.cho_solve(cho, np.eye(len(mu))), scipy.linalg.cho_solve(cho, np.asarray(mu, dtype=np.float64))


def precision_errors(sinv_x, sinvmu_x, mu, sinv, sinvmu):
    """(max |sinv - sinv_x| / sqrt(diag diag^T), max |sinvmu - sinvmu_x| / (sqrt(diag) sqrt(mu^T sinv_x mu))), diag that
    of sinv_x: the second scale is the Cauchy-Schwarz bound of |sinvmu_i|."""
    dg = np.sqrt(np.diag(sinv_x))
    e_s = float(np.max(np.abs(ld(sinv) - sinv_x) / np.outer(dg, dg)))
    e_m = float(np.max(np.abs(ld(sinvmu) - sinvmu_x) / (dg * np.sqrt(ld(mu).dot(sinvmu_x)))))
    return e_s, e_m


def sweep_cases():
    return [(ydeg, K, noise) for ydeg in SWEEP for K in SWEEP[ydeg] for noise in NOISE]


def star_problems(ydeg, K, noise, A=None):
    """The three stars of one case as dense problems: a list of dicts with s, A [K, N] (the oracle's unless given, e.g.
    the device's own), t, flux, r = flux - baseline_mean, d [K], b, C (long double), sinv, sinvmu."""
    t, flux, d = case_inputs(ydeg, K, noise)
    if A is None:
        A = oracle_design(ydeg, t)
    out = []
    for s in range(S):
        sinv, sinvmu = prior_precision(A[s], 1.0 / d[s], prior_seed(ydeg, K, s))
        out.append(dict(s=s, A=A[s], t=t[s], flux=flux[s], r=flux[s] - BASELINE_MEAN[s], d=d[s], b=BASELINE_VAR[s],
                        C=data_cov(d[s], BASELINE_VAR[s], K), sinv=sinv, sinvmu=sinvmu))
    return out


def selfcheck_bound(N, cw):
    """What ||W ycov - I||_inf may be in long double: 64 N 2^-64 cond(W)."""
    return 64 * N * 2.0 ** -64 * cw


def measure_yardstick(ydeg, cases=None):
    """(yardstick, worst cond_2(W), worst selfcheck / its bound) of one degree over `cases` [(K, noise)] (default: all
    of the sweep's), on the oracle's design matrices."""
    if cases is None:
        cases = [(K, noise) for K in SWEEP[ydeg] for noise in NOISE]
    worst, wcond, wself = 0.0, 0.0, 0.0
    N = (ydeg + 1) ** 2
    for K, noise in cases:
        for q in star_problems(ydeg, K, noise):
            x = arbiter(q["A"], q["r"], q["C"], q["sinv"], q["sinvmu"])
            cw = cond2(x["W"])
            worst = max(worst, *errors(x, *restatement(q["A"], q["r"], q["C"], q["sinv"], q["sinvmu"])))
            wcond = max(wcond, cw)
            wself = max(wself, float(x["selfcheck"]) / selfcheck_bound(N, cw))
    return worst, wcond, wself


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    for _ydeg in sorted(SWEEP):
        _y, _c, _s = measure_yardstick(_ydeg)
        print("ydeg %2d  yardstick %.2e  worst cond2(W) %.1f  selfcheck / bound %.2e" % (_ydeg, _y, _c, _s))
