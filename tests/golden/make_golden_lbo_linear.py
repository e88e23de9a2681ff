#!/usr/bin/env python
"""
Generates tests/golden/lbo_linear.npz, the fixture of the leave-block-out checks
with linear regressors marginalised out, by EXECUTING THE REFERENCE's own
StarryProcess.log_likelihood (reference sp.py:1051-1188) with the MATRIX
baseline_var = b + U Lambda U^T, once on all cadences of a star and once per
block with the block's cadences REMOVED (t, flux, the data variances and the
sub-matrix of baseline_var all restricted to the cadences that remain):

    make -C oracle ref && python tests/golden/make_golden_lbo_linear.py

    lpd_B = lnL(all cadences) - lnL(cadences outside B)

is the log predictive density of the held-out block under C~ = C + U Lambda U^T.

Harness and inputs are make_golden_linear.py's, read from its fixture linear.npz:
S = 3, K = 65, q = 5, the same U, Lambda, trended flux and data_cov per set.
Sets: marg, cond, tau, all normalized=False (a normalised process rescales its
covariance by the mean over the cadences it is given: a difference of two
reference likelihoods is then not a conditional density of one Gaussian).
Partitions: p0 = [0, 16, 32, 48, 64, 65], p1 = [0, 1, 3, 35, 64, 65], p2 = single
cadences.

The reference's ``predict`` cannot take a matrix baseline_var with held-out
times, so mu, var and cov come from brute-force conditioning in NumPy on the
reference's own C~ = cov + D + b + U Lambda U^T and mean.

Asserted here: cond(C~) <= 1e5 (the cap of the other fixtures), and per block
lambda_min(G~) / lambda_min(G) >= 1e-2 with G~ = (C~^-1)_BB, G = (C^-1)_BB: the
downdate G~ = G - Z_B Z_B^T loses at most two digits.  (Both hold with the Lambda
of linear.npz, no variance had to be lowered: cond(C~) 2.0e4 to 3.9e4, the ratios
0.017 -- the block of 32 cadences of p1 -- to 0.88.)

Per set <c>:            <c>_lnl_all (S,), <c>_cond (S,), <c>_data_cov
Per set and partition:  <c>_<p>_lnl_out, <c>_<p>_lpd (S, nb); <c>_<p>_mu, <c>_<p>_var (S, K);
                        <c>_<p>_cov (S, sum b^2): the blocks' covariances, flattened one after another;
                        <c>_<p>_ratio (S, nb): lambda_min(G~) / lambda_min(G)
Shared: t, flux, p, i, u, baseline_mean, baseline_var, basis, basis_var, p0_edges, p1_edges, p2_edges.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle.refharness.loadref import load_reference  # noqa: E402

warnings.simplefilter("ignore")
ref = load_reference()
SP = ref.sp.StarryProcess

SETS = [("marg", dict(marginalize_over_inclination=True)), ("cond", dict(marginalize_over_inclination=False)),
        ("tau", dict(marginalize_over_inclination=True, tau=2.0))]


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def main():
    mom = np.load(os.path.join(OUT, "moments_L15.npz"))
    g = np.load(os.path.join(OUT, "linear.npz"))
    t, flux, U, lam = g["t"], g["flux"], g["basis"], g["basis_var"]
    S, K = flux.shape
    assert (S, K, U.shape[1]) == (3, 65, 5)
    ULU = (U * lam) @ U.T
    parts = {"p0": np.array([0, 16, 32, 48, 64, 65]), "p1": np.array([0, 1, 3, 35, 64, 65]), "p2": np.arange(K + 1)}
    out = {k: g[k] for k in ("t", "flux", "p", "i", "u", "baseline_mean", "baseline_var", "basis", "basis_var")}
    for pn, e in parts.items():
        out[pn + "_edges"] = e.astype(np.int32)
    for name, ckw in SETS:
        sp = SP(ydeg=15, normalized=False, **ckw)
        # fixture moments: the comparison is free of the platform noise of Sigma_y
        sp._mean_ylm = mom["default_mean_ylm"]
        sp._cov_ylm = mom["default_cov_ylm"]
        sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm,
                                         marginalize_over_inclination=ckw["marginalize_over_inclination"],
                                         covpts=sp._covpts, ydeg=15)
        dcov = g[name + "_data_cov"]
        out[name + "_data_cov"] = dcov
        lnl_all, conds = np.empty(S), np.empty(S)
        res = {pn: dict(lnl_out=np.empty((S, len(e) - 1)), mu=np.empty((S, K)), var=np.empty((S, K)),
                        cov=np.empty((S, int((np.diff(e) ** 2).sum()))), ratio=np.empty((S, len(e) - 1)))
               for pn, e in parts.items()}
        for s in range(S):
            dvec = np.array(np.broadcast_to(dcov if dcov.ndim == 0 else dcov[s], (K,)))
            kw = dict(i=g["i"][s], p=g["p"][s], u=list(g["u"][s]))
            bm, b = g["baseline_mean"][s], g["baseline_var"][s]

            def lnl(keep):
                return float(A(sp.log_likelihood(t[keep], flux[s][keep], dvec[keep], baseline_mean=bm,
                                                 baseline_var=b + ULU[np.ix_(keep, keep)], **kw)))

            lnl_all[s] = lnl(np.ones(K, dtype=bool))
            C = A(sp.cov(t, **kw)) + np.diag(dvec) + b
            Ct = C + ULU
            mean = A(sp.mean(t, **kw)).reshape(-1) + bm
            conds[s] = np.linalg.cond(Ct)
            assert conds[s] <= 1e5, (name, s, conds[s])
            Ci, Cti = np.linalg.inv(C), np.linalg.inv(Ct)
            for pn, e in parts.items():
                R, o = res[pn], 0
                for j, (lo, hi) in enumerate(zip(e[:-1], e[1:])):
                    keep = np.ones(K, dtype=bool)
                    keep[lo:hi] = False
                    R["lnl_out"][s, j] = lnl(keep)
                    c = Ct[np.ix_(keep, ~keep)]
                    sol = np.linalg.solve(Ct[np.ix_(keep, keep)], np.column_stack([flux[s][keep] - mean[keep], c]))
                    cv = Ct[lo:hi, lo:hi] - c.T @ sol[:, 1:]
                    cv = 0.5 * (cv + cv.T)
                    R["mu"][s, lo:hi] = mean[lo:hi] + c.T @ sol[:, 0]
                    R["var"][s, lo:hi] = np.diag(cv)
                    n = hi - lo
                    R["cov"][s, o:o + n * n] = cv.reshape(-1)
                    o += n * n
                    gt = 0.5 * (Cti[lo:hi, lo:hi] + Cti[lo:hi, lo:hi].T)
                    gg = 0.5 * (Ci[lo:hi, lo:hi] + Ci[lo:hi, lo:hi].T)
                    R["ratio"][s, j] = np.linalg.eigvalsh(gt)[0] / np.linalg.eigvalsh(gg)[0]
                    assert R["ratio"][s, j] >= 1e-2, (name, pn, s, j, R["ratio"][s, j])
                print("  %-4s star %d %s cond=%.3g lnl_all=%+.10e min ratio=%.3f lpd[0]=%+.8e"
                      % (name, s, pn, conds[s], lnl_all[s], R["ratio"][s].min(), lnl_all[s] - R["lnl_out"][s, 0]))
        out[name + "_lnl_all"] = lnl_all
        out[name + "_cond"] = conds
        for pn, R in res.items():
            out["%s_%s_lpd" % (name, pn)] = lnl_all[:, None] - R["lnl_out"]
            for k, v in R.items():
                out["%s_%s_%s" % (name, pn, k)] = v
    path = os.path.join(OUT, "lbo_linear.npz")
    np.savez_compressed(path, **out)
    print("wrote lbo_linear.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
