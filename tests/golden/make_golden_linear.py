#!/usr/bin/env python
"""
Generates tests/golden/linear.npz, the fixture of the likelihood with linear
regressors marginalised out, by EXECUTING THE REFERENCE's own
StarryProcess.log_likelihood (reference sp.py:1051-1188) with a MATRIX
baseline_var = b + U Lambda U^T (its docstring, sp.py:1115-1121; Luger et al.
2017, Eq. 4):

    make -C oracle ref && python tests/golden/make_golden_linear.py

Same harness and inputs as make_golden_loo.py (oracle/refharness: the reference's
own Python on an eager Theano stand-in; the ``default`` moments of
moments_L15.npz): S = 3 stars, each with its own period, inclination, limb
darkening, baseline mean and scalar baseline variance b, K = 65 cadences.

The basis U (K, 5): three segment offsets with edges 0, 20, 41, 65, then a
linear and a quadratic column x, x^2 in x = 2 (t - t_0) / (t_1 - t_0) - 1 over the
whole light curve; Lambda = diag(1e-4, 1e-4, 1e-4, 2.5e-5, 2.5e-5).  The flux of
make_golden_loo.py has U . (3e-3, -4e-3, 1e-3, 2e-3, -1e-3) added.

Four sets, each with another form of data_cov:

    marg   marginalised over inclination     data_cov scalar
    cond   conditional on the inclination    data_cov (S,)
    tau    time-variable, tau = 2.0          data_cov (S, K)
    norm   marginalised, normalized=True     data_cov scalar

Per set <c>:

    <c>_lnlike  (S,)       log_likelihood(..., baseline_var = b + U Lambda U^T)
    <c>_lnlike0 (S,)       log_likelihood(..., baseline_var = b)
    <c>_w_mean  (S, q)     generalised least squares with the Gaussian prior, in NumPy, on the reference's own
    <c>_w_cov   (S, q, q)  C = cov + D + b and mean:  w_cov = (Lambda^-1 + U^T C^-1 U)^-1,
                           w_mean = w_cov U^T C^-1 (flux - mean - baseline_mean)
    <c>_cond    (S,)       cond(C + U Lambda U^T), asserted <= 1e5 (the cap of the other fixtures)
    <c>_data_cov

Shared: t (K,), flux (S, K), p, i, u, baseline_mean, baseline_var, basis (K, q),
basis_var (q,), w_true (q,).
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

S, K = 3, 65


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def main():
    mom = np.load(os.path.join(OUT, "moments_L15.npz"))
    rng = np.random.RandomState(65)
    t = np.linspace(0, 3.0, K)
    p = np.array([0.9, 1.1, 0.75])
    inc = np.array([55.0, 70.0, 35.0])
    u = np.array([[0.0, 0.0], [0.4, 0.2], [0.3, 0.1]])
    bmean = np.array([1e-4, 0.0, -2e-4])
    bvar = np.array([1e-6, 0.0, 2e-6])
    flux = np.array([4e-3 * (0.5 + 0.2 * s) * np.sin(2 * np.pi * t / p[s] + s) for s in range(S)])
    flux += 5e-4 * rng.randn(S, K)
    edges = [0, 20, 41, 65]
    x = 2.0 * (t - t[0]) / (t[-1] - t[0]) - 1.0
    U = np.zeros((K, 5))
    for j in range(3):
        U[edges[j]:edges[j + 1], j] = 1.0
    U[:, 3] = x
    U[:, 4] = x * x
    lam = np.array([1e-4, 1e-4, 1e-4, 2.5e-5, 2.5e-5])
    w_true = np.array([3e-3, -4e-3, 1e-3, 2e-3, -1e-3])
    flux = flux + (U @ w_true)[None, :]
    ULU = (U * lam) @ U.T
    out = dict(t=t, flux=flux, p=p, i=inc, u=u, baseline_mean=bmean, baseline_var=bvar, basis=U, basis_var=lam,
               w_true=w_true)
    sets = [
        ("marg", dict(marginalize_over_inclination=True), False, np.float64(1e-6)),
        ("cond", dict(marginalize_over_inclination=False), False, 1e-6 * (1.0 + 0.5 * rng.rand(S))),
        ("tau", dict(marginalize_over_inclination=True, tau=2.0), False, 1e-6 * (1.0 + rng.rand(S, K))),
        ("norm", dict(marginalize_over_inclination=True), True, np.float64(1e-6)),
    ]
    for name, ckw, normalized, dcov in sets:
        sp = SP(ydeg=15, normalized=normalized, **ckw)
        # fixture moments: the comparison is free of the platform noise of Sigma_y
        sp._mean_ylm = mom["default_mean_ylm"]
        sp._cov_ylm = mom["default_cov_ylm"]
        sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm,
                                         marginalize_over_inclination=ckw["marginalize_over_inclination"],
                                         covpts=sp._covpts, ydeg=15)
        ll, ll0, conds = np.empty(S), np.empty(S), np.empty(S)
        wm, wc = np.empty((S, 5)), np.empty((S, 5, 5))
        for s in range(S):
            dc = dcov if dcov.ndim == 0 else dcov[s]
            dvec = np.broadcast_to(dc, (K,))
            kw = dict(i=inc[s], p=p[s], u=list(u[s]))
            ll[s] = float(A(sp.log_likelihood(t, flux[s], dc, baseline_mean=bmean[s], baseline_var=bvar[s] + ULU, **kw)))
            ll0[s] = float(A(sp.log_likelihood(t, flux[s], dc, baseline_mean=bmean[s], baseline_var=bvar[s], **kw)))
            C = A(sp.cov(t, **kw)) + np.diag(dvec) + bvar[s]
            r = flux[s] - A(sp.mean(t, **kw)).reshape(-1) - bmean[s]
            conds[s] = np.linalg.cond(C + ULU)
            assert conds[s] <= 1e5, (name, s, conds[s])
            CiU = np.linalg.solve(C, U)
            wc[s] = np.linalg.inv(np.diag(1.0 / lam) + U.T @ CiU)
            wc[s] = 0.5 * (wc[s] + wc[s].T)
            wm[s] = wc[s] @ (CiU.T @ r)
            print("  %-4s star %d cond=%.3g lnlike=%+.10e lnlike0=%+.10e w_mean[0]=%+.6e"
                  % (name, s, conds[s], ll[s], ll0[s], wm[s, 0]))
        out[name + "_data_cov"] = np.asarray(dcov)
        out[name + "_lnlike"] = ll
        out[name + "_lnlike0"] = ll0
        out[name + "_w_mean"] = wm
        out[name + "_w_cov"] = wc
        out[name + "_cond"] = conds
    path = os.path.join(OUT, "linear.npz")
    np.savez_compressed(path, **out)
    print("wrote linear.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
