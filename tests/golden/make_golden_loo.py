#!/usr/bin/env python
"""
Generates tests/golden/loo.npz, the leave-one-out fixture, by EXECUTING THE
REFERENCE's own StarryProcess.predict (reference sp.py:767-903) with one cadence
held out, once per star and cadence:

    make -C oracle ref && python tests/golden/make_golden_loo.py

Same harness and inputs as make_golden_predict_ensemble.py (oracle/refharness: the
reference's own Python on an eager Theano stand-in; the ``default`` moments of
moments_L15.npz), with S = 3 stars, each with its own period, inclination, limb
darkening, baseline mean and variance, and K = 65 cadences: one past a 64-row tile
edge.  All sets are ``normalized=False``: the reference's predict refuses a
normalised process.  One set per branch, each with another form of data_cov:

    marg   marginalised over inclination     data_cov scalar
    cond   conditional on the inclination    data_cov (S,)
    tau    time-variable, tau = 2.0          data_cov (S, K)

The recipe, for star s and cadence k: call the reference's

    predict(t[-k], flux[s][-k], data_cov[-k], t_sample=[t[k]], i, p, u, baseline_mean, baseline_var)

(x[-k]: x without entry k) and store what it says about DATUM k,

    <c>_mu[s, k]  = mu_ref + baseline_mean[s]
    <c>_var[s, k] = K_ref + data_var[s, k]

Per set <c> also: <c>_data_cov and <c>_cond (S,) = cond(C) of every star's full
K x K covariance C = cov + D + baseline_var, asserted <= 1e5 (the bound of
make_golden_predict_ensemble.py: the reference's own float64 result is then good
to ~1e-11 of the prior scale).  The noise variances are 1e-6 to 2e-6 on a prior
variance of 1.4e-3.  Shared: t (K,), flux (S, K), p, i, u, baseline_mean,
baseline_var.
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
    out = dict(t=t, flux=flux, p=p, i=inc, u=u, baseline_mean=bmean, baseline_var=bvar)
    sets = [
        ("marg", dict(marginalize_over_inclination=True), np.float64(1e-6)),
        ("cond", dict(marginalize_over_inclination=False), 1e-6 * (1.0 + 0.5 * rng.rand(S))),
        ("tau", dict(marginalize_over_inclination=True, tau=2.0), 1e-6 * (1.0 + rng.rand(S, K))),
    ]
    for name, ckw, dcov in sets:
        sp = SP(ydeg=15, normalized=False, **ckw)
        # fixture moments: the comparison is free of the platform noise of Sigma_y
        sp._mean_ylm = mom["default_mean_ylm"]
        sp._cov_ylm = mom["default_cov_ylm"]
        sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm,
                                         marginalize_over_inclination=ckw["marginalize_over_inclination"],
                                         covpts=sp._covpts, ydeg=15)
        mus, vars_, conds = np.empty((S, K)), np.empty((S, K)), np.empty(S)
        for s in range(S):
            dc = dcov if dcov.ndim == 0 else dcov[s]
            dvec = np.broadcast_to(dc, (K,))
            kw = dict(i=inc[s], p=p[s], u=list(u[s]))
            C = A(sp.cov(t, **kw)) + np.diag(dvec) + bvar[s]
            conds[s] = np.linalg.cond(C)
            assert conds[s] <= 1e5, (name, s, conds[s])
            for k in range(K):
                keep = np.arange(K) != k
                mu, Kpost = sp.predict(t[keep], flux[s][keep], dc if np.ndim(dc) == 0 else dc[keep],
                                       t_sample=t[k:k + 1], baseline_mean=bmean[s], baseline_var=bvar[s], **kw)
                mus[s, k] = A(mu).reshape(-1)[0] + bmean[s]
                vars_[s, k] = A(Kpost).reshape(-1)[0] + dvec[k]
            print("  %-4s star %d cond(C)=%.3g mu[0]=%+.8e var[0]=%.8e" % (name, s, conds[s], mus[s, 0], vars_[s, 0]))
        out[name + "_data_cov"] = np.asarray(dcov)
        out[name + "_mu"] = mus
        out[name + "_var"] = vars_
        out[name + "_cond"] = conds
    path = os.path.join(OUT, "loo.npz")
    np.savez_compressed(path, **out)
    print("wrote loo.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
