#!/usr/bin/env python
"""
Generates tests/golden/predict_ensemble.npz by EXECUTING THE REFERENCE's own
StarryProcess.predict (reference sp.py:767-903) once per star:

    make -C oracle ref && python tests/golden/make_golden_predict_ensemble.py

Same harness as make_golden_temporal.py (oracle/refharness: the reference's own
Python on an eager Theano stand-in), on the ``default`` moments of
moments_L15.npz as gen_predict of make_golden.py does.  S = 5 stars, each with
its own period, inclination, limb darkening, baseline mean and variance and its
own row of sample times; K = 100 observed and Ks = 29 sample times, so that
K + Ks + 1 = 130 crosses a 64-row tile edge of the padded system.  One set per
branch, each with another form of data_cov:

    marg   marginalised over inclination     data_cov scalar
    cond   conditional on the inclination    data_cov (S,)
    tau    time-variable, tau = 2.0          data_cov (S, K)

Per set <c>: <c>_data_cov, <c>_mu (S, Ks), <c>_K (S, Ks, Ks), <c>_cond (S,) =
cond(K_tt) of every star, asserted <= 1e5 (make_golden_temporal.py's bound: the
reference's own float64 result is then good to ~1e-11 of the prior scale).  The
noise variances are 1e-6 to 2e-6 on a prior variance of 1.4e-3: with gen_predict's
2.5e-7 the K = 100 systems have cond(K_tt) = 2e5 (largest eigenvalue 0.05 - 0.07).
Shared: t (K,), ts (S, Ks),
flux (S, K), p, i, u, baseline_mean, baseline_var.
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

S, K, KS = 5, 100, 29


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def main():
    mom = np.load(os.path.join(OUT, "moments_L15.npz"))
    rng = np.random.RandomState(29)
    t = np.linspace(0, 3.0, K)
    ts = np.sort(rng.uniform(-0.3, 3.4, size=(S, KS)), axis=1)
    p = np.array([0.9, 1.1, 0.75, 1.6, 1.25])
    inc = np.array([55.0, 70.0, 35.0, 80.0, 62.0])
    u = np.array([[0.0, 0.0], [0.4, 0.2], [0.3, 0.1], [0.4, 0.2], [0.1, 0.05]])
    bmean = np.array([1e-4, 0.0, -2e-4, 3e-4, 5e-5])
    bvar = np.array([1e-6, 0.0, 2e-6, 5e-7, 1e-6])
    flux = np.array([4e-3 * (0.5 + 0.2 * s) * np.sin(2 * np.pi * t / p[s] + s) for s in range(S)])
    flux += 5e-4 * rng.randn(S, K)
    out = dict(t=t, ts=ts, flux=flux, p=p, i=inc, u=u, baseline_mean=bmean, baseline_var=bvar)
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
        mus, Ks_, conds = [], [], []
        for s in range(S):
            dc = dcov if dcov.ndim == 0 else dcov[s]
            kw = dict(i=inc[s], p=p[s], u=list(u[s]))
            Ktt = A(sp.cov(t, **kw)) + (np.diag(dc) if np.ndim(dc) == 1 else dc * np.eye(K)) + bvar[s]
            cond = np.linalg.cond(Ktt)
            assert cond <= 1e5, (name, s, cond)
            mu, Kpost = sp.predict(t, flux[s], dc, t_sample=ts[s], baseline_mean=bmean[s], baseline_var=bvar[s], **kw)
            mus.append(A(mu))
            Ks_.append(A(Kpost))
            conds.append(cond)
            print("  %-4s star %d cond(K_tt)=%.3g mu[0]=%+.8e K[0,0]=%.8e" % (name, s, cond, mus[-1][0], Ks_[-1][0, 0]))
        out[name + "_data_cov"] = np.asarray(dcov)
        out[name + "_mu"] = np.array(mus)
        out[name + "_K"] = np.array(Ks_)
        out[name + "_cond"] = np.array(conds)
    path = os.path.join(OUT, "predict_ensemble.npz")
    np.savez_compressed(path, **out)
    print("wrote predict_ensemble.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
