#!/usr/bin/env python
"""
Generates tests/golden/norm_series.npz, the fixture of the normalisation series at
orders other than 20 and at large z, by EXECUTING THE REFERENCE's own
StarryProcess.log_likelihood and StarryProcess.cov (reference sp.py:674-727,
1052-1188, ops/norm/norm.py:26-44):

    make -C oracle ref && python tests/golden/make_golden_norm.py

Same harness as the other make_golden_*.py (oracle/refharness: the reference's own
Python on an eager Theano stand-in).  Inputs: the ensemble of
tests/test_norm_series_host.py -- ydeg 5, S = 3 stars, K = 65 cadences, every star
with its own times, period, inclination, noise and baseline -- at its two sets of
hyperparameters,

    inbox   r 20, a .4, b .27, c 0.40, n 10     z ~ 0.016
    sharp   the same with c 0.50                z ~ 0.04

both branches (marg: marginalised over inclination, cond: conditional on it),
normalization_order in ORDERS = (0, 2, 20, 21), normalization_zmax = inf.

Stored per <case> in {inbox, sharp} and <branch> in {marg, cond}:

    <case>_mean_ylm, <case>_cov_ylm     the reference's own moments (the oracle is fed
                                        with them: the comparison is free of the
                                        platform noise of Sigma_y)
    <case>_<branch>_lnlike  (4, S)      log_likelihood per order and star
    <case>_<branch>_cov     (4, K, K)   cov of star 0 per order
    <case>_<branch>_z       (S,)        the expansion parameter z = m / mu^2

Shared: ydeg, orders, t (S, K), flux (S, K), p, i, u, data_var, baseline_mean,
baseline_var.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle.refharness.loadref import load_reference  # noqa: E402

import test_norm_series_host as cases  # noqa: E402

warnings.simplefilter("ignore")
ref = load_reference()
SP = ref.sp.StarryProcess

ORDERS = (0, 2, 20, 21)


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def main():
    S, K = cases.S, cases.K
    t, flux = cases.times(), cases.fluxes()
    out = dict(ydeg=np.array(cases.YDEG), orders=np.array(ORDERS), t=t, flux=flux, p=cases.PERIODS, i=cases.INCS,
               u=cases.U, data_var=cases.DATA_VAR, baseline_mean=cases.BASELINE_MEAN, baseline_var=cases.BASELINE_VAR)
    for case in ("inbox", "sharp"):
        for tag, marg in (("marg", True), ("cond", False)):
            lnl, cov, z = np.empty((len(ORDERS), S)), np.empty((len(ORDERS), K, K)), np.empty(S)
            for k, order in enumerate(ORDERS):
                sp = SP(ydeg=cases.YDEG, marginalize_over_inclination=marg, normalized=True,
                        normalization_order=order, normalization_zmax=np.inf, **cases.HP[case])
                out[case + "_mean_ylm"], out[case + "_cov_ylm"] = A(sp._mean_ylm), A(sp._cov_ylm)
                for s in range(S):
                    kw = dict(i=cases.INCS[s], p=cases.PERIODS[s], u=list(cases.U))
                    lnl[k, s] = float(A(sp.log_likelihood(t[s], flux[s], cases.DATA_VAR[s],
                                                          baseline_mean=cases.BASELINE_MEAN[s],
                                                          baseline_var=cases.BASELINE_VAR[s], **kw)))
                    z[s] = float(A(sp._z))
                    if s == 0:
                        cov[k] = A(sp.cov(t[0], **kw))
                print("  %-5s %-4s order %2d  z %s  lnlike %s" % (case, tag, order, z, lnl[k]))
            assert np.all(np.isfinite(lnl)) and np.all(np.isfinite(cov))
            out["%s_%s_lnlike" % (case, tag)] = lnl
            out["%s_%s_cov" % (case, tag)] = cov
            out["%s_%s_z" % (case, tag)] = z
    path = os.path.join(OUT, "norm_series.npz")
    np.savez_compressed(path, **out)
    print("wrote norm_series.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
