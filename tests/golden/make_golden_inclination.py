#!/usr/bin/env python
"""
Generates tests/golden/inclination.npz by EXECUTING THE REFERENCE's conditional
StarryProcess.log_likelihood (reference sp.py:1052-1188 with
marginalize_over_inclination=False, what calibrate/inclination.py:9-76 calls once
per light curve, sample and inclination):

    make -C oracle ref && python tests/golden/make_golden_inclination.py

Same harness as make_golden.py (oracle/refharness: the reference's own Python on
an eager Theano stand-in).  The moments are the ``default`` set of
moments_L15.npz, injected into the reference instance as
make_golden_ylm_conditional.py does.  Three stars of K = 200 cadences, each with
its own period, limb darkening, noise and baselines, at seven inclinations,
normalised and not:

  t [S, K], flux [S, K], data_cov [S] (star 1: per-cadence variances in
  data_cov_vec [K]), p [S], u [S, 2], baseline_mean [S], baseline_var [S],
  inc [P] (degrees), lnlike_norm [S, P], lnlike_raw [S, P].
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


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def instance(normalized):
    mom = np.load(os.path.join(OUT, "moments_L15.npz"))
    sp = SP(ydeg=15, normalized=normalized, marginalize_over_inclination=False)
    sp._mean_ylm = mom["default_mean_ylm"]
    sp._cov_ylm = mom["default_cov_ylm"]
    sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm, marginalize_over_inclination=False,
                                     covpts=sp._covpts, ydeg=15)
    return sp, mom


def main():
    rng = np.random.RandomState(4321)
    S, K = 3, 200
    inc = np.array([0.0, 5.0, 22.5, 37.0, 60.0, 89.9, 90.0])
    t = np.sort(rng.uniform(0, 4, (S, K)), axis=1)
    p = np.array([0.8, 1.3, 2.1])
    u = np.array([[0.0, 0.0], [0.4, 0.2], [0.1, 0.3]])
    data_cov = np.array([1e-6, 4e-6, 2.5e-7])
    data_cov_vec = data_cov[1] * (1 + rng.rand(K))
    bm = np.array([0.0, 1e-3, -2e-3])
    bv = np.array([0.0, 1e-4, 1e-6])
    sp0, mom = instance(False)
    N = mom["default_mean_ylm"].shape[0]
    L = np.linalg.cholesky(mom["default_cov_ylm"] + 1e-12 * np.eye(N))
    flux = np.empty((S, K))
    for s in range(S):
        y = mom["default_mean_ylm"] + L @ rng.randn(N)
        Ad = A(sp0._flux.design_matrix(t[s], 50.0, p[s], u[s]))
        flux[s] = Ad @ y + np.sqrt(data_cov[s]) * rng.randn(K) + bm[s]
    out = dict(t=t, flux=flux, data_cov=data_cov, data_cov_vec=data_cov_vec, p=p, u=u, baseline_mean=bm,
               baseline_var=bv, inc=inc)
    for tag, normalized in (("norm", True), ("raw", False)):
        sp, _ = instance(normalized)
        ll = np.empty((S, inc.shape[0]))
        for s in range(S):
            dc = data_cov_vec if s == 1 else data_cov[s]
            for k, i in enumerate(inc):
                ll[s, k] = float(A(sp.log_likelihood(t[s], flux[s], dc, i=i, p=p[s], u=u[s], baseline_mean=bm[s],
                                                     baseline_var=bv[s])))
        out["lnlike_" + tag] = ll
        print(tag, ll)
    np.savez_compressed(os.path.join(OUT, "inclination.npz"), **out)


if __name__ == "__main__":
    main()
