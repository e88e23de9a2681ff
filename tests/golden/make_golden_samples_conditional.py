#!/usr/bin/env python
"""
Generates tests/golden/samples_conditional.npz by EXECUTING THE REFERENCE's conditional, time-variable
StarryProcess.log_likelihood (reference sp.py:1052-1188 with marginalize_over_inclination=False, a Matern-3/2
temporal kernel and the normalised flux -- the process of docs/notebooks/TimeVariabilityInference.ipynb, whose free
parameters are r, a (mu), b (sigma), c, n, i, p, tau):

    make -C oracle ref && python tests/golden/make_golden_samples_conditional.py

Same harness as make_golden.py (oracle/refharness: the reference's own Python on an eager Theano stand-in).  Here the
reference computes its OWN moments from the hyperparameters, one process per vector.  One light curve of K = 60
cadences, six vectors (r, a, b, c, n, i, p, tau), at ydeg 5 and at ydeg 15:

  t [K], flux [K], data_cov (scalar), samples [6, 8] = (r, a, b, c, n, i, p, tau), lnlike_L5 [6], lnlike_L15 [6].

The vectors keep b <= 0.5 and moderate r: where the reference's own moments carry their rounding noise in the high
degrees (tests/test_upstream_grid.py) the distance to an exact evaluation is the reference's error.  Before writing,
the script checks that the CPU oracle on ``oracle.ylm_moments_quadrature`` moments stays within the project's bound
for such a comparison (LNLIKE_BOX_TOL of tests/test_gpu_upstream_device.py) of every recorded value.
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

LNLIKE_BOX_TOL = 5e-5      # tests/test_gpu_upstream_device.py

SAMPLES = np.array([
    # r      a     b     c     n     i     p     tau
    [20.0, 0.40, 0.27, 0.10, 10.0, 60.0, 1.00, 3.0],
    [15.0, 0.30, 0.40, 0.08, 5.0, 75.0, 1.30, 1.5],
    [25.0, 0.55, 0.20, 0.12, 15.0, 40.0, 0.80, 6.0],
    [12.0, 0.20, 0.45, 0.15, 3.0, 85.0, 2.10, 0.7],
    [30.0, 0.60, 0.15, 0.05, 20.0, 25.0, 0.65, 10.0],
    [18.0, 0.45, 0.35, 0.10, 8.0, 55.0, 1.70, 2.2],
])


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def oracle_value(ydeg, row, t, flux, data_cov):
    from oracle import sp_oracle as orc
    from starry_process_amd import upstream

    r, a, b, c, n, i, p, tau = row
    s, _ = upstream.size_moments(r, None, ydeg)
    alpha, beta = upstream.ab_to_alphabeta(a, b)
    mu, Sig = orc.ylm_moments_quadrature(s, s[None, :], alpha, beta, c, n, ydeg)
    op = orc.OracleProcess(mu, Sig, ydeg=ydeg, marginalize_over_inclination=False, normalized=True, tau=tau,
                           temporal_kernel=orc.Matern32Kernel)
    return op.log_likelihood(t, flux, data_cov, i=i, p=p)


def main():
    rng = np.random.RandomState(77)
    K = 60
    t = np.sort(rng.uniform(0.0, 5.0, K))
    data_cov = 1e-6
    # a light curve of the first vector's process, from the reference itself (un-normalised draw, unit mean)
    r, a, b, c, n, i, p, tau = SAMPLES[0]
    gen = SP(ydeg=15, r=r, a=a, b=b, c=c, n=n, tau=tau, temporal_kernel=ref.temporal.Matern32Kernel, normalized=False,
             marginalize_over_inclination=False, seed=3)
    cov = A(gen.cov(t, i=i, p=p)) + data_cov * np.eye(K)
    mean = A(gen.mean(t, i=i, p=p))
    flux = 1.0 + mean + np.linalg.cholesky(cov) @ rng.randn(K)
    flux = flux / np.mean(flux) - 1.0
    out = dict(t=t, flux=flux, data_cov=np.float64(data_cov), samples=SAMPLES)
    for ydeg in (5, 15):
        ll = np.empty(len(SAMPLES))
        for k, row in enumerate(SAMPLES):
            r, a, b, c, n, i, p, tau = row
            sp = SP(ydeg=ydeg, r=r, a=a, b=b, c=c, n=n, tau=tau, temporal_kernel=ref.temporal.Matern32Kernel,
                    normalized=True, marginalize_over_inclination=False)
            ll[k] = float(A(sp.log_likelihood(t, flux, data_cov, i=i, p=p)))
            own = oracle_value(ydeg, row, t, flux, data_cov)
            err = abs(own - ll[k]) / abs(ll[k])
            print("ydeg %2d vector %d: reference %.12g  oracle on quadrature moments %.12g  (%.2e)" % (ydeg, k, ll[k], own, err))
            assert np.isfinite(ll[k]) and err < LNLIKE_BOX_TOL, (ydeg, k, ll[k], own)
        out["lnlike_L%d" % ydeg] = ll
    np.savez_compressed(os.path.join(OUT, "samples_conditional.npz"), **out)


if __name__ == "__main__":
    main()
