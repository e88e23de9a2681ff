#!/usr/bin/env python
"""
Generates tests/golden/ylm_conditional.npz by EXECUTING THE REFERENCE's
StarryProcess.sample_ylm_conditional (reference sp.py:518-641):

    make -C oracle ref && python tests/golden/make_golden_ylm_conditional.py

Same harness as make_golden.py (oracle/refharness: the reference's own Python on
an eager Theano stand-in).  The reference draws its deviates through
``random_normal`` (sp.py:640); the generator replaces that function, in this
process only, to read the Gaussian out of the sampler:

  * zeros                 -> every sample is ymu;
  * np.eye(N), N samples  -> sample j is ymu + cho_factor(ycov)[:, j], i.e. the
                             rows of cho_factor(ycov)^T (saved as the factor).

It also saves the first 5 samples of a fresh instance with the stream left alone
(RandomState(seed).normal(size=(N, 5))).

Per case <c>:  <c>_t, <c>_flux, <c>_data_cov, <c>_ymu, <c>_ycho (lower factor of
ycov), <c>_samples (5 x N), plus the scalar inputs.  The moments are the
``default`` set of moments_L{ydeg}.npz, with Sigma_y^-1 and Sigma_y^-1 mu_y
recomputed through the reference's own cho_factor / cho_solve (sp.py:267-271).
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
cho_factor, cho_solve = ref.math.cho_factor, ref.math.cho_solve


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def instance(ydeg, marg, seed):
    mom = np.load(os.path.join(OUT, "moments_L%d.npz" % ydeg))
    sp = SP(ydeg=ydeg, normalized=False, marginalize_over_inclination=marg, seed=seed)
    N = (ydeg + 1) ** 2
    sp._mean_ylm = mom["default_mean_ylm"]
    sp._cov_ylm = mom["default_cov_ylm"]
    sp._cho_cov_ylm = cho_factor(sp._cov_ylm)
    sp._LInv = cho_solve(sp._cho_cov_ylm, np.eye(N))
    sp._LInvmu = cho_solve(sp._cho_cov_ylm, sp._mean_ylm)
    sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm, marginalize_over_inclination=marg,
                                     covpts=sp._covpts, ydeg=ydeg)
    return sp, mom


def light_curve(sp, mom, t, i, p, u, noise, rng):
    """A light curve of a map drawn from the prior, plus white noise (the flux's only role is to be plausible)."""
    N = mom["default_mean_ylm"].shape[0]
    L = np.linalg.cholesky(mom["default_cov_ylm"] + 1e-12 * np.eye(N))
    y = mom["default_mean_ylm"] + L @ rng.randn(N)
    Ad = A(sp._flux.design_matrix(t, i, p, u))
    return Ad @ y + np.sqrt(noise) * rng.randn(t.shape[0])


def run(name, ydeg, marg, K, i, p, u, data_cov_fn, baseline_mean, baseline_var, seed, out):
    rng = np.random.RandomState(1000 + len(out))
    t = np.linspace(0, 2, K)
    sp, mom = instance(ydeg, marg, seed)
    N = (ydeg + 1) ** 2
    data_cov = data_cov_fn(t, rng)
    flux = light_curve(sp, mom, t, i, p, u, 1e-6, rng) + baseline_mean
    kw = dict(i=i, p=p, u=u, baseline_mean=baseline_mean, baseline_var=baseline_var)

    # fresh instance, stream untouched: the first 5 samples
    samples = A(sp.sample_ylm_conditional(t, flux, data_cov, nsamples=5, **kw))
    real = ref.sp.random_normal
    try:
        ref.sp.random_normal = lambda rng_, shape: np.zeros(tuple(int(s) for s in shape))
        ymu = A(sp.sample_ylm_conditional(t, flux, data_cov, nsamples=1, **kw))[0]
        ref.sp.random_normal = lambda rng_, shape: np.eye(N)
        rows = A(sp.sample_ylm_conditional(t, flux, data_cov, nsamples=N, **kw))
    finally:
        ref.sp.random_normal = real
    ycho = (rows - ymu[None, :]).T
    out.update({
        name + "_t": t, name + "_flux": flux, name + "_data_cov": np.asarray(data_cov, dtype=np.float64),
        name + "_ymu": ymu, name + "_ycho": np.tril(ycho), name + "_samples": samples,
        name + "_scalars": np.array([ydeg, float(marg), i, p, baseline_mean, baseline_var, seed]),
        name + "_u": np.asarray(u, dtype=np.float64),
    })
    sd = np.sqrt(np.diag(ycho @ ycho.T))
    print("  %-4s N=%3d K=%4d  ymu[0]=%+.6e  sd[0]=%.3e  samples[0,0]=%+.6e" % (
        name, N, K, ymu[0], sd[0], samples[0, 0]))


def main():
    out = {}
    # (a) tests/test_sample.py's shape: conditional inclination, scalar data_cov
    run("a", 15, False, 300, 60.0, 1.0, [0.0, 0.0], lambda t, r: 1e-6, 0.0, 0.0, 3, out)
    # (b) marginal flag, K = 1000, per-cadence variances, baseline variance, limb darkening
    run("b", 15, True, 1000, 70.0, 1.3, [0.3, 0.1], lambda t, r: 1e-6 * (1.0 + 0.5 * r.rand(t.shape[0])),
        0.0, 1e-6, 11, out)
    # (c) full data covariance: per-cadence variances plus a correlated term
    run("c", 15, True, 60, 55.0, 0.8, [0.4, 0.2],
        lambda t, r: np.diag(1e-6 * (1.0 + r.rand(t.shape[0])))
        + 2e-7 * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.05 ** 2), 1e-4, 0.0, 5, out)
    # (d) ydeg 5
    run("d", 5, False, 200, 40.0, 0.7, [0.0, 0.0], lambda t, r: 4e-6, 0.0, 1e-6, 7, out)
    path = os.path.join(OUT, "ylm_conditional.npz")
    np.savez_compressed(path, **out)
    print("wrote ylm_conditional.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
