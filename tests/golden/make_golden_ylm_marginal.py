#!/usr/bin/env python
"""
Generates tests/golden/ylm_marginal.npz by EXECUTING THE REFERENCE once per grid inclination and mixing in NumPy:

    make -C oracle ref && python tests/golden/make_golden_ylm_marginal.py

Same harness as make_golden_ylm_conditional.py.  At each inclination of the grid the reference's
StarryProcess.sample_ylm_conditional (sp.py:518-641) is read out with the zeros / identity trick (zeros: ymu_j;
np.eye(N): the rows of cho_factor(ycov_j)^T) and its conditional log_likelihood (sp.py:1052-1188,
marginalize_over_inclination=False, normalized=False) gives lnL_j.  The mixture is formed here:

    pinc_j ~ sin(i_j) width_j exp(lnL_j)   (trapezoid widths, half intervals at the ends)
    ymu = sum_j pinc_j ymu_j,   ycov = sum_j pinc_j (ycov_j + (ymu_j - ymu)(ymu_j - ymu)^T)

Per case <c>: <c>_t, <c>_flux, <c>_dvar, <c>_inc, <c>_u, <c>_scalars (ydeg, p, baseline_mean, baseline_var), <c>_ymu,
<c>_ycov_tril (the lower triangle, row by row), <c>_pinc and <c>_ref_dev: the reference's own deviation (mean, covariance,
in posterior sd) from the covariance-form arbiter of tests/test_ylm_marginal_host.py -- the reference conditions in the
precision form (Sigma_y^-1 + A^T C^-1 A)^-1, which loses cond(Sigma_y) eps.
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
from test_ylm_marginal_host import arbiter, default_logw, deviation, make_star, mix, softmax  # noqa: E402

warnings.simplefilter("ignore")
ref = load_reference()
SP = ref.sp.StarryProcess
cho_factor, cho_solve = ref.math.cho_factor, ref.math.cho_solve


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def instance(ydeg):
    mom = np.load(os.path.join(OUT, "moments_L%d.npz" % ydeg))
    sp = SP(ydeg=ydeg, normalized=False, marginalize_over_inclination=False, seed=0)
    N = (ydeg + 1) ** 2
    sp._mean_ylm = mom["default_mean_ylm"]
    sp._cov_ylm = mom["default_cov_ylm"]
    sp._cho_cov_ylm = cho_factor(sp._cov_ylm)
    sp._LInv = cho_solve(sp._cho_cov_ylm, np.eye(N))
    sp._LInvmu = cho_solve(sp._cho_cov_ylm, sp._mean_ylm)
    sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm, marginalize_over_inclination=False,
                                     covpts=sp._covpts, ydeg=ydeg)
    return sp


def run(name, ydeg, K, inc, seed, out):
    st = make_star(ydeg, K, seed)
    sp = instance(ydeg)
    N, P = (ydeg + 1) ** 2, len(inc)
    ymu_inc, ycov_inc, lnl = np.empty((P, N)), np.empty((P, N, N)), np.empty(P)
    real = ref.sp.random_normal
    try:
        for j, i in enumerate(inc):
            kw = dict(i=float(i), p=st["p"], u=list(st["u"]), baseline_mean=st["bmean"], baseline_var=st["bvar"])
            ref.sp.random_normal = lambda rng_, shape: np.zeros(tuple(int(s) for s in shape))
            ymu_inc[j] = A(sp.sample_ylm_conditional(st["t"], st["flux"], st["dvar"], nsamples=1, **kw))[0]
            ref.sp.random_normal = lambda rng_, shape: np.eye(N)
            rows = A(sp.sample_ylm_conditional(st["t"], st["flux"], st["dvar"], nsamples=N, **kw))
            ycho = np.tril((rows - ymu_inc[j][None, :]).T)
            ycov_inc[j] = ycho @ ycho.T
            lnl[j] = float(A(sp.log_likelihood(st["t"], st["flux"], st["dvar"], **kw)))
    finally:
        ref.sp.random_normal = real
    logw = default_logw(inc)
    pinc = softmax(logw + lnl)
    ymu, ycov = mix(pinc, ymu_inc, ycov_inc)
    arb = arbiter(ydeg, st, inc, logw)
    dm, dc = deviation(ymu, ycov, arb)
    dp = np.max(np.abs(pinc - arb["pinc"]))
    out.update({
        name + "_t": st["t"], name + "_flux": st["flux"], name + "_dvar": st["dvar"], name + "_inc": np.asarray(inc),
        name + "_u": st["u"], name + "_scalars": np.array([ydeg, st["p"], st["bmean"], st["bvar"]]),
        name + "_ymu": ymu, name + "_ycov_tril": ycov[np.tril_indices(N)], name + "_pinc": pinc,
        name + "_ref_dev": np.array([dm, dc]),
    })
    print("  %-4s N=%3d K=%4d P=%d  reference against the arbiter: mean %.2e sd, cov %.2e sd sd, pinc %.2e" % (
        name, N, K, P, dm, dc, dp))


def main():
    out = {}
    run("a", 5, 40, np.array([10.0, 30.0, 50.0, 70.0, 90.0]), 41, out)
    run("b", 15, 100, np.array([30.0, 60.0, 85.0]), 42, out)
    path = os.path.join(OUT, "ylm_marginal.npz")
    np.savez_compressed(path, **out)
    print("wrote ylm_marginal.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
