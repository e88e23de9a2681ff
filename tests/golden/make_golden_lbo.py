#!/usr/bin/env python
"""
Generates tests/golden/lbo.npz, the leave-block-out fixture, by EXECUTING THE
REFERENCE's own StarryProcess.predict (reference sp.py:767-903) with one block of
consecutive cadences held out, once per star and block:

    make -C oracle ref && python tests/golden/make_golden_lbo.py

The harness, the inputs and the three sets are those of make_golden_loo.py (S = 3
stars, K = 65 cadences, ``normalized=False``; the same random stream, so t, flux
and the data variances are loo.npz's own):

    marg   marginalised over inclination     data_cov scalar
    cond   conditional on the inclination    data_cov (S,)
    tau    time-variable, tau = 2.0          data_cov (S, K)

Two partitions of the cadences, as edges:

    p0   [0, 16, 32, 48, 64, 65]     four blocks of 16 and a last one of 1
    p1   [0, 1, 3, 35, 64, 65]       widths 1, 2, 32, 29, 1

The recipe, for star s and block B = [e_j, e_j+1): call the reference's

    predict(t[-B], flux[s][-B], data_cov[-B], t_sample=t[B], i, p, u, baseline_mean, baseline_var)

(x[-B]: x without the entries of B) and store what it says about the DATA of B,

    <c>_p<j>_mu[s, B]     = mu_ref + baseline_mean[s]                     (S, K)
    <c>_p<j>_cov[s, ...]  = K_ref + diag(data_var[s, B]), row-major,      (S, sum of b^2)
                            the blocks one behind the other (``unpack_cov`` below)

Per set <c> also <c>_data_cov and <c>_cond (S,) = cond(C) of every star's full
K x K covariance C = cov + D + baseline_var, asserted <= 1e5 as make_golden_loo.py
does.  Shared: t (K,), flux (S, K), p, i, u, baseline_mean, baseline_var, and the
two edge arrays p0_edges, p1_edges.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

S, K = 3, 65
PARTITIONS = {"p0": [0, 16, 32, 48, 64, 65], "p1": [0, 1, 3, 35, 64, 65]}


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def unpack_cov(flat, edges):
    """The blocks' covariance matrices (a list of [b, b]) from one star's row of <c>_p<j>_cov."""
    out, o = [], 0
    for a, b in zip(edges[:-1], edges[1:]):
        n = int(b - a)
        out.append(np.asarray(flat[o:o + n * n]).reshape(n, n))
        o += n * n
    assert o == len(flat)
    return out


def main():
    from oracle.refharness.loadref import load_reference

    warnings.simplefilter("ignore")
    ref = load_reference()
    SP = ref.sp.StarryProcess
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
    for pn, edges in PARTITIONS.items():
        out[pn + "_edges"] = np.array(edges, dtype=np.int32)
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
        conds = np.empty(S)
        res = {pn: (np.empty((S, K)), [[] for _ in range(S)]) for pn in PARTITIONS}
        for s in range(S):
            dc = dcov if dcov.ndim == 0 else dcov[s]
            dvec = np.broadcast_to(dc, (K,))
            kw = dict(i=inc[s], p=p[s], u=list(u[s]))
            C = A(sp.cov(t, **kw)) + np.diag(dvec) + bvar[s]
            conds[s] = np.linalg.cond(C)
            assert conds[s] <= 1e5, (name, s, conds[s])
            for pn, edges in PARTITIONS.items():
                mus, covs = res[pn]
                for a, b in zip(edges[:-1], edges[1:]):
                    keep = np.ones(K, dtype=bool)
                    keep[a:b] = False
                    mu, Kpost = sp.predict(t[keep], flux[s][keep], dc if np.ndim(dc) == 0 else dc[keep],
                                           t_sample=t[a:b], baseline_mean=bmean[s], baseline_var=bvar[s], **kw)
                    mus[s, a:b] = A(mu).reshape(-1) + bmean[s]
                    covs[s].append((A(Kpost).reshape(b - a, b - a) + np.diag(dvec[a:b])).reshape(-1))
            print("  %-4s star %d cond(C)=%.3g" % (name, s, conds[s]))
        out[name + "_data_cov"] = np.asarray(dcov)
        out[name + "_cond"] = conds
        for pn in PARTITIONS:
            out["%s_%s_mu" % (name, pn)] = res[pn][0]
            out["%s_%s_cov" % (name, pn)] = np.array([np.concatenate(c) for c in res[pn][1]])
    path = os.path.join(OUT, "lbo.npz")
    np.savez_compressed(path, **out)
    print("wrote lbo.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
