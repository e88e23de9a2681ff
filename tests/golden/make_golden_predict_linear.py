#!/usr/bin/env python
"""
Generates tests/golden/predict_linear.npz: conditional light curves under the model flux = process + U w + noise,
w ~ N(0, diag lambda), from the REFERENCE's own covariances (reference sp.py:674-765 ``cov``, 767-903 ``predict``):

    make -C oracle ref && python tests/golden/make_golden_predict_linear.py

Same harness and moments as make_golden_predict_ensemble.py.  S = 3 stars, K = 100 observed and Ks = 29 sample times,
q = 5 regressors: three segment offsets (edges 0, 35, 70, 100) and the Legendre columns P_1, P_2 over the whole light
curve; the regressors at the sample times are linear.offset_basis_at / polynomial_basis_at's (host NumPy).  The last
lambda of every star is 0: that regressor is switched off.  K + Ks + 1 + q = 135 crosses a 64-row tile edge.

    marg, cond, tau   the reference's ``cov`` on the concatenated times [ts; t]; + [U_s; U] Lambda [U_s; U]^T, the
                      noise and baseline_var; conditioned densely in NumPy (Cholesky of C~_tt):
                      <c>_mu (S, Ks), <c>_K (S, Ks, Ks) for process + trend at the sample times
    same_t            the reference's own predict(t_sample=None, baseline_var = b + U Lambda U^T): its broadcast puts
                      the matrix into the cross and prior blocks too, which is the case U_s = U (marginal branch):
                      same_t_mu (S, K), same_t_K (S, K, K)

Per set <c>_data_cov and <c>_cond (S,) = cond(C~_tt) of every star, asserted <= 1e5 (make_golden_temporal.py's bound).
The noise variances are 2e-6 to 4e-6.  Shared: t (K,), ts (S, Ks), flux (S, K), p, i, u, baseline_mean, baseline_var,
edges, basis (K, q), basis_sample (S, Ks, q), basis_var (S, q).  The file holds arrays only.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle.refharness.loadref import load_reference  # noqa: E402
from starry_process_amd import linear  # noqa: E402

warnings.simplefilter("ignore")
ref = load_reference()
SP = ref.sp.StarryProcess

S, K, KS, Q = 3, 100, 29, 5


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def condition(Ctt, Cst, Css, r, mean):
    """mean + C_st C_tt^-1 r and C_ss - C_st C_tt^-1 C_st^T through the Cholesky factor of C_tt."""
    L = np.linalg.cholesky(Ctt)
    Y = np.linalg.solve(L, Cst.T).T
    y = np.linalg.solve(L, r)
    Kp = Css - Y @ Y.T
    return mean + Y @ y, 0.5 * (Kp + Kp.T)


def main():
    mom = np.load(os.path.join(OUT, "moments_L15.npz"))
    rng = np.random.RandomState(31)
    t = np.linspace(0, 3.0, K)
    ts = np.sort(rng.uniform(-0.3, 3.4, size=(S, KS)), axis=1)
    p = np.array([0.9, 1.1, 1.6])
    inc = np.array([55.0, 70.0, 80.0])
    u = np.array([[0.0, 0.0], [0.4, 0.2], [0.1, 0.05]])
    bmean = np.array([1e-4, 0.0, -2e-4])
    bvar = np.array([1e-6, 0.0, 5e-7])
    edges = np.array([0, 35, 70, K])
    U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t, 2))
    Us = np.array([linear.stack_bases(linear.offset_basis_at(ts[s], t, edges), linear.polynomial_basis_at(ts[s], t, 2))
                   for s in range(S)])
    assert U.shape == (K, Q) and Us.shape == (S, KS, Q)
    lam = np.array([[1e-5, 2e-5, 1e-5, 4e-6, 0.0], [2e-5, 1e-5, 3e-5, 1e-6, 0.0], [5e-6, 5e-6, 2e-5, 2e-6, 0.0]])
    w = rng.randn(S, Q) * np.sqrt(lam)
    flux = np.array([4e-3 * (0.5 + 0.2 * s) * np.sin(2 * np.pi * t / p[s] + s) for s in range(S)])
    flux += 5e-4 * rng.randn(S, K) + w @ U.T
    out = dict(t=t, ts=ts, flux=flux, p=p, i=inc, u=u, baseline_mean=bmean, baseline_var=bvar, edges=edges, basis=U,
               basis_sample=Us, basis_var=lam)
    sets = [
        ("marg", dict(marginalize_over_inclination=True), np.float64(2e-6)),
        ("cond", dict(marginalize_over_inclination=False), 2e-6 * (1.0 + 0.5 * rng.rand(S))),
        ("tau", dict(marginalize_over_inclination=True, tau=2.0), 2e-6 * (1.0 + rng.rand(S, K))),
        ("same_t", dict(marginalize_over_inclination=True), np.float64(2e-6)),
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
            noise = np.diag(dc) if np.ndim(dc) == 1 else dc * np.eye(K)
            ULU = (U * lam[s]) @ U.T
            if name == "same_t":
                Ctt = A(sp.cov(t, **kw)) + noise + bvar[s] + ULU
                mu, Kpost = sp.predict(t, flux[s], dc, baseline_mean=bmean[s], baseline_var=bvar[s] + ULU, **kw)
                mu, Kpost = A(mu), A(Kpost)
            else:
                B = np.concatenate([Us[s], U])
                Call = A(sp.cov(np.concatenate([ts[s], t]), **kw)) + bvar[s] + (B * lam[s]) @ B.T
                Ctt = Call[KS:, KS:] + noise
                mean = float(A(sp.mean(t, **kw))[0])
                mu, Kpost = condition(Ctt, Call[:KS, KS:], Call[:KS, :KS], (flux[s] - bmean[s]) - mean, mean)
            cond = np.linalg.cond(Ctt)
            assert cond <= 1e5, (name, s, cond)
            mus.append(mu)
            Ks_.append(Kpost)
            conds.append(cond)
            print("  %-6s star %d cond(C~_tt)=%.3g mu[0]=%+.8e K[0,0]=%.8e" % (name, s, cond, mu[0], Kpost[0, 0]))
        out[name + "_data_cov"] = np.asarray(dcov)
        out[name + "_mu"] = np.array(mus)
        out[name + "_K"] = np.array(Ks_)
        out[name + "_cond"] = np.array(conds)
    path = os.path.join(OUT, "predict_linear.npz")
    np.savez_compressed(path, **out)
    print("wrote predict_linear.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
