"""Conditional likelihoods on a grid of inclinations (sp_lnlike_inclinations) at the reference's calibrate defaults
(64 stars x 10 posterior samples x 100 inclinations, calibrate/defaults.json), against the dense route -- one
replicated star per (star, sample, inclination) through sp_lnlike_ensemble(conditional = 1) -- timed on a subset of
the triples and scaled to the whole workload.  HIP events, normalised process, scalar variances.

  basis   plan (per star) + model (per moment set and inclination) + triples, one library call
  dense   K x K assembly A Sigma_y A^T, normalisation, Cholesky, reduction per triple

Prints one JSON line per shape (K = 1000 at ydeg 15, K = 3000 at ydeg 20): milliseconds per call of the basis route
(median of the timed calls), milliseconds per triple of the dense route on one call of `DENSE` triples, the dense route's time
scaled to the workload, their ratio, and the largest relative difference between the routes on the subset.

    python tools/bench_inclinations.py [reps]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd.engine import Engine, make_stars  # noqa: E402

SHAPES = [(1000, 15), (3000, 20)]
S, J, P = 64, 10, 100
DENSE = 64


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main(reps=5):
    for K, L in SHAPES:
        e = Engine(L, 2, 0)
        mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % L))
        rng = np.random.RandomState(K)
        t = np.sort(rng.uniform(0, 4, (S, K)), axis=1)
        p = 0.6 + rng.rand(S)
        flux = 1e-3 * np.sin(2 * np.pi * t / p[:, None]) + 1e-3 * rng.randn(S, K)
        stars = make_stars(S, period=p, data_var=1e-6, baseline_var=1e-6)
        # S J distinct moment sets (the drawn posterior samples): the golden set scaled
        scale = 0.5 + rng.rand(S * J)
        mu = e.f64(scale[:, None] * mom["default_mean_ylm"][None, :])
        cov = e.f64(scale[:, None, None] * mom["default_cov_ylm"][None, :, :])
        sel = np.arange(S * J, dtype=np.int32).reshape(S, J)
        sel[:, 0] = 0          # (draw 0 of every star uses set 0: the dense subset below runs on one resident set)
        inc = np.linspace(0, 90, P) * np.pi / 180
        rta1 = e.rTA1L(np.zeros((1, 2)))
        td, fd = e.f64(t), e.f64(flux)
        out = {}

        def basis():
            out["v"], _ = e.lnlike_inclinations(td, fd, stars, rta1, mu, cov, inc, select=sel, zmax=np.inf)

        ms_basis = timed(basis, reps)
        got = out["v"].cpu().numpy()
        # dense: DENSE triples (every star with draw 0, inclinations spread over the grid) as replicated stars
        idx = [(s % S, 0, (7 * s) % P) for s in range(DENSE)]
        tt = e.f64(np.stack([t[s] for s, _, _ in idx]))
        ff = e.f64(np.stack([flux[s] for s, _, _ in idx])[:, None, :])
        st = make_stars(DENSE, period=[p[s] for s, _, _ in idx], inc_deg=[inc[k] * 180 / np.pi for _, _, k in idx],
                        data_var=1e-6, baseline_var=1e-6)
        sd = e.stars_to_device(st)
        rd = e.f64(rta1)
        e.set_moments_dev(mu[0], cov[0])

        def dense():
            out["d"], _ = e.lnlike_ensemble(tt, ff, sd, conditional=True, rta1=rd, normalized=True, zmax=np.inf)

        dense_ms = timed(dense, reps)
        ref = out["d"].cpu().numpy()
        mine = np.array([got[s, j, k] for s, j, k in idx])
        per = dense_ms / DENSE
        total = per * S * J * P
        print(json.dumps(dict(K=K, ydeg=L, triples=S * J * P, basis_ms=round(ms_basis, 3),
                              dense_ms_per_triple=round(per, 4), dense_ms_scaled=round(total, 1),
                              speedup=round(total / ms_basis, 1),
                              max_rel_diff=float(np.max(np.abs(mine - ref) / np.abs(ref))))), flush=True)
        del e


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
