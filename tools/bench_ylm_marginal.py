"""Surface-map posterior with the inclination marginalised (sp_ylm_conditional_inclinations) against the
dense route (StarryProcess._ylm_marginal_dense: ylm_conditional on star x inclination pseudo-stars, weights from the
dense likelihood, the mixture with torch), timed with HIP events:

  S = 64, K = 1000, ydeg 15, P = 100   and   S = 32, K = 3000, ydeg 20, P = 100,   with and without the covariance.

The two routes alternate in one process; after a warm-up each figure is the median of 5 calls.  The dense route is timed
on the first `dense_stars` stars (default 2) and scaled to S: its cost is linear in the stars, which it works one by one.
One JSON line per shape and return_cov: ms per call for both routes, the speed-up, the share of the 78.6 TFLOP/s fp64
matrix peak the mixture product reaches on the flops it executes (lower 64 x 64 tiles of stack stack^T and
spread spread^T, padding included; from a separate timing of the call without the covariance), and the largest deviation
between the routes over the dense stars in posterior sd.

    python tools/bench_ylm_marginal.py [dense_stars] > profiles/ylm_marginal.txt
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd import StarryProcess  # noqa: E402

SHAPES = [(64, 1000, 15, 100), (32, 3000, 20, 100)]
PEAK = 78.6e12
REPS = 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    nd = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    for S, K, L, P in SHAPES:
        mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % L))
        sp = StarryProcess(ydeg=L, normalized=False, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"])
        rng = np.random.RandomState(S + K)
        t = np.linspace(0, 3, K)
        p = 0.6 + rng.rand(S)
        flux = 1e-3 * np.sin(2 * np.pi * t[None, :] / p[:, None]) + 1e-3 * rng.randn(S, K)
        inc = np.linspace(0, 90, P)
        logw = sp._log_weights(sp._inc_prior_weights(inc, None))
        tt, ff, stars, utab, diag = sp._ensemble_args(t, flux, 1e-6, None, p, None, 0.0, 1e-6)
        n, Np = 2 * L + 1, 64 * (((L + 1) ** 2 + 63) // 64)
        nt = Np // 64
        flops = S * (nt * (nt + 1) // 2) * 2 * 64 * 64 * (32 * ((P * n + 31) // 32) + 32 * ((P + 31) // 32))

        def new(cov):
            return sp._ylm_marginal(tt, ff, stars, utab, diag, inc, logw, cov, 0, None)

        def dense(cov):
            return [sp._ylm_marginal_dense(tt[s], ff[s], 1e-6, inc, logw, p[s], utab[0], 0.0, 1e-6, return_cov=cov)
                    for s in range(nd)]

        res = {}
        for cov in (True, False):
            t_new, out = timed(lambda: new(cov))
            t_den, ref = timed(lambda: dense(cov))
            t_new2, _ = timed(lambda: new(cov))
            t_den2, _ = timed(lambda: dense(cov))
            dev = 0.0
            for s in range(nd):
                sd = torch.sqrt(torch.diagonal(ref[s][2])) if cov else res[True][s]
                dev = max(dev, float(torch.max(torch.abs(out[1][s] - ref[s][1]) / sd)))
                if cov:
                    dev = max(dev, float(torch.max(torch.abs(out[2][s] - ref[s][2]) / torch.outer(sd, sd))))
            if cov:
                res[True] = [torch.sqrt(torch.diagonal(ref[s][2])) for s in range(nd)]
                t_cov = min(t_new, t_new2)
            line = dict(S=S, K=K, ydeg=L, P=P, return_cov=cov, new_ms=[round(t_new, 3), round(t_new2, 3)],
                        dense_ms_scaled=[round(t_den * S / nd, 1), round(t_den2 * S / nd, 1)], dense_stars=nd,
                        speedup=round(min(t_den, t_den2) * S / nd / min(t_new, t_new2), 1), routes_dev_sd=dev)
            if not cov:
                prod_ms = t_cov - min(t_new, t_new2)   # stack, products and final pass
                line.update(cov_stage_ms=round(prod_ms, 3), product_gflop_executed=round(flops / 1e9, 2),
                            cov_stage_frac_peak=round(flops / (prod_ms * 1e-3) / PEAK, 3))
            print(json.dumps(line), flush=True)
        del sp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
