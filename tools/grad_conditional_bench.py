#!/usr/bin/env python
"""Time of the conditional branch's ensemble gradient in one device sweep (grad.EnsembleGradientConditional,
sp_lnlike_grad_conditional) beside the star-by-star route of the same tree (grad.ensemble_gradient_conditional), at the
headline shape: 64 stars, K = 1000, ydeg 15, the synthetic stars of SURVEY 8d with each star's own inclination.

    python tools/grad_conditional_bench.py [--stars 64] [--cadences 1000] [--calls 30] [--baseline-calls 2]
                                           [--sweep-only] [--out profiles/grad_conditional.txt]

Device events around every call of the sweep alone (the moments already on the device) and around every call of the
whole facade (moments with tangents, sweep, contraction, the one transfer), after 3 warm-up calls: median [min .. max]
of `--calls` calls.  The baseline is timed with the host clock around whole calls (it synchronises through its own
transfers).  --sweep-only: the warm-up and three sweeps, nothing else (the run to put under rocprofv3 --kernel-trace
--stats).  Needs a GPU: there is no other path."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from starry_process_amd.grad import EnsembleGradientConditional, ensemble_gradient_conditional  # noqa: E402
from starry_process_amd.synthetic import synthetic_star  # noqa: E402
from starry_process_amd.upstream_device import ylm_moments_device  # noqa: E402

HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return "%.3f [%.3f .. %.3f]" % (np.median(ms), ms[0], ms[-1])


def timed(fn, calls):
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=64)
    ap.add_argument("--cadences", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    S, K = a.stars, a.cadences
    sts = [synthetic_star(s, K) for s in range(S)]
    t, flux = np.array([s["t"] for s in sts]), np.array([s["flux"] for s in sts])
    p, inc = np.array([s["p"] for s in sts]), np.array([s["i"] for s in sts])
    eg = EnsembleGradientConditional(t, flux, ferr=1e-3, p=p, i=inc)
    e = eg._e
    e.set_moments_dev(*ylm_moments_device(e, **HP))

    def sweep():
        return e.lnlike_grad_conditional(eg._t, eg._flux, eg._stars, eg._rta1, workspace=eg._ws)

    for _ in range(3):
        sweep()
    torch.cuda.synchronize()
    if a.sweep_only:
        for _ in range(3):
            sweep()
        torch.cuda.synchronize()
        return
    ms_sweep = timed(sweep, a.calls)
    for _ in range(3):
        total, g = eg(wrt=("i", "p"), **HP)
    ms_call = timed(lambda: eg(wrt=("i", "p"), **HP), a.calls)
    ms_base = []
    for k in range(a.baseline_calls + 1):
        t0 = time.perf_counter()
        total0, g0, _ = ensemble_gradient_conditional(t, flux, ferr=1e-3, p=p, i=inc, **HP)
        torch.cuda.synchronize()
        if k:                                   # (the first call warms the single-star graph up)
            ms_base.append(1e3 * (time.perf_counter() - t0))
    scale = max(abs(g0[k]) for k in HP)
    dev = max(max(abs(g[k] - g0[k]) for k in HP) / scale,
              np.abs(g["i"] - g0["i"]).max() / np.abs(g0["i"]).max(), np.abs(g["p"] - g0["p"]).max() / np.abs(g0["p"]).max())
    lines = [
        "conditional-branch ensemble gradient: one MI355X, ydeg 15, S = %d, K = %d, normalized, data variance 1e-6" % (S, K),
        "(milliseconds: median [min .. max]; device events, 3 warm-up calls, %d timed calls; the baseline: host clock" % a.calls,
        " around %d whole calls after one warm-up call)" % a.baseline_calls,
        "",
        "  sp_lnlike_grad_conditional, the sweep alone          %s" % stats(ms_sweep),
        "  EnsembleGradientConditional(...)(wrt=('i', 'p'))     %s" % stats(ms_call),
        "  ensemble_gradient_conditional (star by star)         %s" % stats(ms_base),
        "  star by star over the one-sweep call                 %.1f" % (np.median(ms_base) / np.median(ms_call)),
        "",
        "  same inputs, both routes: total %.12g against %.12g; largest deviation of the gradient's entries" % (total, total0),
        "  (r, a, b, c, n relative to the largest of them; i and p relative to their largest): %.3g" % dev,
        "  workspace of the sweep: %d bytes" % eg._ws.numel(),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
