"""The inclination grid with its gradient (Engine.lnlike_inclinations_grad, sp_lnlike_inclinations_grad) against the
value-only grid on the same plan and against the dense conditional sweep, timed with HIP events on device-resident
inputs:

  grad       Engine.lnlike_inclinations_grad: S stars x P inclinations, values, Pd directional derivatives and the
             mixture over the grid, from the plan of sp_incl_plan_data
  value      sp_lnlike_inclinations_planned on the same plan and the same moments: what the gradient costs over the value
  facade     EnsembleGradientInclinations.__call__: the upstream's moments and tangents, the sweep, one transfer
  dense      EnsembleGradientConditional.__call__ on the same S stars at ONE inclination each: the K x K route; per
             (star, inclination) it is compared with grad / P

at 64 stars, K = 1000, ydeg 15 and K = 3000, ydeg 20, P = 100 inclinations, Pd = 5 directions (r, a, b, c, n), a
normalised process.  With --wrt (names out of p, baseline_mean, baseline_var, log_var, separated by commas) three more:

  grad_stars    the same call with the per-star slots of --wrt (sp_lnlike_inclinations_grad_stars): what each star's own
                derivatives cost over the shared gradient
  facade_stars  EnsembleGradientInclinations.__call__(wrt=...)
  tangent       Engine.incl_plan_tangent, the plan's derivative along the periods: once per data set, not per call

and the lines go to profiles/incl_grad_stars.txt.  Every shape runs in a child process of its own under its own time limit.  Per shape one JSON line:
milliseconds of each route (3 warm-up calls, then ROUNDS interleaved rounds of REPS timed calls; the median of the
rounds' medians and their lowest and highest) and the ratios.  The lines go to --out (profiles/incl_grad.txt).

    python tools/bench_incl_grad.py [--reps 10] [--rounds 5] [--timeout 300] [--out profiles/incl_grad.txt]
                                    [--wrt p,baseline_mean,baseline_var,log_var]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

# (ydeg, S, K, P)
SHAPES = [(15, 64, 1000, 100), (20, 64, 3000, 100)]
HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)


def timed(fn, reps):
    import torch

    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def shape(ydeg, S, K, P, reps, rounds, wrt=()):
    import torch

    from starry_process_amd._lib import check
    from starry_process_amd.grad import EnsembleGradientConditional, EnsembleGradientInclinations, _moment_tangents

    rng = np.random.RandomState(K)
    tt = np.ascontiguousarray(np.broadcast_to(np.linspace(0, 30.0 * K / 1000, K), (S, K)))
    p = rng.uniform(0.5, 3.0, S)
    flux = 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K)
    inc = np.linspace(0.0, 90.0, P)
    eg = EnsembleGradientInclinations(tt, flux, ferr=1e-3, p=p, inc=inc, ydeg=ydeg)
    egc = EnsembleGradientConditional(tt, flux, ferr=1e-3, p=p, i=rng.uniform(30.0, 85.0, S), ydeg=ydeg)
    assert eg._dense.size == 0
    e = eg._e
    names = ("r", "a", "b", "c", "n")
    mu, Sig, dmu, dSig = _moment_tangents(e, {}, names, **HP)
    n = 2 * ydeg + 1

    def grad():
        return e.lnlike_inclinations_grad(eg._plan, eg._stars, eg._rta1, mu, Sig, dmu, dSig, eg._inc_rad,
                                          logw=eg._logw_dev)

    vout = e.empty(S, 1, P)
    vstat = torch.zeros(S, 1, P, dtype=torch.int32, device=e.device)
    ntab = int(eg._rta1.shape[0])
    vws = e._scratch(e._L.sp_lnlike_inclinations_workspace_bytes(e._h, S, 1, ntab, 1, P))

    def value():
        check(e._L.sp_lnlike_inclinations_planned(
            e._h, S, 1, e._p(eg._plan), e._p(eg._stars), e._p(eg._rta1), ntab, 1, e._p(mu), e._p(Sig), 1, None, P,
            e._p(eg._inc_rad), 1, 20, 0.023, e._p(vout), e._p(vstat), e._p(vws), e._stream()))

    def facade():
        return eg(**HP)

    def dense():
        return egc(**HP)

    routes = dict(grad=grad, value=value, facade=facade, dense=dense)
    if wrt:
        from starry_process_amd.grad import _WRT_INCL

        mask = sum(1 << _WRT_INCL.index(k) for k in set(wrt))

        def grad_stars():
            return e.lnlike_inclinations_grad(eg._plan, eg._stars, eg._rta1, mu, Sig, dmu, dSig, eg._inc_rad,
                                              logw=eg._logw_dev, star_tangent=eg._ptan if mask & 1 else None,
                                              star_mask=mask)

        def facade_stars():
            return eg(wrt=wrt, **HP)

        def tangent():
            return e.incl_plan_tangent(eg._t, eg._flux, eg._stars, eg._plan, eg._diag)

        routes.update(grad_stars=grad_stars, facade_stars=facade_stars, tangent=tangent)
    for _ in range(3):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    diff = float((grad()[0] - vout[:, 0, :]).abs().max())
    got = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            got[k].append(timed(fn, reps))

    def stats(x):
        return dict(median=round(float(np.median(x)), 3), low=round(min(x), 3), high=round(max(x), 3))

    med = {k: float(np.median(v)) for k, v in got.items()}
    extra = {}
    if wrt:
        extra = dict(wrt=list(wrt), grad_stars_ms=stats(got["grad_stars"]), facade_stars_ms=stats(got["facade_stars"]),
                     tangent_ms=stats(got["tangent"]), grad_stars_over_grad=round(med["grad_stars"] / med["grad"], 2),
                     facade_stars_over_facade=round(med["facade_stars"] / med["facade"], 2),
                     grad_stars_us_per_star_inclination=round(1e3 * med["grad_stars"] / (S * P), 3))
    print(json.dumps(dict(
        what="incl_grad", ydeg=ydeg, n=n, S=S, K=K, P=P, Pd=len(names), reps=reps, rounds=rounds,
        grad_ms=stats(got["grad"]), value_ms=stats(got["value"]), facade_ms=stats(got["facade"]),
        dense_ms=stats(got["dense"]), grad_over_value=round(med["grad"] / med["value"], 2),
        grad_us_per_star_inclination=round(1e3 * med["grad"] / (S * P), 3),
        dense_us_per_star_inclination=round(1e3 * med["dense"] / S, 3),
        dense_over_grad_per_star_inclination=round((med["dense"] / S) / (med["grad"] / (S * P)), 1),
        max_abs_value_difference=diff, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--out", default=None, help="profiles/incl_grad.txt, or profiles/incl_grad_stars.txt with --wrt")
    ap.add_argument("--wrt", default="", help="per-star names, separated by commas: also time the call with them")
    ap.add_argument("--shape", type=int, default=None, help="(internal) run this one shape in this process")
    a = ap.parse_args()
    wrt = tuple(k for k in a.wrt.split(",") if k)
    if wrt:
        from starry_process_amd.grad import _check_wrt_inclinations

        _check_wrt_inclinations(wrt)
    out = a.out or os.path.join(ROOT, "profiles", "incl_grad_stars.txt" if wrt else "incl_grad.txt")
    if a.shape is not None:
        ydeg, S, K, P = SHAPES[a.shape]
        shape(ydeg, S, K, P, a.reps, a.rounds, wrt)
        return 0
    lines = []
    for k in range(len(SHAPES)):
        # a fresh child per shape under its own time limit; nothing more is started after one that fails
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--shape", str(k),
               "--reps", str(a.reps), "--rounds", str(a.rounds)] + (["--wrt", ",".join(wrt)] if wrt else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print("shape %d: exit status %d; stopping" % (k, r.returncode), file=sys.stderr)
            return r.returncode
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
