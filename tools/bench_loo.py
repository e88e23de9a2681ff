"""Leave-one-out predictive checks (Engine.loo_ensemble, sp_loo_ensemble) against the route composed from the entry
points that existed before it, timed with HIP events on device-resident inputs:

  fused      Engine.loo_ensemble: C assembled in the corner of the system, the identity through the factorisation,
             two passes over Y = L^-T; no C^-1, no [S, Kr, Kr] buffer
  composed   the same covariance from Engine.cov_marginal / cov_conditional into [S, K, K], the data variances and the
             baseline variance added in torch, Engine.spd_inverse (full C^-1), then ``diagonal`` and a batched
             matrix-vector product in torch and the five rows from alpha and d

at 64 stars x K = 1000, ydeg 15, and 32 stars x K = 3000, ydeg 20, both branches, a normalised process.  Every shape
runs in a child process of its own under its own time limit.  Per shape one JSON line: milliseconds of both routes
(3 warm-up calls, then ROUNDS interleaved rounds of REPS timed calls; the median of the rounds' medians and their
lowest and highest), the ratio, the scratch bytes of each route (peak allocation beyond the results) and the largest
difference between the two results (z, relative to max|z|).  The lines go to --out (profiles/loo.txt).

    python tools/bench_loo.py [--reps 10] [--rounds 5] [--timeout 300] [--out profiles/loo.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

SHAPES = [(15, 64, 1000, True), (15, 64, 1000, False), (20, 32, 3000, True), (20, 32, 3000, False)]


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


def shape(ydeg, S, K, marginal, reps, rounds):
    import torch

    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import make_stars

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    sp = StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"],
                       marginalize_over_inclination=marginal)
    e, f = sp._engine, sp._flux
    rng = np.random.RandomState(K)
    tt = np.ascontiguousarray(np.broadcast_to(np.linspace(0, 30.0 * K / 1000, K), (S, K)))
    p = rng.uniform(0.5, 3.0, S)
    flux = 1.0 + 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K)
    bvar = 1e-6
    stars = make_stars(S, period=p, inc_deg=rng.uniform(30.0, 85.0, S), baseline_mean=1.0, baseline_var=bvar)
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab = mv = None
    if marginal:
        tab, mv = e.kernel_table(rta1, 300)
    t, fl, sd = e.f64(tt), e.f64(flux), e.stars_to_device(stars)
    diag = e.f64(1e-6 * (1 + rng.rand(S, K)))
    ws = e.loo_workspace(S, K, 300, not marginal)
    kw = dict(diag=diag, conditional=not marginal, covpts=300, tab=tab, meanvar=mv, rta1=rta1)

    def fused():
        return e.loo_ensemble(t, fl, sd, workspace=ws, **kw)

    def composed():
        if marginal:
            C, _ = e.cov_marginal(t, stars, 300, tab, mv)
        else:
            C, _, _ = e.cov_conditional(t, stars, rta1)
        C.diagonal(dim1=1, dim2=2).add_(diag)
        C += bvar
        inv, _, _ = e.spd_inverse(C)
        r = fl - 1.0                                     # (normalised: the GP's mean is zero; baseline_mean = 1)
        d = inv.diagonal(dim1=1, dim2=2)
        alpha = torch.bmm(inv, r.unsqueeze(2)).squeeze(2)
        var, z = 1.0 / d, alpha / d.sqrt()
        return torch.stack([fl - alpha / d, var, z, -0.5 * torch.log(2 * np.pi * var) - 0.5 * z * z])

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref = composed()
    torch.cuda.synchronize()
    peak_composed = torch.cuda.max_memory_allocated() - base - ref.numel() * 8
    zc = ref[2].clone()
    del ref
    torch.cuda.empty_cache()
    got = fused()[0]
    torch.cuda.synchronize()
    diff = float((got[:, 2] - zc).abs().max() / zc.abs().max())
    del got, zc
    for _ in range(3):
        fused()
        composed()
    torch.cuda.synchronize()
    gf, gc = [], []
    for _ in range(rounds):
        gf.append(timed(fused, reps))
        gc.append(timed(composed, reps))
    Kr = (K + 63) // 64 * 64

    def stats(x):
        return dict(median=round(float(np.median(x)), 3), low=round(min(x), 3), high=round(max(x), 3))

    print(json.dumps(dict(
        what="loo", ydeg=ydeg, S=S, K=K, branch="marginal" if marginal else "conditional", reps=reps, rounds=rounds,
        fused_ms=stats(gf), composed_ms=stats(gc), composed_over_fused=round(float(np.median(gc) / np.median(gf)), 2),
        fused_workspace_bytes=int(ws.numel()), composed_scratch_bytes=int(peak_composed),
        inverse_bytes_not_allocated=int(8 * S * Kr * Kr), max_rel_difference_z=diff)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo.txt"))
    ap.add_argument("--shape", type=int, default=None, help="(internal) run this one shape in this process")
    a = ap.parse_args()
    if a.shape is not None:
        ydeg, S, K, marginal = SHAPES[a.shape]
        shape(ydeg, S, K, marginal, a.reps, a.rounds)
        return 0
    lines = []
    for k in range(len(SHAPES)):
        # a fresh child per shape under its own time limit; nothing more is started after one that fails
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--shape", str(k),
               "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print("shape %d: exit status %d; stopping" % (k, r.returncode), file=sys.stderr)
            return r.returncode
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
