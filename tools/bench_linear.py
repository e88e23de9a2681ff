"""The likelihood with linear regressors marginalised out (Engine.lnlike_linear, sp_lnlike_linear) against two
yardsticks, neither of which is the code under test, timed with HIP events on device-resident inputs:

  linear     Engine.lnlike_linear: C assembled in the corner of the system, the residual and the q regressors riding
             through the factorisation, one pass along the 1 + q rows and a q x q system per star
  plain      Engine.lnlike_ensemble (unplanned) on the same stars without regressors: what the regressors cost
  composed   the reference's matrix baseline_var done on the device: the covariance from Engine.cov_marginal /
             cov_conditional into [S, K, K], the data variances, the baseline variance and U Lambda U^T added in torch,
             Engine.cho_factor and Engine.cho_solve, the likelihood from the solve and the factor's diagonal

at 64 stars x K = 1000, ydeg 15, and 32 stars x K = 3000, ydeg 20, both branches, a normalised process, q = 4 (two
offsets, a linear and a quadratic column) and q = 20 (17 offsets and a cubic).  Every configuration runs in a child
process of its own under its own time limit.  Per configuration one JSON line: milliseconds of the three routes
(3 warm-up calls, then ROUNDS interleaved rounds of REPS timed calls; the median of the rounds' medians and their
lowest and highest), the ratios, the scratch bytes of each route and the largest relative difference between the
likelihoods of the linear and the composed route.  The lines go to --out (profiles/linear.txt).

    python tools/bench_linear.py [--reps 10] [--rounds 5] [--timeout 300] [--out profiles/linear.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

SHAPES = [(ydeg, S, K, marginal, q) for ydeg, S, K in ((15, 64, 1000), (20, 32, 3000)) for marginal in (True, False)
          for q in (4, 20)]


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


def shape(ydeg, S, K, marginal, q, reps, rounds):
    import torch

    from starry_process_amd import StarryProcess, linear
    from starry_process_amd.engine import make_stars

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    sp = StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"],
                       marginalize_over_inclination=marginal)
    e, f = sp._engine, sp._flux
    rng = np.random.RandomState(K)
    t1 = np.linspace(0, 30.0 * K / 1000, K)
    tt = np.ascontiguousarray(np.broadcast_to(t1, (S, K)))
    p = rng.uniform(0.5, 3.0, S)
    noff, deg = (2, 2) if q == 4 else (17, 3)
    edges = np.round(np.linspace(0, K, noff + 1)).astype(int)
    U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t1, deg))
    assert U.shape == (K, q)
    lam = np.array([1e-4] * noff + [2.5e-5] * deg)
    w = rng.randn(S, q) * np.sqrt(lam)
    flux = 1.0 + 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K) + w @ U.T
    bvar = 1e-6
    stars = make_stars(S, period=p, inc_deg=rng.uniform(30.0, 85.0, S), baseline_mean=1.0, baseline_var=bvar)
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab = mv = None
    if marginal:
        tab, mv = e.kernel_table(rta1, 300)
    t, fl, sd = e.f64(tt), e.f64(flux), e.stars_to_device(stars)
    fl3 = fl.unsqueeze(1).contiguous()
    diag = e.f64(1e-6 * (1 + rng.rand(S, K)))
    Ud = e.f64(np.ascontiguousarray(np.broadcast_to(U.T, (S, q, K))))
    lamd = e.f64(np.ascontiguousarray(np.broadcast_to(lam, (S, q))))
    ULU = e.f64((U * lam) @ U.T)
    ws = e.lnlike_linear_workspace(S, K, q, 300, not marginal)
    ws0 = e.workspace(S, K, 1)
    kw = dict(diag=diag, conditional=not marginal, covpts=300, tab=tab, meanvar=mv, rta1=rta1)

    def lin():
        return e.lnlike_linear(t, fl, sd, Ud, lamd, workspace=ws, **kw)

    def plain():
        return e.lnlike_ensemble(t, fl3, sd, workspace=ws0, **kw)

    def composed():
        if marginal:
            C, _ = e.cov_marginal(t, stars, 300, tab, mv)
        else:
            C, _, _ = e.cov_conditional(t, stars, rta1)
        C.diagonal(dim1=1, dim2=2).add_(diag)
        C += bvar
        C += ULU
        L, _ = e.cho_factor(C)
        r = fl - 1.0                                     # (normalised: the GP's mean is zero; baseline_mean = 1)
        x = e.cho_solve(L, r.unsqueeze(2)).squeeze(2)
        return -0.5 * (r * x).sum(1) - L.diagonal(dim1=1, dim2=2).log().sum(1) - 0.5 * K * np.log(2 * np.pi)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref = composed()
    torch.cuda.synchronize()
    peak_composed = torch.cuda.max_memory_allocated() - base - ref.numel() * 8
    got = lin()
    torch.cuda.synchronize()
    assert not bool(got[4].any()), got[4]
    diff = float(((got[0] - ref) / ref).abs().max())
    gain = float((got[0] - got[1]).median())
    diff0 = float(((got[1] - plain()[0]) / got[1]).abs().max())
    del ref, got
    torch.cuda.empty_cache()
    for _ in range(3):
        lin()
        plain()
        composed()
    torch.cuda.synchronize()
    gl, gp, gc = [], [], []
    for _ in range(rounds):
        gl.append(timed(lin, reps))
        gp.append(timed(plain, reps))
        gc.append(timed(composed, reps))

    def stats(x):
        return dict(median=round(float(np.median(x)), 3), low=round(min(x), 3), high=round(max(x), 3))

    print(json.dumps(dict(
        what="linear", ydeg=ydeg, S=S, K=K, q=q, branch="marginal" if marginal else "conditional", reps=reps,
        rounds=rounds, linear_ms=stats(gl), plain_ms=stats(gp), composed_ms=stats(gc),
        linear_over_plain=round(float(np.median(gl) / np.median(gp)), 3),
        composed_over_linear=round(float(np.median(gc) / np.median(gl)), 2),
        linear_workspace_bytes=int(ws.numel()), plain_workspace_bytes=int(ws0.numel()),
        composed_scratch_bytes=int(peak_composed), max_rel_difference_lnlike=diff,
        max_rel_difference_lnlike0_vs_plain=diff0, median_lnlike_minus_lnlike0=round(gain, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear.txt"))
    ap.add_argument("--shape", type=int, default=None, help="(internal) run this one configuration in this process")
    a = ap.parse_args()
    if a.shape is not None:
        ydeg, S, K, marginal, q = SHAPES[a.shape]
        shape(ydeg, S, K, marginal, q, a.reps, a.rounds)
        return 0
    lines = []
    for k in range(len(SHAPES)):
        # a fresh child per configuration under its own time limit; nothing more is started after one that fails
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--shape", str(k),
               "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print("configuration %d: exit status %d; stopping" % (k, r.returncode), file=sys.stderr)
            return r.returncode
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
