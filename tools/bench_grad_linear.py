"""The gradient sweep with linear regressors marginalised out (Engine.lnlike_grad_linear, sp_lnlike_grad_linear) against
the plain sweep with the per-star derivatives (Engine.lnlike_grad_marginal_stars) on the same stars in the same run,
timed with HIP events on device-resident inputs:

  linear     C^-1 as the plain sweep takes it, ONE pass over its lower tiles for C^-1 [p, q, 1, r, U] on the matrix
             cores, the q x q stage, the mixing, the scalars, one pass over the lower tiles for B B^T, the scatter and
             the period / tau sums
  plain      the same stars without regressors: what the regressors cost

at 64 stars x K = 1000, ydeg 15, and 32 stars x K = 3000, ydeg 20, a normalised process, q = 4 (two offsets, a linear
and a quadratic column), q = 20 (17 offsets and a cubic) and q = 32 (eight segments of an offset and a cubic each).
Every shape runs in a child process of its own under its own time limit.  Per (shape, q) one JSON line: milliseconds of
the two routes (3 warm-up calls, then ROUNDS interleaved rounds of REPS timed calls; the median of the rounds' medians
and their lowest and highest), the ratio, the workspace bytes of each route and the largest relative difference between
the likelihoods of the sweep and of Engine.lnlike_linear.  The lines go to --out (profiles/grad_linear.txt).

    python tools/bench_grad_linear.py [--reps 10] [--rounds 5] [--timeout 300] [--out profiles/grad_linear.txt]

For a kernel trace (run on its own, no timing in the same run):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_grad_linear.py --shape 0 --trace 20 --calls 10

runs `--calls` calls of the plain sweep and of the sweep with q = 20 regressors of shape 0 and nothing else.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

SHAPES = [(15, 64, 1000), (20, 32, 3000)]
QS = (4, 20, 32)


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


def regressors(K, q, t1):
    """(U [K, q], lam [q]) of the bench: offsets first, then the trends."""
    from starry_process_amd import linear

    if q == 32:
        edges = np.round(np.linspace(0, K, 9)).astype(int)
        U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t1, 3, edges))
        noff = 8
    else:
        noff, deg = (2, 2) if q == 4 else (17, 3)
        edges = np.round(np.linspace(0, K, noff + 1)).astype(int)
        U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t1, deg))
    assert U.shape == (K, q)
    return U, np.array([1e-4] * noff + [2.5e-5] * (q - noff))


def setup(ydeg, S, K, qs):
    """The engine, the plain sweep and one sweep with regressors per q, as closures on device-resident inputs."""
    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import make_stars

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    sp = StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"])
    e, f = sp._engine, sp._flux
    rng = np.random.RandomState(K)
    t1 = np.linspace(0, 30.0 * K / 1000, K)
    tt = np.ascontiguousarray(np.broadcast_to(t1, (S, K)))
    p = rng.uniform(0.5, 3.0, S)
    base = 1.0 + 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K)
    stars = make_stars(S, period=p, baseline_mean=1.0, baseline_var=1e-6)
    f._bind()
    tab, mv = e.kernel_table(e.f64(e.rTA1L(np.array([[0.3, 0.1]]))), 300)
    t, sd = e.f64(tt), e.stars_to_device(stars)
    diag = e.f64(1e-6 * (1 + rng.rand(S, K)))
    ws0 = e.grad_workspace(S, K, 300, 1)
    fl0 = e.f64(base)

    def plain():
        return e.lnlike_grad_marginal_stars(t, fl0, sd, tab, mv, diag=diag, covpts=300, workspace=ws0)

    lin = {}
    for q in qs:
        U, lam = regressors(K, q, t1)
        fl = e.f64(base + (rng.randn(S, q) * np.sqrt(lam)) @ U.T)
        Ud = e.f64(np.ascontiguousarray(np.broadcast_to(U.T, (S, q, K))))
        lamd = e.f64(np.ascontiguousarray(np.broadcast_to(lam, (S, q))))
        ws = e.grad_linear_workspace(S, K, q, 300)

        def call(fl=fl, Ud=Ud, lamd=lamd, ws=ws):
            return e.lnlike_grad_linear(t, fl, sd, Ud, lamd, tab, mv, diag=diag, covpts=300, workspace=ws)

        def value(fl=fl, Ud=Ud, lamd=lamd):
            return e.lnlike_linear(t, fl, sd, Ud, lamd, diag=diag, covpts=300, tab=tab, meanvar=mv, return_cov=False)

        lin[q] = (call, value, int(ws.numel()))
    return plain, lin, int(ws0.numel())


def shape(ydeg, S, K, reps, rounds):
    import torch

    plain, lin, ws0 = setup(ydeg, S, K, QS)
    diff = {}
    for q, (call, value, _) in lin.items():
        got, ref = call(), value()
        torch.cuda.synchronize()
        assert not bool(got[6].any()), got[6]
        diff[q] = float(((got[0] - ref[0]) / ref[0]).abs().max())
    for _ in range(3):
        plain()
        for q in QS:
            lin[q][0]()
    torch.cuda.synchronize()
    gp, gl = [], {q: [] for q in QS}
    for _ in range(rounds):
        gp.append(timed(plain, reps))
        for q in QS:
            gl[q].append(timed(lin[q][0], reps))

    def stats(x):
        return dict(median=round(float(np.median(x)), 3), low=round(min(x), 3), high=round(max(x), 3))

    for q in QS:
        print(json.dumps(dict(
            what="grad_linear", ydeg=ydeg, S=S, K=K, q=q, reps=reps, rounds=rounds, linear_ms=stats(gl[q]),
            plain_ms=stats(gp), linear_over_plain=round(float(np.median(gl[q]) / np.median(gp)), 3),
            linear_workspace_bytes=lin[q][2], plain_workspace_bytes=ws0,
            workspace_ratio=round(lin[q][2] / ws0, 4), max_rel_difference_lnlike_vs_lnlike_linear=diff[q])), flush=True)


def trace(ydeg, S, K, q, calls):
    import torch

    plain, lin, _ = setup(ydeg, S, K, (q,))
    for _ in range(calls):
        plain()
    for _ in range(calls):
        lin[q][0]()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_linear.txt"))
    ap.add_argument("--shape", type=int, default=None, help="(internal) run this one shape in this process")
    ap.add_argument("--trace", type=int, default=None, metavar="Q",
                    help="with --shape: only --calls calls of the plain sweep and of the sweep with Q regressors")
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    if a.shape is not None:
        ydeg, S, K = SHAPES[a.shape]
        if a.trace is not None:
            trace(ydeg, S, K, a.trace, a.calls)
        else:
            shape(ydeg, S, K, a.reps, a.rounds)
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
