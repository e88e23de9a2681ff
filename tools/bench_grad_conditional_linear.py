"""The conditional-branch gradient sweep with linear regressors marginalised out
(Engine.lnlike_grad_conditional_linear, sp_lnlike_grad_conditional_linear) against the plain conditional sweep
(Engine.lnlike_grad_conditional) on the same stars in the same run, timed with HIP events on device-resident inputs:

  linear     the plain sweep's forward, ONE pass over the lower tiles of C^-1 for C^-1 [p, q, 1, r, U] on the matrix
             cores, the q x q stage, the mixing, the scalars, then the tile kernel with the 64 x 64 block of B B^T in
             the place of alpha alpha^T, and the plain sweep's tail
  plain      the same stars without regressors: what the regressors cost

at 64 stars x K = 1000, ydeg 15, and 32 stars x K = 3000, ydeg 20, a normalised process, q = 4, 20 and 32 (the bases of
tools/bench_grad_linear.py).  Every shape runs in a child process of its own under its own time limit.  Per (shape, q)
one JSON line: milliseconds of the two routes (3 warm-up calls, then ROUNDS interleaved rounds of REPS timed calls; the
median of the rounds' medians and their lowest and highest), the difference and the ratio, the workspace bytes of each
route and the largest relative difference between the likelihoods of the sweep and of Engine.lnlike_linear on the
conditional branch.  The lines go to --out (profiles/grad_conditional_linear.txt).

    python tools/bench_grad_conditional_linear.py [--reps 10] [--rounds 5] [--timeout 400] [--out FILE]

For a kernel trace (run on its own, no timing in the same run):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_grad_conditional_linear.py --shape 0 --trace 20

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_grad_linear import QS, SHAPES, regressors, timed  # noqa: E402


def setup(ydeg, S, K, qs):
    """The engine at the golden moments, the plain sweep and one sweep with regressors per q, as closures on
    device-resident inputs."""
    from starry_process_amd.engine import get_engine, make_stars

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    e = get_engine(ydeg, 2)
    e.set_moments(mom["default_mean_ylm"], mom["default_cov_ylm"])
    rng = np.random.RandomState(K)
    t1 = np.linspace(0, 30.0 * K / 1000, K)
    tt = np.ascontiguousarray(np.broadcast_to(t1, (S, K)))
    p = rng.uniform(0.5, 3.0, S)
    inc = rng.uniform(30.0, 85.0, S)
    base = 1.0 + 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K)
    sd = e.stars_to_device(make_stars(S, period=p, inc_deg=inc, baseline_mean=1.0, baseline_var=1e-6))
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    t = e.f64(tt)
    diag = e.f64(1e-6 * (1 + rng.rand(S, K)))
    ws0 = e.grad_conditional_workspace(S, K)
    fl0 = e.f64(base)

    def plain():
        return e.lnlike_grad_conditional(t, fl0, sd, rta1, diag=diag, workspace=ws0)

    ws = e.grad_conditional_linear_workspace(S, K, max(qs))       # (one scratch for every q: the largest)
    lin = {}
    for q in qs:
        U, lam = regressors(K, q, t1)
        fl = e.f64(base + (rng.randn(S, q) * np.sqrt(lam)) @ U.T)
        Ud = e.f64(np.ascontiguousarray(np.broadcast_to(U.T, (S, q, K))))
        lamd = e.f64(np.ascontiguousarray(np.broadcast_to(lam, (S, q))))
        nbytes = int(e._L.sp_lnlike_grad_conditional_linear_workspace_bytes(e._h, S, K, q))

        def call(fl=fl, Ud=Ud, lamd=lamd):
            return e.lnlike_grad_conditional_linear(t, fl, sd, Ud, lamd, rta1, diag=diag, workspace=ws)

        def value(fl=fl, Ud=Ud, lamd=lamd):
            return e.lnlike_linear(t, fl, sd, Ud, lamd, diag=diag, conditional=True, rta1=rta1, return_cov=False)

        lin[q] = (call, value, nbytes)
    return plain, lin, int(ws0.numel())


def shape(ydeg, S, K, reps, rounds):
    import torch

    plain, lin, ws0 = setup(ydeg, S, K, QS)
    diff = {}
    for q in QS:
        got, ref = lin[q][0](), lin[q][1]()
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
            what="grad_conditional_linear", ydeg=ydeg, S=S, K=K, q=q, reps=reps, rounds=rounds, linear_ms=stats(gl[q]),
            plain_ms=stats(gp), linear_minus_plain_ms=round(float(np.median(gl[q]) - np.median(gp)), 3),
            linear_over_plain=round(float(np.median(gl[q]) / np.median(gp)), 3), linear_workspace_bytes=lin[q][2],
            plain_workspace_bytes=ws0, workspace_ratio=round(lin[q][2] / ws0, 4),
            max_rel_difference_lnlike_vs_lnlike_linear=diff[q])), flush=True)


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
    ap.add_argument("--timeout", type=int, default=400, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_conditional_linear.txt"))
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
