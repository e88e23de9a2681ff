"""Conditional light curves with linear regressors marginalised out (Engine.predict_linear, sp_predict_linear), timed with
HIP events on device-resident inputs against

  plain      Engine.predict_ensemble without a basis on the same stars in the same rounds: the difference is what the
             regressors cost (q more riding rows through the factorisation, the Gram matrix and the q x q finish, the
             matrix-core pass over Y in place of predict_reduce_kernel and, in full mode, C += Z Z^T)

at 64 stars x K = Ks = 1000, ydeg 15, and 32 stars x K = Ks = 3000, ydeg 20, marginal branch, with q = 4, 20 and 32
regressors (segment offsets, then Legendre columns over the whole light curve; the regressors at the sample times from
linear.offset_basis_at / polynomial_basis_at) in the modes "diag" and full covariance.  Every case runs in a child
process of its own under its own time limit.  Per case one JSON line: milliseconds of the two routes (3 warm-up calls,
then ROUNDS interleaved rounds of REPS timed calls; the median of the rounds' medians and their lowest and highest), the
ratio, the workspace bytes of both routes and the largest difference between the two routes' means when every variance is
zero.  The lines go to --out (profiles/predict_linear.txt).

    python tools/bench_predict_linear.py [--reps 10] [--rounds 5] [--timeout 300] [--out profiles/predict_linear.txt]

One case alone (--case N --reps 2 --rounds 1) under a kernel trace gives the times of predict_reduce_linear_kernel and of
predict_reduce_kernel<true> on the same Y.
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
CASES = [(k, q, mode) for k in range(len(SHAPES)) for q in (4, 20, 32) for mode in ("diag", True)]


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


def case(ydeg, S, K, q, mode, reps, rounds):
    import torch

    from starry_process_amd import StarryProcess, linear
    from starry_process_amd.engine import make_stars

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    sp = StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], normalized=False)
    e, f = sp._engine, sp._flux
    Ks = K
    rng = np.random.RandomState(K)
    t1 = np.linspace(0, 30.0 * K / 1000, K)
    tt = np.ascontiguousarray(np.broadcast_to(t1, (S, K)))
    ts1 = np.sort(rng.uniform(-1.0, t1[-1] + 2.0, Ks))                      # gaps filled and a forecast past the end
    tsd = np.ascontiguousarray(np.broadcast_to(ts1, (S, Ks)))
    p = rng.uniform(0.5, 3.0, S)
    flux = 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K)
    noff = q if q < 8 else q - 3
    edges = np.round(np.linspace(0, K, noff + 1)).astype(int)
    U, Us = linear.offset_basis(K, edges), linear.offset_basis_at(ts1, t1, edges)
    if q >= 8:
        U = linear.stack_bases(U, linear.polynomial_basis(t1, 3))
        Us = linear.stack_bases(Us, linear.polynomial_basis_at(ts1, t1, 3))
    lamh = np.ascontiguousarray(np.broadcast_to(np.where(np.arange(q) < noff, 1e-4, 2.5e-5), (S, q)))
    flux = flux + (rng.randn(S, q) * np.sqrt(lamh)) @ U.T
    stars = make_stars(S, period=p, inc_deg=rng.uniform(30.0, 85.0, S), baseline_mean=0.0, baseline_var=1e-6)
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab, mv = e.kernel_table(rta1, 300)
    t, ts, fl, sd = e.f64(tt), e.f64(tsd), e.f64(flux), e.stars_to_device(stars)
    diag = e.f64(1e-6 * (1 + rng.rand(S, K)))
    Ud = e.f64(np.ascontiguousarray(np.broadcast_to(U.T, (S, q, K))))
    Usd = e.f64(np.ascontiguousarray(np.broadcast_to(Us, (S, Ks, q))))
    lam = e.f64(lamh)
    wl = e.predict_linear_workspace(S, K, Ks, q, 300)
    plain_bytes = int(e._L.sp_predict_workspace_bytes(e._h, S, K, Ks, 300))
    kw = dict(diag=diag, covpts=300, tab=tab, meanvar=mv, rta1=rta1, mode=mode)

    def fused():
        return e.predict_linear(t, ts, fl, sd, Ud, lam, Usd, workspace=wl, **kw)

    def plain():
        return e.predict_ensemble(t, ts, fl, sd, **kw)

    ref = plain()
    zero = e.predict_linear(t, ts, fl, sd, Ud, torch.zeros_like(lam), Usd, workspace=wl, **kw)
    got = fused()
    torch.cuda.synchronize()
    dmu = float((zero[0] - ref[0]).abs().max() / ref[0].abs().max())
    flags = int(got[6].abs().max()) | int(got[2].abs().max())
    del ref, zero, got
    for _ in range(3):
        fused()
        plain()
    torch.cuda.synchronize()
    gf, gl = [], []
    for _ in range(rounds):
        gf.append(timed(fused, reps))
        gl.append(timed(plain, reps))

    def stats(x):
        return dict(median=round(float(np.median(x)), 3), low=round(min(x), 3), high=round(max(x), 3))

    print(json.dumps(dict(
        what="predict_linear", ydeg=ydeg, S=S, K=K, Ks=Ks, branch="marginal", q=q, mode="full" if mode is True else mode,
        reps=reps, rounds=rounds, fused_ms=stats(gf), plain_ms=stats(gl),
        fused_over_plain=round(float(np.median(gf) / np.median(gl)), 3),
        fused_minus_plain_ms=round(float(np.median(gf) - np.median(gl)), 3),
        fused_workspace_bytes=int(wl.numel()), plain_workspace_bytes=plain_bytes,
        y_bytes_per_call=int(8 * S * Ks * K), max_rel_difference_mu_at_zero_variance=dmu, status_flags=flags)),
        flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_linear.txt"))
    ap.add_argument("--case", type=int, default=None, help="(internal) run this one case in this process")
    a = ap.parse_args()
    if a.case is not None:
        k, q, mode = CASES[a.case]
        ydeg, S, K = SHAPES[k]
        case(ydeg, S, K, q, mode, a.reps, a.rounds)
        return 0
    lines = []
    for k in range(len(CASES)):
        # a fresh child per case under its own time limit; nothing more is started after one that fails
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", str(k),
               "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print("case %d: exit status %d; stopping" % (k, r.returncode), file=sys.stderr)
            return r.returncode
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        # (written after every case: a later case that fails leaves the earlier lines)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
