"""Leave-block-out predictive checks with linear regressors marginalised out (Engine.lbo_linear, sp_lbo_linear), timed
with HIP events on device-resident inputs against

  plain      Engine.lbo_ensemble without a basis on the same stars in the same rounds: the difference is what the
             regressors cost (the column pass W^T = U^T Y, the Gram matrix and the q x q finish, T and y~, and the
             downdate in the band kernel)
  composed   the route composed from the entry points that existed before: the covariance from Engine.cov_marginal /
             cov_conditional into [S, K, K], the data variances, the baseline variance and U Lambda U^T added in torch,
             Engine.spd_inverse (full C~^-1), the diagonal blocks cut out in torch, ``torch.linalg.cholesky`` /
             ``cholesky_inverse`` / ``solve_triangular`` batched over stars and blocks (blocks of one cadence:
             elementwise), and a batched matrix-vector product for alpha~ = C~^-1 r

at 64 stars x K = 1000, ydeg 15, and 32 stars x K = 3000, ydeg 20, both branches, a normalised process, with q = 4, 20
and 32 regressors (segment offsets, then Legendre columns over the whole light curve) and blocks of 64, 8 and 1 cadences
-- the last is the route loo_ensemble(basis=...) takes.  Every case runs in a child process of its own under its own
time limit.  Per case one JSON line: milliseconds of the three routes (3 warm-up calls, then ROUNDS interleaved rounds of
REPS timed calls; the median of the rounds' medians and their lowest and highest), the ratios, the scratch bytes and the
largest differences between the fused and the composed results (u and lpd, relative to max|u| and max(1, |lpd|)).  The
lines go to --out (profiles/lbo_linear.txt).

    python tools/bench_lbo_linear.py [--reps 10] [--rounds 5] [--timeout 300] [--out profiles/lbo_linear.txt]
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
CASES = [(k, q, b) for k in range(len(SHAPES)) for q in (4, 20, 32) for b in (64, 8, 1)]


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


def case(ydeg, S, K, marginal, q, block, reps, rounds):
    import torch

    from starry_process_amd import StarryProcess, linear
    from starry_process_amd.engine import block_edges, make_stars

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    sp = StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"],
                       marginalize_over_inclination=marginal)
    e, f = sp._engine, sp._flux
    rng = np.random.RandomState(K)
    tt = np.ascontiguousarray(np.broadcast_to(np.linspace(0, 30.0 * K / 1000, K), (S, K)))
    p = rng.uniform(0.5, 3.0, S)
    flux = 1.0 + 1e-2 * np.sin(2 * np.pi * tt / p[:, None]) + 1e-3 * rng.randn(S, K)
    noff = q if q < 8 else q - 3
    U = linear.offset_basis(K, np.round(np.linspace(0, K, noff + 1)).astype(int))
    if q >= 8:
        U = linear.stack_bases(U, linear.polynomial_basis(tt[0], 3))
    lamh = np.ascontiguousarray(np.broadcast_to(np.where(np.arange(q) < noff, 1e-4, 2.5e-5), (S, q)))
    flux = flux + (rng.randn(S, q) * np.sqrt(lamh)) @ U.T
    bvar = 1e-6
    stars = make_stars(S, period=p, inc_deg=rng.uniform(30.0, 85.0, S), baseline_mean=1.0, baseline_var=bvar)
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab = mv = None
    if marginal:
        tab, mv = e.kernel_table(rta1, 300)
    t, fl, sd = e.f64(tt), e.f64(flux), e.stars_to_device(stars)
    diag = e.f64(1e-6 * (1 + rng.rand(S, K)))
    eh = block_edges(block, K)
    nb = len(eh) - 1
    ed = torch.as_tensor(eh, dtype=torch.int32).to(e.device)
    nfull, tail = K // block, K % block
    ws = e.lbo_workspace(S, K, 300, not marginal, nb)
    wl = e.lbo_linear_workspace(S, K, q, 300, not marginal, nb)
    Ud = e.f64(np.ascontiguousarray(np.broadcast_to(U.T, (S, q, K))))
    lam = e.f64(lamh)
    kw = dict(diag=diag, conditional=not marginal, covpts=300, tab=tab, meanvar=mv, rta1=rta1)

    def fused():
        return e.lbo_linear(t, fl, sd, ed, Ud, lam, return_cov=True, workspace=wl, **kw)

    def plain():
        return e.lbo_ensemble(t, fl, sd, ed, return_cov=True, workspace=ws, **kw)

    def blocks(G, alpha, y):
        """(mu, var, u, lpd, cov) of the blocks G [S, n, b, b], alpha, y [S, n, b]"""
        if G.shape[-1] == 1:
            d = G[..., 0]
            u = alpha / d.sqrt()
            return y - alpha / d, 1.0 / d, u, -0.5 * u * u + 0.5 * d.log() - 0.5 * np.log(2 * np.pi), 1.0 / G
        LG = torch.linalg.cholesky(G)
        u = torch.linalg.solve_triangular(LG, alpha.unsqueeze(-1), upper=False).squeeze(-1)
        cov = torch.cholesky_inverse(LG)
        mu = y - torch.matmul(cov, alpha.unsqueeze(-1)).squeeze(-1)
        lpd = -0.5 * (u * u).sum(-1) + LG.diagonal(dim1=-2, dim2=-1).log().sum(-1) - 0.5 * G.shape[-1] * np.log(2 * np.pi)
        return mu, cov.diagonal(dim1=-2, dim2=-1), u, lpd, cov

    def composed():
        if marginal:
            C, _ = e.cov_marginal(t, stars, 300, tab, mv)
        else:
            C, _, _ = e.cov_conditional(t, stars, rta1)
        C.diagonal(dim1=1, dim2=2).add_(diag)
        C += bvar
        C += torch.bmm(Ud.transpose(1, 2) * lam[:, None, :], Ud)
        inv, _, _ = e.spd_inverse(C)
        r = fl - 1.0                                     # (normalised: the GP's mean is zero; baseline_mean = 1)
        alpha = torch.bmm(inv, r.unsqueeze(2)).squeeze(2)
        n = nfull * block
        G = inv[:, :n, :n].reshape(S, nfull, block, nfull, block).diagonal(dim1=1, dim2=3).permute(0, 3, 1, 2)
        res = [blocks(G.contiguous(), alpha[:, :n].reshape(S, nfull, block), fl[:, :n].reshape(S, nfull, block))]
        if tail:
            res.append(blocks(inv[:, n:K, n:K].unsqueeze(1).contiguous(), alpha[:, n:].unsqueeze(1),
                              fl[:, n:].unsqueeze(1)))
        u = torch.cat([x[2].reshape(S, -1) for x in res], dim=1)
        lpd = torch.cat([x[3].reshape(S, -1) for x in res], dim=1)
        return u, lpd, res

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref = composed()
    torch.cuda.synchronize()
    held = sum(x.numel() * 8 for blk in ref[2] for x in blk) + (ref[0].numel() + ref[1].numel()) * 8
    peak_composed = torch.cuda.max_memory_allocated() - base - held
    uc, lc = ref[0].clone(), ref[1].clone()
    del ref
    torch.cuda.empty_cache()
    got = fused()
    torch.cuda.synchronize()
    du = float((got[0][:, 2] - uc).abs().max() / uc.abs().max())
    dl = float(((got[1] - lc).abs() / lc.abs().clamp(min=1.0)).max())
    flags = int(got[6].abs().max())
    del got, uc, lc
    for _ in range(3):
        fused()
        composed()
        plain()
    torch.cuda.synchronize()
    gf, gc, gl = [], [], []
    for _ in range(rounds):
        gf.append(timed(fused, reps))
        gc.append(timed(composed, reps))
        gl.append(timed(plain, reps))
    Kr = (K + 63) // 64 * 64

    def stats(x):
        return dict(median=round(float(np.median(x)), 3), low=round(min(x), 3), high=round(max(x), 3))

    print(json.dumps(dict(
        what="lbo_linear", ydeg=ydeg, S=S, K=K, branch="marginal" if marginal else "conditional", q=q, block=block,
        nblocks=nb, reps=reps, rounds=rounds, fused_ms=stats(gf), plain_ms=stats(gl), composed_ms=stats(gc),
        composed_over_fused=round(float(np.median(gc) / np.median(gf)), 2),
        fused_over_plain=round(float(np.median(gf) / np.median(gl)), 3),
        fused_minus_plain_ms=round(float(np.median(gf) - np.median(gl)), 3),
        fused_workspace_bytes=int(wl.numel()), plain_workspace_bytes=int(ws.numel()),
        composed_scratch_bytes=int(peak_composed),
        inverse_bytes_not_allocated=int(8 * S * Kr * Kr), max_rel_difference_u=du, max_rel_difference_lpd=dl,
        status_flags=flags)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbo_linear.txt"))
    ap.add_argument("--case", type=int, default=None, help="(internal) run this one case in this process")
    a = ap.parse_args()
    if a.case is not None:
        k, q, block = CASES[a.case]
        ydeg, S, K, marginal = SHAPES[k]
        case(ydeg, S, K, marginal, q, block, a.reps, a.rounds)
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
