"""Surface-map posterior (sp_ylm_conditional_batched) against the straightforward route through the library's
existing entry points, timed with HIP events at the issue's shapes:

  fused      design matrix -> Bt = (D^-1/2 A)^T, G = Bt Bt^T (lower tiles, matrix cores), epilogue (Sherman-Morrison)
             -> cho_factor(W), cho_solve(rhs), cho_solve(I) = ycov, cho_factor(ycov)
  straight   design matrix -> C = D + b 1 1^T (K x K) -> cho_factor(C) -> cho_solve(C, [A | r]) (N + 1 right-hand
             sides) -> A^T (C^-1 A), A^T C^-1 r by sp_gemm_nt -> + Sigma_y^-1 -> the same four N x N steps

Prints one JSON line per shape: milliseconds per call (median of the timed calls) for both routes, their ratio,
and the largest difference of ymu between the routes in posterior standard deviations.

    python tools/bench_ylm_conditional.py [reps]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd._lib import check  # noqa: E402
from starry_process_amd.engine import Engine, make_stars  # noqa: E402

SHAPES = [(64, 1000, 15), (32, 3000, 20)]


def inputs(e, S, K, L):
    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % L))
    rng = np.random.RandomState(S + K)
    t = np.linspace(0, 3, K)
    p = 0.6 + rng.rand(S)
    flux = 1e-3 * np.sin(2 * np.pi * t[None, :] / p[:, None]) + 1e-3 * rng.randn(S, K)
    stars = make_stars(S, period=p, inc_deg=20 + 65 * rng.rand(S), data_var=1e-6, baseline_var=1e-6)
    sinv, sinvmu = e.ylm_precision(mom["default_mean_ylm"], mom["default_cov_ylm"])
    return dict(t=e.f64(np.broadcast_to(t, (S, K)).copy()), flux=e.f64(flux), stars=stars,
                rta1=e.f64(e.rTA1L(np.zeros((1, 2)))), sinv=sinv, sinvmu=sinvmu)


def fused(e, d):
    ymu, ycov, ycho, _ = e.ylm_conditional(d["t"], d["flux"], d["stars"], d["rta1"], d["sinv"], d["sinvmu"])
    return ymu, ycov


def straight(e, d):
    Lb, h, st, P = e._L, e._h, e._stream(), e._p
    S, K = d["flux"].shape
    N = e.N
    A = e.design_matrix(d["t"], d["stars"], d["rta1"])                      # [S, K, N]
    C = torch.full((S, K, K), float(d["stars"]["baseline_var"][0]), dtype=torch.float64, device=e.device)
    C.diagonal(dim1=1, dim2=2).add_(float(d["stars"]["data_var"][0]))
    check(Lb.sp_cho_factor(h, P(C), K, K, K * K, S, None, st))
    X = torch.cat([A, d["flux"][:, :, None]], dim=2).contiguous()            # [S, K, N + 1]
    Y = X.clone()
    check(Lb.sp_cho_solve(h, P(C), K, K, K * K, P(Y), N + 1, S, st))           # C^-1 [A | r]
    At = A.transpose(1, 2).contiguous()                                       # [S, N, K]
    Yt = Y.transpose(1, 2).contiguous()                                       # [S, N + 1, K]
    G = torch.empty(S, N, N + 1, dtype=torch.float64, device=e.device)
    e.gemm_nt_batched(At, Yt, G)                                              # [A^T C^-1 A | A^T C^-1 r]
    W = (G[:, :, :N] + d["sinv"]).contiguous()
    ymu = (G[:, :, N] + d["sinvmu"]).contiguous()
    check(Lb.sp_cho_factor(h, P(W), N, N, N * N, S, None, st))
    check(Lb.sp_cho_solve(h, P(W), N, N, N * N, P(ymu), 1, S, st))
    ycov = torch.eye(N, dtype=torch.float64, device=e.device).repeat(S, 1, 1)
    check(Lb.sp_cho_solve(h, P(W), N, N, N * N, P(ycov), N, S, st))
    ycho = ycov.clone()
    check(Lb.sp_cho_factor(h, P(ycho), N, N, N * N, S, None, st))
    return ymu, ycov


def timed(fn, e, d, reps):
    for _ in range(2):
        out = fn(e, d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(e, d)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for S, K, L in SHAPES:
        e = Engine(L, 2, 0)
        d = inputs(e, S, K, L)
        # alternate the two routes so that drift of the machine hits both alike
        tf, (m1, c1) = timed(fused, e, d, reps)
        ts, (m2, _) = timed(straight, e, d, reps)
        tf2, _ = timed(fused, e, d, reps)
        ts2, _ = timed(straight, e, d, reps)
        sd = torch.sqrt(torch.diagonal(c1, dim1=1, dim2=2))
        diff = float(torch.max(torch.abs(m1 - m2) / sd).item())
        print(json.dumps(dict(S=S, K=K, ydeg=L, fused_ms=[round(tf, 3), round(tf2, 3)],
                              straight_ms=[round(ts, 3), round(ts2, 3)],
                              speedup=round(min(ts, ts2) / min(tf, tf2), 2), ymu_diff_sd=diff)), flush=True)
        del e, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
