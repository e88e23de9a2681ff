"""Posterior maps of a time-variable process (sp_ylm_conditional_temporal) on the GPU, phase by phase:

  system    the design matrix, C = (A Sigma_y A^T) o k + data_cov and the residual            (HIP events)
  inverse   C^-1 (sp_spd_inverse_batched), its symmetric image and C^-1 r                     (HIP events)
  frames    sp_ylm_conditional_temporal alone: the panels, G_j C^-1, the downdates, mirrors   (HIP events)
  mean      the same call without covariances (return_cov=False)                              (HIP events)
  call      StarryProcess.ylm_conditional_temporal end to end, with and without covariances, downloads included
  sample    sample_ylm_conditional_temporal, nsamples = 10, end to end

Shapes: K = 1000 observed times, T = 100 frames at ydeg 15 (the figure DESIGN.md 16 and the README quote), and K = 300,
T = 50 at ydeg 5.  The frames' algorithmic flops are 2 K^2 N + 2 K N^2 per frame (G_j C^-1, then the downdate of a full
N x N block); the executed count pads K and N to 64 and halves the downdate (lower tiles).  Their fraction of the
78.6 TFLOP/s fp64 peak is reported for the `frames` phase.  One JSON line per shape, milliseconds are medians of `reps`
calls.

    python tools/bench_ylm_conditional_temporal.py [reps]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd import StarryProcess  # noqa: E402
from starry_process_amd.temporal import Matern32Kernel  # noqa: E402

PEAK = 78.6e12
SHAPES = ((1000, 100, 15), (300, 50, 5))
I, P, U = 65.0, 0.8, [0.2, 0.1]


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def host_timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for K, T, ydeg in SHAPES:
        mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
        sp = StarryProcess(ydeg=ydeg, tau=2.0, temporal_kernel=Matern32Kernel, normalized=False,
                           marginalize_over_inclination=False, mean_ylm=mom["default_mean_ylm"],
                           cov_ylm=mom["default_cov_ylm"])
        e = sp._engine
        N = e.N
        t = np.linspace(0, 3, K)
        t_map = np.linspace(0, 3.6, T)
        flux = 1e-2 * np.random.RandomState(1).randn(K)
        dcov = np.asarray(1e-6)
        system = lambda: sp._ylm_temporal_system(t, flux, dcov, I, P, U, 0.0, 0.0)      # noqa: E731
        g_system = timed(system, reps)
        A, C, r0, Sig, mu = system()
        Kr = (K + 63) // 64 * 64

        def inverse():
            low, _, info = e.spd_inverse(C, full=False)
            low = torch.tril(low[0])
            Cinv = (low + torch.tril(low, -1).T).contiguous()
            Rp = torch.zeros(1, Kr, dtype=torch.float64, device=e.device)
            Rp[:, :K] = r0[None, :]
            return Cinv, e.gemm_nt(Rp, Cinv), info

        g_inverse = timed(inverse, reps)
        Cinv, Z, info = inverse()
        assert int(info[0].item()) == 0
        td, tm = e.f64(t), e.f64(t_map)
        out = e.empty(1, T, N)
        ycov = e.empty(T, N, N)
        L = e._L

        def frames(with_cov):
            ws = e._scratch(L.sp_ylm_conditional_temporal_workspace_bytes(e._h, K, T, 1, int(with_cov)))
            rc = L.sp_ylm_conditional_temporal(e._h, K, T, 1, e._p(A), N, e._p(Sig), N, e._p(Cinv), e._p(Z), Kr,
                                               e._p(td), e._p(tm), 2.0, 1, e._p(info), e._p(out),
                                               e._p(ycov if with_cov else None), e._p(ws), e._stream())
            assert rc == 0, rc

        g_frames = timed(lambda: frames(True), reps)
        g_mean = timed(lambda: frames(False), reps)
        kw = dict(t_map=t_map, i=I, p=P, u=U)
        h_cov = host_timed(lambda: sp.ylm_conditional_temporal(t, flux, 1e-6, **kw), max(3, reps // 3))
        h_mean = host_timed(lambda: sp.ylm_conditional_temporal(t, flux, 1e-6, return_cov=False, **kw), max(3, reps // 3))
        h_smp = host_timed(lambda: sp.sample_ylm_conditional_temporal(t, flux, 1e-6, nsamples=10, seed=1, **kw),
                           max(3, reps // 3))
        Np = (N + 63) // 64 * 64
        ntl = Np // 64
        alg = T * (2.0 * K * K * N + 2.0 * K * N * N)
        exe = T * (2.0 * Kr * Kr * Np + 2.0 * Kr * 64 * 64 * ntl * (ntl + 1) / 2)
        print(json.dumps(dict(
            K=K, T=T, ydeg=ydeg, system_ms=round(g_system, 3), inverse_ms=round(g_inverse, 3),
            frames_ms=round(g_frames, 3), frames_mean_only_ms=round(g_mean, 3),
            gflop_alg=round(alg * 1e-9, 2), gflop_exec=round(exe * 1e-9, 2),
            frames_frac_peak_exec=round(exe / (g_frames * 1e-3) / PEAK, 3),
            call_with_cov_ms=round(h_cov, 2), call_mean_only_ms=round(h_mean, 2), sample10_ms=round(h_smp, 2),
            cov_download_mb=round(8e-6 * T * N * N, 1))), flush=True)
        del sp, e, A, C, Cinv, out, ycov
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
