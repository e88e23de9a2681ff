"""Time-variable surface maps (sp_temporal_gram, sp_ylm_temporal, sp_flux_rows) on the GPU, phase by phase:

  gram      K_t = k(t, t, tau) (Matern-3/2) and its Cholesky factor           (HIP events around the call)
  pass1     Wt[n] = Ly U[n]^T, the first triangular product                  (the library's own event pairs, kind 6)
  pass2     Y[n] = Lt Wt[n]^T, the second                                    (kind 7)
  ylm       the whole sp_ylm_temporal call: packs + both passes               (HIP events)
  flux      F[n, k] = A[k] . Y[n, k]                                          (HIP events)
  host      the NumPy draw of U, its upload and the download of Y, which bound the end-to-end sample_ylm(t)

Shapes: Nt = 1000 at ydeg 15 with ns = 1, 10, 64, and Nt = 3000 at ydeg 20 with ns = 10.  The passes' algorithmic
flops are N^2 Nt + Nt^2 N per sample (two triangular products); their fraction of the 78.6 TFLOP/s fp64 peak is
reported beside the executed (64-padded) count.  One JSON line per shape, milliseconds are medians of `reps` calls.

    python tools/bench_temporal_maps.py [reps]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd.engine import Engine, make_stars  # noqa: E402

PEAK = 78.6e12
SHAPES = ((1000, 15, 1), (1000, 15, 10), (1000, 15, 64), (3000, 20, 10))


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
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def passes(e, Lt, Ly, U, reps):
    """Median device milliseconds and summed flops (algorithmic, executed) of the two triangular passes."""
    t1, t2 = [], []
    for _ in range(reps):
        e.profile_begin(256, kinds=("tri1", "tri2"))
        e.ylm_temporal(Lt, Ly, U)
        n1, ms1, fl1, fp1 = e.profile_kind("tri1", padded=True)
        n2, ms2, fl2, fp2 = e.profile_kind("tri2", padded=True)
        t1.append(ms1)
        t2.append(ms2)
    return float(np.median(t1)), float(np.median(t2)), (fl1, fp1, n1), (fl2, fp2, n2)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    mom_cache = {}
    for Nt, ydeg, ns in SHAPES:
        e = Engine(ydeg, 2, 0)
        N = e.N
        if ydeg not in mom_cache:
            mom_cache[ydeg] = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))["default_cov_ylm"]
        Ly, info = e.cho_factor(mom_cache[ydeg])
        assert int(info[0].item()) == 0
        t = np.linspace(0, 50, Nt)
        td = e.f64(t)
        g_gram = timed(lambda: e.temporal_gram(td, 25.0, "matern32"), reps)
        Lt, info = e.temporal_gram(td, 25.0, "matern32")
        assert int(info[0].item()) == 0
        rng = np.random.RandomState(1)
        Uh = rng.normal(size=(ns, Nt, N))
        U = e.f64(Uh)
        ms1, ms2, (fl1, fp1, n1), (fl2, fp2, n2) = passes(e, Lt, Ly, U, reps)
        g_ylm = timed(lambda: e.ylm_temporal(Lt, Ly, U), reps)
        Y = e.ylm_temporal(Lt, Ly, U)
        A = e.design_matrix(t[None, :], make_stars(1, period=0.8, inc_deg=65.0), e.f64(e.rTA1L([0.2, 0.1])))[0]
        g_flux = timed(lambda: e.flux_rows(A, Y, normalized=True), reps)
        h_draw = host_timed(lambda: np.random.RandomState(1).normal(size=(ns, Nt, N)), max(3, reps // 3))
        h_up = host_timed(lambda: e.f64(Uh), max(3, reps // 3))
        h_down = host_timed(lambda: Y.cpu().numpy(), max(3, reps // 3))
        alg = ns * (N * N * Nt + Nt * Nt * N)
        assert abs(fl1 + fl2 - alg) <= 1e-9 * alg, (fl1 + fl2, alg)
        print(json.dumps(dict(
            Nt=Nt, ydeg=ydeg, ns=ns, gram_ms=round(g_gram, 4), pass1_ms=round(ms1, 4), pass2_ms=round(ms2, 4),
            pass_launches=[n1, n2], ylm_call_ms=round(g_ylm, 4), flux_ms=round(g_flux, 4),
            gflop_alg=round(alg * 1e-9, 3), gflop_exec=round((fp1 + fp2) * 1e-9, 3),
            passes_frac_peak=round(alg / ((ms1 + ms2) * 1e-3) / PEAK, 3),
            passes_frac_peak_exec=round((fp1 + fp2) / ((ms1 + ms2) * 1e-3) / PEAK, 3),
            pass1_frac_peak=round(fl1 / (ms1 * 1e-3) / PEAK, 3), pass2_frac_peak=round(fl2 / (ms2 * 1e-3) / PEAK, 3),
            host_draw_ms=round(h_draw, 2), upload_ms=round(h_up, 2), download_ms=round(h_down, 2))), flush=True)
        del e, Lt, Ly, U, Y, A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
