"""Per-pixel variance maps (Engine.pixel_var, sp_pixel_var_batched) on the default 150 x 300 Mollweide grid against the
route composed from the entry points that existed before it, timed with HIP events:

  fused      Engine.pixel_var(M, cov): one kernel, no workspace
  composed   sp_gemm_nt for T[b] = M cov[b] into an [S, npts, N] buffer, then (T * M).sum(-1) in torch

at ydeg 15 with S = 1 and S = 100 covariances and at ydeg 20 with S = 32.  Prints one JSON line per shape: the
milliseconds of both routes (median of the timed calls, two interleaved rounds each), their ratio, the flop rate the
fused kernel executes (rows padded to 32, N to a multiple of 64) and the useful one (2 npts N^2 S) as fractions of the
78.6 TFLOP/s fp64 matrix peak, the scratch bytes of each route (peak allocation beyond the result), the number of
timed calls, and the largest difference between the two results relative to the largest variance.

    python tools/bench_pixel_var.py [reps]          (20 timed calls per round by default)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd._lib import check  # noqa: E402
from starry_process_amd.engine import Engine  # noqa: E402
from starry_process_amd.pixel import mollweide_grid  # noqa: E402

PEAK = 78.6e12


def allocated(t):
    """Bytes the caching allocator holds for tensor t: its blocks are multiples of 512 bytes."""
    return 512 * ((t.numel() * t.element_size() + 511) // 512)


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


def shape(ydeg, S, reps):
    e = Engine(ydeg, 2, 0)
    N = e.N
    M = e.pixel_transform(e.f64(mollweide_grid(150, 300)))
    npts = int(M.shape[0])
    cov = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))["default_cov_ylm"]
    scale = np.random.RandomState(S).uniform(0.5, 1.0, size=S)
    stack = e.f64(cov)[None] * e.f64(scale)[:, None, None]
    T = e.empty(S, npts, N)

    def composed():
        # (cov symmetric: the NT product's B operand, read by rows, is cov^T)
        check(e._L.sp_gemm_nt(e._h, e._p(M), N, 0, e._p(stack), N, N * N, e._p(T), N, npts * N, npts, N, N, 1.0, 0, 0, S,
                              e._stream()))
        return (T * M).sum(-1)

    def fused():
        return e.pixel_var(M, stack)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref = composed()
    torch.cuda.synchronize()
    peak_composed = torch.cuda.max_memory_allocated() - base - allocated(ref)
    del ref
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = fused()
    torch.cuda.synchronize()
    peak_fused = torch.cuda.max_memory_allocated() - base - allocated(got)
    ref = composed()
    ok = ~torch.isnan(ref)
    assert torch.equal(torch.isnan(got), ~ok)
    diff = float((got[ok] - ref[ok]).abs().max() / ref[ok].abs().max())
    del ref, got
    gf, gc = [], []
    for _ in range(2):
        gf.append(timed(fused, reps))
        gc.append(timed(composed, reps))
    rows, Np = 32 * ((npts + 31) // 32), 64 * ((N + 63) // 64)
    executed, useful = 2.0 * rows * Np * Np * S, 2.0 * npts * N * N * S
    print(json.dumps(dict(
        what="pixel_var", ydeg=ydeg, S=S, npts=npts, reps=reps, fused_ms=[round(x, 4) for x in gf],
        composed_ms=[round(x, 4) for x in gc], composed_over_fused=round(min(gc) / min(gf), 2),
        fused_executed_peak_fraction=round(executed / (min(gf) * 1e-3) / PEAK, 3),
        fused_useful_peak_fraction=round(useful / (min(gf) * 1e-3) / PEAK, 3),
        fused_scratch_bytes=int(peak_fused), composed_T_bytes=int(T.numel() * 8),
        composed_scratch_bytes_with_torch_temporaries=int(peak_composed + T.numel() * 8),
        max_rel_difference=diff)), flush=True)
    del e, T, M, stack
    torch.cuda.empty_cache()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for ydeg, S in ((15, 1), (15, 100), (20, 32)):
        shape(ydeg, S, reps)


if __name__ == "__main__":
    main()
