"""Pixel-space methods (sp_pixel_*) on the GPU against the host NumPy route, timed with HIP events:

  transform  M = pi pT A1 on the default 150 x 300 Mollweide grid, ydeg 15 and 20
             (host: pT in NumPy, then pi pT @ A1)
  render     640 maps (64 stars x 10 posterior samples) at ydeg 15 on that grid, unit background
             (host: np.tensordot(y, M)); also a bare sp_gemm_nt of the same shape, the render's bound
  cov_pix    (M Sigma) M^T at 2 000 points, ydeg 15 (host: (M @ Sigma) @ M.T)

Prints one JSON line per measurement: GPU milliseconds (median of the timed calls, two interleaved rounds), host
milliseconds (one call), their ratio.

    python tools/bench_pixel.py [reps]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from oracle import sp_oracle as orc  # noqa: E402
from starry_process_amd._lib import check  # noqa: E402
from starry_process_amd.engine import Engine  # noqa: E402
from starry_process_amd.pixel import mollweide_grid  # noqa: E402
from test_gpu_pixel import pT_np, random_xyz  # noqa: E402


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


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def report(what, gpu, host, **kw):
    print(json.dumps(dict(what=what, gpu_ms=[round(g, 4) for g in gpu], host_ms=round(host, 2),
                          speedup=round(host / min(gpu), 1), **kw)), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    grid = mollweide_grid(150, 300)
    for L in (15, 20):
        e = Engine(L, 2, 0)
        xyz = e.f64(grid)
        g = [timed(lambda: e.pixel_transform(xyz), reps) for _ in range(2)]
        A1 = orc._A1(L)
        h, _ = host_ms(lambda: np.pi * pT_np(L, *grid) @ A1)
        report("transform", g, h, ydeg=L, npix=grid.shape[1])
        del e
        torch.cuda.empty_cache()

    e = Engine(15, 2, 0)
    N, npix, nmaps = e.N, grid.shape[1], 640
    M = e.pixel_transform(e.f64(grid))
    y = e.f64(0.01 * np.random.RandomState(1).randn(nmaps, N))
    out = e.empty(nmaps, npix)

    def bare():
        check(e._L.sp_gemm_nt(e._h, e._p(y), N, 0, e._p(M), N, 0, e._p(out), npix, 0, nmaps, npix, N, 1.0, 0, 0, 1,
                              e._stream()))

    gr, gb = [], []
    for _ in range(2):
        gr.append(timed(lambda: e.pixel_render(M, y, True), reps))
        gb.append(timed(bare, reps))
    Mh, yh = M.cpu().numpy(), y.cpu().numpy()

    def host_render():
        yy = yh.copy()
        yy[:, 0] += 1
        return np.tensordot(yy, Mh, axes=[[1], [1]])

    h, _ = host_ms(host_render)
    report("render", gr, h, ydeg=15, nmaps=nmaps, npix=npix, bare_gemm_ms=[round(x, 4) for x in gb],
           render_over_gemm=round(min(gr) / min(gb), 3), gflop_per_s=round(2.0 * nmaps * npix * N / min(gr) * 1e-6, 1))

    npts = 2000
    Mp = e.pixel_transform(e.f64(random_xyz(npts, 5)))
    cov = np.load(os.path.join(ROOT, "tests", "golden", "moments_L15.npz"))["default_cov_ylm"]
    cd = e.f64(cov)
    g = [timed(lambda: e.pixel_cov(Mp, cd), reps) for _ in range(2)]
    Mph = Mp.cpu().numpy()
    h, _ = host_ms(lambda: (Mph @ cov) @ Mph.T)
    report("cov_pix", g, h, ydeg=15, npts=npts)


if __name__ == "__main__":
    main()
