"""calibrate.generate (csrc/sp_generate.hip) on the GPU, phase by phase, at the reference's defaults (ydeg 30,
nlon 300: 45 000 pixels, npts 1000) for nlc = 50 and 1000:

  setup     the pixel transform M at the grid and sp_generate_gram: W P^T, G = (W P)^T (W P) + eps I, its factor
            (once per grid: generate() keeps it on the engine)                                 (HIP events)
  paint     sp_generate_paint, chunks of 512 stars as generate() runs it                        (HIP events)
  project   sp_generate_project: (W X) (W P^T)^T on the matrix cores, the solve, the smoothing  (HIP events)
  design    sp_design_matrix alone, in the chunks sp_generate_flux uses                         (HIP events)
  flux      the whole sp_generate_flux call (design matrices + products + normalisation + noise) (HIP events)
  draw      the host draws (draw_spots), and the whole generate() call after the setup          (wall clock)

setup and project report their fraction of the 78.6 TFLOP/s fp64 peak (algorithmic flops: N^2 npix for the
symmetric Gram, 2 N npix nlc for the projection); the other phases are not bound by the matrix cores.  With --numpy
the host restatement of the Gram matrix (W P)^T (W P) is timed once beside it.  One JSON line per nlc.

    python tools/bench_generate.py [reps] [--numpy]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from starry_process_amd import calibrate_generate as cg  # noqa: E402
from starry_process_amd.engine import get_engine, make_stars  # noqa: E402

PEAK = 78.6e12


def timed(fn, reps):
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


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 5
    gen = cg.update_with_defaults()["generate"]
    e = get_engine(gen["ydeg"], 2)
    N, nlon, K = e.N, gen["nlon"], gen["npts"]
    lat, lon, w, xyz = cg.grid(nlon)
    npix = lat.size * lon.size

    def setup():
        e._gen_setup = None
        return e.generate_setup(nlon, 1e-12)

    ms_setup = timed(setup, max(2, reps // 2))
    WPT, L = e.generate_setup(nlon, 1e-12)
    t = np.linspace(0, gen["tmax"], K)
    rta1 = e.f64(e.rTA1L(gen["u"]))
    for nlc in (50, 1000):
        d = cg.draw_spots(0, dict(gen, nlc=nlc))
        off = d["offsets"]
        chunks = [(c0, min(nlc, c0 + cg._PAINT_CHUNK)) for c0 in range(0, nlc, cg._PAINT_CHUNK)]
        args_paint = [(d["spots"][off[a]:off[b]], off[a:b + 1] - off[a]) for a, b in chunks]
        WXs = [e.generate_paint(nlon, s, o)[1] for s, o in args_paint]
        ms_paint = timed(lambda: [e.generate_paint(nlon, s, o) for s, o in args_paint], reps)
        ms_proj = timed(lambda: [e.generate_project(WPT, L, WX, b - a, gen["smoothing"])
                                 for WX, (a, b) in zip(WXs, chunks)], reps)
        y = torch.cat([e.generate_project(WPT, L, WX, b - a, gen["smoothing"]) for WX, (a, b) in zip(WXs, chunks)])
        del WXs
        stars = make_stars(nlc, period=gen["period"], inc_deg=d["incs"])
        chunk = max(1, min(nlc, (256 << 20) // (8 * K * N)))
        td = e.f64(np.tile(t, (chunk, 1)))
        ms_design = timed(lambda: [e.design_matrix(td[:min(chunk, nlc - c0)], stars[c0:c0 + chunk], rta1)
                                   for c0 in range(0, nlc, chunk)], reps)
        noise = e.f64(d["noise"])
        ms_flux = timed(lambda: e.generate_flux(t, stars, rta1, y, noise, gen["ferr"], "mean"), reps)
        ms_draw = wall(lambda: cg.draw_spots(0, dict(gen, nlc=nlc)), max(2, reps // 2))
        ms_gen = wall(lambda: cg.generate(generate=dict(nlc=nlc)), max(2, reps // 2))
        fl_setup, fl_proj = float(N) * N * npix, 2.0 * N * npix * nlc
        print(json.dumps(dict(
            nlc=nlc, ydeg=gen["ydeg"], npix=npix, npts=K, setup_ms=round(ms_setup, 3), paint_ms=round(ms_paint, 3),
            project_ms=round(ms_proj, 3), design_ms=round(ms_design, 3), flux_ms=round(ms_flux, 3),
            flux_only_ms=round(ms_flux - ms_design, 3), draw_ms=round(ms_draw, 2), generate_call_ms=round(ms_gen, 2),
            setup_frac_peak=round(fl_setup / (ms_setup * 1e-3) / PEAK, 3),
            project_frac_peak=round(fl_proj / (ms_proj * 1e-3) / PEAK, 3))), flush=True)
        torch.cuda.empty_cache()
    if "--numpy" in sys.argv:
        P = e.pixel_transform(xyz).cpu().numpy() / np.pi
        WP = P * np.repeat(w, lon.size)[:, None]
        t0 = time.perf_counter()
        WP.T @ WP
        print(json.dumps(dict(numpy_gram_ms=round(1e3 * (time.perf_counter() - t0), 1),
                              threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)


if __name__ == "__main__":
    main()
