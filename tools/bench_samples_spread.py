"""The batched-samples shape of bench.bench_samples (one K = 1000 light curve, ydeg 15, 64 samples per call, six steps
in flight) in the modes of calibrate.SampleBatches: the five columns (r, a, b, c, n) through bench.bench_samples itself,
then -- the same harness: pre-warm, fresh samples every step, one timed call -- the seven columns with free baseline
terms, a fixed spot-size spread and a free one.  One JSON line per mode.

    python tools/bench_samples_spread.py [steps] [mode ...]      modes: five seven dr_fixed dr_free all_free
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

MODES = {"seven": dict(free=("baseline_mean", "baseline_log_var")), "dr_fixed": dict(dr=5.0), "dr_free": dict(dr="free"),
         "all_free": dict(dr="free", free=("baseline_mean", "baseline_log_var"))}


def bench_mode(mode, ydeg=15, Kc=1000, F=6, steps=120, device=0):
    from starry_process_amd.calibrate import SampleBatches
    from starry_process_amd.engine import engine_slots, make_stars
    from starry_process_amd.synthetic import synthetic_star

    st = synthetic_star(0, Kc)
    slots = engine_slots(ydeg, bench.UDEG, device, F)
    e0 = slots[0][0]
    kw = MODES[mode]
    sb = SampleBatches(slots, e0.f64(st["t"][None, :]), e0.f64(st["flux"][None, None, :]),
                       make_stars(1, period=st["p"], data_var=1e-6), e0.f64(e0.rTA1L([0.0, 0.0])), bench.COVPTS, **kw)
    g = sb.group
    rng = np.random.RandomState(7)

    def draw(n):      # bench.bench_samples' box, with dr in [2, 8] degrees, m in +-1e-3, v in [-6, -4]
        cols = [rng.uniform(15.0, 25.0, n)]
        if kw.get("dr") == "free":
            cols.append(rng.uniform(2.0, 8.0, n))
        cols += [rng.uniform(0.3, 0.5, n), rng.uniform(0.2, 0.35, n), rng.uniform(0.08, 0.12, n), rng.uniform(5.0, 12.0, n)]
        if "baseline_mean" in kw.get("free", ()):
            cols.append(rng.uniform(-1e-3, 1e-3, n))
        if "baseline_log_var" in kw.get("free", ()):
            cols.append(rng.uniform(-6.0, -4.0, n))
        return np.column_stack(cols)

    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.3:
        sb(draw(3 * F * g))
        torch.cuda.synchronize()
    smp = draw(steps * g)
    t0 = time.perf_counter()
    out = sb(smp)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vals = out.cpu().numpy()
    return {"mode": mode, "columns": list(sb.columns), "ydeg": ydeg, "K": Kc, "samples_per_call": g, "steps": steps,
            "steps_in_flight": F, "evals_per_s": g * steps / dt, "ms_per_step": 1e3 * dt / steps,
            "host_enqueue_ms_per_step": 1e3 * host / steps, "finite": bool(np.isfinite(vals).all())}


if __name__ == "__main__":
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    modes = sys.argv[2:] or ["five"] + list(MODES)
    for mode in modes:
        if mode == "five":
            r = bench.bench_samples(torch, 15, 1000, 1, 6, steps, 0)
            r = {"mode": "five", **{k: r[k] for k in ("evals_per_s", "ms_per_step", "host_enqueue_ms_per_step", "upstream_ms",
                                                      "finite")}}
        else:
            r = bench_mode(mode, steps=steps)
        print(json.dumps(r), flush=True)
