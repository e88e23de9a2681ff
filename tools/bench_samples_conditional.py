"""The batched samples of a conditional, time-variable process (the reference's TimeVariabilityInference tutorial): one
light curve, ydeg 15, K = 1000, Matern-3/2 with tau = 3, free i, p, tau, 64 samples per step, six steps in flight
(calibrate.SampleBatches(conditional=True, free=("i", "p", "tau"))).  The harness is bench.bench_samples' (pre-warm,
fresh samples every step, one timed call).  Beside it: the same rows one process per row (what
StarryProcess.log_likelihood_samples did for such a process before it had a batched route, and still does for what
the batch does not serve), and the yardstick, bench.py's other_shapes conditional rate at cfg3 (64 stars that share
the handle's one moment set, no upstream in the step).  One JSON line per mode.

    python tools/bench_samples_conditional.py [steps] [mode ...]      modes: batched fallback yardstick
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

YDEG, K, TAU, F = 15, 1000, 3.0, 6


def draw(rng, n):
    """bench.bench_samples' box, then i in [30, 85] degrees, p within 20 % of the star's, tau in [1, 6]."""
    return np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.3, 0.5, n), rng.uniform(0.2, 0.35, n),
                            rng.uniform(0.08, 0.12, n), rng.uniform(5.0, 12.0, n), rng.uniform(30.0, 85.0, n),
                            rng.uniform(0.8, 1.2, n), rng.uniform(1.0, 6.0, n)])


def star():
    from starry_process_amd.synthetic import synthetic_star

    return synthetic_star(0, K)


def bench_batched(steps, device=0):
    from starry_process_amd.calibrate import SampleBatches
    from starry_process_amd.engine import engine_slots, make_stars

    st = star()
    slots = engine_slots(YDEG, bench.UDEG, device, F)
    e0 = slots[0][0]
    sb = SampleBatches(slots, e0.f64(st["t"][None, :]), e0.f64(st["flux"][None, None, :]),
                       make_stars(1, period=st["p"], tau=TAU, data_var=1e-6), e0.f64(e0.rTA1L([0.0, 0.0])), bench.COVPTS,
                       temporal="matern32", conditional=True, free=("i", "p", "tau"))
    g = sb.group
    rng = np.random.RandomState(7)
    scale = np.array([1, 1, 1, 1, 1, 1, st["p"], 1.0])
    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.3:
        sb(draw(rng, 3 * F * g) * scale)
        torch.cuda.synchronize()
    smp = draw(rng, steps * g) * scale
    t0 = time.perf_counter()
    out = sb(smp)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vals = out.cpu().numpy()
    return {"mode": "batched", "columns": list(sb.columns), "ydeg": YDEG, "K": K, "samples_per_call": g, "steps": steps,
            "steps_in_flight": F, "evals_per_s": g * steps / dt, "ms_per_step": 1e3 * dt / steps,
            "host_enqueue_ms_per_step": 1e3 * host / steps, "finite": bool(np.isfinite(vals).all())}


def bench_fallback(rows=48):
    from starry_process_amd import StarryProcess

    st = star()
    rng = np.random.RandomState(7)
    scale = np.array([1, 1, 1, 1, 1, 1, st["p"], 1.0])

    def one(row):
        r, a, b, c, n, i, p, tau = row
        sp = StarryProcess(r=r, a=a, b=b, c=c, n=n, ydeg=YDEG, tau=tau, marginalize_over_inclination=False,
                           upstream="device")
        return float(sp.log_likelihood(st["t"], st["flux"], 1e-6, i=i, p=p))

    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.3:
        one(draw(rng, 1)[0] * scale)
    smp = draw(rng, rows) * scale
    t0 = time.perf_counter()
    vals = [one(row) for row in smp]
    dt = time.perf_counter() - t0
    return {"mode": "fallback", "rows": rows, "evals_per_s": rows / dt, "ms_per_eval": 1e3 * dt / rows,
            "finite": bool(np.isfinite(vals).all())}


def bench_yardstick(device=0):
    r = bench.bench_shape(torch, None, ydeg=YDEG, Kc=K, S=64, tspan=4.0, tau=None, u=(0.0, 0.0), conditional=True, F=4,
                          steps=24, device=device)
    return {"mode": "yardstick", **{k: r[k] for k in ("stars", "steps", "steps_in_flight", "evals_per_s", "ms_per_step",
                                                      "finite")}}


if __name__ == "__main__":
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    for mode in sys.argv[2:] or ["batched", "fallback", "yardstick"]:
        r = {"batched": lambda: bench_batched(steps), "fallback": bench_fallback, "yardstick": bench_yardstick}[mode]()
        print(json.dumps(r), flush=True)
