"""Sums of two spot populations under a sampler: cfg2's light curve (ydeg 15, K = 1000, one star), 64 samples per step,
evaluations/s of three paths in ONE process with alternating legs:

    a   one population, batched (calibrate.SampleBatches: the shape of bench.bench_samples)
    b   two populations, batched (SampleBatches(populations=2): sp_polar_moments_samples_sum)
    c   two populations through the per-sample path: (StarryProcess(row 1, upstream="device") + StarryProcess(row 2,
        upstream="device")).log_likelihood, one evaluation at a time

    python tools/bench_samples_sum.py [steps] [rounds]      one JSON line per leg and round, then the medians
    python tools/bench_samples_sum.py trace a|b [steps]     the batched leg alone, for a kernel trace taken around it
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

YDEG, K, F = 15, 1000, 6


def draw(rng, n, C):
    """bench.bench_samples' box, per population."""
    cols = []
    for _ in range(C):
        cols += [rng.uniform(15.0, 25.0, n), rng.uniform(0.3, 0.5, n), rng.uniform(0.2, 0.35, n),
                 rng.uniform(0.04, 0.06, n), rng.uniform(5.0, 12.0, n)]
    return np.column_stack(cols)


def batches(C, st, device=0):
    from starry_process_amd.calibrate import SampleBatches
    from starry_process_amd.engine import engine_slots, make_stars

    slots = engine_slots(YDEG, bench.UDEG, device, F)
    e0 = slots[0][0]
    return SampleBatches(slots, e0.f64(st["t"][None, :]), e0.f64(st["flux"][None, None, :]),
                         make_stars(1, period=st["p"], data_var=1e-6), e0.f64(e0.rTA1L([0.0, 0.0])), bench.COVPTS,
                         populations=C)


def leg_batched(sb, C, rng, steps):
    g = sb.group
    sb(draw(rng, F * g, C))
    torch.cuda.synchronize()
    smp = draw(rng, steps * g, C)
    t0 = time.perf_counter()
    out = sb(smp)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return g * steps / dt, int(np.isfinite(out.cpu().numpy()).sum())


def leg_per_sample(st, rng, n):
    from starry_process_amd import StarryProcess

    smp = draw(rng, n, 2)
    t0 = time.perf_counter()
    fin = 0
    for row in smp:
        parts = [StarryProcess(r=r, a=a, b=b, c=c, n=n_, upstream="device") for r, a, b, c, n_ in row.reshape(2, 5)]
        fin += int(np.isfinite(float((parts[0] + parts[1]).log_likelihood(st["t"], st["flux"], 1e-6, p=st["p"]))))
    return n / (time.perf_counter() - t0), fin


if __name__ == "__main__":
    from starry_process_amd.synthetic import synthetic_star

    st = synthetic_star(0, K)
    rng = np.random.RandomState(7)
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        C = {"a": 1, "b": 2}[sys.argv[2]]
        steps = int(sys.argv[3]) if len(sys.argv) > 3 else 12
        rate, fin = leg_batched(batches(C, st), C, rng, steps)
        print(json.dumps({"leg": sys.argv[2], "steps": steps, "evals_per_s": rate, "finite": fin}), flush=True)
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sb = {1: batches(1, st), 2: batches(2, st)}
    leg_per_sample(st, rng, 4)          # (warm: the size integral's memo, the engines' tables)
    rates = {"a": [], "b": [], "c": []}
    for rd in range(rounds):
        for leg in ("a", "b", "c"):
            if leg == "c":
                rate, fin = leg_per_sample(st, rng, 48)
            else:
                rate, fin = leg_batched(sb[1 if leg == "a" else 2], 1 if leg == "a" else 2, rng, steps)
            rates[leg].append(rate)
            print(json.dumps({"round": rd, "leg": leg, "evals_per_s": rate, "finite": fin}), flush=True)
    med = {leg: float(np.median(v)) for leg, v in rates.items()}
    print(json.dumps({"median_evals_per_s": med, "b_over_c": med["b"] / med["c"], "b_over_a": med["b"] / med["a"],
                      "ydeg": YDEG, "K": K, "samples_per_step": sb[2].group, "steps": steps, "rounds": rounds}), flush=True)
