"""Conditional light curves of an ensemble on one GPU: the loop over single-star ``predict`` calls against one
``predict_ensemble`` call on the same inputs (marginal branch, S = 64 stars, K = Ks = 1000, ydeg 15).

  cov    predict_ensemble(return_cov=True)   against the loop
  diag   predict_ensemble(return_cov="diag") against the loop
  mean   predict_ensemble(return_cov=False)  against the loop

The loop is S calls of StarryProcess.predict, one star each: what served an ensemble before.  Every configuration
runs in a fresh process of its own, under its own time limit; one that fails or runs out of time ends the run.
Inside a process the two routes ALTERNATE: each of `repeats` rounds times one window of the loop and one window of
the ensemble call, so that both see the same state of a shared host.  A window is timed on the host clock from
NumPy arguments to NumPy results (the download is a device synchronise) and holds `inner` calls, chosen so that
it lasts about 50 ms or more; `warmup` rounds come first.  Reported per route: the median, minimum and maximum
time of ONE call over the rounds; then the ratio of the medians and the worst case over the rounds (the loop's
fastest window over the ensemble's slowest).  The device part alone (Engine.predict_ensemble on device tensors,
HIP events around ten calls) and the workspace are reported beside it; the cov configuration also times the
download of the S covariances alone.

    python tools/bench_predict.py [--stars 64] [--K 1000] [--Ks 1000] [--warmup 2] [--repeats 9] [--timeout 300]
    python tools/bench_predict.py --config diag      (one configuration, in this process)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

CONFIGS = ("cov", "diag", "mean")
MODES = {"cov": True, "diag": "diag", "mean": False}


def inputs(S, K, Ks):
    rng = np.random.RandomState(8)
    t = np.linspace(0, 4, K)
    ts = np.sort(rng.uniform(-0.5, 4.5, size=(S, Ks)), axis=1)
    p = 0.7 + 1.3 * rng.rand(S)
    flux = np.array([1e-2 * np.sin(2 * np.pi * t / p[s] + s) for s in range(S)]) + 1e-3 * rng.randn(S, K)
    return t, ts, flux, p


def stats(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def window(fn, inner):
    """Milliseconds per call of `inner` calls in one timed window."""
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / inner


def run_config(name, S, K, Ks, warmup, repeats):
    import torch

    from starry_process_amd import StarryProcess

    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L15.npz"))
    sp = StarryProcess(ydeg=15, normalized=False, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"])
    t, ts, flux, p = inputs(S, K, Ks)
    kw = dict(baseline_mean=1e-4, baseline_var=1e-6)

    def loop():
        return [sp.predict(t, flux[s], 1e-6, t_sample=ts[s], p=p[s], **kw) for s in range(S)]

    def ens():
        return sp.predict_ensemble(t, flux, 1e-6, t_sample=ts, p=p, return_cov=MODES[name], **kw)

    for _ in range(max(1, warmup)):
        loop()
        ens()
    # calls per window: about 50 ms of work or more
    n_loop = max(1, int(np.ceil(50.0 / window(loop, 1))))
    n_ens = max(1, int(np.ceil(50.0 / window(ens, 1))))
    lm, em = [], []
    for _ in range(repeats):
        lm.append(window(loop, n_loop))
        em.append(window(ens, n_ens))
    out = dict(config=name, stars=S, K=K, Ks=Ks, warmup=warmup, rounds=repeats, loop_calls_per_window=n_loop,
               ensemble_calls_per_window=n_ens, loop_ms=stats(lm), ensemble_ms=stats(em),
               loop_over_ensemble=round(float(np.median(lm) / np.median(em)), 2),
               loop_over_ensemble_worst=round(min(lm) / max(em), 2))
    # the device part alone: device tensors in, device tensors out
    e = sp._engine
    tt, fl, stars, utab, diag = sp._ensemble_args(t, flux, 1e-6, None, p, None, kw["baseline_mean"], kw["baseline_var"])
    rta1 = e.f64(e.rTA1L(utab))
    tab, mv = e.kernel_table(rta1, sp._covpts)
    td, tsd, fd, sd = e.f64(tt), e.f64(ts), e.f64(fl), e.stars_to_device(stars)

    def dev():
        return e.predict_ensemble(td, tsd, fd, sd, covpts=sp._covpts, tab=tab, meanvar=mv, mode=MODES[name])

    dev()
    n_dev = 10
    dms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n_dev):
            dev()
        b.record()
        b.synchronize()
        dms.append(a.elapsed_time(b) / n_dev)
    out["device_ms"] = stats(dms)
    out["workspace_bytes"] = int(e._L.sp_predict_workspace_bytes(e._h, S, K, Ks, sp._covpts))
    if name == "cov":
        # the download of the S covariances alone: what bounds the full-covariance call end to end
        cov = dev()[1]
        out["download_MB"] = round(cov.numel() * 8 / 2 ** 20, 1)
        out["download_ms"] = stats([window(lambda: cov.cpu().numpy(), 1) for _ in range(repeats)])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=64)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--Ks", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per configuration")
    ap.add_argument("--config", choices=CONFIGS, default=None)
    a = ap.parse_args()
    if a.config:
        run_config(a.config, a.stars, a.K, a.Ks, a.warmup, a.repeats)
        return 0
    res = {}
    for name in CONFIGS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--config", name,
               "--stars", str(a.stars), "--K", str(a.K), "--Ks", str(a.Ks), "--warmup", str(a.warmup),
               "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps(dict(config=name, error="exit status %d" % r.returncode)), flush=True)
            return 1      # (nothing more is started on the GPU after a failure)
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(dict(
        summary=True, stars=a.stars, K=a.K, Ks=a.Ks,
        loop_over_ensemble={k: res[k]["loop_over_ensemble"] for k in CONFIGS},
        loop_over_ensemble_worst={k: res[k]["loop_over_ensemble_worst"] for k in CONFIGS},
        diag_over_cov=round(res["diag"]["ensemble_ms"]["median"] / res["cov"]["ensemble_ms"]["median"], 3),
        workspace_bytes=res["cov"]["workspace_bytes"])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
