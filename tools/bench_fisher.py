#!/usr/bin/env python
"""Time of the ensemble's Fisher information (grad.EnsembleFisher, sp_fisher_marginal) at the headline shape: 64 stars,
K = 1000, P = 5 (r, a, b, c, n), ydeg 15, the cadences and periods of the synthetic stars of SURVEY 8d.

    python tools/bench_fisher.py [--stars 64] [--cadences 1000] [--calls 10] [--no-kernels] [--out profiles/fisher.txt]

Device events around every call of the sweep alone (tables and tangents already on the device) and around every call of
the whole facade (moments, tables, tangents, sweep, the transfers), after 2 warm-up calls: median [min .. max].  The
device time per kernel kind comes from a CHILD process (this script with --sweep-only under rocprofv3 --kernel-trace
--stats, started before this process touches the GPU); --no-kernels leaves it out.  The fraction of the fp64 matrix
peak (78.6 TFLOP/s) counts the flops the P products EXECUTE, 2 P roundup(K, 64)^3 per star.  Nothing here compares with
an earlier commit: the capability is new.  Needs a GPU: there is no other path."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)
NAMES = ("r", "a", "b", "c", "n")
PEAK = 78.6e12


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return "%.3f [%.3f .. %.3f]" % (np.median(ms), ms[0], ms[-1])


def timed(fn, calls):
    import torch

    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def setup(S, K):
    """(the facade, sweep(): one sp_fisher_marginal call on the facade's own tables and tangents)."""
    import torch

    from starry_process_amd.grad import EnsembleFisher
    from starry_process_amd.synthetic import synthetic_star

    sts = [synthetic_star(s, K) for s in range(S)]
    t, p = np.array([s["t"] for s in sts]), np.array([s["p"] for s in sts])
    ef = EnsembleFisher(t, ferr=1e-3, p=p)
    e = ef._e
    x0 = {"r": HP["r"], "dr": None, "a": HP["a"], "b": HP["b"]}
    hp0 = dict(x0, c=HP["c"], n=HP["n"])
    torch.cuda.synchronize()
    with torch.cuda.stream(ef._stream):
        yp0, mean0, (mu, Sig, tab, mv) = ef._tables(e, **hp0)
        at_point = torch.cuda.Event()
        at_point.record(ef._stream)
    dy, dm, _ = ef._table_tangents(x0, hp0, True, at_point, yp0, mean0, mu, Sig)
    torch.cuda.synchronize()
    DY, DM = torch.stack([dy[k] for k in NAMES]), torch.stack([dm[k] for k in NAMES])
    ws = ef._workspace(len(NAMES))

    def sweep():
        return e.fisher_marginal(ef._t, ef._stars, tab, mv, DY, DM, diag=ef._diag, covpts=ef._covpts, workspace=ws)

    return ef, sweep, ws


def kernel_table(S, K, sweeps=3):
    """Lines: the device time per kernel of one sweep, from a child process under rocprofv3 (None if it is not there)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, None
    d = tempfile.mkdtemp(prefix="fisher_ks_")
    try:
        subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                        os.path.abspath(__file__), "--sweep-only", str(sweeps), "--stars", str(S), "--cadences", str(K)],
                       check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, None
        rows = list(csv.DictReader(open(files[0])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    # the child runs 2 warm-up sweeps and `sweeps` more, and the set-up's table kernels (small)
    n = sweeps + 2
    lines, products = [], 0.0
    total = sum(int(r["TotalDurationNs"]) for r in rows)
    for r in rows[:14]:
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:56]
        ms = int(r["TotalDurationNs"]) / 1e6 / n
        lines.append("    %-56s %6.1f launches  %8.3f ms  %5.1f %%" % (name, int(r["Calls"]) / n, ms,
                                                                      100.0 * int(r["TotalDurationNs"]) / total))
        if "128, 128" in r["Name"] or "128,128" in r["Name"]:
            products += ms
    lines.append("    %-56s %20s %8.3f ms" % ("every kernel", "", total / 1e6 / n))
    return lines, products


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=64)
    ap.add_argument("--cadences", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sweep-only", type=int, default=0)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, K, P = a.stars, a.cadences, len(NAMES)
    klines = products = None
    if not a.sweep_only and not a.no_kernels:
        klines, products = kernel_table(S, K)          # (before this process opens the GPU)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    ef, sweep, ws = setup(S, K)
    for _ in range(2):
        sweep()
    torch.cuda.synchronize()
    if a.sweep_only:
        for _ in range(a.sweep_only):
            sweep()
        torch.cuda.synchronize()
        return
    ms_sweep = timed(sweep, a.calls)
    for _ in range(2):
        F = ef(**HP)
    ms_call = timed(lambda: ef(**HP), a.calls)
    from starry_process_amd.grad import cramer_rao

    Kr = (K + 63) // 64 * 64
    flops = 2.0 * P * float(Kr) ** 3 * S
    w = np.linalg.eigvalsh(F)
    _, sigma = cramer_rao(F[:3, :3])
    lines = [
        "ensemble Fisher information: one MI355X, ydeg 15, S = %d, K = %d, P = %d (r, a, b, c, n), normalized," % (S, K, P),
        "data variance 1e-6 (milliseconds: median [min .. max]; device events, 2 warm-up calls, %d timed calls)" % a.calls,
        "",
        "  sp_fisher_marginal, the sweep alone          %s" % stats(ms_sweep),
        "  EnsembleFisher(...)(r, a, b, c, n)            %s" % stats(ms_call),
        "  workspace of the sweep: %d bytes (every star resident)" % ws.numel(),
        "",
        "  flops the P products execute (2 P Kr^3 per star, Kr = %d): %.3g per call" % (Kr, flops),
        "  over the whole sweep: %.1f TFLOP/s, %.3f of the fp64 matrix peak (78.6 TFLOP/s)" % (
            flops / (np.median(ms_sweep) * 1e-3) / 1e12, flops / (np.median(ms_sweep) * 1e-3) / PEAK),
    ]
    if klines:
        if products:
            lines.append("  over the products' own kernel time (%.3f ms):  %.1f TFLOP/s, %.3f of the peak" % (
                products, flops / (products * 1e-3) / 1e12, flops / (products * 1e-3) / PEAK))
        lines += ["", "  device time per kernel, one sweep (rocprofv3 --kernel-trace --stats, a separate run):"] + klines
    lines += ["", "  F's eigenvalues: %s" % " ".join("%.4g" % v for v in w),
              "  Cramer-Rao sigma of (r, a, b) with c and n held fixed: %s" % " ".join("%.4g" % v for v in sigma)]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
