#!/usr/bin/env python
"""Time of the conditional branch's Fisher information (grad.EnsembleFisherConditional, sp_fisher_conditional) at the
headline shape: 64 stars, K = 1000, P = 7 (r, a, b, c, n, i, p), ydeg 15, the cadences and periods of the synthetic
stars of SURVEY 8d at inclinations spread over 32 .. 83 degrees.

    python tools/bench_fisher_conditional.py [--stars 64] [--cadences 1000] [--calls 10] [--no-kernels]
                                             [--out profiles/fisher_conditional.txt]

Device events around every call of the sweep alone (moments and their tangents already on the device) and around every
call of the whole facade (moments, tangents, sweep, the transfers), after 2 warm-up calls: median [min .. max].  The
device time per kernel kind comes from a CHILD process (this script with --sweep-only under rocprofv3 --kernel-trace
--stats, in a run of its own, started before this process touches the GPU); --no-kernels leaves it out.  The fraction of
the fp64 matrix peak (78.6 TFLOP/s) counts the flops the products EXECUTE, with Kr = roundup(K, 64), per star and
parameter: the raw tangent, 2 Kr^2 N (+ 2 Kr N^2 for a hyperparameter, whose A dSigma comes first), and C^-1 dC, 2 Kr^3.
Nothing here compares with an earlier commit: the capability is new.  Needs a GPU: there is no other path."""
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
STAR_NAMES = ("i", "p")
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
    """(the facade, sweep(): one sp_fisher_conditional call on the facade's own moments and tangents, its workspace)."""
    import torch

    from starry_process_amd.grad import EnsembleFisherConditional
    from starry_process_amd.synthetic import synthetic_star

    sts = [synthetic_star(s, K) for s in range(S)]
    t, p = np.array([s["t"] for s in sts]), np.array([s["p"] for s in sts])
    inc = np.linspace(32.0, 83.0, S) if S > 1 else np.array([57.0])
    ef = EnsembleFisherConditional(t, ferr=1e-3, p=p, i=inc)
    e = ef._e
    dmu, dSig = ef._moment_tangents(NAMES, *[HP[k] for k in NAMES])
    torch.cuda.synchronize()
    ws = ef._workspace(len(NAMES) + len(STAR_NAMES))

    def sweep():
        return e.fisher_conditional(ef._t, ef._stars, ef._rta1, dmu, dSig, star_params=STAR_NAMES, diag=ef._diag,
                                    workspace=ws)

    return ef, sweep, ws


def kernel_table(S, K, sweeps=3):
    """Lines: the device time per kernel of one sweep, from a child process under rocprofv3 (None if it is not there)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, None
    d = tempfile.mkdtemp(prefix="fisher_cond_ks_")
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
    # the child runs 2 warm-up sweeps and `sweeps` more, and the set-up's upstream kernels (small)
    n = sweeps + 2
    lines, products = [], 0.0
    total = sum(int(r["TotalDurationNs"]) for r in rows)
    for r in rows[:16]:
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:56]
        ms = int(r["TotalDurationNs"]) / 1e6 / n
        lines.append("    %-56s %6.1f launches  %8.3f ms  %5.1f %%" % (name, int(r["Calls"]) / n, ms,
                                                                      100.0 * int(r["TotalDurationNs"]) / total))
        if "mm_nt_kernel" in r["Name"] or "gemm_nt_kernel" in r["Name"]:
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
    S, K, Ph, P = a.stars, a.cadences, len(NAMES), len(NAMES) + len(STAR_NAMES)
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
        ef(**HP)
    ms_call = timed(lambda: ef(**HP), a.calls)
    from starry_process_amd.grad import cramer_rao, cramer_rao_ensemble

    N = ef._e.N
    Kr = (K + 63) // 64 * 64
    flops = S * (P * (2.0 * Kr * Kr * N + 2.0 * float(Kr) ** 3) + Ph * 2.0 * Kr * N * N)
    # (a normalised light curve does not fix the amplitude: the bounds are taken about r, a, b, c with n held fixed)
    F4 = ef(params=NAMES[:4], **HP)
    _, sigma_known = cramer_rao(F4)
    cr = cramer_rao_ensemble(ef.per_star, 4, ef.status)
    si = cr["sigma_star_known"][:, 0]
    lines = [
        "conditional-branch Fisher information: one MI355X, ydeg 15, S = %d, K = %d, P = %d (r, a, b, c, n, i, p)," % (S, K, P),
        "normalized, data variance 1e-6 (milliseconds: median [min .. max]; device events, 2 warm-up calls, %d timed calls)"
        % a.calls,
        "",
        "  sp_fisher_conditional, the sweep alone             %s" % stats(ms_sweep),
        "  EnsembleFisherConditional(...)(r, a, b, c, n)       %s" % stats(ms_call),
        "  workspace of the sweep: %d bytes (every star resident)" % ws.numel(),
        "",
        "  flops the products execute (per star: P (2 Kr^2 N + 2 Kr^3) + P_h 2 Kr N^2, Kr = %d, N = %d): %.3g per call"
        % (Kr, N, flops),
        "  over the whole sweep: %.1f TFLOP/s, %.3f of the fp64 matrix peak (78.6 TFLOP/s)" % (
            flops / (np.median(ms_sweep) * 1e-3) / 1e12, flops / (np.median(ms_sweep) * 1e-3) / PEAK),
    ]
    if klines:
        if products:
            lines.append("  over the products' own kernel time (%.3f ms, the forward's products included):  %.1f TFLOP/s, "
                         "%.3f of the peak" % (products, flops / (products * 1e-3) / 1e12,
                                               flops / (products * 1e-3) / PEAK))
        lines += ["", "  device time per kernel, one sweep (rocprofv3 --kernel-trace --stats, a separate run):"] + klines
    lines += ["", "  stars of status 0: %d of %d" % (int((ef.status == 0).sum()), S),
              "  Cramer-Rao sigma of (r, a, b, c), n held fixed, inclinations and periods known:        %s"
              % " ".join("%.4g" % v for v in sigma_known),
              "  the same with every star's inclination and period marginalised:                       %s"
              % " ".join("%.4g" % v for v in cr["sigma_shared"]),
              "  Cramer-Rao sigma of a star's inclination [degrees] at known hyperparameters: min %.3g, median %.3g, max %.3g"
              % (np.nanmin(si), np.nanmedian(si), np.nanmax(si))]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
