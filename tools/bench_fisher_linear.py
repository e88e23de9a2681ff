#!/usr/bin/env python
"""Time of the Fisher sweeps with linear regressors marginalised out (sp_fisher_marginal_linear,
sp_fisher_conditional_linear) against the plain sweeps, in the same rounds:

    python tools/bench_fisher_linear.py [--shapes 64x1000x15,32x3000x20] [--q 4,20,32] [--branches marginal,conditional]
                                        [--rounds 5] [--calls 10] [--no-kernels] [--out profiles/fisher_linear.txt]

Per shape S x K x ydeg and branch: the sweep alone (tables or moments and their tangents already on the device, every
star resident), without a basis and with q regressors per star -- segment offsets on four quarters, Legendre trends per
quarter, then random systematics columns, lambda = 1e-4.  Device events; 3 warm-up calls of every variant, then
``rounds`` interleaved rounds (plain, q = 4, 20, 32, plain, ...) of ``calls`` calls each; a round's figure is its time
per call; printed: the median of the rounds [their range] and the ratio of the medians to the plain sweep's.  The
traffic the extra stage cannot avoid is one read of the P tangents and two of C^-1 per star (E_i = d_i C Z reads the
tangents, V = C^-1 U and X_i = C^-1 E_i the inverse; the second of those reads it P times from cache): (P + 2) Kr^2
doubles per star, printed beside the time.  The device time per kernel comes from a CHILD process (this script with
--sweep-only under rocprofv3 --kernel-trace --stats, in a run of its own, started before this process touches the
GPU), for the first shape's marginal sweep at the largest q; --no-kernels leaves it out.  Needs a GPU."""
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
LAMBDA = 1.0e-4


def basis_of(t, q):
    """(K, q): four segment offsets, Legendre P_1 .. P_3 per segment, random columns -- the first q of them."""
    from starry_process_amd.linear import offset_basis, polynomial_basis

    K = t.size
    edges = [(j * K) // 4 for j in range(5)]
    U = np.concatenate([offset_basis(K, edges), polynomial_basis(t, 3, edges), np.random.RandomState(K).randn(K, 16)],
                       axis=1)
    return np.ascontiguousarray(U[:, :q])


def setup(branch, S, K, ydeg, qs):
    """{0: plain sweep(), q: sweep() with q regressors}, P, and the objects that own the device memory."""
    import torch

    from starry_process_amd.grad import EnsembleFisher, EnsembleFisherConditional
    from starry_process_amd.synthetic import synthetic_star

    sts = [synthetic_star(s, K) for s in range(S)]
    t, p = np.array([s["t"] for s in sts]), np.array([s["p"] for s in sts])
    sweeps, keep = {}, []
    if branch == "marginal":
        ef = EnsembleFisher(t, ferr=1e-3, p=p, ydeg=ydeg)
        e, P = ef._e, len(NAMES)
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

        def make(ws, **kw):
            return lambda: e.fisher_marginal(ef._t, ef._stars, tab, mv, DY, DM, diag=ef._diag, covpts=ef._covpts,
                                             workspace=ws, **kw)

        ws = e.fisher_linear_workspace(S, K, P, max(qs), ef._covpts)
    else:
        inc = np.linspace(32.0, 83.0, S) if S > 1 else np.array([57.0])
        ef = EnsembleFisherConditional(t, ferr=1e-3, p=p, i=inc, ydeg=ydeg)
        e, P = ef._e, len(NAMES) + len(STAR_NAMES)
        dmu, dSig = ef._moment_tangents(NAMES, *[HP[k] for k in NAMES])
        torch.cuda.synchronize()

        def make(ws, **kw):
            return lambda: e.fisher_conditional(ef._t, ef._stars, ef._rta1, dmu, dSig, star_params=STAR_NAMES,
                                                diag=ef._diag, workspace=ws, **kw)

        ws = e.fisher_conditional_linear_workspace(S, K, P, max(qs))
    # (one workspace, the largest, for every variant: each holds every star)
    sweeps[0] = make(ws)
    for q in qs:
        B = e.f64(np.stack([basis_of(t[s], q).T for s in range(S)]))
        lam = e.f64(np.full((S, q), LAMBDA))
        sweeps[q] = make(ws, basis=B, basis_var=lam)
        keep += [B, lam]
    return sweeps, P, (ef, keep)


def per_call(fn, calls):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def kernel_table(shape, q, sweeps=3):
    """Lines: the device time per kernel of one marginal sweep with q regressors, from a child process under rocprofv3
    (None if it is not there)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    d = tempfile.mkdtemp(prefix="fisher_lin_ks_")
    try:
        subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                        os.path.abspath(__file__), "--sweep-only", str(sweeps), "--shapes", shape, "--q", str(q)],
                       check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    n = sweeps + 3                          # (the child runs 3 warm-up sweeps and `sweeps` more, and the set-up's kernels)
    total = sum(int(r["TotalDurationNs"]) for r in rows)
    lines, extra = [], 0.0
    for r in rows:
        own = "fl_" in r["Name"] or "fisher_finish" in r["Name"]
        if own:
            extra += int(r["TotalDurationNs"]) / 1e6 / n
        if own or len(lines) < 12:
            name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:56]
            lines.append("    %-56s %6.1f launches  %8.3f ms  %5.1f %%" % (
                name, int(r["Calls"]) / n, int(r["TotalDurationNs"]) / 1e6 / n, 100.0 * int(r["TotalDurationNs"]) / total))
    lines.append("    %-56s %20s %8.3f ms" % ("every kernel", "", total / 1e6 / n))
    lines.append("    %-56s %20s %8.3f ms" % ("the regressors' own kernels (fl_*) and the finish", "", extra))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1000x15,32x3000x20")
    ap.add_argument("--q", default="4,20,32")
    ap.add_argument("--branches", default="marginal,conditional")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sweep-only", type=int, default=0)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes, qs = a.shapes.split(","), [int(q) for q in a.q.split(",")]
    klines = None
    if not a.sweep_only and not a.no_kernels:
        klines = kernel_table(shapes[0], max(qs))          # (before this process opens the GPU)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    if a.sweep_only:
        S, K, ydeg = [int(v) for v in shapes[0].split("x")]
        sweeps, _, keep = setup("marginal", S, K, ydeg, qs[-1:])
        for _ in range(3 + a.sweep_only):
            sweeps[qs[-1]]()
        torch.cuda.synchronize()
        return
    lines = ["Fisher sweeps with q regressors per star marginalised out against the plain sweeps: one MI355X, normalized,",
             "data variance 1e-6, lambda = %g (milliseconds per call: median of %d interleaved rounds of %d calls [range of"
             % (LAMBDA, a.rounds, a.calls), "the rounds]; device events, 3 warm-up calls of every variant)", ""]
    for shape in shapes:
        S, K, ydeg = [int(v) for v in shape.split("x")]
        Kr = (K + 63) // 64 * 64
        for branch in a.branches.split(","):
            sweeps, P, keep = setup(branch, S, K, ydeg, qs)
            for fn in sweeps.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {q: [] for q in sweeps}
            for _ in range(a.rounds):
                for q, fn in sweeps.items():
                    ms[q].append(per_call(fn, a.calls))
            med = {q: float(np.median(v)) for q, v in ms.items()}
            gb = S * (P + 2) * Kr * Kr * 8.0 / 1e9
            lines.append("  %s branch, S = %d, K = %d, ydeg %d, P = %d  (the extra stage's unavoidable traffic: %.2f GB)"
                         % (branch, S, K, ydeg, P, gb))
            for q in sweeps:
                extra = med[q] - med[0]
                lines.append("    %-12s %9.3f [%9.3f .. %9.3f]   x %.4f of the plain sweep%s" % (
                    "plain" if q == 0 else "q = %d" % q, med[q], min(ms[q]), max(ms[q]), med[q] / med[0],
                    "" if q == 0 else "   extra %.3f ms = %.0f GB/s of that traffic" % (extra, gb / (extra * 1e-3))
                    if extra > 0 else ""))
            lines.append("")
            print("\n".join(lines[-(len(ms) + 2):]), flush=True)          # (progress: the whole text follows at the end)
            del sweeps, keep
            torch.cuda.empty_cache()
    if klines:
        lines += ["  device time per kernel, one marginal sweep at %s, q = %d (rocprofv3 --kernel-trace --stats, a separate"
                  % (shapes[0], max(qs)), "  run; the twelve largest and every kernel of the regressors' stage):"] + klines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
