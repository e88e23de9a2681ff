"""A/B of the facade's ensemble methods (starry_process_amd/sp.py) between two trees: the same bits, the same time per call.

    python tools/facade_ab.py bits --package DIR --out A.npz      every array the cases return, from DIR's package
    python tools/facade_ab.py compare A.npz B.npz [--out FILE]    by bytes: NaN positions and signed zeros included
    python tools/facade_ab.py time --package DIR --out A.json     wall time per facade call (one JSON line per row)
    python tools/facade_ab.py report --parent P1.json .. --new N1.json .. [--out FILE]

``--package DIR`` is the directory that holds ``starry_process_amd`` (a checkout with its library built); one process
imports one tree.  The caller starts every ``bits`` and ``time`` run as a fresh process under its own time limit and
alternates the trees.

bits: S = 3 stars -- a healthy one, one with a negative ``data_cov`` (its covariance does not factor), one limb-darkened
-- on both branches, with ``tau`` set and unset, normalised (the default ``zmax`` and 5e-4) and not, at K = 2 and 65
(the lower bound; the first size past a 64-wide band and tile), ydeg 5: log_likelihood_ensemble (dense and ragged),
loo / lbo and their ensemble forms (block 7 and an edge list, with and without ``cov``), with regressors q = 1 and 17
also log_likelihood_linear and its ensemble form; for a process that is not normalised predict_ensemble and
sample_conditional_ensemble (variances, full covariance, mean alone, other sample times, with and without
``basis_sample``); for a static one ylm_conditional_ensemble (nsamples = 2), log_likelihood_inclinations_ensemble and
ylm_conditional_marginal_ensemble on P = 5 inclinations, where the star with the negative variance takes the dense route.

time: S = 4, K = 64 (host-dominated) and S = 64, K = 1000 (device-dominated), ydeg 15, marginal branch, not normalised,
with and without q = 8 regressors: log_likelihood_ensemble, loo_ensemble, lbo_ensemble (block 16),
log_likelihood_linear_ensemble, predict_ensemble (variances).  3 warm-up calls, then 3 rounds of 10 timed calls (the
results are NumPy arrays, so a call ends synchronised); a row gives the median of the rounds' medians.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _process(package, ydeg, **kw):
    sys.path.insert(0, os.path.abspath(package))
    import starry_process_amd
    from starry_process_amd import StarryProcess

    assert os.path.dirname(os.path.dirname(os.path.abspath(starry_process_amd.__file__))) == os.path.abspath(package)
    mom = np.load(os.path.join(ROOT, "tests", "golden", "moments_L%d.npz" % ydeg))
    return StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def _flatten(name, value, into):
    if isinstance(value, dict):
        for k, v in value.items():
            _flatten("%s.%s" % (name, k), v, into)
    elif isinstance(value, (tuple, list)):
        for k, v in enumerate(value):
            _flatten("%s.%d" % (name, k), v, into)
    else:
        assert name not in into, name
        into[name] = np.ascontiguousarray(np.asarray(value))


def _inputs(K, q):
    S = 3
    rng = np.random.RandomState(100 * K + q)
    t = np.linspace(0.0, 4.0, K)
    p = np.array([1.3, 2.1, 0.7])
    inc = np.array([75.0, 40.0, 60.0])
    flux = 1e-2 * np.sin(2 * np.pi * t[None, :] / p[:, None]) + 1e-3 * rng.randn(S, K)
    u = np.array([[0.0, 0.0], [0.0, 0.0], [0.4, 0.2]])
    dvar = np.array([1e-6, -1.0, 2e-6])                       # (star 1 does not factor)
    diag = dvar[:, None] * (1.0 + 0.5 * rng.rand(S, K))
    U = np.column_stack([np.ones(K), rng.randn(K, q - 1)]) if q else None
    lam = 1e-4 * (0.5 + rng.rand(q)) if q else None
    ts = np.linspace(0.1, 4.5, 5)
    Us = np.column_stack([np.ones(5), rng.randn(5, q - 1)]) if q else None
    kw = dict(i=inc, p=p, u=u, baseline_mean=np.array([0.0, 1e-3, -1e-3]), baseline_var=np.array([0.0, 1e-6, 1e-5]))
    return t, flux, dvar, diag, U, lam, ts, Us, kw


def bits(package, out):
    import torch

    arrays = {}
    sp0 = None
    for normalized, zmax in ((False, None), (True, None), (True, 5e-4)):
        for marginal in (True, False):
            for tau in (None, 0.8):
                extra = {} if zmax is None else dict(normalization_zmax=zmax)
                sp = _process(package, 5, normalized=normalized, marginalize_over_inclination=marginal, tau=tau,
                              udeg=2, seed=3, **extra)
                sp0 = sp0 or sp
                for K in (2, 65):
                    tag = "n%d_z%s_m%d_tau%d_K%d" % (normalized, zmax, marginal, tau is not None, K)
                    _cases(sp, tag, K, normalized, tau, arrays)
    torch.cuda.synchronize()
    np.savez(out, **arrays)
    nan = sum(int(np.isnan(a).sum()) for a in arrays.values() if a.dtype.kind == "f")
    ninf = sum(int(np.isneginf(a).sum()) for a in arrays.values() if a.dtype.kind == "f")
    print(json.dumps(dict(what="bits", package=os.path.abspath(package), arrays=len(arrays),
                          bytes=int(sum(a.nbytes for a in arrays.values())), nan_entries=nan, neg_inf_entries=ninf)))


def _cases(sp, tag, K, normalized, tau, arrays):
    def keep(name, value):
        _flatten("%s.%s" % (tag, name), value, arrays)

    t, flux, dvar, diag, _, _, ts, _, kw = _inputs(K, 0)
    edges = [0, K] if K == 2 else [0, 1, 3, 35, 64, 65]
    one = dict(i=kw["i"][0], p=kw["p"][0], u=kw["u"][2], baseline_mean=1e-3, baseline_var=1e-6)
    for dname, dc in (("var", dvar), ("diag", diag)):
        keep("lnlike_ensemble." + dname, sp.log_likelihood_ensemble(t, flux, dc, **kw))
        keep("loo_ensemble." + dname, sp.loo_ensemble(t, flux, dc, **kw))
        keep("lbo_ensemble.b7." + dname, sp.lbo_ensemble(t, flux, dc, 7, return_cov=True, **kw))
        keep("lbo_ensemble.edges." + dname, sp.lbo_ensemble(t, flux, dc, edges, **kw))
    keep("loo", sp.loo(t, flux[0], diag[0], **one))
    keep("lbo", sp.lbo(t, flux[2], 2e-6, 7, return_cov=True, **one))
    if K > 2:
        n = [K, K - 20, K - 1]
        keep("lnlike_ensemble.ragged",
             sp.log_likelihood_ensemble([t[:m] for m in n], [flux[s, :m] for s, m in enumerate(n)],
                                        [diag[s, :m] for s, m in enumerate(n)], **kw))
    for q in (1, 17):
        t, flux, dvar, diag, U, lam, ts, Us, kw = _inputs(K, q)
        US = np.ascontiguousarray(np.broadcast_to(U, (3,) + U.shape)) * np.array([1.0, 1.0, 0.5])[:, None, None]
        lin = dict(basis=U, basis_var=lam)
        keep("q%d.loo_ensemble" % q, sp.loo_ensemble(t, flux, diag, **lin, **kw))
        keep("q%d.lbo_ensemble.b7.cov" % q, sp.lbo_ensemble(t, flux, diag, 7, return_cov=True, **lin, **kw))
        keep("q%d.lbo_ensemble.edges" % q, sp.lbo_ensemble(t, flux, dvar, edges, basis=US, basis_var=1e-4, **kw))
        keep("q%d.linear_ensemble.cov" % q, sp.log_likelihood_linear_ensemble(t, flux, diag, U, lam, **kw))
        keep("q%d.linear_ensemble" % q,
             sp.log_likelihood_linear_ensemble(t, flux, dvar, US, 1e-4, return_cov=False, **kw))
        keep("q%d.linear" % q, sp.log_likelihood_linear(t, flux[0], diag[0], U, lam, **one))
        keep("q%d.loo" % q, sp.loo(t, flux[2], 2e-6, **lin, **one))
        keep("q%d.lbo" % q, sp.lbo(t, flux[0], diag[0], edges, **lin, **one))
        if not normalized:
            keep("q%d.predict.cov" % q, sp.predict_ensemble(t, flux, diag, **lin, **kw))
            keep("q%d.predict.diag.at" % q,
                 sp.predict_ensemble(t, flux, dvar, t_sample=ts, return_cov="diag", basis_sample=Us, **lin, **kw))
            keep("q%d.predict.mean.at" % q, sp.predict_ensemble(t, flux, diag, t_sample=ts, return_cov=False, **lin, **kw))
            keep("q%d.sample_conditional" % q,
                 sp.sample_conditional_ensemble(t, flux, diag, t_sample=ts, nsamples=2, seed=5, basis_sample=Us, **lin,
                                                **kw))
    if not normalized:
        keep("predict.cov", sp.predict_ensemble(t, flux, diag, **kw))
        keep("predict.diag.at", sp.predict_ensemble(t, flux, dvar, t_sample=ts, return_cov="diag", **kw))
        keep("predict.mean", sp.predict_ensemble(t, flux, diag, return_cov=False, **kw))
        keep("sample_conditional", sp.sample_conditional_ensemble(t, flux, diag, nsamples=2, seed=5, **kw))
        keep("sample_conditional.at", sp.sample_conditional_ensemble(t, flux, dvar, t_sample=ts, nsamples=3, **kw))
    pk = {k: v for k, v in kw.items() if k != "i"}
    inc = np.linspace(10.0, 85.0, 5)
    keep("inclinations", sp.log_likelihood_inclinations_ensemble(t, flux, diag, inc=inc, **pk))
    if not normalized and tau is None:
        keep("ylm_conditional", sp.ylm_conditional_ensemble(t, flux, diag, nsamples=2, seed=7, **kw))
        keep("ylm_conditional.var", sp.ylm_conditional_ensemble(t, flux, dvar, **kw))
        keep("ylm_marginal", sp.ylm_conditional_marginal_ensemble(t, flux, diag, inc=inc, nsamples=2, seed=9, **pk))
        keep("ylm_marginal.mean", sp.ylm_conditional_marginal_ensemble(t, flux, dvar, inc=inc, return_cov=False, **pk))


def compare(a, b, out):
    A, B = np.load(a), np.load(b)
    lines = []
    if A.files != B.files:         # (the names in the order the results gave them: a dict's key order counts)
        lines.append("DIFFERENT: the two files do not hold the same arrays in the same order (%d, %d)"
                     % (len(A.files), len(B.files)))
    differ = [k for k in A.files if k in B.files and
              (A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes())]
    nan = sum(int(np.isnan(A[k]).sum()) for k in A.files if A[k].dtype.kind == "f")
    ninf = sum(int(np.isneginf(A[k]).sum()) for k in A.files if A[k].dtype.kind == "f")
    lines.append("arrays %d, bytes %d, NaN entries %d, -inf entries %d: %s"
                 % (len(A.files), sum(A[k].nbytes for k in A.files), nan, ninf,
                    "all identical by bytes" if not differ and len(lines) == 0 else "%d DIFFER" % len(differ)))
    lines += ["  differs: " + k for k in differ[:40]]
    # (what the normalised runs with zmax = 5e-4 did: stars cut off by z > zmax next to stars that are not)
    cut = [k for k in A.files if "_z0.0005_" in k and k.endswith("lnlike_ensemble.diag")]
    lines += ["  %s: %s" % (k, A[k].tolist()) for k in cut[:4]]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")
    return 1 if differ or lines[0].startswith("DIFFERENT") else 0


def _timed(fn, reps=10, rounds=3, warm=3):
    for _ in range(warm):
        fn()
    meds = []
    for _ in range(rounds):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        meds.append(float(np.median(ms)))
    return float(np.median(meds))


def time_rows(package, out):
    sp = _process(package, 15, normalized=False, marginalize_over_inclination=True, udeg=2)
    from starry_process_amd import linear

    rows = []
    for S, K in ((4, 64), (64, 1000)):
        rng = np.random.RandomState(K)
        t = np.linspace(0, 30.0 * K / 1000, K)
        p = rng.uniform(0.5, 3.0, S)
        flux = 1e-2 * np.sin(2 * np.pi * t[None, :] / p[:, None]) + 1e-3 * rng.randn(S, K)
        diag = 1e-6 * (1 + rng.rand(S, K))
        U = linear.stack_bases(linear.offset_basis(K, np.round(np.linspace(0, K, 6)).astype(int)),
                               linear.polynomial_basis(t, 3))
        assert U.shape == (K, 8)
        kw = dict(i=rng.uniform(30.0, 85.0, S), p=p, u=[0.3, 0.1], baseline_var=1e-6)
        lin = dict(basis=U, basis_var=1e-4)
        calls = {
            "log_likelihood_ensemble": lambda: sp.log_likelihood_ensemble(t, flux, diag, **kw),
            "loo_ensemble": lambda: sp.loo_ensemble(t, flux, diag, **kw),
            "loo_ensemble q=8": lambda: sp.loo_ensemble(t, flux, diag, **lin, **kw),
            "lbo_ensemble b=16": lambda: sp.lbo_ensemble(t, flux, diag, 16, **kw),
            "lbo_ensemble b=16 q=8": lambda: sp.lbo_ensemble(t, flux, diag, 16, **lin, **kw),
            "log_likelihood_linear_ensemble q=8": lambda: sp.log_likelihood_linear_ensemble(t, flux, diag, U, 1e-4, **kw),
            "predict_ensemble": lambda: sp.predict_ensemble(t, flux, diag, return_cov="diag", **kw),
            "predict_ensemble q=8": lambda: sp.predict_ensemble(t, flux, diag, return_cov="diag", **lin, **kw),
        }
        for name, fn in calls.items():
            rows.append(dict(S=S, K=K, call=name, ms=round(_timed(fn), 4)))
            print(json.dumps(rows[-1]), flush=True)
    with open(out, "w") as fh:
        json.dump(dict(package=os.path.abspath(package), rows=rows), fh)


def report(parent, new, out):
    def load(files):
        table = {}
        for f in files:
            for r in json.load(open(f))["rows"]:
                table.setdefault((r["S"], r["K"], r["call"]), []).append(r["ms"])
        return table

    P, N = load(parent), load(new)
    lines = ["wall ms per facade call; parent: median, lowest and highest of its %d rounds; new: median of its %d rounds"
             % (len(parent), len(new)),
             "%3s %5s  %-36s %9s %9s %9s %9s %7s  %s" % ("S", "K", "call", "parent", "low", "high", "new", "ratio", "")]
    outside = 0
    for key in P:
        pm, lo, hi, nm = float(np.median(P[key])), min(P[key]), max(P[key]), float(np.median(N[key]))
        mark = "" if lo <= nm <= hi else ("above" if nm > hi else "below")
        outside += bool(mark)
        lines.append("%3d %5d  %-36s %9.3f %9.3f %9.3f %9.3f %7.3f  %s" % (key + (pm, lo, hi, nm, nm / pm, mark)))
    lines.append("%d of %d rows outside the parent's own spread" % (outside, len(P)))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("bits", "compare", "time", "report"))
    ap.add_argument("files", nargs="*")
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", nargs="+", default=[])
    ap.add_argument("--new", nargs="+", default=[])
    a = ap.parse_args()
    if a.mode == "bits":
        bits(a.package, a.out)
    elif a.mode == "time":
        time_rows(a.package, a.out)
    elif a.mode == "compare":
        return compare(a.files[0], a.files[1], a.out)
    else:
        report(a.parent, a.new, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
