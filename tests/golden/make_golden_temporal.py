#!/usr/bin/env python
"""
Generates tests/golden/temporal.npz by EXECUTING THE REFERENCE's time-variable
StarryProcess.sample_ylm(t) and flux(y, t) (reference sp.py:489-516, 1237-1282,
ops/sample.py:24-33):

    make -C oracle ref && python tests/golden/make_golden_temporal.py

Same harness as make_golden_ylm_conditional.py (oracle/refharness: the
reference's own Python on an eager Theano stand-in).  The moments are the
``default`` set of moments_L{ydeg}.npz, factored by the reference's cho_factor.
The reference draws its deviates through ``random_normal`` (sp.py:513); the
generator replaces that function, in this process only, by
RandomState(seed).normal(size=shape) -- the draw the package makes.

Per case <c>:  <c>_t, <c>_Y (nsamples, Nt, nylm), <c>_flux3 / <c>_flux3n (flux of
Y, not normalised / normalised), <c>_flux2 / <c>_flux2n (flux of Y[0]), and
<c>_scalars = [kernel (1 Matern-3/2, 2 exp-squared), tau, ydeg, nsamples, seed,
cond(K_t)].  The flux is taken at i = 65, p = 0.8, u = [0.2, 0.1].
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle.refharness.loadref import load_reference  # noqa: E402

warnings.simplefilter("ignore")
ref = load_reference()
SP = ref.sp.StarryProcess
cho_factor = ref.math.cho_factor
KERNELS = {1: ref.temporal.Matern32Kernel, 2: ref.temporal.ExpSquaredKernel}
I, P, U = 65.0, 0.8, [0.2, 0.1]


def A(x):
    return np.array(np.asarray(x), dtype=np.float64, copy=True)


def run(name, kind, t, tau, ydeg, ns, seed, out, singular=False):
    mom = np.load(os.path.join(OUT, "moments_L%d.npz" % ydeg))
    sp = SP(ydeg=ydeg, normalized=False, tau=tau, temporal_kernel=KERNELS[kind], seed=seed)
    sp._mean_ylm = mom["default_mean_ylm"]
    sp._cov_ylm = mom["default_cov_ylm"]
    sp._cho_cov_ylm = cho_factor(sp._cov_ylm)
    sp._flux = ref.flux.FluxIntegral(sp._mean_ylm, sp._cov_ylm, marginalize_over_inclination=False,
                                     covpts=sp._covpts, ydeg=ydeg)
    Kt = A(KERNELS[kind](t, t, tau))
    cond = np.linalg.cond(Kt)
    if not singular:
        assert cond <= 1e5, (name, cond)
    real = ref.sp.random_normal
    try:
        ref.sp.random_normal = lambda rng_, shape: np.random.RandomState(seed).normal(
            size=tuple(int(s) for s in shape))
        Y = A(sp.sample_ylm(t, nsamples=ns))
    finally:
        ref.sp.random_normal = real
    assert Y.shape == (ns, t.shape[0], (ydeg + 1) ** 2)
    assert np.isnan(Y).all() if singular else np.isfinite(Y).all()
    rec = {}
    for norm in (False, True):
        sp._normalized = norm
        rec["_flux3" + "n" * norm] = A(sp.flux(Y, t, i=I, p=P, u=U))
        rec["_flux2" + "n" * norm] = A(sp.flux(Y[0], t, i=I, p=P, u=U))
    sp._normalized = False
    assert rec["_flux2"].shape == (t.shape[0],) and rec["_flux2n"].shape == (1, t.shape[0])
    out.update({name + "_t": t, name + "_Y": Y,
                name + "_scalars": np.array([kind, tau, ydeg, ns, seed, cond])})
    out.update({name + k: v for k, v in rec.items()})
    print("  %-2s kind=%d Nt=%4d ydeg=%2d ns=%d cond=%.3g  Y[0,0,0]=%+.6e  flux3[0,0]=%+.6e" % (
        name, kind, t.shape[0], ydeg, ns, cond, Y[0, 0, 0], rec["_flux3"][0, 0]))


def main():
    out = {}
    run("a", 1, np.linspace(0, 20, 65), 2.0, 15, 2, 3, out)        # Nt crosses a 64 edge
    run("b", 1, np.linspace(0, 20, 40), 2.0, 5, 3, 5, out)
    run("c", 2, np.linspace(0, 40, 40), 1.0, 5, 3, 7, out)
    run("d", 2, np.linspace(0, 50, 200), 25.0, 5, 2, 11, out, singular=True)   # K_t does not factor: all NaN
    path = os.path.join(OUT, "temporal.npz")
    np.savez_compressed(path, **out)
    print("wrote temporal.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
