"""
End-to-end gradient of the log-likelihood (the part beyond the single ops): what
the reference obtains by letting Theano chain the ``grad`` / ``L_op`` methods of its Ops through the
graph of ``StarryProcess.log_likelihood`` (sp.py:1052-1188; verified by finite differences in the
reference's tests/test_lnlike.py:100-136).

Here the graph is ``torch.autograd`` over fp64 tensors on the GPU, and its heavy nodes are the
library's own reverse-mode kernels:

  * ``lnL(C, r)``                the factorisation ``sp_cho_factor`` forward; backward in closed form,
                                 ``C_bar = 1/2 (alpha alpha^T - C^-1)``, ``r_bar = -alpha`` with
                                 ``alpha = C^-1 r`` (what chaining ``Cholesky.L_op`` and ``Solve.L_op``,
                                 math.py:40-100, gives; tests/test_gpu_linalg_rev.py shows the two agree),
                                 both solves on the device (``sp_cho_solve``);
  * ``special_tensordotRz``      backward ``sp_special_tensordotRz_rev`` (wigner.h:464-531);
  * the glue between them -- rotation of the moments to the polar frame (flux.py:54-62), mean / variance
    (flux.py:297-308), spline build (flux.py:310-330), the K x K gather interpolation (flux.py:256-276),
    the normalisation correction with its alpha(z), beta(z) series (sp.py:705-727, ops/norm/norm.py:26-44),
    noise and baseline (sp.py:1135-1151) -- is elementwise / small-matrix torch arithmetic that autograd
    differentiates by itself.

``log_likelihood_with_grad`` returns d lnL / d(mu_y, Sigma_y): the gradient with respect to the hot path's
own inputs.  ``hyper_gradient`` takes it on to (r, a, b, c, n): c and n enter the moments as plain scale
factors (contrast.py:21-33), r, a, b through the upstream integrals, whose directional derivatives are
taken by central differences of the device quadrature (upstream_device.py: smooth and accurate to
rounding in its parameters, 0.3 ms per evaluation) -- one reverse sweep through the expensive part, six
cheap upstream evaluations, instead of ten full likelihoods for finite differences of everything.

One star, the marginalised branch (with or without normalisation); this is a diagnostic / optimisation
aid (``mci.optimize()``-style callers), not part of the timed hot path.
"""
import numpy as np

from ._lib import SP_STAR_NO_BASIS
from .defaults import defaults
from .engine import get_engine
from .stars import check_period_inclination, ensemble_stars
from .temporal import kernel_id

__all__ = ["EnsembleGradient", "ensemble_gradient", "log_likelihood_with_grad", "hyper_gradient",
           "EnsembleFisher", "ensemble_fisher", "fisher_max_covpts", "cramer_rao", "EnsembleGradientConditional", "ensemble_gradient_conditional_device", "ensemble_gradient_conditional",
           "EnsembleFisherConditional", "ensemble_fisher_conditional", "cramer_rao_ensemble"]

_cache = {}
_BOUNDS = {"r": (0.0, 90.0), "dr": (0.0, 90.0), "a": (0.0, 1.0), "b": (0.0, 1.0)}      # of the upstream integrals


def _torch():
    import torch

    return torch


def _constants(e, u):
    """Device constants for limb darkening ``u``: dense blockdiag Rx(pi/2), w, W (flux.py:181-231), rTA1L(u)."""
    from . import _lib, hostconst

    torch = _torch()
    key = (e.ydeg, e.device_index, tuple(np.asarray(u, dtype=float).reshape(-1)))
    if key in _cache:
        return _cache[key]
    ydeg, N = e.ydeg, e.N
    Rpk = e.Rx(np.array([0.5 * np.pi]), deriv=False)[0][0].cpu().numpy()
    D = np.zeros((N, N))
    off = 0
    for l in range(ydeg + 1):
        w_ = 2 * l + 1
        D[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = Rpk[off:off + w_ * w_].reshape(w_, w_)
        off += w_ * w_
    wnp, Wnp = hostconst.marginal_constants(ydeg)
    rta1 = np.asarray(e.rTA1L(np.asarray(u, dtype=float).reshape(-1)[: e.udeg])).reshape(-1)
    idx = _lib.index_tables(ydeg)
    rho = rta1[idx["m0"]][idx["l_of"]]
    W = Wnp * rho[:, None] * rho[None, :]
    # w (N): w[l-block] = rTA1[l-block] . wnp[l]  (flux.py:196-198): mean = sum_n w[n] ez[n]
    wv = np.zeros(N)
    off = 0
    for l in range(ydeg + 1):
        w_ = 2 * l + 1
        wv[l * l:(l + 1) ** 2] = rta1[l * l:(l + 1) ** 2] @ wnp[off:off + w_ * w_].reshape(w_, w_)
        off += w_ * w_
    _cache[key] = (e.f64(D), e.f64(wv), e.f64(W), e.f64(rta1))
    return _cache[key]


def _functions(e):
    torch = _torch()

    class SpecialTensordotRz(torch.autograd.Function):
        @staticmethod
        def forward(ctx, W, M, theta):
            ctx.save_for_backward(W, M, theta)
            return e.special_tensordotRz(W, M.contiguous(), theta)

        @staticmethod
        def backward(ctx, bf):
            W, M, theta = ctx.saved_tensors
            bM, _ = e.special_tensordotRz_rev(W, M.contiguous(), theta, bf.contiguous())
            return None, bM, None

    class GaussianLogLike(torch.autograd.Function):
        """-1/2 r^T C^-1 r - 1/2 log det C - K/2 log 2 pi; -inf when C is not positive definite."""

        @staticmethod
        def forward(ctx, C, r):
            K = C.shape[0]
            L, info = e.cho_factor(C.contiguous())
            if int(info.max().item()) != 0:
                ctx.failed = True
                return C.new_tensor(-float("inf"))
            ctx.failed = False
            alpha = e.cho_solve(L, r.reshape(K, 1).contiguous()).reshape(K)
            ctx.save_for_backward(L, alpha)
            return -0.5 * torch.dot(r, alpha) - torch.log(torch.diagonal(L)).sum() - 0.5 * K * np.log(2 * np.pi)

        @staticmethod
        def backward(ctx, g):
            if ctx.failed:
                return None, None
            L, alpha = ctx.saved_tensors
            K = L.shape[0]
            Cinv = e.cho_solve(L, torch.eye(K, dtype=L.dtype, device=L.device))
            return g * 0.5 * (torch.outer(alpha, alpha) - Cinv), -g * alpha

    class DesignMatrix(torch.autograd.Function):
        """A(theta, inc) = ((1_K x rTA1) Rx(-inc)) Rz(theta) Rx(pi/2)  (flux.py:88-105, 278-281); backward with
        the library's reverse rotation (tensordotRz_rev) and the derivative matrices of sp_Rx."""

        @staticmethod
        def forward(ctx, theta, inc, rta1):
            K = theta.shape[0]
            R, dR = e.Rx(np.array([-float(inc.item()), 0.5 * np.pi, -0.5 * np.pi]), deriv=True)
            M0 = rta1.reshape(1, -1).expand(K, -1).contiguous()
            M1 = e.dotRx(M0, R[0])
            A = e.dotRx(e.tensordotRz(M1, theta.contiguous()), R[1])
            ctx.save_for_backward(theta, M0, M1, R, dR)
            return A

        @staticmethod
        def backward(ctx, bA):
            theta, M0, M1, R, dR = ctx.saved_tensors
            bM2 = e.dotRx(bA.contiguous(), R[2])          # Rx(pi/2)^T = Rx(-pi/2)
            bM1, btheta = e.tensordotRz_rev(M1, theta.contiguous(), bM2)
            # M1 = M0 Rx(-inc): d/d inc = -M0 Rx'(-inc)
            binc = -(bM1 * e.dotRx(M0, dR[0])).sum().reshape(1)
            return btheta, binc, None

    return SpecialTensordotRz, GaussianLogLike, DesignMatrix


def _alpha_beta(z, order):
    fac = z * 0.0 + 1.0
    alpha, beta = z * 0.0, z * 0.0
    for n in range(order + 1):
        alpha = alpha + fac
        beta = beta + 2 * n * fac
        fac = fac * z * (2 * n + 3)
    return alpha, beta


def _upstream_eps(N, ukw, like=None):
    """[N] the jitter on the diagonal of Sigma_y (``epsy``, and ``epsy15`` from l = 15 on: upstream_kwargs ``ukw`` or the
    defaults) -- the part of Sigma_y that does not scale with c and n.  NumPy, or a tensor on the device of ``like``."""
    epsy = float(ukw.get("epsy", defaults["epsy"]))
    if like is None:
        eps = np.ones(N) * epsy
    else:
        eps = _torch().full((N,), epsy, dtype=_torch().float64, device=like.device)
    eps[15 ** 2:] = float(ukw.get("epsy15", defaults["epsy15"]))
    return eps


def _cn_chain(gm, gS, c, n, unit=None):
    """(d lnL / dc, d lnL / dn) through the moments mu_y = c n m, Sigma_y - eps = c^2 n S (contrast.py:21-33), from the
    inner products gm = <gmu, mu_y> and gS = <gSig, Sigma_y - eps> of the moments' adjoints (floats or 0-d tensors).
    On the boundary c = 0 or n = 0 the moments at the point hold nothing to divide by, but the derivative is not zero
    there: ``unit()`` returns the same two products against the moments at unit contrast and unit number of spots (one
    more upstream evaluation, made only there), and d/dc = n gm + 2 c n gS, d/dn = c gm + c^2 gS."""
    if c != 0 and n != 0:
        return gm / c + 2.0 * gS / c, gm / n + gS / n
    gm, gS = unit()
    return n * gm + 2.0 * c * n * gS, c * gm + c * c * gS


def _central_ends(name, x, h):
    """(xl, xh) of the central difference about x, a step h max(|x|, 0.1) each way; one-sided within a step of a bound."""
    step = h * max(abs(x), 0.1)
    return max(x - step, _BOUNDS[name][0]), min(x + step, _BOUNDS[name][1])


def _temporal_id(temporal_kernel, tau):
    """The device's kernel selector for ``temporal_kernel`` (a name or one of temporal.py's callables); None without a
    timescale."""
    return (temporal_kernel if isinstance(temporal_kernel, str) else kernel_id(temporal_kernel)) if tau else None


def log_likelihood_with_grad(mean_ylm, cov_ylm, t, flux, data_var, i=defaults["i"], p=defaults["p"], u=None,
                             tau=None, temporal_kernel="matern32", baseline_mean=0.0, baseline_var=0.0,
                             marginalize_over_inclination=True, normalized=True, covpts=defaults["covpts"],
                             ydeg=defaults["ydeg"], udeg=defaults["udeg"],
                             norm_order=defaults["normalization_order"],
                             zmax=defaults["normalization_zmax"], device=None):
    """(lnL, grads) for ONE light curve; NumPy in, NumPy out.  ``grads`` holds d lnL / d of
    "mean_ylm" [N], "cov_ylm" [N, N] (its N^2 entries treated as independent: symmetrise it for a symmetric
    perturbation), "p", "tau" (when a timescale is given) and, on the conditional branch, "i" (per degree)."""
    torch = _torch()
    e = get_engine(ydeg, udeg, device)
    u = np.zeros(e.udeg) if u is None else np.asarray(u, dtype=float).reshape(-1)[: e.udeg]
    D, wv, W, rta1 = _constants(e, u)
    Special, LogLike, Design = _functions(e)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    K = t.shape[0]
    td = e.f64(t)
    leaf = lambda v: e.f64(np.atleast_1d(np.asarray(v, dtype=np.float64))).clone().requires_grad_(True)  # noqa: E731
    mu = leaf(np.asarray(mean_ylm).reshape(-1))
    Sig = e.f64(np.asarray(cov_ylm, dtype=np.float64)).clone().requires_grad_(True)
    per, inc = leaf(p), leaf(i)
    # theta = 2 pi mod(t / p, 1) (flux.py:262, 279): the integer part is data
    tp = td / per
    theta = 2 * np.pi * (tp - torch.floor(tp.detach()))
    if marginalize_over_inclination:
        # polar frame (flux.py:54-62)
        ez = D.t() @ mu
        Ez = D.t() @ (Sig + torch.outer(mu, mu)) @ D
        mean = torch.dot(wv, ez)
        # kernel on the lag grid and its cubic coefficients (flux.py:297-330)
        dx = 2 * np.pi / covpts
        xp = np.arange(-dx, 2 * np.pi + 2.5 * dx, dx)
        yp = Special.apply(W, Ez, e.f64(xp)) - mean ** 2
        y0, y1, y2, y3 = yp[:-3], yp[1:-2], yp[2:-1], yp[3:]
        a0 = y1
        a1 = -y0 / 3.0 - 0.5 * y1 + y2 - y3 / 6.0
        a2 = 0.5 * (y0 + y2) - y1
        a3 = 0.5 * ((y1 - y2) + (y3 - y0) / 3.0)
        # K x K interpolation (flux.py:256-276); the interval index is data
        if K == 1:
            cov = (torch.sum(W * Ez) - mean ** 2).reshape(1, 1)
        else:
            x = torch.abs(theta[:, None] - theta[None, :]).reshape(-1)
            ii = torch.floor(x.detach() / dx).to(torch.int64)
            x0 = (x - e.f64(xp)[ii + 1]) / dx
            cov = (a0[ii] + a1[ii] * x0 + a2[ii] * x0 ** 2 + a3[ii] * x0 ** 3).reshape(K, K)
    else:
        # A = ((1_K x rTA1) Rx(-i)) Rz(theta) Rx(pi/2); mean = (A mu)_0, cov = A Sigma A^T (flux.py:278-281, 337-343)
        A = Design.apply(theta, inc * (np.pi / 180.0), rta1)
        mean = (A @ mu)[0]
        cov = A @ Sig @ A.t()
    tau_leaf = None
    if tau is not None:
        # temporal.py:8-16
        tau_leaf = leaf(tau)
        dt = torch.abs(td[:, None] - td[None, :])
        if temporal_kernel == "matern32":
            xx = np.sqrt(3.0) * dt / tau_leaf
            cov = cov * ((1 + xx) * torch.exp(-xx))
        elif temporal_kernel == "expsquared":
            cov = cov * torch.exp(-(dt ** 2) / (2 * tau_leaf))
        else:
            raise ValueError("temporal_kernel must be 'matern32' or 'expsquared'")
    gp_mean = mean
    zval = 0.0
    if normalized:
        # sp.py:705-727 with mu = 1 + mean; the GP mean of the normalised process is zero (sp.py:669-670)
        mu1 = 1.0 + mean
        m = cov.mean()
        q = cov.sum(dim=1) / (K * m)
        z = m / mu1 ** 2
        pp = 1.0 - q
        alpha, beta = _alpha_beta(z, int(norm_order))
        cov = (alpha / mu1 ** 2) * cov + z * ((alpha + beta) * torch.outer(pp, pp) - alpha * torch.outer(q, q))
        gp_mean = mean * 0.0
        zval = float(z.item())
    dv = np.asarray(data_var, dtype=np.float64)
    noise = e.f64(np.full(K, float(dv)) if dv.ndim == 0 else dv.reshape(-1))
    C = cov + torch.diag(noise) + float(baseline_var)
    r = e.f64(np.asarray(flux, dtype=np.float64).reshape(-1)) - (gp_mean + float(baseline_mean))
    lnl = LogLike.apply(C, r)
    leaves = {"mean_ylm": mu, "cov_ylm": Sig, "p": per}
    if not marginalize_over_inclination:
        leaves["i"] = inc
    if tau_leaf is not None:
        leaves["tau"] = tau_leaf
    if not bool(torch.isfinite(lnl)) or (normalized and zval > zmax):
        return -np.inf, {k: np.zeros(tuple(v.shape)) if v.numel() > 1 else 0.0 for k, v in leaves.items()}
    lnl.backward()
    grads = {}
    for k, v in leaves.items():
        g = v.grad if v.grad is not None else torch.zeros_like(v)
        grads[k] = g.cpu().numpy() if v.numel() > 1 else float(g.item())
    return float(lnl.item()), grads


def hyper_gradient(t, flux, data_var, r=defaults["r"], dr=defaults["dr"], a=defaults["a"], b=defaults["b"],
                   c=defaults["c"], n=defaults["n"], h=1e-4, upstream_kwargs=None, moments0=None, exact=True,
                   **kwargs):
    """(lnL, {"r": ., "a": ., "b": ., "c": ., "n": ., "p": ., ...}): the log-likelihood of one light curve and its
    gradient with respect to the spot hyperparameters (moments by the device quadrature, upstream_device.py;
    "dr" too when a spread of radii is given) and whatever else ``log_likelihood_with_grad`` differentiates
    (p; i on the conditional branch; tau).
    kwargs: as for ``log_likelihood_with_grad`` (i, p, u, tau, normalized, marginalize_over_inclination, ...);
    moments0: (mu_y, Sigma_y) the value and the moment gradient are taken at, when they are not the device
    quadrature's own (a process built with upstream="reference": same integrals, the reference's rounding);
    upstream_kwargs: the constructor's numerical keywords of the moment integrals (epsy, epsy15, sfac, ...).
    r, a and b: with one radius (dr = None) the moments' EXACT tangents (the quadrature rule differentiated with
    respect to its exponents, the sigmoid profile with respect to its radius: ylm_moments_device_grad -- what the
    reference's analytic latitude derivatives are, ops/include/latitude.h:21-173); with a spread of radii, or
    exact=False, central differences of the moments, one-sided within a step of the bounds [0, 1]
    (ops/exceptions.py:30-48 raises outside); c = 0 or n = 0 (no spots: Sigma_y = diag(eps), mu_y = 0)
    has a zero gradient in the other of the two and is returned as such."""
    from .upstream_device import ylm_moments_device

    ydeg = kwargs.get("ydeg", defaults["ydeg"])
    e = get_engine(ydeg, kwargs.get("udeg", defaults["udeg"]), kwargs.get("device"))

    ukw = dict(upstream_kwargs or {})

    def moments(r_, dr_, a_, b_, c_=c, n_=n):
        mu, Sig = ylm_moments_device(e, r=r_, dr=dr_, a=a_, b=b_, c=c_, n=n_, **ukw)
        return mu.cpu().numpy(), Sig.cpu().numpy()

    mu, Sig = moments(r, dr, a, b)
    mu_at, Sig_at = (mu, Sig) if moments0 is None else (np.asarray(moments0[0]), np.asarray(moments0[1]))
    lnl, g = log_likelihood_with_grad(mu_at, Sig_at, t, flux, data_var, **kwargs)
    gmu, gSig = g["mean_ylm"], g["cov_ylm"]
    eps = np.diag(_upstream_eps(mu.shape[0], ukw))        # Sigma_y - eps: the part that scales with c and n
    inner = lambda m_, S_: (gmu @ m_, np.sum(gSig * (S_ - eps)))          # noqa: E731
    out = {k: v for k, v in g.items() if k not in ("mean_ylm", "cov_ylm")}
    if c != 0 and n != 0:
        gc, gn = _cn_chain(*inner(mu, Sig), c, n)
    else:
        # _cn_chain's boundary rule with the surviving factor left inside the moments (at c = 0: the moments at c = 1
        # and the given n; at n = 0: at n = 1 and the given c) -- the same derivative, rounded in another order
        gm, gS = inner(*moments(r, dr, a, b, c_=c if c != 0 else 1.0, n_=n if n != 0 else 1.0))
        gc, gn = gm if (c == 0 and n != 0) else 0.0, gm + gS if (n == 0 and c != 0) else 0.0
    out.update({"c": float(gc), "n": float(gn)})
    x0 = {"r": r, "dr": dr, "a": a, "b": b}
    if dr is None and exact:
        # one radius: the moments' exact tangents (upstream_device.ylm_moments_device_grad)
        from .upstream_device import ylm_moments_device_grad

        _, _, dmu, dSig = ylm_moments_device_grad(e, r=r, a=a, b=b, c=c, n=n, **ukw)
        dmu, dSig = dmu.cpu().numpy(), dSig.cpu().numpy()
        for k, name in enumerate(("r", "a", "b")):
            out[name] = float(gmu @ dmu[k] + np.sum(gSig * dSig[k]))
        return lnl, out
    for name in ("r", "dr", "a", "b"):
        if x0[name] is None:
            continue
        x = float(x0[name])
        xl, xh = _central_ends(name, x, h)
        m0, S0_ = (mu, Sig) if xl == x else moments(*[xl if k == name else x0[k] for k in x0])   # (x0: r, dr, a, b)
        m1, S1_ = (mu, Sig) if xh == x else moments(*[xh if k == name else x0[k] for k in x0])
        out[name] = float(gmu @ ((m1 - m0) / (xh - xl)) + np.sum(gSig * ((S1_ - S0_) / (xh - xl))))
    return lnl, out


# the per-star derivatives of EnsembleGradient(wrt=...), in the order of the device's row (SP_STARBAR slots 0-4)
_WRT = ("p", "tau", "baseline_mean", "baseline_var", "log_var")


def _check_wrt(wrt, has_tau, has_basis=False):
    """``wrt`` as a tuple of known names (None stays None); ValueError otherwise.  No device work."""
    if wrt is None:
        return None
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    for name in wrt:
        if name not in _WRT and name != "basis_var":
            raise ValueError("wrt: unknown name %r (one of %s)" % (name, ", ".join(_WRT + ("basis_var",))))
    if "tau" in wrt and not has_tau:
        raise ValueError("wrt: 'tau' needs a timescale (EnsembleGradient(..., tau=...))")
    if "basis_var" in wrt and not has_basis:
        raise ValueError("wrt: 'basis_var' needs regressors (EnsembleGradient(..., basis=..., basis_var=...))")
    return wrt


class _EnsembleSweep(object):
    """What the two ensemble gradients share: their data and star records on the GPU."""

    def _setup(self, t, flux, ferr, p, i, u, ydeg, baseline_mean, baseline_var, tau, temporal_kernel, device):
        """Host work first (every ValueError before a device is touched), then ``self._open`` for the engine and the
        uploads: t, flux, the per-cadence variances (or None), the star records, rTA1L of the distinct limb-darkening
        sets and the temporal kernel's id; synchronised on return.  Returns the host records and sets."""
        S, K = flux.shape[0], flux.shape[-1]
        if K < 2:
            raise ValueError("at least two cadences")
        check_period_inclination(p)
        udeg = defaults["udeg"]
        var = np.asarray(ferr, dtype=np.float64) ** 2
        t, stars, utab, diag = ensemble_stars((S, K), t, p, i, u, udeg, baseline_mean, baseline_var,
                                              np.broadcast_to(var, (S, K)) if var.ndim == 2 else var,
                                              tau=float(tau) if tau else 0.0)
        e = self._e = self._open(ydeg, udeg, device)
        self.S, self.K = S, K
        self._t, self._flux = e.f64(t), e.f64(np.ascontiguousarray(flux))
        self._diag = None if diag is None else e.f64(diag)
        self._stars = e.stars_to_device(stars)
        self._rta1 = e.f64(e.rTA1L(utab))
        self._temporal = _temporal_id(temporal_kernel, tau)
        _torch().cuda.synchronize(e.device)
        return stars, utab


class _MarginalSweep(_EnsembleSweep):
    """What the marginal branch's sweeps (gradient, Fisher information) share beyond their data: four engines on four
    streams, the kernel tables at a point and the tables' tangents with respect to the hyperparameters."""

    def _open(self, ydeg, udeg, device):
        from .engine import engine_slots

        # the sweep's handle + three more for the tables' finite differences: a table evaluation is a latency chain
        # of a dozen small kernels (0.3 ms); nine of them in a row on ONE stream outlast the sweep they should hide
        # behind (3.2 against 2.5 ms), three streams of three do not
        slots = engine_slots(ydeg, udeg, device, 4)
        (e, self._stream), self._side = slots[0], slots[1:]
        return e

    def _configure(self, covpts, normalized, h, upstream_kwargs, exact):
        """The tail of the constructors: the numerical keywords the sweeps share."""
        self._covpts, self._exact = int(defaults["covpts"] if covpts is None else covpts), bool(exact)
        self._normalized, self._h, self._ukw = bool(normalized), float(h), dict(upstream_kwargs or {})

    def _at_point(self, r, a, b, c, n, dr):
        """(tab, mv, the arguments of ``_table_tangents``): the device drained, the tables at the point enqueued on the main
        stream, the event behind them recorded.  Ends there: the caller's sweep is enqueued BEFORE the side streams' work."""
        torch = _torch()
        x0 = {"r": float(r), "dr": dr, "a": float(a), "b": float(b)}
        hp0 = dict(x0, c=float(c), n=float(n))
        torch.cuda.synchronize(self._e.device)
        with torch.cuda.stream(self._stream):
            yp0, mean0, (mu, Sig, tab, mv) = self._tables(self._e, **hp0)
            at_point = torch.cuda.Event()
            at_point.record(self._stream)
        return tab, mv, (x0, hp0, self._exact and dr is None, at_point, yp0, mean0, mu, Sig)

    def _tables(self, eng, **hp):
        """(yp [ntab, np], mean [ntab]) of the kernel tables at the given hyperparameters, on eng's stream."""
        from .upstream_device import ylm_moments_device

        mu, Sig = ylm_moments_device(eng, **hp, **self._ukw)
        eng.set_moments_dev(mu, Sig)
        tab, mv = eng.kernel_table(self._rta1, self._covpts)
        return tab[:, 0, :], mv[:, 0], (mu, Sig, tab, mv)

    def _table_tangents(self, x0, hp0, exact, at_point, yp0, mean0, mu, Sig):
        """({name: d yp / d name [ntab, np]}, {name: d mean / d name [ntab]}, events) for r, a, b, c, n (and dr when
        x0["dr"] is given), enqueued on the three side streams; the caller's stream waits for ``events`` before it reads
        them.  x0: {"r", "dr", "a", "b"}, hp0: x0 with c and n; at_point: the event behind the tables at the point
        (yp0, mean0, from the moments mu, Sig) on the main stream.  exact: the moments' exact tangents for r, a, b
        (``ylm_moments_device_grad``), central differences of the table (step h) otherwise."""
        import torch

        r, a, b, c, n = hp0["r"], hp0["a"], hp0["b"], hp0["c"], hp0["n"]
        dy, dm, events = {}, {}, []

        def central(eng, name):
            xl, xh = _central_ends(name, float(x0[name]), self._h)
            yl, ml, _ = self._tables(eng, **dict(hp0, **{name: xl}))
            yh, mh, _ = self._tables(eng, **dict(hp0, **{name: xh}))
            dy[name], dm[name] = (yh - yl) / (xh - xl), (mh - ml) / (xh - xl)

        def tangent(eng, stream, tang, k, name):
            # The table is linear in Sigma_y + mu_y mu_y^T and its mean in mu_y (flux.py:297-320): with the moments
            # (dmu, X - dmu dmu^T), X = dSigma + dmu mu^T + mu dmu^T, the table kernels return f[X] - dmean^2 and
            # dmean, and d yp = f[X] - 2 mean dmean.  One table evaluation per parameter, no step size.
            mu1, dmu, dSig = tang
            d1 = dmu[k]
            cross = torch.outer(d1, mu1)
            eng.set_moments_dev(d1, dSig[k] + cross + cross.t() - torch.outer(d1, d1))
            tk, mk = eng.kernel_table(self._rta1, self._covpts)
            dmean = mk[:, 0]
            stream.wait_event(at_point)         # (mean0 is the main stream's; recorded before the sweep was enqueued)
            dy[name] = tk[:, 0, :] + (dmean * (dmean - 2.0 * mean0))[:, None]
            dm[name] = dmean

        (e1, s1), (e2, s2), (e3, s3) = self._side
        with torch.cuda.stream(s1):
            if exact:
                # the moments again, with their tangents, beside the main stream (which only waits for the value)
                from .upstream_device import ylm_moments_device_grad

                mu1, _, dmu, dSig = ylm_moments_device_grad(e1, r=r, a=a, b=b, c=c,
                                                            n=n, **self._ukw)
                tang = (mu1, dmu, dSig)
                have_tangents = torch.cuda.Event()
                have_tangents.record(s1)
                tangent(e1, s1, tang, 0, "r")
                tangent(e1, s1, tang, 1, "a")
            else:
                central(e1, "r")
                if x0["dr"] is not None:
                    central(e1, "dr")
            events.append(torch.cuda.Event())
            events[-1].record(s1)
        with torch.cuda.stream(s2):
            if exact:
                s2.wait_event(have_tangents)
                tangent(e2, s2, tang, 2, "b")
            else:
                central(e2, "a")
                central(e2, "b")
            events.append(torch.cuda.Event())
            events[-1].record(s2)
        with torch.cuda.stream(s3):
            eu = e3
            # c and n, exactly: mu_y = c n m, Sigma_y = c^2 n S + eps; the second moment f = yp + mean^2 is linear in
            # Sigma_y + mu_y mu_y^T:  f = c^2 n f_S + c^2 n^2 f_mm + f_eps,  mean = c n m1
            # (the tables at the point are the main stream's: they are ready long before the sweep is)
            s3.wait_event(at_point)
            ypA, meanA, muA, SigA = yp0, mean0, mu, Sig
            eps = _upstream_eps(muA.shape[0], self._ukw, like=muA)
            zero_mu = torch.zeros_like(muA)
            eu.set_moments_dev(muA, torch.zeros_like(SigA))
            t_mm, _ = eu.kernel_table(self._rta1, self._covpts)             # f_mm part: yp = c^2 n^2 f_mm - mean^2
            eu.set_moments_dev(zero_mu, torch.diag(eps))
            t_eps, _ = eu.kernel_table(self._rta1, self._covpts)            # f_eps (mean 0)
            f = ypA + meanA[:, None] ** 2
            f_mm = t_mm[:, 0, :] + meanA[:, None] ** 2
            f_eps = t_eps[:, 0, :]
            f_S = f - f_mm - f_eps
            if c != 0 and n != 0:
                dy["c"] = 2.0 * (f - f_eps) / c - 2.0 * meanA[:, None] ** 2 / c
                dm["c"] = meanA / c
                dy["n"] = (f_S + 2.0 * f_mm) / n - 2.0 * meanA[:, None] ** 2 / n
                dm["n"] = meanA / n
            else:
                # On the boundary c = 0 or n = 0 the tables at the point hold nothing to divide by: take them at unit
                # contrast and unit number of spots instead (f is a polynomial in c and n: f = c^2 n f_S' + c^2 n^2 f_mm'
                # + f_eps, mean = c n m1), one more upstream evaluation -- what hyper_gradient returns there too.
                from .upstream_device import ylm_moments_device

                mu1, Sig1 = ylm_moments_device(eu, **dict(hp0, c=1.0, n=1.0), **self._ukw)
                eu.set_moments_dev(mu1, torch.zeros_like(Sig1))
                t1, mv1 = eu.kernel_table(self._rta1, self._covpts)
                m1 = mv1[:, 0]
                f_mm1 = t1[:, 0, :] + m1[:, None] ** 2
                eu.set_moments_dev(zero_mu, Sig1 - torch.diag(eps))
                tS, _ = eu.kernel_table(self._rta1, self._covpts)
                f_S1 = tS[:, 0, :]
                cc, nn = c, n
                dy["c"] = 2.0 * cc * nn * f_S1 + 2.0 * cc * nn * nn * f_mm1 - 2.0 * cc * nn * nn * m1[:, None] ** 2
                dm["c"] = nn * m1
                dy["n"] = cc * cc * f_S1 + 2.0 * cc * cc * nn * f_mm1 - 2.0 * cc * cc * nn * m1[:, None] ** 2
                dm["n"] = cc * m1
            events.append(torch.cuda.Event())
            events[-1].record(s3)
        return dy, dm, events


class _RegressorVariances(object):
    """``upload_basis_var`` of the four sweeps that take ``basis=``: they keep the basis in ``_basis`` (None without
    one), its variances in ``_basis_var`` and the number of regressors in ``_q``."""

    def upload_basis_var(self, basis_var):
        """New prior variances of the regressors' weights -- scalar, (q,) or (S, q), finite and >= 0 -- for the calls
        that follow; the basis stays on the device."""
        from .linear import check_regressor_variances

        if self._basis is None:
            raise ValueError("`basis_var` needs regressors (%s(..., basis=..., basis_var=...))" % type(self).__name__)
        lam = check_regressor_variances(basis_var, self.S, self._q)
        self._basis_var = self._e.f64(lam)


class EnsembleGradient(_MarginalSweep, _RegressorVariances):
    """Log-likelihood of an ENSEMBLE of light curves and its gradient with respect to the spot hyperparameters
    (r, a, b, c, n[, dr]) in ONE device sweep per evaluation -- what ``theano.grad`` of the summed
    ``sp.log_likelihood`` is in the reference (tests/test_lnlike.py:100-136, calibrate/log_prob.py:53-91), for every
    star of the batch at once.  Marginal branch, scalar or per-cadence data variance; one light curve per star
    (flux [S, K]) or M of them on the star's one covariance (flux [S, M, K]: the shared-covariance form of
    sp.py:1162-1171 -- with S = 1 the gradient of what ``calibrate.get_log_prob`` evaluates).

        eg = EnsembleGradient(t, flux, ferr=1e-3, p=periods)       # data -> GPU, once
        lnl, grad = eg(r=20., a=.4, b=.27, c=.1, n=10.)             # lnl: sum over stars; grad: dict
        eg.lnlike                                                   # per-star values of the last call

    How: d lnL / dC = (alpha alpha^T - C^-1) / 2 with C^-1 from the factorisation's own machinery
    (sp_spd_inverse_batched: the identity rides through the blocked Cholesky), pulled back on the device through the
    normalisation and the cubic interpolation to the adjoint of each star's kernel TABLE (304 numbers) and flux mean
    (sp_lnlike_grad_marginal).  The chain from the hyperparameters to the table is short and cheap -- moments by the
    device quadrature, then the table kernels -- and is differentiated there: exactly in c and n (the moments are
    mu_y = c n m, Sigma_y = c^2 n S + eps, contrast.py:21-33, and the table is linear in Sigma_y + mu_y mu_y^T), and
    since round 5 exactly in r, a, b too: the moments come with their tangents (ylm_moments_device_grad: the
    quadrature rule differentiated with respect to its exponents -- the reference's analytic latitude derivatives,
    ops/include/latitude.h:21-173), and one table evaluation per parameter turns a tangent of the moments into the
    tangent of the table, on two more streams while the sweep runs.  With a spread of radii (dr) or exact=False:
    central differences of the table (step h), as in round 4.

    Linear regressors (``basis``, ``basis_var``): flux = process + U w + noise with w ~ N(0,
    diag(basis_var)), the model of ``log_likelihood_linear_ensemble`` -- segment offsets, instrumental trends,
    systematics vectors, marginalised without the K x K matrix.  ``basis`` (K, q) shared or (S, K, q), ``basis_var``
    scalar, (q,) or (S, q), validated as that method validates them; one light curve per star.  The call then returns
    the marginalised likelihood and ITS gradient (sp_lnlike_grad_linear), ``wrt`` also takes "basis_var" -- (S, q), the
    derivative with respect to the prior variances themselves, finite at 0 -- and ``w_mean`` (S, q) holds the posterior
    mean of the weights after a call.  ``upload_basis_var`` changes the variances without sending the basis again (a
    sampler's step in lambda)."""

    def __init__(self, t, flux, ferr=1.0e-3, p=1.0, u=None, ydeg=15, baseline_var=0.0, baseline_mean=0.0,
                 normalized=True, covpts=None, tau=None, temporal_kernel="matern32", device=None, h=1.0e-4,
                 upstream_kwargs=None, exact=True, basis=None, basis_var=None):
        flux = np.asarray(flux, dtype=np.float64)
        if flux.ndim not in (2, 3):
            raise ValueError("flux must be (S, K) or (S, M, K)")
        M = flux.shape[1] if flux.ndim == 3 else 1
        from .linear import _regressor_args

        if basis is not None and flux.ndim == 3:
            raise ValueError("regressors are served for one light curve per star: `flux` must be (S, K) with a `basis`")
        U, Ut, lam = _regressor_args(basis, basis_var, flux.shape[0], flux.shape[1],
                                     "a `basis` needs the prior variances of its weights, `basis_var`")
        # (the star records carry no inclination on the marginal branch: make_stars' own default)
        stars, utab = self._setup(t, flux, ferr, p, None, u, ydeg, baseline_mean, baseline_var, tau, temporal_kernel,
                                  device)
        e = self._e
        self._ntab = utab.shape[0]
        self._table = _torch().as_tensor(stars["table"].astype(np.int64), device=e.device)
        self._configure(covpts, normalized, h, upstream_kwargs, exact)
        self._basis = self._basis_var = self.w_mean = None
        self._q = 0
        if U is None:
            self._ws = e.grad_workspace(self.S, self.K, self._covpts, M)
        else:
            self._q = U.shape[2]
            self._basis = e.f64(Ut)
            self._basis_var = e.f64(lam)
            self._ws = e.grad_linear_workspace(self.S, self.K, self._q, self._covpts)
            _torch().cuda.synchronize(e.device)
        self.lnlike = None

    _WRT = _WRT

    def __call__(self, r=defaults["r"], a=defaults["a"], b=defaults["b"], c=defaults["c"], n=defaults["n"], dr=None,
                 wrt=None):
        """(sum of the stars' log-likelihoods, {"r": ., "a": ., "b": ., "c": ., "n": .[, "dr": .]}).

        wrt: None, or a tuple of names out of ("p", "tau", "baseline_mean", "baseline_var", "log_var"): the dict then
        also holds the derivatives with respect to the stars' OWN parameters, from the same device sweep
        (sp_lnlike_grad_marginal_stars) and the same one transfer: "p", "baseline_mean", "baseline_var", "log_var" as
        arrays [S] -- d lnL_s / d of star s's period, baseline mean, baseline variance and the log of a common factor
        on its data variances (ferr^2, scalar or per cadence; with s_s^2 = exp(log_var) ferr_s^2) -- and "tau" as a
        float, the sum over the stars (the constructor takes one timescale).  Where the ensemble shares a baseline (or a
        noise factor), as in calibrate/log_prob.py:7-106, the derivative with respect to the shared value is the sum of
        the array.  A star the likelihood rejects adds zeros.  d/dp is the derivative of the interpolant inside its
        segments, as ``log_likelihood_with_grad``'s.

        With regressors: the likelihood and every derivative above are those of the marginalised model; wrt may hold
        "basis_var": an array [S, q], d lnL_s / d of the prior variance of star s's regressor j.  New prior variances:
        ``upload_basis_var`` ahead of the call."""
        import torch

        wrt = _check_wrt(wrt, self._temporal is not None, self._basis is not None)
        e = self._e
        # main stream: the tables at the point, then the sweep
        tab, mv, point = self._at_point(r, a, b, c, n, dr)
        with torch.cuda.stream(self._stream):
            sweep_kw = dict(diag=self._diag, covpts=self._covpts, temporal=self._temporal,
                            normalized=self._normalized, workspace=self._ws)
            sbar = lbar = wmean = None
            if self._basis is not None:
                lnl, ybar, mbar, sbar, lbar, wmean, status = e.lnlike_grad_linear(
                    self._t, self._flux, self._stars, self._basis, self._basis_var, tab, mv, **sweep_kw)
                if wrt is None:
                    sbar = None
            elif wrt is None:
                lnl, ybar, mbar, status = e.lnlike_grad_marginal(self._t, self._flux, self._stars, tab, mv, **sweep_kw)
            else:
                lnl, ybar, mbar, sbar, status = e.lnlike_grad_marginal_stars(self._t, self._flux, self._stars, tab, mv,
                                                                             **sweep_kw)
        # three more streams, meanwhile: the tables' derivatives
        dy, dm, events = self._table_tangents(*point)
        with torch.cuda.stream(self._stream):
            for ev in events:
                self._stream.wait_event(ev)
            # adjoints per table: the stars that share a flux operator add up
            Yb = torch.zeros(self._ntab, ybar.shape[1], dtype=torch.float64, device=e.device).index_add_(0, self._table, ybar)
            Mb = torch.zeros(self._ntab, dtype=torch.float64, device=e.device).index_add_(0, self._table, mbar)
            names = [k for k in ("r", "dr", "a", "b", "c", "n") if k in dy]
            # ONE transfer for everything the host wants: [gradient | per-star values | per-star status]
            parts = [lnl, status.to(torch.float64)]
            if names:
                DY, DM = torch.stack([dy[k] for k in names]), torch.stack([dm[k] for k in names])
                parts.insert(0, (DY * Yb).sum(dim=(1, 2)) + (DM * Mb).sum(dim=1))
            if sbar is not None:
                parts.append(sbar.reshape(-1))
            if lbar is not None:
                parts += [lbar.reshape(-1), wmean.reshape(-1)]
            host = torch.cat(parts).cpu().numpy()    # (on the main stream, which has waited for the others)
        ng = len(names)
        self.lnlike = host[ng:ng + self.S].copy()
        self.status = host[ng + self.S:ng + 2 * self.S].astype(np.uint32)
        total = float(self.lnlike.sum())
        grad = {k: float(v) for k, v in zip(names, host[:ng])}
        if lbar is not None:
            sq = self.S * self._q
            self.w_mean = host[-sq:].reshape(self.S, self._q).copy()
            if wrt is not None and "basis_var" in wrt:
                grad["basis_var"] = host[-2 * sq:-sq].reshape(self.S, self._q).copy()
            host = host[:-2 * sq]
        if sbar is not None:
            sb = host[ng + 2 * self.S:].reshape(self.S, -1)
            for k in wrt:
                if k == "basis_var":
                    continue
                col = sb[:, self._WRT.index(k)]
                grad[k] = float(col.sum()) if k == "tau" else col.copy()
        return total, grad


def ensemble_gradient(t, flux, ferr=1.0e-3, p=1.0, r=defaults["r"], a=defaults["a"], b=defaults["b"],
                      c=defaults["c"], n=defaults["n"], dr=None, wrt=None, **kwargs):
    """One-shot form of ``EnsembleGradient``: (sum of log-likelihoods, {"r": ., "a": ., "b": ., "c": ., "n": .});
    wrt: the per-star derivatives to return as well (``EnsembleGradient.__call__``)."""
    # (before any data goes to the device)
    wrt = _check_wrt(wrt, bool(kwargs.get("tau")), kwargs.get("basis") is not None)
    return EnsembleGradient(t, flux, ferr=ferr, p=p, **kwargs)(r=r, a=a, b=b, c=c, n=n, dr=dr, wrt=wrt)


# the hyperparameters the Fisher information may be taken about, in the order of its default rows
_FISHER_PARAMS = ("r", "a", "b", "c", "n", "dr")


def _check_params(params, has_dr):
    """``params`` as a tuple of distinct names out of (r, a, b, c, n, dr); ValueError otherwise, and for "dr" without a
    spread of radii.  No device work."""
    params = (params,) if isinstance(params, str) else tuple(params)
    if not params:
        raise ValueError("params: at least one name (out of %s)" % ", ".join(_FISHER_PARAMS))
    for k, name in enumerate(params):
        if name not in _FISHER_PARAMS:
            raise ValueError("params: unknown name %r (one of %s)" % (name, ", ".join(_FISHER_PARAMS)))
        if name in params[:k]:
            raise ValueError("params: %r is named twice" % (name,))
    if "dr" in params and not has_dr:
        raise ValueError("params: 'dr' needs a spread of radii (dr=...)")
    return params


def _fisher_regressors(basis, basis_var, S, K):
    """The ``basis=``, ``basis_var=`` pair of the Fisher classes, checked on the host (``linear.check_regressors``):
    (Ut [S, q, K], lam [S, q], q), or (None, None, 0) without a basis.  ValueError for one of the pair without the
    other, a shape that does not fit, more than MAX_REGRESSORS columns, a non-finite basis, a negative or non-finite
    variance.  No device work."""
    from .linear import _regressor_args

    U, Ut, lam = _regressor_args(basis, basis_var, S, K, "a `basis` needs the prior variances of its weights, `basis_var`")
    return (None, None, 0) if U is None else (Ut, lam, U.shape[2])


class _FisherRegressors(_RegressorVariances):
    """What the two Fisher classes share for ``basis=``: the upload behind ``_setup`` and the engine call's keywords."""

    def _regressor_kwargs(self):
        """The engine call's ``basis=``, ``basis_var=``; nothing without regressors (the call is then the plain one)."""
        return {"basis": self._basis, "basis_var": self._basis_var} if self._q else {}

    def _upload_regressors(self, Ut, lam, q):
        self._q = q
        self._basis = self._basis_var = None
        if q:
            self._basis, self._basis_var = self._e.f64(Ut), self._e.f64(lam)
            _torch().cuda.synchronize(self._e.device)


def fisher_max_covpts(P):
    """The largest lag grid ``covpts`` the Fisher sweep serves for P parameters: its tangent kernel keeps P + 1 tables
    of covpts + 4 doubles beside 1152 doubles of tile vectors in 60 KB of LDS (sp_fisher_marginal refuses beyond) --
    1084 for P = 5, 928 for P = 6 (r, a, b, c, n and dr)."""
    return (60 * 1024 // 8 - 1152) // (int(P) + 1) - 4


class EnsembleFisher(_MarginalSweep, _FisherRegressors):
    """Expected (Fisher) information of an ENSEMBLE of light curves about the spot hyperparameters, in one device sweep
    and without any flux: how well S light curves with these cadences, periods and noise CAN constrain (r, a, b, c, n
    [, dr]) -- the design question behind the reference's calibration runs, which it answers with a sampler over a
    synthetic ensemble.  Marginal branch; per star, with C_s the covariance ``EnsembleGradient`` factors and m_s the
    mean of its flux GP (the flux mean when not normalised, else 0: sp.py:669-672),

        F_s[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1,        F = sum_s F_s

        ef = EnsembleFisher(t, ferr=1e-3, p=periods)            # cadences and star records -> GPU, once
        F = ef(r=20., a=.4, b=.27, c=.1, n=10.)                  # [5, 5]
        ef.per_star, ef.status, ef.names                         # [S, 5, 5], [S], ("r", "a", "b", "c", "n")
        cov, sigma = cramer_rao(F)                               # the Laplace / Cramer-Rao error bars

    t: (K,) or (S, K); the number of stars is t's or p's.  The tangents of the kernel tables are ``EnsembleGradient``'s
    (exact in r, a, b, c, n; central differences of step h with a spread of radii or exact=False); the device forms the
    tangents of the covariances from them, C^-1 d_i C on the matrix cores and the pair traces (sp_fisher_marginal,
    DESIGN.md 17).  max_workspace_bytes: a bound on the device scratch; the stars are then worked through in groups,
    with the same bits.

    basis, basis_var: q <= 32 linear regressors per star marginalised out, as ``EnsembleGradient(basis=...)`` takes
    them -- (K, q) or (S, K, q); scalar, (q,) or (S, q), finite and >= 0.  The star's covariance is then C + U diag(
    basis_var) U^T: F is the information that is left about the hyperparameters when the regressors' weights (segment
    offsets, trends, systematics) are nuisance parameters, and ``cramer_rao(F)`` the Laplace error bar at an optimum
    ``EnsembleGradient(basis=...)`` served (sp_fisher_marginal_linear).  ``upload_basis_var`` changes the
    variances without sending the basis again; a variance of zero switches its regressor off exactly."""

    def __init__(self, t, ferr=1.0e-3, p=1.0, u=None, ydeg=15, baseline_var=0.0, normalized=True, covpts=None,
                 tau=None, temporal_kernel="matern32", device=None, h=1.0e-4, upstream_kwargs=None, exact=True,
                 max_workspace_bytes=None, basis=None, basis_var=None):
        t = np.asarray(t, dtype=np.float64)
        if t.ndim not in (1, 2):
            raise ValueError("t must be (K,) or (S, K)")
        S = t.shape[0] if t.ndim == 2 else (np.asarray(p).shape[0] if np.ndim(p) == 1 else 1)
        regressors = _fisher_regressors(basis, basis_var, S, t.shape[-1])      # (before anything touches the device)
        stars, utab = self._setup(t, np.zeros((S, t.shape[-1])), ferr, p, None, u, ydeg, 0.0, baseline_var, tau,
                                  temporal_kernel, device)
        self._flux = None
        self._upload_regressors(*regressors)
        self._configure(covpts, normalized, h, upstream_kwargs, exact)
        self._max_ws = None if max_workspace_bytes is None else int(max_workspace_bytes)
        self._ws = None
        self.per_star = self.status = self.names = self.tangents = None

    def _workspace(self, P):
        """Scratch for P parameters: every star at once, or as many as ``max_workspace_bytes`` allows."""
        e = self._e
        if self._q:
            need = int(e._L.sp_fisher_linear_workspace_bytes(e._h, self.S, self.K, P, self._q, self._covpts))
        else:
            need = int(e._L.sp_fisher_workspace_bytes(e._h, self.S, self.K, P, self._covpts))
        nbytes = need if self._max_ws is None else min(need, self._max_ws)
        if self._ws is None or self._ws.numel() != nbytes:
            self._ws = e._scratch(nbytes)
        return self._ws

    def __call__(self, r=defaults["r"], a=defaults["a"], b=defaults["b"], c=defaults["c"], n=defaults["n"], dr=None,
                 params=("r", "a", "b", "c", "n"), return_tangents=False):
        """F [P, P] (NumPy), the sum of the stars' blocks in the order of ``params`` (names out of r, a, b, c, n and,
        with a spread of radii ``dr``, "dr").  Afterwards ``per_star`` [S, P, P], ``status`` [S] (the library's per-star
        flags: a star with z > zmax holds zeros, one whose covariance does not factor or whose light curve is ragged
        NaN) and ``names``; F adds the stars of status 0 in index order.  return_tangents: ``tangents`` [S, P, K, K],
        the d_i C the device formed."""
        import torch

        names = _check_params(params, dr is not None)
        if self._covpts > fisher_max_covpts(len(names)):        # (before anything goes to the device)
            raise ValueError("EnsembleFisher: covpts = %d is beyond the Fisher sweep's limit for %d parameters, "
                             "covpts <= %d (P + 1 tables of covpts + 4 doubles in 60 KB of LDS); name fewer ``params`` "
                             "or build the object with a smaller covpts" %
                             (self._covpts, len(names), fisher_max_covpts(len(names))))
        e = self._e
        tab, mv, point = self._at_point(r, a, b, c, n, dr)
        dy, dm, events = self._table_tangents(*point)
        with torch.cuda.stream(self._stream):
            for ev in events:
                self._stream.wait_event(ev)
            DY, DM = torch.stack([dy[k] for k in names]), torch.stack([dm[k] for k in names])
            out = e.fisher_marginal(self._t, self._stars, tab, mv, DY, DM, diag=self._diag, covpts=self._covpts,
                                    temporal=self._temporal, normalized=self._normalized,
                                    workspace=self._workspace(len(names)), return_tangents=return_tangents,
                                    **self._regressor_kwargs())
            per_star, status = out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.uint32)
            self.tangents = out[2].cpu().numpy() if return_tangents else None
        self.per_star, self.status, self.names = per_star, status, names
        return per_star[status == 0].sum(axis=0)


def ensemble_fisher(t, ferr=1.0e-3, p=1.0, r=defaults["r"], a=defaults["a"], b=defaults["b"], c=defaults["c"],
                    n=defaults["n"], dr=None, params=("r", "a", "b", "c", "n"), **kwargs):
    """One-shot form of ``EnsembleFisher``: F [P, P]."""
    params = _check_params(params, dr is not None)          # (before anything goes to the device)
    return EnsembleFisher(t, ferr=ferr, p=p, **kwargs)(r=r, a=a, b=b, c=c, n=n, dr=dr, params=params)


def cramer_rao(F):
    """(cov, sigma) of a Fisher matrix F [P, P]: cov = F^-1 from a symmetric eigendecomposition, sigma = sqrt(diag(cov)):
    the Cramer-Rao bound on the parameters' covariance, and the Laplace error bars at an optimum.  Everything NaN when
    F holds a non-finite entry or is not positive definite (an eigenvalue <= 0 to rounding: some direction of parameter space the
    data cannot constrain).  Host only."""
    F = np.asarray(F, dtype=np.float64)
    if F.ndim != 2 or F.shape[0] != F.shape[1]:
        raise ValueError("F must be a square matrix")
    P = F.shape[0]
    bad = np.full((P, P), np.nan), np.full(P, np.nan)
    if not np.all(np.isfinite(F)):
        return bad
    w, V = np.linalg.eigh(0.5 * (F + F.T))
    if not w[0] > P * np.finfo(np.float64).eps * w[-1]:          # (singular to rounding counts as singular)
        return bad
    cov = (V / w) @ V.T
    cov = 0.5 * (cov + cov.T)
    return cov, np.sqrt(np.diag(cov))


def ensemble_gradient_conditional(t, flux, ferr=1.0e-3, p=1.0, i=defaults["i"], r=defaults["r"], a=defaults["a"],
                                  b=defaults["b"], c=defaults["c"], n=defaults["n"], upstream_kwargs=None, **kwargs):
    """The CONDITIONAL branch for an ensemble (each star at its own inclination i_s; tests/test_lnlike.py:100-136 verifies
    the gradient on both branches): (sum_s lnL_s, {"r", "a", "b", "c", "n": floats, "i", "p": arrays [S]}, lnL [S]).

    The hyperparameters enter every star through the SAME (mu_y, Sigma_y), so the chain through the upstream is taken
    once: the moments' adjoints of the stars (one reverse sweep per star over the library's reverse-mode kernels,
    ``log_likelihood_with_grad``: C = A Sigma_y A^T, the design matrix's adjoint through sp_dotRx / sp_tensordotRz_rev)
    are summed, then contracted with the moments' exact tangents (``ylm_moments_device_grad``) -- one upstream
    evaluation per gradient instead of one per star and parameter.  Star by star on the host (6.5 ms each at K = 1000):
    an optimiser's aid, not a timed path; the one-sweep device form of this branch is ``EnsembleGradientConditional``
    (the marginal branch's: ``EnsembleGradient``).
    kwargs: as for ``log_likelihood_with_grad`` (u, tau, normalized, baseline_*, ydeg, ...)."""
    from .upstream_device import ylm_moments_device_grad

    flux = np.asarray(flux, dtype=np.float64)
    if flux.ndim != 2:
        raise ValueError("flux must be (S, K)")
    S, K = flux.shape
    t = np.asarray(t, dtype=np.float64)
    t = np.broadcast_to(t, (S, K)) if t.ndim == 1 else t
    per = lambda x: np.broadcast_to(np.asarray(x, dtype=np.float64), (S,))          # noqa: E731
    var = np.asarray(ferr, dtype=np.float64) ** 2
    e = get_engine(kwargs.get("ydeg", defaults["ydeg"]), kwargs.get("udeg", defaults["udeg"]), kwargs.get("device"))
    ukw = dict(upstream_kwargs or {})
    mu, Sig, dmu, dSig = [x.cpu().numpy() for x in ylm_moments_device_grad(e, r=r, a=a, b=b, c=c, n=n, **ukw)]
    gmu, gSig = np.zeros_like(mu), np.zeros_like(Sig)
    lnl, gi, gp = np.zeros(S), np.zeros(S), np.zeros(S)
    for s in range(S):
        v = var if var.ndim == 0 else (var[s] if var.ndim == 2 else var)
        lnl[s], g = log_likelihood_with_grad(mu, Sig, t[s], flux[s], v, i=float(per(i)[s]), p=float(per(p)[s]),
                                             marginalize_over_inclination=False, **kwargs)
        gmu += g["mean_ylm"]
        gSig += g["cov_ylm"]
        gi[s], gp[s] = g["i"], g["p"]
    from .upstream_device import ylm_moments_device

    eps = np.diag(_upstream_eps(mu.shape[0], ukw))
    inner = lambda m_, S_: (float(gmu @ m_), float(np.sum(gSig * (S_ - eps))))          # noqa: E731
    out = {name: float(gmu @ dmu[k] + np.sum(gSig * dSig[k])) for k, name in enumerate(("r", "a", "b"))}
    out["c"], out["n"] = _cn_chain(*inner(mu, Sig), float(c), float(n), unit=lambda: inner(
        *[x.cpu().numpy() for x in ylm_moments_device(e, r=r, a=a, b=b, c=1.0, n=1.0, **ukw)]))
    out["i"], out["p"] = gi, gp
    return float(lnl.sum()), out, lnl


# the per-star derivatives of EnsembleGradientConditional(wrt=...), in the order of the device's row (SP_STARBAR slots 0-4)
_WRT_COND = ("p", "i", "baseline_mean", "baseline_var", "log_var")


def _check_wrt_conditional(wrt, has_basis=False):
    """``wrt`` as a tuple of names the conditional sweep serves (None stays None); ValueError otherwise.  No device
    work."""
    if wrt is None:
        return None
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    for name in wrt:
        if name == "tau":
            raise ValueError("wrt: 'tau' is not differentiated on the conditional branch (the sweep applies the temporal "
                             "kernel but takes no derivative with respect to its timescale; the marginal branch does: "
                             "EnsembleGradient)")
        if name not in _WRT_COND and name != "basis_var":
            raise ValueError("wrt: unknown name %r (one of %s)" % (name, ", ".join(_WRT_COND + ("basis_var",))))
    if "basis_var" in wrt and not has_basis:
        raise ValueError("wrt: 'basis_var' needs regressors (EnsembleGradientConditional(..., basis=..., basis_var=...))")
    return wrt


class EnsembleGradientConditional(_EnsembleSweep, _RegressorVariances):
    """The CONDITIONAL branch (``marginalize_over_inclination=False``: star s at its own inclination i_s) of the ensemble
    log-likelihood and its gradient in ONE device sweep per evaluation -- what ``ensemble_gradient_conditional`` computes
    star by star through the autograd graph, for the whole batch at once (sp_lnlike_grad_conditional).

        eg = EnsembleGradientConditional(t, flux, ferr=1e-3, p=periods, i=inclinations)     # data -> GPU, once
        lnl, grad = eg(r=20., a=.4, b=.27, c=.1, n=10., wrt=("i", "p"))   # lnl: sum over stars; grad: dict
        eg.lnlike                                                         # per-star values of the last call

    The sweep returns every star's d lnL_s / d(mu_y, Sigma_y); they are summed over the stars in a fixed order and
    contracted with the moments' exact tangents (``ylm_moments_device_grad``) on the device -- c and n in closed form,
    with the rule of ``ensemble_gradient_conditional`` on the boundary c = 0 or n = 0 -- and one small transfer leaves
    the GPU per call.  One light curve per star; scalar or per-cadence ``ferr``; ``tau``: the temporal kernel
    multiplies the covariance (no derivative with respect to it on this branch).

    Linear regressors (``basis``, ``basis_var``): flux = process + U w + noise with w ~ N(0,
    diag(basis_var)), the model of ``log_likelihood_linear_ensemble`` and of ``EnsembleGradient(basis=...)``, validated
    as they validate it.  The call then returns the marginalised likelihood and ITS gradient
    (sp_lnlike_grad_conditional_linear): every name keeps its meaning, ``wrt`` also takes "basis_var" -- (S, q), the
    derivative with respect to the prior variances themselves, finite at 0 -- and ``w_mean`` (S, q) holds the posterior
    mean of the weights after a call.  ``upload_basis_var`` changes the variances without sending the basis again."""

    _WRT = _WRT_COND
    _basis = None       # (no regressors until the constructor has uploaded some)

    def __init__(self, t, flux, ferr=1.0e-3, p=1.0, i=defaults["i"], u=None, ydeg=15, baseline_var=0.0,
                 baseline_mean=0.0, normalized=True, tau=None, temporal_kernel="matern32", device=None,
                 upstream_kwargs=None, basis=None, basis_var=None):
        flux = np.asarray(flux, dtype=np.float64)
        if flux.ndim != 2:
            raise ValueError("flux must be (S, K)")
        from .linear import _regressor_args

        U, Ut, lam = _regressor_args(basis, basis_var, flux.shape[0], flux.shape[1],
                                     "a `basis` needs the prior variances of its weights, `basis_var`")
        # (the inclinations' bounds are not checked on this branch)
        self._setup(t, flux, ferr, p, i, u, ydeg, baseline_mean, baseline_var, tau, temporal_kernel, device)
        self._normalized, self._ukw = bool(normalized), dict(upstream_kwargs or {})
        self._basis = self._basis_var = self.w_mean = None
        self._q = 0
        if U is None:
            self._ws = self._e.grad_conditional_workspace(self.S, self.K)
        else:
            self._q = U.shape[2]
            self._basis = self._e.f64(Ut)
            self._basis_var = self._e.f64(lam)
            self._ws = self._e.grad_conditional_linear_workspace(self.S, self.K, self._q)
            _torch().cuda.synchronize(self._e.device)
        self.lnlike = self.status = None

    _open = staticmethod(get_engine)

    def __call__(self, r=defaults["r"], a=defaults["a"], b=defaults["b"], c=defaults["c"], n=defaults["n"], wrt=None):
        """(sum of the stars' log-likelihoods, {"r": ., "a": ., "b": ., "c": ., "n": .}).

        wrt: None, or a tuple of names out of ("i", "p", "baseline_mean", "baseline_var", "log_var"): the dict then also
        holds arrays [S], d lnL_s / d of star s's inclination (per DEGREE, as ``log_likelihood_with_grad`` returns it),
        period (the integer part of t / p is data), baseline mean, baseline variance and the log of a common factor on
        its data variances -- from the same sweep and the same transfer.  A star the likelihood rejects adds zeros.

        With regressors: the likelihood and every derivative above are those of the marginalised model; wrt may hold
        "basis_var": an array [S, q], d lnL_s / d of the prior variance of star s's regressor j.  New prior variances:
        ``upload_basis_var`` ahead of the call."""
        import torch

        from .upstream_device import ylm_moments_device, ylm_moments_device_grad

        wrt = _check_wrt_conditional(wrt, self._basis is not None)
        e = self._e
        r, a, b, c, n = float(r), float(a), float(b), float(c), float(n)
        mu, Sig, dmu, dSig = ylm_moments_device_grad(e, r=r, a=a, b=b, c=c, n=n, **self._ukw)
        e.set_moments_dev(mu, Sig)
        sweep_kw = dict(diag=self._diag, temporal=self._temporal, normalized=self._normalized, workspace=self._ws)
        tail = []
        if self._basis is None:
            lnl, mubar, sigbar, sbar, status = e.lnlike_grad_conditional(self._t, self._flux, self._stars, self._rta1,
                                                                         **sweep_kw)
        else:
            lnl, mubar, sigbar, sbar, lbar, wmean, status = e.lnlike_grad_conditional_linear(
                self._t, self._flux, self._stars, self._basis, self._basis_var, self._rta1, **sweep_kw)
            tail = [lbar.reshape(-1), wmean.reshape(-1)]
        # the stars' adjoints added up (a reduction over the leading axis: no atomics, the same order every call)
        gmu, gSig = mubar.sum(dim=0), sigbar.sum(dim=0)
        eps = _upstream_eps(mu.shape[0], self._ukw, like=mu)
        g_rab = dmu @ gmu + (dSig * gSig).sum(dim=(1, 2))
        inner = lambda m_, S_: (torch.dot(gmu, m_), (gSig * (S_ - torch.diag(eps))).sum())          # noqa: E731
        g_c, g_n = _cn_chain(*inner(mu, Sig), c, n, unit=lambda: inner(
            *ylm_moments_device(e, r=r, a=a, b=b, c=1.0, n=1.0, **self._ukw)))
        # ONE transfer: [gradient | per-star values | per-star status | per-star derivatives]
        # (with regressors, behind them: d lnL / d basis_var | the weights' posterior means)
        host = torch.cat([g_rab, torch.stack([g_c, g_n]), lnl, status.to(torch.float64), sbar.reshape(-1)] + tail).cpu().numpy()
        S = self.S
        self.lnlike = host[5:5 + S].copy()
        self.status = host[5 + S:5 + 2 * S].astype(np.uint32)
        grad = {k: float(v) for k, v in zip(("r", "a", "b", "c", "n"), host[:5])}
        if tail:
            sq = S * self._q
            self.w_mean = host[-sq:].reshape(S, self._q).copy()
            if wrt is not None and "basis_var" in wrt:
                grad["basis_var"] = host[-2 * sq:-sq].reshape(S, self._q).copy()
            host = host[:-2 * sq]
        if wrt is not None:
            sb = host[5 + 2 * S:].reshape(S, -1)
            for k in wrt:
                if k == "basis_var":
                    continue
                col = sb[:, _WRT_COND.index(k)]
                grad[k] = col * (np.pi / 180.0) if k == "i" else col.copy()
        return float(self.lnlike.sum()), grad


def ensemble_gradient_conditional_device(t, flux, ferr=1.0e-3, p=1.0, i=defaults["i"], r=defaults["r"], a=defaults["a"],
                                         b=defaults["b"], c=defaults["c"], n=defaults["n"], wrt=("i", "p"), **kwargs):
    """One-shot form of ``EnsembleGradientConditional`` with the return of ``ensemble_gradient_conditional``:
    (sum_s lnL_s, {"r", "a", "b", "c", "n": floats, and the names of ``wrt``: arrays [S]}, lnL [S]).  ``basis``,
    ``basis_var`` among the keywords: the regressors of the marginalised model, and "basis_var" a name of ``wrt``."""
    wrt = _check_wrt_conditional(wrt, kwargs.get("basis") is not None)          # (before any data goes to the device)
    eg = EnsembleGradientConditional(t, flux, ferr=ferr, p=p, i=i, **kwargs)
    total, grad = eg(r=r, a=a, b=b, c=c, n=n, wrt=wrt)
    return total, grad, eg.lnlike


# what the conditional branch's Fisher information may be taken about: the shared hyperparameters (the moments' exact
# tangents have no spread of radii) and each star's own parameters
_FISHER_COND_PARAMS = ("r", "a", "b", "c", "n")
_FISHER_STAR_PARAMS = ("i", "p")


def _check_conditional_params(params, star_params):
    """(params, star_params) as tuples of distinct names out of (r, a, b, c, n) and (i, p); ValueError otherwise, and
    when both are empty.  No device work."""
    out = []
    for what, given, known in (("params", params, _FISHER_COND_PARAMS), ("star_params", star_params, _FISHER_STAR_PARAMS)):
        given = (given,) if isinstance(given, str) else tuple(given)
        for k, name in enumerate(given):
            if name not in known:
                raise ValueError("%s: unknown name %r (one of %s)" % (what, name, ", ".join(known)))
            if name in given[:k]:
                raise ValueError("%s: %r is named twice" % (what, name))
        out.append(given)
    if not out[0] and not out[1]:
        raise ValueError("params and star_params: at least one name between them")
    return out[0], out[1]


def _moment_tangents(e, ukw, names, r, a, b, c, n):
    """The engine's moments set at the point; (mu, Sig, dmu [Ph, N], dSig [Ph, N, N]) on the device, the tangents in the
    order of ``names`` (None, None without any): r, a, b from the quadrature's exact tangents, c and n in closed form --
    mu_y = c n m, Sigma_y - eps = c^2 n S (contrast.py:21-33) -- with the unit-contrast evaluation on the boundary c = 0 or
    n = 0 (``_cn_chain``).  A name's tangent does not depend on which other names are asked for."""
    import torch

    from .upstream_device import ylm_moments_device, ylm_moments_device_grad

    mu, Sig, dmu, dSig = ylm_moments_device_grad(e, r=r, a=a, b=b, c=c, n=n, **ukw)
    e.set_moments_dev(mu, Sig)
    if not names:
        return mu, Sig, None, None
    tang = {name: (dmu[k], dSig[k]) for k, name in enumerate(("r", "a", "b"))}
    if "c" in names or "n" in names:
        eps = torch.diag(_upstream_eps(mu.shape[0], ukw, like=mu))
        if c != 0 and n != 0:
            tang["c"] = (mu / c, 2.0 * (Sig - eps) / c)
            tang["n"] = (mu / n, (Sig - eps) / n)
        else:
            mu1, Sig1 = ylm_moments_device(e, r=r, a=a, b=b, c=1.0, n=1.0, **ukw)
            S1 = Sig1 - eps
            tang["c"] = (n * mu1, 2.0 * c * n * S1)
            tang["n"] = (c * mu1, c * c * S1)
    return mu, Sig, torch.stack([tang[k][0] for k in names]), torch.stack([tang[k][1] for k in names])


class EnsembleFisherConditional(_EnsembleSweep, _FisherRegressors):
    """Expected (Fisher) information of an ENSEMBLE of light curves on the CONDITIONAL branch (star s at its own
    inclination i_s), in one device sweep and without any flux: how well these cadences, periods and noise CAN constrain
    the shared spot hyperparameters (r, a, b, c, n) AND every star's own inclination and period.  Per star, with C_s the
    covariance ``EnsembleGradientConditional`` factors and m_s the mean of its flux GP (the flux mean when not normalised,
    else 0),

        F_s[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1

    over the star's parameters: ``params``, then ``star_params``.

        ef = EnsembleFisherConditional(t, ferr=1e-3, p=periods, i=inclinations)     # cadences, star records -> GPU, once
        F_shared = ef(r=20., a=.4, b=.27, c=.1, n=10.)          # [5, 5]: the information at KNOWN inclinations and periods
        ef.per_star, ef.status, ef.names, ef.star_names          # [S, 7, 7], [S], ("r", ..., "n"), ("i", "p")
        cr = cramer_rao_ensemble(ef.per_star, 5, ef.status)      # bounds with the other block marginalised

    t: (K,) or (S, K); the number of stars is t's, p's or i's.  The moments' tangents are ``ylm_moments_device_grad``'s for
    r, a, b and closed forms for c and n; the device forms the design matrices' tangents with respect to i and p, the
    tangents of the covariances, C^-1 d_i C on the matrix cores and the pair traces (sp_fisher_conditional, DESIGN.md
    18).  Inclinations in degrees: the rows and columns of "i" are per degree.  max_workspace_bytes: a bound on the device
    scratch; the stars are then worked through in groups, with the same bits.

    basis, basis_var: q <= 32 linear regressors per star marginalised out, as ``EnsembleFisher(basis=...)`` takes them:
    the information with the regressors' weights as nuisance parameters, the error bar at an optimum of
    ``EnsembleGradientConditional(basis=...)`` (sp_fisher_conditional_linear); ``upload_basis_var`` changes
    the variances without sending the basis again."""

    _open = staticmethod(get_engine)

    def __init__(self, t, ferr=1.0e-3, p=1.0, i=defaults["i"], u=None, ydeg=15, baseline_var=0.0, normalized=True,
                 tau=None, temporal_kernel="matern32", device=None, upstream_kwargs=None, max_workspace_bytes=None,
                 basis=None, basis_var=None):
        t = np.asarray(t, dtype=np.float64)
        if t.ndim not in (1, 2):
            raise ValueError("t must be (K,) or (S, K)")
        S = t.shape[0] if t.ndim == 2 else max([np.asarray(x).shape[0] for x in (p, i) if np.ndim(x) == 1] or [1])
        regressors = _fisher_regressors(basis, basis_var, S, t.shape[-1])      # (before anything touches the device)
        # (the inclinations' bounds are not checked on this branch)
        self._setup(t, np.zeros((S, t.shape[-1])), ferr, p, i, u, ydeg, 0.0, baseline_var, tau, temporal_kernel, device)
        self._flux = None
        self._upload_regressors(*regressors)
        self._normalized, self._ukw = bool(normalized), dict(upstream_kwargs or {})
        self._max_ws = None if max_workspace_bytes is None else int(max_workspace_bytes)
        self._ws = None
        self.per_star = self.status = self.names = self.star_names = self.tangents = None

    def _workspace(self, P):
        """Scratch for P parameters: every star at once, or as many as ``max_workspace_bytes`` allows."""
        e = self._e
        if self._q:
            need = int(e._L.sp_fisher_conditional_linear_workspace_bytes(e._h, self.S, self.K, P, self._q))
        else:
            need = int(e._L.sp_fisher_conditional_workspace_bytes(e._h, self.S, self.K, P))
        nbytes = need if self._max_ws is None else min(need, self._max_ws)
        if self._ws is None or self._ws.numel() != nbytes:
            self._ws = e._scratch(nbytes)
        return self._ws

    def _moment_tangents(self, names, r, a, b, c, n):
        """The engine's moments set at the point; (dmu [Ph, N], dSig [Ph, N, N]) in the order of ``names``."""
        return _moment_tangents(self._e, self._ukw, names, r, a, b, c, n)[2:]

    def __call__(self, r=defaults["r"], a=defaults["a"], b=defaults["b"], c=defaults["c"], n=defaults["n"],
                 params=("r", "a", "b", "c", "n"), star_params=("i", "p"), return_tangents=False):
        """F_shared [P_h, P_h] (NumPy): the sum over the stars of the hyperparameter blocks, in the order of ``params`` --
        the information about them at KNOWN inclinations and periods.  Afterwards ``per_star`` [S, P, P] over ``params``
        + ``star_params`` (names out of r, a, b, c, n; out of i, p -- "i" per degree), ``status`` [S] (the library's
        per-star flags: a star with z > zmax holds zeros, one whose covariance does not factor or whose light curve is
        ragged NaN), ``names`` and ``star_names``; F_shared adds the stars of status 0 in index order.  return_tangents:
        ``tangents`` [S, P, K, K], the d_i C the device formed."""
        names, star_names = _check_conditional_params(params, star_params)
        e = self._e
        r, a, b, c, n = float(r), float(a), float(b), float(c), float(n)
        dmu, dSig = self._moment_tangents(names, r, a, b, c, n)
        Ph, P = len(names), len(names) + len(star_names)
        out = e.fisher_conditional(self._t, self._stars, self._rta1, dmu, dSig, star_params=star_names, diag=self._diag,
                                   temporal=self._temporal, normalized=self._normalized, workspace=self._workspace(P),
                                   return_tangents=return_tangents, **self._regressor_kwargs())
        per_star, status = out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.uint32)
        # the device's order (hyperparameters, i, p) -> params + star_params; "i" per degree
        device_order = list(names) + [k for k in _FISHER_STAR_PARAMS if k in star_names]
        perm = [device_order.index(k) for k in names + star_names]
        scale = np.array([np.pi / 180.0 if k == "i" else 1.0 for k in names + star_names])
        per_star = per_star[:, perm][:, :, perm] * scale[:, None] * scale[None, :]
        self.tangents = None
        if return_tangents:
            self.tangents = out[2].cpu().numpy()[:, perm] * scale[None, :, None, None]
        self.per_star, self.status, self.names, self.star_names = per_star, status, names, star_names
        return per_star[status == 0][:, :Ph, :Ph].sum(axis=0)


def ensemble_fisher_conditional(t, ferr=1.0e-3, p=1.0, i=defaults["i"], r=defaults["r"], a=defaults["a"],
                                b=defaults["b"], c=defaults["c"], n=defaults["n"], params=("r", "a", "b", "c", "n"),
                                star_params=("i", "p"), **kwargs):
    """One-shot form of ``EnsembleFisherConditional``: (F_shared [P_h, P_h], per_star [S, P, P], status [S])."""
    params, star_params = _check_conditional_params(params, star_params)          # (before anything goes to the device)
    ef = EnsembleFisherConditional(t, ferr=ferr, p=p, i=i, **kwargs)
    F = ef(r=r, a=a, b=b, c=c, n=n, params=params, star_params=star_params)
    return F, ef.per_star, ef.status


def cramer_rao_ensemble(per_star, n_shared, status=None):
    """Cramer-Rao bounds of an ensemble whose stars share ``n_shared`` hyperparameters and have parameters of their own:
    per_star [S, P, P] the stars' Fisher blocks (``EnsembleFisherConditional.per_star``), rows and columns ordered
    hyperparameters (h) first, then the star's own (*).  The joint Fisher matrix is an ARROW: shared block sum_s F_s[h, h],
    star blocks F_s[*, *], cross blocks F_s[h, *]; it is never formed.  Returns a dict:

      cov_shared [P_h, P_h], sigma_shared [P_h]   the bound on the hyperparameters with every star's own parameters
                                                  marginalised: the inverse of the Schur complement
                                                  sum_s (F_hh - F_h* F_**^-1 F_*h)_s
      sigma_star [S, P_star]                      each star's own parameters with the hyperparameters marginalised:
                                                  F_**^-1 + F_**^-1 F_*h cov_shared F_h* F_**^-1
      sigma_star_known [S, P_star]                the same with the hyperparameters known: F_**^-1

    status [S] (or None): the stars with a nonzero entry are left out of the sums and hold NaN.  NaN as in
    ``cramer_rao``: a singular or non-finite block makes what depends on it NaN (a star block: the shared bound and every
    star's marginalised bound; the shared Schur complement -- the full set (r, a, b, c, n) of a normalised process, DESIGN.md
    17 --: the shared bound and the marginalised star bounds, not the known-hyperparameter ones).  Host only."""
    F = np.asarray(per_star, dtype=np.float64)
    if F.ndim != 3 or F.shape[1] != F.shape[2]:
        raise ValueError("per_star must be [S, P, P]")
    S, P = F.shape[0], F.shape[1]
    Ph = int(n_shared)
    if not 0 <= Ph <= P:
        raise ValueError("n_shared must lie in 0 .. P")
    Ps = P - Ph
    ok = np.ones(S, dtype=bool) if status is None else np.asarray(status).reshape(S) == 0
    schur = np.zeros((Ph, Ph))
    cov_ss = np.full((S, Ps, Ps), np.nan)
    known = np.full((S, Ps), np.nan)
    for s in np.flatnonzero(ok):
        Fhh, Fhs, Fss = F[s, :Ph, :Ph], F[s, :Ph, Ph:], F[s, Ph:, Ph:]
        if Ps:
            cov_ss[s], known[s] = cramer_rao(Fss)
            with np.errstate(invalid="ignore"):          # (a singular star block: NaN goes on)
                schur = schur + (Fhh - Fhs @ cov_ss[s] @ Fhs.T)
        else:
            schur = schur + Fhh
    if Ph:
        cov_shared, sigma_shared = cramer_rao(schur)
    else:
        cov_shared, sigma_shared = np.zeros((0, 0)), np.zeros(0)
    sigma_star = np.full((S, Ps), np.nan)
    for s in np.flatnonzero(ok):
        if not Ps:
            continue
        with np.errstate(invalid="ignore"):
            X = cov_ss[s] @ F[s, :Ph, Ph:].T              # F_**^-1 F_*h
            sigma_star[s] = np.sqrt(np.diag(cov_ss[s] + X @ cov_shared @ X.T))
    return dict(cov_shared=cov_shared, sigma_shared=sigma_shared, sigma_star=sigma_star, sigma_star_known=known)


# the largest degree the inclination grid's kernels serve (2 ydeg + 1 <= 61 rows, one per lane of a wavefront)
_INCL_GRAD_MAX_YDEG = 30


def _or_flags(status):
    """Bitwise or of the library's per-star flags over the last axis of a device tensor."""
    out = 0
    for bit in (1, 2, 4, 8, 16):
        out = out + ((status & bit) != 0).any(dim=-1).to(status.dtype) * bit
    return out


# the per-star derivatives of EnsembleGradientInclinations(wrt=...), in the order of the device's row (slots 0-3 of
# sp_lnlike_inclinations_grad_stars) and of ``star_grad``
_WRT_INCL = ("p", "baseline_mean", "baseline_var", "log_var")


def _check_wrt_inclinations(wrt):
    """``wrt`` as a tuple of names the inclination grid serves (None stays None); ValueError otherwise.  No device
    work."""
    if wrt is None:
        return None
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    for name in wrt:
        if name == "i":
            raise ValueError("wrt: 'i' is marginalised on the grid (its posterior is ``pinc``); "
                             "EnsembleGradientConditional differentiates at known inclinations")
        if name == "tau":
            raise ValueError("wrt: 'tau': a time-variable process has no rank-(2 ydeg + 1) basis (EnsembleGradient "
                             "differentiates the marginal branch with respect to it)")
        if name not in _WRT_INCL:
            raise ValueError("wrt: unknown name %r (one of %s)" % (name, ", ".join(_WRT_INCL)))
    return wrt


class EnsembleGradientInclinations(_EnsembleSweep):
    """The ensemble log-likelihood with every star's inclination marginalised EXACTLY on a grid, and its gradient:

        lnL_s = log sum_j w_j exp(lnL_s(i_j)),      lnL_s(i_j) the conditional branch at grid inclination i_j

    with w_j the prior weights ``StarryProcess._inc_prior_weights(inc, inc_weights)`` (sin i di by default) -- the
    quantity the marginal branch (``EnsembleGradient``) approximates to second moments and ``ylm_conditional_marginal``
    uses as ``pinc``.  The grid runs through the rank-(2 ydeg + 1) Fourier basis (sp_lnlike_inclinations_grad, DESIGN.md
    22): no K x K matrix, cost linear in K.

        eg = EnsembleGradientInclinations(t, flux, ferr=1e-3, p=periods, inc=np.linspace(0, 90, 100))   # data -> GPU, once
        lnl, grad = eg(r=20., a=.4, b=.27, c=.1, n=10., params=("r", "a", "b", "c", "n"))
        eg.lnlike (S,), eg.per_star (S, Pd), eg.pinc (S, P), eg.lnlike_grid (S, P), eg.status (S,), eg.names
        lnl, grad = eg(r=20., a=.4, b=.27, c=.1, n=10., wrt=("p", "baseline_mean", "baseline_var", "log_var"))
        grad["p"] (S,), ..., eg.star_grad (S, 4)       # d lnL_s / d of star s's own period, baselines, noise factor

    t: (K,) or (S, K); flux (S, K); ferr: a scalar, (S,) or (S, K); p, baseline_mean, baseline_var: scalars or (S,); u:
    (udeg,) or (S, udeg); inc in degrees.  The constructor uploads the data and plans it once (sp_incl_plan_data, and
    the plan's tangent along each star's period, sp_incl_plan_tangent).  A
    star the basis cannot take (SP_STAR_NO_BASIS in ``status``: partial phase coverage, fewer distinct phases than
    2 ydeg + 1, a variance <= 0) goes through the dense conditional sweep instead, replicated over the grid
    inclinations, and enters the same mixture.  ydeg <= 30.

    Not served: a time-variable process (``tau``), a full ``data_cov`` matrix or a matrix ``baseline_var`` (refused here;
    ``EnsembleGradientConditional`` takes ``tau`` at known inclinations); derivatives with respect to the spread of radii
    dr or to a star's limb darkening; more than one light curve per star; a multi-stream form."""

    _open = staticmethod(get_engine)

    def __init__(self, t, flux, ferr=1.0e-3, p=1.0, inc=np.linspace(0, 90, 100), inc_weights=None, u=None, ydeg=15,
                 baseline_mean=0.0, baseline_var=0.0, normalized=True, tau=None, data_cov=None, device=None,
                 upstream_kwargs=None):
        from .sp import StarryProcess

        flux = np.asarray(flux, dtype=np.float64)
        if flux.ndim != 2:
            raise ValueError("flux must be (S, K)")
        if tau:
            raise NotImplementedError("a time-variable process (tau) has no rank-(2 ydeg + 1) basis: use "
                                      "EnsembleGradientConditional at known inclinations")
        if data_cov is not None:
            raise NotImplementedError("data_cov: the inclination grid takes per-cadence variances only, through ferr "
                                      "(scalar, (S,) or (S, K)); a full covariance matrix needs the dense route, "
                                      "EnsembleGradientConditional")
        if np.ndim(baseline_var) > 1:
            raise NotImplementedError("a matrix baseline_var needs the dense route, EnsembleGradientConditional")
        if int(ydeg) > _INCL_GRAD_MAX_YDEG:
            raise ValueError("ydeg = %d: the inclination grid serves ydeg <= %d" % (int(ydeg), _INCL_GRAD_MAX_YDEG))
        inc = np.atleast_1d(np.asarray(inc, dtype=np.float64)).reshape(-1)
        check_period_inclination(None, inc)
        if inc.size < 1:
            raise ValueError("at least one inclination")
        self._inc = inc
        self._logw = StarryProcess._log_weights(StarryProcess._inc_prior_weights(inc, inc_weights))
        stars, _ = self._setup(t, flux, ferr, p, defaults["i"], u, ydeg, baseline_mean, baseline_var, None, "matern32",
                               device)
        e = self._e
        self._normalized, self._ukw = bool(normalized), dict(upstream_kwargs or {})
        self._inc_rad, self._logw_dev = e.f64(inc * (np.pi / 180)), e.f64(self._logw)
        self._plan, pstat = e.incl_plan_data(self._t, self._flux, self._stars, self._diag)
        self._ptan = e.incl_plan_tangent(self._t, self._flux, self._stars, self._plan, self._diag)
        self._dense = np.flatnonzero(pstat.cpu().numpy().astype(np.uint32) & SP_STAR_NO_BASIS)
        # a star of the dense route: its record once per grid inclination
        self._dense_stars = []
        for s in self._dense:
            rep = np.repeat(stars[s:s + 1], inc.size)
            rep["inc"] = inc * (np.pi / 180)
            self._dense_stars.append(e.stars_to_device(rep))
        self.lnlike = self.per_star = self.pinc = self.lnlike_grid = self.status = self.names = self.star_grad = None

    def _dense_star(self, k, dmu, dSig, star=False):
        """(lnlike_grid [P], lnmix, dlnmix [Pd], pinc [P], status) of the k-th star of the dense route, on the device:
        the conditional sweep at the engine's moments on the star replicated over the grid, then the same mixture.
        star: a sixth entry, the sweep's per-star row (p, i, baseline_mean, baseline_var, log_var) mixed with pinc, the
        inclination's slot dropped: [4] in the order of ``_WRT_INCL``."""
        import torch

        e, s, P = self._e, int(self._dense[k]), self._inc.size
        rows = lambda x: None if x is None else x[s:s + 1].expand(P, -1).contiguous()          # noqa: E731
        lnl, mubar, sigbar, sbar, status = e.lnlike_grad_conditional(
            rows(self._t), rows(self._flux), self._dense_stars[k], self._rta1, diag=rows(self._diag),
            temporal=self._temporal, normalized=self._normalized)
        ninf = torch.full_like(lnl, -np.inf)
        lnl = torch.where(torch.isnan(lnl), ninf, lnl)
        a = self._logw_dev + lnl
        live = a > -np.inf
        if not bool(live.any()):
            zero = torch.zeros_like(lnl)
            out = (lnl, ninf[0], torch.zeros(dmu.shape[0], dtype=lnl.dtype, device=lnl.device), zero, status)
            return out + (torch.zeros(4, dtype=lnl.dtype, device=lnl.device),) if star else out
        lnmix = torch.logsumexp(a, dim=0)
        pinc = torch.where(live, torch.exp(a - lnmix), torch.zeros_like(a))
        z1, z2 = torch.zeros_like(mubar), torch.zeros_like(sigbar)
        gmu = (pinc[:, None] * torch.where(live[:, None], mubar, z1)).sum(dim=0)
        gSig = (pinc[:, None, None] * torch.where(live[:, None, None], sigbar, z2)).sum(dim=0)
        out = (lnl, lnmix, dmu @ gmu + (dSig * gSig).sum(dim=(1, 2)), pinc, status)
        if star:
            sb = sbar[:, [0, 2, 3, 4]]
            out += ((pinc[:, None] * torch.where(live[:, None], sb, torch.zeros_like(sb))).sum(dim=0),)
        return out

    def __call__(self, r=defaults["r"], a=defaults["a"], b=defaults["b"], c=defaults["c"], n=defaults["n"],
                 params=("r", "a", "b", "c", "n"), wrt=None):
        """(sum over the stars of finite value of lnL_s, in index order; {name: d / d name} over ``params``, any subset
        of r, a, b, c, n -- a sub-block has the bits of the matching columns of the full call).  Afterwards ``lnlike``
        [S], ``per_star`` [S, Pd] (d lnL_s / d params), ``pinc`` [S, P] (each star's inclination posterior on the grid),
        ``lnlike_grid`` [S, P], ``status`` [S] (the flags of the star's grid points or-ed; SP_STAR_NO_BASIS: the star took
        the dense route) and ``names``.

        wrt: None, a name or a tuple of names out of ("p", "baseline_mean", "baseline_var", "log_var"): the dict then also
        holds arrays [S], d lnL_s / d of star s's own period (the integer part of t / p is data), baseline mean, baseline
        variance and the log of a common factor on its data variances (not on baseline_var) -- the mixture over the grid
        of the conditional derivatives, sum_j pinc_sj d lnL_s(i_j) / d theta_s, from the same sweep and the same transfer.
        ``star_grad`` [S, 4] then holds them in that fixed order, NaN in a slot that was not asked for (None after a call
        without ``wrt``).  A grid entry at -inf contributes zero; a star whose whole grid is -inf gets zeros."""
        import torch

        names, _ = _check_conditional_params(params, ())
        wrt = _check_wrt_inclinations(wrt)
        mask = 0
        for k in wrt or ():
            mask |= 1 << _WRT_INCL.index(k)
        e = self._e
        r, a, b, c, n = float(r), float(a), float(b), float(c), float(n)
        mu, Sig, dmu, dSig = _moment_tangents(e, self._ukw, names, r, a, b, c, n)
        S, P, Pd = self.S, self._inc.size, len(names)
        grid, _, lnmix, dlnmix, pinc, status, *star = e.lnlike_inclinations_grad(
            self._plan, self._stars, self._rta1, mu, Sig, dmu, dSig, self._inc_rad, logw=self._logw_dev,
            normalized=self._normalized, star_tangent=self._ptan if mask & 1 else None, star_mask=mask)
        stat = _or_flags(status)
        for k, s in enumerate(self._dense):
            grid[s], lnmix[s], dlnmix[s], pinc[s], st, *sb = self._dense_star(k, dmu, dSig, star=bool(mask))
            stat[s] = _or_flags(st) | SP_STAR_NO_BASIS
            if mask:
                asked = torch.tensor([bool(mask >> q & 1) for q in range(4)], device=sb[0].device)
                star[1][s] = torch.where(asked, sb[0], torch.full_like(sb[0], np.nan))
        # ONE transfer: [per-star values | per-star gradients | grid | posteriors | status | per-star derivatives]
        host = torch.cat([lnmix, dlnmix.reshape(-1), grid.reshape(-1), pinc.reshape(-1),
                          stat.to(torch.float64)] + ([star[1].reshape(-1)] if mask else [])).cpu().numpy()
        o = np.cumsum([0, S, S * Pd, S * P, S * P, S, 4 * S if mask else 0])
        self.lnlike, self.per_star = host[o[0]:o[1]].copy(), host[o[1]:o[2]].reshape(S, Pd).copy()
        self.lnlike_grid, self.pinc = host[o[2]:o[3]].reshape(S, P).copy(), host[o[3]:o[4]].reshape(S, P).copy()
        self.status, self.names = host[o[4]:o[5]].astype(np.uint32), names
        self.star_grad = host[o[5]:o[6]].reshape(S, 4).copy() if mask else None
        total, g = 0.0, np.zeros(Pd)
        for s in range(S):          # (index order)
            if np.isfinite(self.lnlike[s]):
                total += self.lnlike[s]
                g += self.per_star[s]
        grad = {k: float(v) for k, v in zip(names, g)}
        for k in wrt or ():
            grad[k] = self.star_grad[:, _WRT_INCL.index(k)].copy()
        return float(total), grad


def ensemble_gradient_inclinations(t, flux, ferr=1.0e-3, p=1.0, inc=np.linspace(0, 90, 100), r=defaults["r"],
                                   a=defaults["a"], b=defaults["b"], c=defaults["c"], n=defaults["n"],
                                   params=("r", "a", "b", "c", "n"), wrt=None, **kwargs):
    """One-shot form of ``EnsembleGradientInclinations``: (sum_s lnL_s, {name: float, and the names of ``wrt``: arrays
    [S]}, lnL [S])."""
    _check_conditional_params(params, ())          # (before anything goes to the device)
    wrt = _check_wrt_inclinations(wrt)
    eg = EnsembleGradientInclinations(t, flux, ferr=ferr, p=p, inc=inc, **kwargs)
    total, grad = eg(r=r, a=a, b=b, c=c, n=n, params=params, wrt=wrt)
    return total, grad, eg.lnlike
