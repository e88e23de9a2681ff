"""
``StarryProcess``: source-compatible front end of the reference class
(reference ``sp.py:38-1396``) restricted to the log-likelihood hot path:

    sp = StarryProcess(r=..., a=..., b=..., c=..., n=..., ydeg=15, ...)
    sp.mean(t, i, p, u); sp.cov(t, i, p, u)
    sp.log_likelihood(t, flux, data_cov, i, p, u, baseline_mean, baseline_var)

Keyword names, defaults, argument meaning and error behaviour follow the
reference (``sp.py:39-51, 643-703, 1052-1188``).  Results are eager NumPy values
with a no-op ``.eval()`` so scripts written for the lazy Theano graph run
unchanged.  Every number on the path mean / cov / log_likelihood is produced on
the GPU by ``libsp_hip.so``.

The Ylm moments (mu_y, Sigma_y) come from the hyperparameters through the host
module ``upstream`` (reference sp.py:257-266); they can also be injected with
``mean_ylm= / cov_ylm=`` (what the tests and ``bench.py`` do with the golden
moments).

Addition over the reference: ``log_likelihood_ensemble`` evaluates many stars,
each with its own period / inclination / limb darkening / noise, in one batched
device call -- the calibrate-style use case the reference describes but leaves
unimplemented (joss/paper.md:160-172).
"""
import numpy as np

from .defaults import defaults
from .engine import block_edges, get_engine
from .flux import FluxIntegral
from .linear import _regressor_args
from .ops import AlphaBetaOp, CheckBoundsOp, Eager, _is_torch
from .pixel import latlon_to_xyz, mollweide_grid
from .stars import SampleColumns, check_period_inclination, ensemble_stars, ipt_in_bounds, make_stars  # noqa: F401
from .temporal import kernel_id

__all__ = ["StarryProcess", "StarryProcessSum"]


def _neg_inf_if_nan(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), -np.inf, x)


def _one_star_regressors(basis, basis_var, required=False):
    """``basis`` (K, q) and ``basis_var`` scalar or (q,) of one light curve as the ensemble calls take them ((1, K, q),
    the variances as given); None stays None unless the basis is ``required``.  ValueError for another shape."""
    if basis is None and not required:
        return None, basis_var
    U = np.asarray(basis, dtype=np.float64)
    if U.ndim != 2:
        raise ValueError("`basis` must be (K, q)")
    if basis_var is not None and np.ndim(basis_var) > 1:
        raise ValueError("`basis_var` must be a scalar or (q,)")
    return U[None], basis_var


# how log_likelihood_linear and its ensemble form end their refusal of a matrix `baseline_var`
_BASIS_HINT = ", and the structured part as `basis`, `basis_var`"


def _dense_ensemble_input(name, t, flux, data_cov, baseline_var, baseline_hint=""):
    """(t, flux (S, K), data_cov, S, K) in float64 for the ensemble method ``name``, or the refusals of what the model
    checks do not serve, in this order: ragged input, a flux that is not (S, K), a full-matrix ``data_cov`` ((K, K)
    with S = K is (S, K) variances) and a matrix ``baseline_var`` (``baseline_hint`` ends that message)."""
    try:
        flux = np.asarray(flux, dtype=np.float64)
        tt = np.asarray(t, dtype=np.float64)
    except (ValueError, TypeError):
        raise ValueError("%s does not serve ragged input (lists of light curves of different lengths): "
                         "pass `t` and `flux` as (S, K) arrays" % name)
    if flux.ndim != 2:
        raise ValueError("`flux` must be (S, K)")
    S, K = flux.shape
    dc = np.asarray(data_cov, dtype=np.float64)
    if dc.ndim > 2 or (dc.ndim == 2 and dc.shape == (K, K) and S != K):
        raise NotImplementedError("%s does not serve a full-matrix `data_cov`: pass a scalar, (S,) or "
                                  "(S, K) variances" % name)
    if np.ndim(baseline_var) >= 2:
        raise NotImplementedError("%s does not serve a matrix `baseline_var`: pass a scalar or (S,)%s"
                                  % (name, baseline_hint))
    return tt, flux, dc, S, K


def _one_curve(name, flux, data_cov, baseline_var, baseline_hint=""):
    """(flux (1, K), data_cov a scalar or (1, K)) of the one-light-curve method ``name`` as its ensemble form takes
    them, or its refusals: a full-matrix ``data_cov``, a ``baseline_var`` that is no scalar, a flux that is no row."""
    dc = np.asarray(data_cov, dtype=np.float64)
    if dc.ndim >= 2:
        raise NotImplementedError("%s does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances" % name)
    if np.ndim(baseline_var) >= 1:
        raise NotImplementedError("%s does not serve a matrix `baseline_var`: pass a scalar%s" % (name, baseline_hint))
    try:
        flux = np.asarray(flux, dtype=np.float64).reshape(1, -1)
    except (ValueError, TypeError):
        raise ValueError("`flux` must be one light curve of K cadences")
    return flux, (dc.reshape(1, -1) if dc.ndim == 1 else dc)


def _star_fallback_args(s_, t, flux, stars, utab, diag):
    """Star ``s_`` of an ensemble as the one-star dense routes take it: (t, flux, data_cov, period, u, baseline_mean,
    baseline_var)."""
    return (t[s_], flux[s_], diag[s_] if diag is not None else stars["data_var"][s_], stars["period"][s_],
            utab[stars["table"][s_]], stars["baseline_mean"][s_], stars["baseline_var"][s_])


def _one_star_noise(n, K, data_cov, **star_kw):
    """(stars, diag) of n records with one light curve's noise: a scalar ``data_cov`` in the records, a vector as the
    per-cadence variances diag (n, K)."""
    stars = make_stars(n, data_var=float(data_cov) if data_cov.ndim == 0 else 0.0, **star_kw)
    return stars, (None if data_cov.ndim == 0 else np.broadcast_to(data_cov, (n, K)))


def _linear_extras(Ud, wmean, lnlike0):
    """What a result with regressors adds: ``lnlike0``, ``w_mean`` and ``trend`` = U w_mean, formed on the device (a
    weight switched off contributes an exact zero)."""
    trend = (Ud * wmean[:, :, None]).sum(dim=1)
    return {"lnlike0": _neg_inf_if_nan(lnlike0.cpu().numpy()), "w_mean": wmean.cpu().numpy(),
            "trend": trend.cpu().numpy()}


def _affine_samples(e, mu, L, z):
    """mu_s + L_s z_s of S stars on the device: mu [S, n], L [S, n, n] contiguous, the host deviates z (S, n, ns)
    -> [S, ns, n]."""
    S, n, ns = z.shape
    zt = e.f64(np.ascontiguousarray(np.swapaxes(z, 1, 2)))
    smp = e.empty(S, ns, n)
    e.gemm_nt_batched(zt, L, smp)                             # (L_s z_s)^T
    smp += mu[:, None, :]
    return smp


def sample_columns(params, marginalize_over_inclination, time_variable):
    """``stars.SampleColumns.from_params`` as a tuple: (params, the same names in the batch's order, whether dr is a
    column, the free terms in that order)."""
    cols = SampleColumns.from_params(params, marginalize_over_inclination, time_variable)
    return cols.params, cols.names, cols.dr_free, cols.free


class StarryProcess(object):
    def __init__(
        self,
        r=defaults["r"],
        dr=defaults["dr"],
        c=defaults["c"],
        n=defaults["n"],
        tau=defaults["tau"],
        temporal_kernel=defaults["temporal_kernel"],
        marginalize_over_inclination=defaults["marginalize_over_inclination"],
        normalized=defaults["normalized"],
        covpts=defaults["covpts"],
        **kwargs
    ):
        mu = kwargs.pop("mu", None)
        sigma = kwargs.pop("sigma", None)
        mean_ylm = kwargs.pop("mean_ylm", None)
        cov_ylm = kwargs.pop("cov_ylm", None)
        if mu is None and sigma is None:
            a = kwargs.pop("a", defaults["a"])
            b = kwargs.pop("b", defaults["b"])
        elif (kwargs.get("a", None) is None and kwargs.get("b", None) is None) and (
            mu is not None and sigma is not None
        ):
            from .upstream import gauss2beta

            a, b = gauss2beta(mu, sigma)
        else:
            raise ValueError("Must provide either `a` and `b` *or* `mu` and `sigma`.")

        if tau is None:
            self._tau = 0.0
            self._time_variable = False
            self._temporal = None
        else:
            self._tau = float(CheckBoundsOp(name="tau", lower=0, upper=np.inf)(tau))
            self._time_variable = True
            self._temporal = kernel_id(temporal_kernel)

        self._ydeg = int(kwargs.get("ydeg", defaults["ydeg"]))
        assert self._ydeg >= 5, "Degree of map must be >= 5."
        self._udeg = int(kwargs.get("udeg", defaults["udeg"]))
        assert self._udeg >= 0, "Degree of limb darkening must be >= 0."
        self._nylm = (self._ydeg + 1) ** 2
        self._covpts = int(covpts)
        self._kwargs = kwargs
        self._normalized = bool(normalized)
        self._normN = int(kwargs.get("normalization_order", defaults["normalization_order"]))
        self._normzmax = float(kwargs.get("normalization_zmax", defaults["normalization_zmax"]))
        self._get_alpha_beta = AlphaBetaOp(self._normN)
        self._marginalize_over_inclination = bool(marginalize_over_inclination)
        self._r, self._dr, self._a, self._b, self._c, self._n = r, dr, a, b, c, n

        self._engine = get_engine(self._ydeg, self._udeg, kwargs.get("device"))
        dev_moments = None
        from_hyper = mean_ylm is None or cov_ylm is None
        if from_hyper:
            # upstream="reference" (default): the reference's algorithm on the host, comparable
            # digit by digit on the same host; upstream="device": the same integrals by exact
            # quadrature of rotations on the GPU (upstream_device.py), ~50x faster and free of
            # the reference's rounding noise in the high degrees
            how = kwargs.get("upstream", "reference")
            ukw = {k: v for k, v in kwargs.items() if k not in ("ydeg", "upstream")}
            if how == "device":
                from .upstream_device import ylm_moments_device

                dev_moments = ylm_moments_device(self._engine, r=r, dr=dr, a=a, b=b, c=c, n=n, **ukw)
            elif how == "reference":
                from .upstream import ylm_moments

                mean_ylm, cov_ylm = ylm_moments(r=r, dr=dr, a=a, b=b, c=c, n=n, ydeg=self._ydeg, **ukw)
            else:
                raise ValueError("upstream must be 'reference' or 'device'")
        self._dev_moments = dev_moments
        self._from_hyper = from_hyper      # built from (r, dr, a, b, c, n), not from explicit moments
        if dev_moments is None:
            self._host_moments = (np.asarray(mean_ylm, dtype=np.float64).reshape(-1),
                                  np.asarray(cov_ylm, dtype=np.float64))
            if self._host_moments[0].shape != (self._nylm,) or self._host_moments[1].shape != (self._nylm, self._nylm):
                raise ValueError("mean_ylm / cov_ylm have the wrong shape for ydeg=%d" % self._ydeg)
        else:
            self._host_moments = None      # copied back only if somebody asks (properties below)

        self._flux = FluxIntegral(
            dev_moments[0] if dev_moments is not None else self._host_moments[0],
            dev_moments[1] if dev_moments is not None else self._host_moments[1],
            udeg=self._udeg,
            marginalize_over_inclination=self._marginalize_over_inclination,
            covpts=self._covpts,
            ydeg=self._ydeg,
            device=kwargs.get("device"),
        )
        self._z = None
        # Mollweide image size (sp.py:243-244) and its transform, formed on the device at first use
        self._mx = int(kwargs.get("mx", defaults["mx"]))
        self._my = int(kwargs.get("my", defaults["my"]))
        self._M = None

    def _moments_np(self):
        if self._host_moments is None:
            self._host_moments = tuple(x.cpu().numpy() for x in self._dev_moments)
        return self._host_moments

    _mean_ylm = property(lambda self: self._moments_np()[0])
    _cov_ylm = property(lambda self: self._moments_np()[1])

    # -- hyperparameters (read-only views, sp.py:286-367) -------------------------
    a = property(lambda self: self._a)
    b = property(lambda self: self._b)
    r = property(lambda self: self._r)
    dr = property(lambda self: self._dr)
    c = property(lambda self: self._c)
    n = property(lambda self: self._n)
    tau = property(lambda self: self._tau)
    ydeg = property(lambda self: self._ydeg)
    udeg = property(lambda self: self._udeg)
    normalized = property(lambda self: self._normalized)
    covpts = property(lambda self: self._covpts)
    marginalize_over_inclination = property(lambda self: self._marginalize_over_inclination)
    mean_ylm = property(lambda self: Eager(self._mean_ylm))
    cov_ylm = property(lambda self: Eager(self._cov_ylm))

    # -- sums of processes (sp.py:1190-1197, 1335-1400) -------------------------------
    def __add__(self, other):
        return StarryProcessSum(self, other)

    def __radd__(self, other):
        if isinstance(other, (int, float)) and other == 0:
            return self          # so that sum([sp1, sp2, ...]) works
        return self.__add__(other)

    def log_jac(self):
        """Log |Jacobian| of the (a, b) -> (mu, sigma) transform (sp.py:1004-1050)."""
        from .upstream import log_jac

        return Eager(np.float64(log_jac(self._a, self._b, **self._kwargs)))

    # -- mean / cov (sp.py:643-703) --------------------------------------------------
    def mean(self, t, i=defaults["i"], p=defaults["p"], u=defaults["u"][: defaults["udeg"]]):
        if self._normalized:
            return Eager(np.zeros_like(np.asarray(t, dtype=np.float64).reshape(-1)))
        return self._flux.mean(t, i, p, u)

    def _device_cov(self, t, i, p, u):
        f = self._flux
        t, i, p, u = f._ingest(t, i, p, u)
        f._bind()
        e = self._engine
        stars = make_stars(1, period=p, inc_deg=i, tau=self._tau)
        if self._marginalize_over_inclination:
            tab, mv = f._table(u)
            cov, z = e.cov_marginal(t[None, :], stars, self._covpts, tab, mv, temporal=self._temporal,
                                    normalized=self._normalized, norm_order=self._normN)
            fmean = mv[0, 0]
        else:
            cov, mean, z = e.cov_conditional(t[None, :], stars, f._rta1(u), temporal=self._temporal,
                                             normalized=self._normalized, norm_order=self._normN)
            fmean = mean[0]
        if self._normalized:
            self._z = float(z[0].item())
        return t, cov[0], fmean

    def cov(self, t, i=defaults["i"], p=defaults["p"], u=defaults["u"][: defaults["udeg"]]):
        _, cov, _ = self._device_cov(t, i, p, u)
        return Eager(cov.cpu().numpy())

    # -- log likelihood (sp.py:1052-1188) ------------------------------------------------
    def log_likelihood(
        self,
        t,
        flux,
        data_cov,
        i=defaults["i"],
        p=defaults["p"],
        u=defaults["u"][: defaults["udeg"]],
        baseline_mean=defaults["baseline_mean"],
        baseline_var=defaults["baseline_var"],
    ):
        f = self._flux
        t, i, p, u = f._ingest(t, i, p, u)
        K = t.shape[0]
        flux = np.asarray(flux, dtype=np.float64)
        F = flux.reshape(1, K) if flux.ndim == 1 else flux.reshape(-1, K)
        data_cov = np.asarray(data_cov, dtype=np.float64)
        bmean = np.asarray(baseline_mean, dtype=np.float64)
        bvar = np.asarray(baseline_var, dtype=np.float64)
        simple = data_cov.ndim <= 1 and bmean.ndim == 0 and bvar.ndim == 0
        e = self._engine
        f._bind()
        if simple:
            stars = make_stars(1, period=p, inc_deg=i, tau=self._tau, baseline_var=float(bvar),
                               baseline_mean=float(bmean),
                               data_var=float(data_cov) if data_cov.ndim == 0 else 0.0)
            diag = e.f64(data_cov.reshape(1, K)) if data_cov.ndim == 1 else None
            rta1 = f._rta1(u)
            tab = mv = None
            if self._marginalize_over_inclination:
                tab, mv = f._table(u)
            out, status = e.lnlike_ensemble(
                e.f64(t[None, :]), e.f64(F[None, :, :]), e.stars_to_device(stars), diag=diag,
                conditional=not self._marginalize_over_inclination, covpts=self._covpts, tab=tab,
                meanvar=mv, rta1=rta1, temporal=self._temporal, normalized=self._normalized,
                norm_order=self._normN, zmax=self._normzmax)
            return Eager(_neg_inf_if_nan(out.cpu().numpy())[0])
        # general data / baseline covariances: assemble on the device, add the
        # extra terms with tensor ops, then the batched factorisation
        tt, cov, fmean = self._device_cov(t, i, p, u)
        C = cov.clone()
        if data_cov.ndim == 0:
            C.diagonal().add_(float(data_cov))
        elif data_cov.ndim == 1:
            C.diagonal().add_(e.f64(data_cov))
        else:
            C += e.f64(data_cov)
        C += e.f64(bvar) if bvar.ndim else float(bvar)
        gp_mean = 0.0 if self._normalized else fmean
        resid = e.f64(F) - (gp_mean + (e.f64(bmean) if bmean.ndim else float(bmean)))
        out, status = e.cholesky_lnlike(C[None, :, :], resid[None, :, :])
        val = _neg_inf_if_nan(out.cpu().numpy())[0]
        if self._normalized and self._z is not None and self._z > self._normzmax:
            val = -np.inf
        return Eager(val)

    def log_likelihood_samples(
        self,
        t,
        flux,
        data_cov,
        samples,
        i=defaults["i"],
        p=defaults["p"],
        u=defaults["u"][: defaults["udeg"]],
        baseline_mean=defaults["baseline_mean"],
        baseline_var=defaults["baseline_var"],
        depth=6,
        out_of_bounds="raise",
        params=("r", "a", "b", "c", "n"),
    ):
        """``log_likelihood(t, flux, data_cov, ...)`` of THIS process's settings (degree, normalisation, lag grid,
        temporal kernel, spot-size spread dr) at many hyperparameter vectors: samples (ns, 5) = rows of (r, a, b, c, n)
        -> (ns,) values, each what ``StarryProcess(r=r, a=a, b=b, c=c, n=n, <same settings>,
        upstream="device").log_likelihood(...)`` returns.  What a sampler does with the reference one call at a time
        (sp.py:1052-1062 driven by calibrate/sample.py:95-107) is here ONE batched device step per 64 samples
        (calibrate.SampleBatches) -- marginalised, normalised processes and conditional ones (normalised or not), with
        or without a temporal kernel, with scalar or per-cadence data variance and scalar baseline terms; anything else
        is evaluated sample by sample.  ``params`` names the columns of ``samples``: r, a, b, c, n and, each at most
        once, "dr", "baseline_mean", "baseline_log_var" (log10 of the baseline variance), "i" (inclination in degrees; a
        process that does not marginalise over it), "p" (period) and "tau" (timescale; a process built with one): the
        free parameters of the reference's log-probability (calibrate/log_prob.py:24-47, 93-103) and of its
        time-variability tutorial.  Such a column overrides the constructor's value or the argument of the same name.
        Bounds of the three: i in [0, 90], p >= 0 (flux.py:233-254), tau > 0.  ``out_of_bounds="inf"``: samples outside
        the reference's parameter bounds (a ValueError there and, by default, here) get -inf and are not evaluated."""
        cols = SampleColumns.from_params(params, self._marginalize_over_inclination, self._time_variable, dr=self._dr)
        return self._log_likelihood_samples(cols, t, flux, data_cov, samples, i, p, u, baseline_mean, baseline_var, depth,
                                            out_of_bounds)

    def _sample_process(self, cols, hyper, dr, kw):
        """The process of one sample on the sample-by-sample route: ``hyper`` (r, a, b, c, n), ``dr`` its spread."""
        r, a, b, c, n = hyper
        return StarryProcess(r=r, dr=dr, a=a, b=b, c=c, n=n, **kw)

    def _log_likelihood_samples(self, cols, t, flux, data_cov, samples, i, p, u, baseline_mean, baseline_var, depth,
                                out_of_bounds, ordered=False):
        """log_likelihood_samples on the column layout ``cols``; ``ordered``: the columns are in the layout's own order
        already."""
        from .calibrate import MAX_STREAMS_SAMPLES, SampleBatches, clamp_depth
        from .engine import engine_slots

        f = self._flux
        t, i, p, u = f._ingest(t, i, p, u)
        K = t.shape[0]
        free = cols.free
        samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
        if samples.shape[1] != len(cols.params):
            raise ValueError("samples must be (ns, %d): %s" % (len(cols.params), ", ".join(cols.params)))
        # the columns in the layout's own order (stars.SampleColumns)
        samples = np.ascontiguousarray(samples if ordered else samples[:, cols.permutation])
        if out_of_bounds == "raise":
            cols.check_ipt(samples)
        if out_of_bounds == "inf":
            ok = cols.in_bounds(samples)
            if not ok.all():
                out = np.full(samples.shape[0], -np.inf)
                if ok.any():
                    out[ok] = np.asarray(self._log_likelihood_samples(cols, t, flux, data_cov, samples[ok], i, p, u,
                                                                      baseline_mean, baseline_var, depth, "raise",
                                                                      ordered=True))
                return Eager(out)
        elif out_of_bounds != "raise":
            raise ValueError("out_of_bounds must be 'raise' or 'inf'")
        flux = np.asarray(flux, dtype=np.float64)
        F = flux.reshape(1, K) if flux.ndim == 1 else flux.reshape(-1, K)
        data_cov = np.asarray(data_cov, dtype=np.float64)
        bmean, bvar = np.asarray(baseline_mean, dtype=np.float64), np.asarray(baseline_var, dtype=np.float64)
        if "baseline_mean" in free:
            bmean = np.float64(0.0)       # (a placeholder: the column overrides the argument)
        if "baseline_log_var" in free:
            bvar = np.float64(0.0)
        batched = ((self._normalized or not self._marginalize_over_inclination) and K >= 2
                   and data_cov.ndim <= 1 and bmean.ndim == 0 and bvar.ndim == 0)
        if not batched:
            kw = dict(self._kwargs)
            kw.update(tau=self._tau if self._time_variable else None, temporal_kernel=self._temporal or "matern32",
                      marginalize_over_inclination=self._marginalize_over_inclination, normalized=self._normalized,
                      covpts=self._covpts, upstream="device")
            out = []
            hyper, drs, fields = cols.split(samples)
            for k in range(hyper.shape[0]):
                at = {key: v[k] for key, v in fields.items()}        # (this sample's free terms over the arguments)
                if "tau" in at:
                    kw["tau"] = at["tau"]
                out.append(float(self._sample_process(cols, hyper[k], cols.take_dr(drs, k), kw).log_likelihood(
                    t, flux, data_cov, i=at.get("inc_deg", i), p=at.get("period", p), u=u,
                    baseline_mean=at.get("baseline_mean", baseline_mean), baseline_var=at.get("baseline_var", baseline_var))))
            return Eager(np.array(out))
        dr = cols.dr
        key = (t.tobytes(), F.tobytes(), data_cov.tobytes(), float(p), float(i),
               tuple(np.asarray(u, dtype=float).reshape(-1)), float(bmean), float(bvar), int(depth), dr, free)
        cache = self.__dict__.get("_sample_batches")
        if cache is None or cache[0] != key:
            # (the data set is planned once and kept: a sampler calls this with the same data every iteration)
            slots = engine_slots(self._ydeg, self._udeg, self._kwargs.get("device"),
                                 clamp_depth(depth, limit=MAX_STREAMS_SAMPLES))
            e0 = slots[0][0]
            stars = make_stars(1, period=p, inc_deg=i, tau=self._tau, baseline_var=float(bvar), baseline_mean=float(bmean),
                               data_var=float(data_cov) if data_cov.ndim == 0 else 0.0)
            ukw = {k: self._kwargs[k] for k in ("epsy", "epsy15", "spts", "eps4", "smoothing", "sfac", "cutoff", "abmin",
                                                "log_alpha_max", "log_beta_max") if k in self._kwargs}
            sb = SampleBatches(slots, e0.f64(t[None, :]), e0.f64(F[None, :, :]), stars,
                               e0.f64(e0.rTA1L(np.asarray(u, dtype=np.float64))), self._covpts,
                               diag_dev=e0.f64(data_cov.reshape(1, K)) if data_cov.ndim == 1 else None,
                               temporal=self._temporal, norm_order=self._normN, zmax=self._normzmax, upstream_kwargs=ukw,
                               dr=dr, free=free, conditional=not self._marginalize_over_inclination,
                               normalized=self._normalized, populations=cols.populations)
            cache = self._sample_batches = (key, sb)
        out = cache[1](samples)
        import torch

        torch.cuda.synchronize(out.device)
        return Eager(_neg_inf_if_nan(out[:, 0].cpu().numpy()))

    def log_likelihood_grad(
        self,
        t,
        flux,
        data_cov,
        i=defaults["i"],
        p=defaults["p"],
        u=defaults["u"][: defaults["udeg"]],
        baseline_mean=defaults["baseline_mean"],
        baseline_var=defaults["baseline_var"],
    ):
        """(lnL, grads): the log-likelihood of ONE light curve (scalar or per-point data variance, scalar
        baseline terms) and its gradient -- what ``theano.grad(sp.log_likelihood(...), [r, a, b, c, n, p, ...])``
        is in the reference (grad.py: one reverse sweep through the library's reverse-mode kernels).  A process
        built from hyperparameters returns d/d(r, dr, a, b, c, n) and d/dp, d/dtau, d/di (conditional branch);
        one built from explicit moments returns d/d(mean_ylm, cov_ylm) in their place."""
        from .grad import hyper_gradient, log_likelihood_with_grad

        kw = dict(i=float(np.asarray(i)), p=float(np.asarray(p)), u=np.asarray(u, dtype=np.float64),
                  tau=self._tau if self._time_variable else None,
                  temporal_kernel=self._temporal or "matern32", baseline_mean=float(baseline_mean),
                  baseline_var=float(baseline_var),
                  marginalize_over_inclination=self._marginalize_over_inclination, normalized=self._normalized,
                  covpts=self._covpts, ydeg=self._ydeg, udeg=self._udeg, norm_order=self._normN,
                  zmax=self._normzmax, device=self._kwargs.get("device"))
        if self._from_hyper:
            # (whichever upstream built the moments: the chain rule through the hyperparameters runs on the
            #  device quadrature, whose moments are the same integrals -- upstream_device.py)
            ukw = {k: self._kwargs[k] for k in ("epsy", "epsy15", "spts", "eps4", "smoothing", "sfac", "cutoff",
                                                "abmin", "log_alpha_max", "log_beta_max") if k in self._kwargs}
            lnl, g = hyper_gradient(t, flux, data_cov, r=self._r, dr=self._dr, a=self._a, b=self._b, c=self._c,
                                    n=self._n, upstream_kwargs=ukw,
                                    moments0=None if self._dev_moments is not None else self._host_moments, **kw)
        else:
            lnl, g = log_likelihood_with_grad(self._mean_ylm, self._cov_ylm, t, flux, data_cov, **kw)
        return Eager(np.float64(lnl)), g

    # -- prior samples (sp.py:489-516, 729-765, 1237-1282) -------------------------------
    # The random numbers are NumPy's: the reference's Theano RandomStream cannot be
    # reproduced, so these methods are pinned by their moments, not by sample values.
    def _rng(self, seed):
        return np.random.RandomState(self._kwargs.get("seed", 0) if seed is None else seed)

    @property
    def cho_cov_ylm(self):
        """Lower Cholesky factor of Sigma_y (sp.py:436-441), factored on the device."""
        L, info = self._engine.cho_factor(self._cov_ylm)
        L = L.cpu().numpy()
        return Eager(np.full_like(L, np.nan) if int(info.reshape(-1)[0].item()) else L)

    # -- the process in pixel space (sp.py:443-487, 1199-1235) --------------------------------
    def _moments_dev(self):
        return self._dev_moments if self._dev_moments is not None else self._host_moments

    def _latlon_transform(self, latlon):
        """M at the lat/lon points (degrees, shape (..., 2), flattened) on the device (visualize.py:86-91)."""
        assert not _is_torch(latlon), "Input must be a numerical ndarray."
        lat, lon = np.asarray(latlon).reshape(-1, 2).T
        return self._engine.pixel_transform(latlon_to_xyz(lat * np.pi / 180, lon * np.pi / 180).reshape(3, -1))

    def mean_pix(self, latlon):
        """The prior mean at lat/lon points in degrees, ``latlon`` of shape (..., 2): shape (npts,)
        (sp.py:443-464, A mu_y)."""
        M = self._latlon_transform(latlon)
        return Eager(self._engine.pixel_render(M, self._moments_dev()[0], unit_background=False).cpu().numpy())

    def cov_pix(self, latlon):
        """The prior covariance at lat/lon points in degrees, ``latlon`` of shape (..., 2): shape (npts, npts),
        exactly symmetric (sp.py:466-487, (A Sigma_y) A^T)."""
        M = self._latlon_transform(latlon)
        return Eager(self._engine.pixel_cov(M, self._moments_dev()[1]).cpu().numpy())

    def var_pix(self, latlon, ycov=None):
        """The variance at lat/lon points in degrees, ``latlon`` of shape (..., 2) as in ``mean_pix``: the diagonal of
        ``cov_pix(latlon)`` without the npts x npts matrix, shape (npts,).  ``ycov``, a covariance of the Ylm
        coefficients or a stack of them of shape (..., nylm, nylm) (NumPy or a tensor on the device: what
        ``ylm_conditional`` and its ensemble / temporal / marginal forms return), replaces the prior's: shape
        (..., npts).  A posterior variance can round to a tiny negative number; it is returned as computed.
        Served for ydeg <= 20 (``Engine.pixel_var``); ValueError above, where ``cov_pix`` remains."""
        M = self._latlon_transform(latlon)
        cov = self._moments_dev()[1] if ycov is None else ycov
        return Eager(self._engine.pixel_var(M, cov).cpu().numpy())

    def mollweide_var(self, ycov=None, std=False):
        """The variance of the surface on the Mollweide grid of ``mollweide``: shape (my, mx) for the prior
        (``ycov=None``), (..., my, mx) for a covariance or stack ``ycov`` of shape (..., nylm, nylm); NaN off the
        ellipse.  ``std=True`` returns the standard deviation sqrt(max(var, 0)) instead.  Served for ydeg <= 20, as
        ``var_pix``."""
        e = self._engine
        if self._M is None:
            self._M = e.pixel_transform(mollweide_grid(self._my, self._mx))
        var = e.pixel_var(self._M, self._moments_dev()[1] if ycov is None else ycov).cpu().numpy()
        if std:
            var = np.sqrt(np.maximum(var, 0.0))      # (NaN stays NaN)
        return Eager(var.reshape(var.shape[:-1] + (self._my, self._mx)))

    def mollweide(self, y, unit_background=True):
        """Mollweide images of the Ylm vectors ``y`` (any shape (..., nylm)): shape (..., my, mx), NaN off the
        ellipse (sp.py:1199-1235).  ``unit_background`` adds 1 to y_0, so an unspotted surface is 1.  The image size
        comes from the constructor keywords ``mx`` and ``my``; the grid's transform is formed once per instance."""
        e = self._engine
        if self._M is None:
            self._M = e.pixel_transform(mollweide_grid(self._my, self._mx))
        img = e.pixel_render(self._M, y, unit_background=unit_background)
        return Eager(img.cpu().numpy().reshape(tuple(img.shape[:-1]) + (self._my, self._mx)))

    def sample_ylm(self, t=None, nsamples=1, seed=None):
        """Samples of the spherical-harmonic coefficients from the prior (sp.py:489-516): shape (nsamples, nylm),
        or (nsamples, ntimes, nylm) when the times ``t`` are given to a time-variable process (``tau`` set).

        The time-variable samples are Y[n] = Lt U[n] Ly^T with Lt the Cholesky factor of the temporal kernel
        k(t, t, tau) (no jitter), Ly that of Sigma_y and U = RandomState(seed).normal(size=(nsamples, ntimes,
        nylm)), ``seed`` defaulting to the constructor's.  As in the reference they have ZERO MEAN: mean_ylm is not
        added.  If either factorisation fails (the exp-squared kernel on a dense cadence is numerically singular),
        every value is NaN, as the reference's cho_factor(on_error="nan") gives; nothing is raised."""
        if t is not None:
            if not self._time_variable:
                raise NotImplementedError("samples at times t need a time-variable process (tau=...)")
            return Eager(self._sample_ylm_temporal(t, nsamples, seed).cpu().numpy())
        u = self._rng(seed).randn(self._nylm, int(nsamples))
        return Eager((self._mean_ylm[:, None] + np.array(self.cho_cov_ylm) @ u).T)

    def _cho_ylm_dev(self):
        """Lower Cholesky factor of Sigma_y on the device (all NaN if it does not factor), once per instance."""
        L = self.__dict__.get("_cho_ylm")
        if L is None:
            L = self._cho_ylm = self._engine.cho_factor(self._moments_dev()[1])[0]
        return L

    def _sample_ylm_temporal(self, t, nsamples, seed):
        e = self._engine
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        Lt, _ = e.temporal_gram(t, self._tau, self._temporal)
        U = self._rng(seed).normal(size=(int(nsamples), t.shape[0], self._nylm))
        return e.ylm_temporal(Lt, self._cho_ylm_dev(), U)

    def sample(self, t, i=defaults["i"], p=defaults["p"], u=defaults["u"][: defaults["udeg"]],
               nsamples=1, eps=defaults["eps"], seed=None):
        """Light curves drawn from the prior, shape (nsamples, ntimes) (sp.py:729-765):
        mean + L z with L the device Cholesky factor of cov(t) + eps I."""
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        cov = np.array(self.cov(t, i, p, u))
        cov[np.diag_indices_from(cov)] += eps
        L, info = self._engine.cho_factor(cov)
        L = L.cpu().numpy()
        if int(info.reshape(-1)[0].item()):
            L = np.full_like(L, np.nan)
        U = self._rng(seed).randn(t.shape[0], int(nsamples))
        return Eager((np.array(self.mean(t, i, p, u))[:, None] + L @ U).T)

    def flux(self, y, t, i=defaults["i"], p=defaults["p"], u=defaults["u"][: defaults["udeg"]]):
        """Light curves of given spherical-harmonic vectors (sp.py:1237-1282), through the device design matrix A.
        A process that is not time-variable takes y (nsamples, nylm) and returns (nsamples, ntimes).  A
        time-variable one takes y (..., ntimes, nylm), one map per time (what ``sample_ylm(t)`` returns), and
        returns F[..., k] = A[k] . y[..., k] with shape (..., ntimes); normalised, each row becomes
        (1 + F) / mean(1 + F) - 1, and a 2-D y gives (1, ntimes) as in the reference."""
        if self._time_variable:
            return self._flux_temporal(y, t, i, p, u)
        y = np.atleast_2d(np.asarray(y, dtype=np.float64))
        A = np.array(self._flux.design_matrix(t, i, p, u))      # (ntimes, nylm)
        flux = (A @ y.T).T
        if self._normalized:
            flux = (1.0 + flux) / np.mean(1.0 + flux, axis=-1).reshape(-1, 1) - 1.0
        return Eager(flux)

    def _flux_temporal(self, y, t, i, p, u):
        e, f = self._engine, self._flux
        t, i, p, u = f._ingest(t, i, p, u)
        y = np.asarray(y, dtype=np.float64)
        if y.ndim < 2 or y.shape[-2:] != (t.shape[0], self._nylm):
            raise ValueError("y must have shape (..., %d, %d) for a time-variable process: one map per time"
                             % (t.shape[0], self._nylm))
        f._bind()
        A = e.design_matrix(t[None, :], make_stars(1, period=p, inc_deg=i), f._rta1(u))[0]
        flux = e.flux_rows(A, y, normalized=self._normalized).cpu().numpy()
        if self._normalized and y.ndim == 2:
            flux = flux.reshape(1, -1)      # (the reference's mean reshaped to (-1, 1) broadcasts a 1-D flux to 2-D)
        return Eager(flux)

    # -- conditioning on data (sp.py:767-1002) ---------------------------------------------
    def predict(
        self,
        t,
        flux,
        data_cov,
        t_sample=None,
        i=defaults["i"],
        p=defaults["p"],
        u=defaults["u"][: defaults["udeg"]],
        baseline_mean=defaults["baseline_mean"],
        baseline_var=defaults["baseline_var"],
    ):
        """Mean and covariance of the light curve distribution conditioned on the observed
        flux (sp.py:767-903).  As in the reference: not implemented for normalized
        processes.  The three covariance blocks come from ONE device assembly on the
        concatenated times [t_sample, t]; the conditioning is one factorisation with the
        cross covariance riding along as extra rows (``sp_gp_condition``)."""
        if self._normalized:
            raise NotImplementedError("Method not implemented when the flux is normalized.")
        e = self._engine
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        K = t.shape[0]
        if t_sample is None:
            tall, Ks = t, K
        else:
            ts = np.asarray(t_sample, dtype=np.float64).reshape(-1)
            Ks = ts.shape[0]
            tall = np.concatenate([ts, t])
        _, cov, fmean = self._device_cov(tall, i, p, u)
        mean = float(fmean)
        if t_sample is None:
            Ktt, Kst, Kss = cov.clone(), cov.clone(), cov.clone()
        else:
            Kss, Kst, Ktt = cov[:Ks, :Ks].clone(), cov[:Ks, Ks:].clone(), cov[Ks:, Ks:].clone()
        data_cov = np.asarray(data_cov, dtype=np.float64)
        if data_cov.ndim == 0:
            Ktt.diagonal().add_(float(data_cov))
        elif data_cov.ndim == 1:
            Ktt.diagonal().add_(e.f64(data_cov))
        else:
            Ktt += e.f64(data_cov)
        bvar = np.asarray(baseline_var, dtype=np.float64)
        bv = e.f64(bvar) if bvar.ndim else float(bvar)
        Ktt += bv
        Kss += bv
        Kst += bv
        y = e.f64(np.asarray(flux, dtype=np.float64).reshape(-1) - np.asarray(baseline_mean, dtype=np.float64))
        mu, Kpost, info = e.gp_condition(Ktt, Kst, Kss, y - mean)
        mu = mu.cpu().numpy() + mean
        Kpost = Kpost.cpu().numpy()
        if int(info.item()):
            mu, Kpost = np.full_like(mu, np.nan), np.full_like(Kpost, np.nan)
        return Eager(mu), Eager(Kpost)

    def sample_conditional(self, t, flux, data_cov, t_sample=None, i=defaults["i"], p=defaults["p"],
                           u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                           baseline_var=defaults["baseline_var"], nsamples=1, eps=1e-12, seed=None):
        """Samples from the conditional distribution (sp.py:905-1002): predict, then
        mean + L z with L the device Cholesky factor of the posterior covariance.  The
        random numbers are NumPy's (the reference's Theano stream cannot be reproduced)."""
        mu, Kpost = self.predict(t, flux, data_cov, t_sample, i, p, u, baseline_mean, baseline_var)
        Kpost = np.array(Kpost)
        Kpost[np.diag_indices_from(Kpost)] += eps
        L, info = self._engine.cho_factor(Kpost)
        L = L.cpu().numpy()
        if int(info.reshape(-1)[0].item()):
            L = np.full_like(L, np.nan)
        z = np.random.RandomState(seed).randn(Kpost.shape[0], int(nsamples))
        return Eager(np.array(mu)[None, :] + (L @ z).T)

    # -- conditioning on the data of an ensemble: S stars in one device call (sp_predict_ensemble) -----------
    def _predict_ensemble_dev(self, t, flux, data_cov, t_sample, i, p, u, baseline_mean, baseline_var, mode,
                              basis=None, basis_var=None, basis_sample=None):
        """(mu, cov / var / None, info) as device tensors: the arguments of the ensemble calls through the engine.
        With ``basis``: ``Engine.predict_linear`` in place of ``Engine.predict_ensemble`` -- its whole tuple, (mu,
        second, info, w_mean, lnlike, lnlike0, status); the regressor arguments are checked on the host before any
        device work."""
        if self._normalized:
            raise NotImplementedError("Method not implemented when the flux is normalized.")
        if basis is None and (basis_var is not None or basis_sample is not None):
            raise ValueError("`basis_var` and `basis_sample` need a `basis`")
        t, flux, stars, utab, diag = self._ensemble_args(t, flux, data_cov, i, p, u, baseline_mean, baseline_var)
        S, K = flux.shape
        ts = None
        if t_sample is not None:
            ts = np.asarray(t_sample, dtype=np.float64)
            if ts.ndim == 1 and ts.shape[0] >= 1:
                ts = np.broadcast_to(ts, (S, ts.shape[0]))
            elif ts.ndim != 2 or ts.shape[0] != S or ts.shape[1] < 1:
                raise ValueError("`t_sample` must be (Ks,) or (S, Ks) with S = %d, not %s" % (S, ts.shape))
            ts = np.ascontiguousarray(ts)
        U, Ut, lam = _regressor_args(basis, basis_var, S, K)
        if basis is not None:
            q, Ks = U.shape[2], (K if ts is None else ts.shape[1])
            Us = None
            if basis_sample is not None:
                Us = np.asarray(basis_sample, dtype=np.float64)
                if Us.shape == (Ks, q):
                    Us = np.broadcast_to(Us, (S, Ks, q))
                if Us.shape != (S, Ks, q):
                    raise ValueError("`basis_sample` must be (Ks, q) or (S, Ks, q) with S = %d, Ks = %d, q = %d, not %s"
                                     % (S, Ks, q, np.shape(basis_sample)))
                if not np.all(np.isfinite(Us)):
                    raise ValueError("`basis_sample` must be finite")
                Us = np.ascontiguousarray(Us)
        e = self._engine
        branch = dict(self._branch(utab, norm=False), diag=diag, mode=mode)
        if basis is not None:
            return e.predict_linear(t, ts, flux, stars, e.f64(Ut), lam, None if Us is None else e.f64(Us), **branch)
        return e.predict_ensemble(t, ts, flux, stars, **branch)

    def _branch(self, utab, norm=True):
        """The opening of an ensemble method, once its refusals are raised: binds the moments, forms rTA1 of the
        limb-darkening sets ``utab`` and, on the marginal branch, the kernel table.  Returns the keywords every engine
        call of the ensemble takes for the instance's branch; ``norm``: with the normalisation's (the predict calls
        take none)."""
        e = self._engine
        self._flux._bind()
        rta1 = e.f64(e.rTA1L(utab))
        tab = mv = None
        if self._marginalize_over_inclination:
            tab, mv = e.kernel_table(rta1, self._covpts)
        kw = dict(conditional=not self._marginalize_over_inclination, covpts=self._covpts, tab=tab, meanvar=mv,
                  rta1=rta1, temporal=self._temporal)
        if norm:
            kw.update(normalized=self._normalized, norm_order=self._normN, zmax=self._normzmax)
        return kw

    def predict_ensemble(self, t, flux, data_cov, t_sample=None, i=None, p=None, u=None, baseline_mean=0.0,
                         baseline_var=0.0, return_cov=True, basis=None, basis_var=None, basis_sample=None):
        """``predict`` for S stars in one device call: the light curve distributions conditioned on the observed
        fluxes, each star with its own period, inclination, limb darkening, baseline and noise.

        t: (K,) or (S, K); flux: (S, K); data_cov: scalar, (S,) or (S, K); t_sample: None (predict at ``t``), (Ks,)
        or (S, Ks); i, p, baseline_mean, baseline_var: scalars or (S,); u: (udeg,) shared or (S, udeg).
        return_cov=True: (mu (S, Ks), cov (S, Ks, Ks)), each covariance exactly symmetric; "diag": (mu, var (S, Ks))
        without forming any Ks x Ks matrix; False: mu alone.  A star whose covariance at the observed times does
        not factor gets NaN in all its outputs (``predict``'s rule, per star).  Not implemented for normalized
        processes, as in the reference.

        ``basis`` (K, q) shared or (S, K, q) and ``basis_var`` scalar, (q,) or (S, q), as
        ``log_likelihood_linear_ensemble`` takes and refuses them: the conditional under the model flux = process +
        U w + noise, w ~ N(0, diag(basis_var)) (sp_predict_linear), the weights marginalised out and their
        uncertainty carried into ``cov`` / ``var``.  ``basis_sample`` (Ks, q) or (S, Ks, q): the regressors at the
        sample times (``linear.offset_basis_at``, ``linear.polynomial_basis_at``) -- the prediction is then process
        + trend, what the data will look like; None: the process alone, the trend removed.  Without ``basis``
        nothing changes."""
        if not (return_cov is True or return_cov is False or (isinstance(return_cov, str) and return_cov == "diag")):
            raise ValueError("`return_cov` must be True, False or \"diag\"")
        mu, second = self._predict_ensemble_dev(t, flux, data_cov, t_sample, i, p, u, baseline_mean, baseline_var,
                                                return_cov, basis, basis_var, basis_sample)[:2]
        if return_cov is False:
            return Eager(mu.cpu().numpy())
        return Eager(mu.cpu().numpy()), Eager(second.cpu().numpy())

    def sample_conditional_ensemble(self, t, flux, data_cov, t_sample=None, i=None, p=None, u=None, baseline_mean=0.0,
                                    baseline_var=0.0, nsamples=1, eps=1e-12, seed=None, basis=None, basis_var=None,
                                    basis_sample=None):
        """Samples from the conditional distributions of S stars, shape (S, nsamples, Ks): ``predict_ensemble``, then
        mu_s + L_s z_s with L_s the Cholesky factor of the posterior covariance + eps I (one batched factorisation)
        and z = RandomState(seed).randn(S, Ks, nsamples) -- the constructor's seed when ``seed`` is None; with one
        star, the deviates ``sample_conditional`` draws.  The product runs on the device.  ``basis``, ``basis_var``
        and ``basis_sample`` as ``predict_ensemble`` takes them."""
        mu, cov = self._predict_ensemble_dev(t, flux, data_cov, t_sample, i, p, u, baseline_mean, baseline_var,
                                             True, basis, basis_var, basis_sample)[:2]
        e = self._engine
        S, Ks = mu.shape
        cov.diagonal(dim1=1, dim2=2).add_(float(eps))
        L, _ = e.cho_factor(cov)                                  # (all NaN for a star that does not factor)
        z = self._rng(seed).randn(S, Ks, int(nsamples))
        return Eager(_affine_samples(e, mu, L.contiguous(), z).cpu().numpy())

    # -- model checking: leave-one-out predictive distributions (sp_loo_ensemble) ---------------------------
    def loo_ensemble(self, t, flux, data_cov, i=None, p=None, u=None, baseline_mean=0.0, baseline_var=0.0,
                     max_workspace_bytes=None, basis=None, basis_var=None):
        """Leave-one-out predictive checks of S light curves in one device call (Rasmussen & Williams 5.4.2): what
        the process, fitted to all the other cadences of a star, predicts for each cadence.  Nothing is refitted:
        with C the covariance ``log_likelihood_ensemble`` factors, r its residual, alpha = C^-1 r, d = diag(C^-1),

            mu[k] = flux[k] - alpha[k] / d[k]    var[k] = 1 / d[k]    z[k] = alpha[k] / sqrt(d[k])
            lpd[k] = -1/2 log(2 pi var[k]) - 1/2 z[k]^2               white = L^-1 r  (C = L L^T)

        Arguments as ``predict_ensemble``: t (K,) or (S, K); flux (S, K); data_cov: scalar, (S,) or (S, K); i, p,
        baseline_mean, baseline_var: scalars or (S,); u: (udeg,) shared or (S, udeg).  The branch is the instance's
        (``marginalize_over_inclination``, ``tau``, ``normalized``); unlike ``predict``, a normalised process is
        served.  ``mu`` and ``var`` are predictive for the DATUM: they include ``baseline_mean`` and the cadence's
        own noise variance (``predict`` at a held-out time gives mu - baseline_mean and var - data_var[k]).

        Returns a dict of NumPy arrays: ``mu``, ``var``, ``z``, ``lpd``, ``white`` (S, K); ``elpd`` = lpd.sum(1),
        ``lnlike`` (-inf where ``log_likelihood_ensemble`` gives -inf) and ``status`` (S,).  A star whose covariance
        does not factor has NaN in its rows.  ``max_workspace_bytes`` caps the device scratch: the stars are then
        worked through in groups, with the same bits.  A full-matrix ``data_cov``, a matrix ``baseline_var`` and
        ragged input (lists of light curves of different lengths) are not served.

        ``basis``, ``basis_var`` (as ``log_likelihood_linear_ensemble`` takes them): the checks of the model flux =
        process + U w + noise, w ~ N(0, diag(basis_var)), through ``lbo_ensemble(..., block=1, basis=...)`` -- see
        there.  ``mu`` and ``var`` then include the trend and the uncertainty of the weights, ``z`` is that call's
        ``u``, ``white`` holds the whitened DETRENDED residual, and the dict gains ``lnlike0``, ``w_mean`` and
        ``trend``."""
        if basis is None and basis_var is not None:
            raise ValueError("`basis_var` needs a `basis`")
        if basis is not None:
            out = self.lbo_ensemble(t, flux, data_cov, 1, i=i, p=p, u=u, baseline_mean=baseline_mean,
                                    baseline_var=baseline_var, max_workspace_bytes=max_workspace_bytes, basis=basis,
                                    basis_var=basis_var, _name="loo_ensemble")
            out["z"] = out.pop("u")
            del out["edges"]
            return out
        tt, flux, dc, S, K = _dense_ensemble_input("loo_ensemble", t, flux, data_cov, baseline_var)
        if K < 2:
            raise ValueError("leave-one-out needs at least two cadences")
        t, flux, stars, utab, diag = self._ensemble_args(tt, flux, dc, i, p, u, baseline_mean, baseline_var)
        loo, lnlike, status = self._engine.loo_ensemble(t, flux, stars, diag=diag,
                                                        max_workspace_bytes=max_workspace_bytes, **self._branch(utab))
        loo = loo.cpu().numpy()
        out = {name: np.ascontiguousarray(loo[:, k]) for k, name in enumerate(("mu", "var", "z", "lpd", "white"))}
        out["elpd"] = out["lpd"].sum(axis=1)
        out["lnlike"] = _neg_inf_if_nan(lnlike.cpu().numpy())
        out["status"] = status.cpu().numpy()
        return out

    def loo(self, t, flux, data_cov, i=defaults["i"], p=defaults["p"], u=defaults["u"][: defaults["udeg"]],
            baseline_mean=defaults["baseline_mean"], baseline_var=defaults["baseline_var"], basis=None,
            basis_var=None):
        """``loo_ensemble`` for one light curve: t, flux (K,); data_cov a scalar or (K,) variances; basis None or
        (K, q); basis_var a scalar or (q,).  The same dict without the leading axis."""
        flux, dc = _one_curve("loo", flux, data_cov, baseline_var)
        basis, basis_var = _one_star_regressors(basis, basis_var)
        out = self.loo_ensemble(np.asarray(t, dtype=np.float64).reshape(-1), flux, dc, i=i, p=p, u=u,
                                baseline_mean=baseline_mean, baseline_var=baseline_var, basis=basis,
                                basis_var=basis_var)
        return {k: v[0] for k, v in out.items()}

    # -- model checking: leave-block-out predictive distributions (sp_lbo_ensemble) -------------------------
    def lbo_ensemble(self, t, flux, data_cov, block, i=None, p=None, u=None, baseline_mean=0.0, baseline_var=0.0,
                     return_cov=False, max_workspace_bytes=None, basis=None, basis_var=None, _name="lbo_ensemble"):
        """Leave-block-out predictive checks of S light curves in one device call (h-block cross-validation): what
        the process, fitted to the cadences OUTSIDE a block B of consecutive ones, predicts for the whole block.
        Nothing is refitted: with C the covariance ``log_likelihood_ensemble`` factors, r its residual, alpha = C^-1 r
        and G = (C^-1)_BB = L_G L_G^T,

            cov_B = G^-1    mu_B = flux_B - G^-1 alpha_B    u_B = L_G^-1 alpha_B    (N(0, I) when the model holds)
            lpd_B = -1/2 u_B^T u_B + sum log (L_G)_ii - b/2 log 2 pi                (log density of the held-out block)

        ``block``: an int b, 1 <= b <= 64 -- blocks of b cadences, the last one shorter -- or a 1-D integer array of
        edges 0 = e_0 < e_1 < ... < e_nb = K with every width between 1 and 64; the partition is common to all stars.
        Wider blocks are not served.  The other arguments, the branches and the refusals are ``loo_ensemble``'s.
        ``mu``, ``var`` and ``cov`` are predictive for the DATA: they include ``baseline_mean`` and the cadences' own
        noise variance.

        Returns a dict of NumPy arrays: ``mu``, ``var``, ``u``, ``white`` (S, K); ``lpd`` (S, nb); ``elpd`` =
        lpd.sum(1); ``edges`` (nb + 1,); ``lnlike`` (-inf where ``log_likelihood_ensemble`` gives -inf) and ``status``
        (S,); with ``return_cov`` also ``cov`` (S, nb, bmax, bmax), bmax the widest block: the block's covariance in the
        corner of its slot, the rest NaN.  A star whose covariance does not factor has NaN in its rows.
        ``max_workspace_bytes`` caps the device scratch: the stars are then worked through in groups, with the same
        bits.

        With ``basis`` (K, q) shared or (S, K, q) and ``basis_var`` scalar, (q,) or (S, q), as
        ``log_likelihood_linear_ensemble`` takes and refuses them, the checks are those of the model flux = process +
        U w + noise, w ~ N(0, diag(basis_var)) (sp_lbo_linear): C above becomes C~ = C + U diag(basis_var) U^T, never
        formed.  ``mu``, ``var`` and ``cov`` are predictive for the DATA, the trend and the uncertainty of the weights
        included -- most of it when a block is a large part of a regressor's support; ``lpd`` of a block is lnlike of
        all cadences minus lnlike of those outside it.  ``white`` then holds the whitened DETRENDED residual L^-1 (r -
        U w_mean), whose covariance under the model is I - T T^T (q degrees of freedom fewer, like the residuals of
        any regression), ``lnlike`` is ``log_likelihood_linear_ensemble``'s, and the dict gains ``lnlike0`` (S,),
        ``w_mean`` (S, q) and ``trend`` (S, K) = U w_mean.  Without ``basis`` nothing changes."""
        if basis is None and basis_var is not None:
            raise ValueError("`basis_var` needs a `basis`")
        tt, flux, dc, S, K = _dense_ensemble_input(_name, t, flux, data_cov, baseline_var)
        edges = block_edges(block, K)
        if basis is not None and K < 2:
            raise ValueError("the checks with regressors need at least two cadences")
        _, Ut, lam = _regressor_args(basis, basis_var, S, K)
        t, flux, stars, utab, diag = self._ensemble_args(tt, flux, dc, i, p, u, baseline_mean, baseline_var)
        e = self._engine
        branch = dict(self._branch(utab), diag=diag, return_cov=return_cov, max_workspace_bytes=max_workspace_bytes)
        extra = {}
        if basis is not None:
            Ud = e.f64(Ut)
            rows, lpd, cov, lnlike, lnlike0, wmean, status = e.lbo_linear(t, flux, stars, edges, Ud, lam, **branch)
            extra = _linear_extras(Ud, wmean, lnlike0)
        else:
            rows, lpd, cov, lnlike, status = e.lbo_ensemble(t, flux, stars, edges, **branch)
        rows = rows.cpu().numpy()
        out = {name: np.ascontiguousarray(rows[:, k]) for k, name in enumerate(("mu", "var", "u", "white"))}
        out["lpd"] = lpd.cpu().numpy()
        out["elpd"] = out["lpd"].sum(axis=1)
        out["edges"] = edges
        if return_cov:
            out["cov"] = cov.cpu().numpy()
        out["lnlike"] = _neg_inf_if_nan(lnlike.cpu().numpy())
        out.update(extra)
        out["status"] = status.cpu().numpy()
        return out

    def lbo(self, t, flux, data_cov, block, i=defaults["i"], p=defaults["p"], u=defaults["u"][: defaults["udeg"]],
            baseline_mean=defaults["baseline_mean"], baseline_var=defaults["baseline_var"], return_cov=False,
            basis=None, basis_var=None):
        """``lbo_ensemble`` for one light curve: t, flux (K,); data_cov a scalar or (K,) variances; basis None or
        (K, q); basis_var a scalar or (q,).  The same dict without the leading axis (``edges`` as it is)."""
        flux, dc = _one_curve("lbo", flux, data_cov, baseline_var)
        basis, basis_var = _one_star_regressors(basis, basis_var)
        out = self.lbo_ensemble(np.asarray(t, dtype=np.float64).reshape(-1), flux, dc, block, i=i, p=p, u=u,
                                baseline_mean=baseline_mean, baseline_var=baseline_var, return_cov=return_cov,
                                basis=basis, basis_var=basis_var)
        return {k: (v if k == "edges" else v[0]) for k, v in out.items()}

    # -- linear regressors marginalised out of the likelihood (sp_lnlike_linear) ------------------------------
    def log_likelihood_linear_ensemble(self, t, flux, data_cov, basis, basis_var, i=None, p=None, u=None,
                                       baseline_mean=0.0, baseline_var=0.0, return_cov=True,
                                       max_workspace_bytes=None):
        """The log likelihood of S light curves with linear regressors marginalised out, in one device call:
        flux = process + U w + noise with w ~ N(0, diag(basis_var)) -- segment offsets, instrumental trends,
        systematics vectors (``starry_process_amd.linear`` builds the usual ones).  It is the reference's
        ``log_likelihood(..., baseline_var=b + U diag(basis_var) U^T)`` (Luger et al. 2017, Eq. 4) without the K x K
        matrix, and it returns the posterior of the weights as well: the detrending itself.  With C = L L^T the
        covariance ``log_likelihood_ensemble`` factors, r its residual, y = L^-1 r, W = L^-1 U, D = diag(sqrt(basis_var)):

            G = I + D W^T W D = L_G L_G^T        v = L_G^-1 D W^T y
            lnlike = -1/2 (y^T y - v^T v) - sum log L_ii - sum log (L_G)_jj - K/2 log 2 pi
            w_mean = D L_G^-T v                  w_cov = D G^-1 D

        basis: (K, q) shared or (S, K, q), 1 <= q <= 32, finite; basis_var: scalar, (q,) or (S, q), finite and >= 0
        (0 switches a regressor off exactly).  The other arguments, the branch of the instance and the refusals are
        ``loo_ensemble``'s.

        Returns a dict of NumPy arrays: ``lnlike`` and ``lnlike0``, the likelihood with and without the regressors
        (S,) (-inf where ``log_likelihood_ensemble`` gives -inf); ``w_mean`` (S, q); ``w_cov`` (S, q, q), exactly
        symmetric (absent with ``return_cov=False``); ``trend`` (S, K) = U w_mean; ``status`` (S,).  A star whose
        covariance does not factor has NaN in its outputs.  ``max_workspace_bytes`` caps the device scratch: the stars
        are then worked through in groups, with the same bits."""
        tt, flux, dc, S, K = _dense_ensemble_input("log_likelihood_linear_ensemble", t, flux, data_cov, baseline_var,
                                                   _BASIS_HINT)
        if K < 2:
            raise ValueError("the likelihood with regressors needs at least two cadences")
        _, Ut, lam = _regressor_args(basis, basis_var, S, K, required=True)
        t, flux, stars, utab, diag = self._ensemble_args(tt, flux, dc, i, p, u, baseline_mean, baseline_var)
        e = self._engine
        branch = self._branch(utab)
        Ud = e.f64(Ut)
        lnlike, lnlike0, wmean, wcov, status = e.lnlike_linear(
            t, flux, stars, Ud, lam, diag=diag, return_cov=return_cov, max_workspace_bytes=max_workspace_bytes,
            **branch)
        out = {"lnlike": _neg_inf_if_nan(lnlike.cpu().numpy()), **_linear_extras(Ud, wmean, lnlike0)}
        if return_cov:
            out["w_cov"] = wcov.cpu().numpy()
            out["trend"] = out.pop("trend")       # (the trend stands after w_cov)
        out["status"] = status.cpu().numpy()
        return out

    def log_likelihood_linear(self, t, flux, data_cov, basis, basis_var, i=defaults["i"], p=defaults["p"],
                              u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                              baseline_var=defaults["baseline_var"], return_cov=True):
        """``log_likelihood_linear_ensemble`` for one light curve: t, flux (K,); data_cov a scalar or (K,) variances;
        basis (K, q); basis_var a scalar or (q,).  The same dict without the leading axis."""
        flux, dc = _one_curve("log_likelihood_linear", flux, data_cov, baseline_var, _BASIS_HINT)
        basis, basis_var = _one_star_regressors(basis, basis_var, required=True)
        out = self.log_likelihood_linear_ensemble(np.asarray(t, dtype=np.float64).reshape(-1), flux, dc, basis,
                                                  basis_var, i=i, p=p, u=u, baseline_mean=baseline_mean,
                                                  baseline_var=baseline_var, return_cov=return_cov)
        return {k: v[0] for k, v in out.items()}

    # -- posterior of the surface map (sp.py:518-641) -------------------------------------
    # W = Sigma_y^-1 + A^T C^-1 A, ymu = W^-1 (Sigma_y^-1 mu_y + A^T C^-1 (flux - baseline_mean)), ycov = W^-1,
    # with A the design matrix at (t, i, p, u) whatever marginalize_over_inclination says (sp.py:620), as in
    # the reference.  A scalar or vector data_cov of positive variances with a scalar baseline_var never forms C
    # (Sherman-Morrison, sp_ylm_conditional_batched); a full matrix, or a variance <= 0, is factored and the data
    # whitened first.
    def _ylm_precision(self):
        """(Sigma_y^-1, Sigma_y^-1 mu_y) on the device, formed once per moment set (sp.py:267-271)."""
        prec = self.__dict__.get("_ylm_prec")
        if prec is None:
            mu, cov = self._dev_moments if self._dev_moments is not None else self._host_moments
            prec = self._ylm_prec = self._engine.ylm_precision(mu, cov)
        return prec

    def _ylm_check(self):
        if self._normalized:
            raise NotImplementedError("Method not implemented when the flux is normalized.")
        if self._time_variable:
            raise NotImplementedError("Method not implemented for time-variable maps.")

    def _ylm_posterior(self, t, flux, data_cov, i, p, u, baseline_mean, baseline_var, with_cho, full=False):
        self._ylm_check()
        e, f = self._engine, self._flux
        t, i, p, u = f._ingest(t, i, p, u)
        K = t.shape[0]
        r = np.asarray(flux, dtype=np.float64).reshape(-1) - np.asarray(baseline_mean, dtype=np.float64)
        if r.shape != (K,):
            raise ValueError("`flux` must have one value per time")
        data_cov = np.asarray(data_cov, dtype=np.float64)
        bvar = np.asarray(baseline_var, dtype=np.float64)
        sinv, sinvmu = self._ylm_precision()
        rta1 = f._rta1(u)
        # the Sherman-Morrison kernel needs every variance > 0; a star with one <= 0 may still have a positive
        # definite C = D + b 1 1^T, so it is factored as such (the reference's cho_factor decides, sp.py:616)
        if not full and data_cov.ndim <= 1 and bvar.ndim == 0 and np.all(data_cov > 0):
            stars, diag = _one_star_noise(1, K, data_cov, period=p, inc_deg=i, baseline_var=float(bvar))
            ymu, ycov, ycho, _ = e.ylm_conditional(t[None, :], r[None, :], stars, rta1, sinv, sinvmu, diag=diag,
                                                   with_cho=with_cho)
        else:
            # full data covariance (or a matrix baseline_var): C = data_cov + baseline_var (sp.py:601-613),
            # C = L L^T, then the same posterior on L^-1 A and L^-1 r
            if data_cov.ndim == 0:
                C = data_cov * np.eye(K)
            elif data_cov.ndim == 1:
                C = np.diag(np.broadcast_to(data_cov, (K,)))
            else:
                C = data_cov
            L, _ = e.cho_factor(C + bvar)
            A = e.design_matrix(t[None, :], make_stars(1, period=p, inc_deg=i), rta1)[0]
            B = e.tri_solve(L, A)
            rw = e.tri_solve(L, e.f64(r))
            ymu, ycov, ycho, _ = e.ylm_conditional_whitened(B[None], rw[None], sinv, sinvmu, with_cho=with_cho)
        return ymu[0], ycov[0], (None if ycho is None else ycho[0])

    def ylm_conditional(self, t, flux, data_cov, i=defaults["i"], p=defaults["p"],
                        u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                        baseline_var=defaults["baseline_var"]):
        """Mean (nylm,) and covariance (nylm, nylm) of the spherical-harmonic coefficients conditioned on the
        observed flux: the Gaussian ``sample_ylm_conditional`` draws from (sp.py:601-636), which the reference
        computes but does not return.  NaN if a covariance on the way is not positive definite."""
        ymu, ycov, _ = self._ylm_posterior(t, flux, data_cov, i, p, u, baseline_mean, baseline_var, False)
        return Eager(ymu.cpu().numpy()), Eager(ycov.cpu().numpy())

    def sample_ylm_conditional(self, t, flux, data_cov, i=defaults["i"], p=defaults["p"],
                               u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                               baseline_var=defaults["baseline_var"], nsamples=1, seed=None):
        """Samples of the spherical-harmonic coefficients conditioned on the observed flux, shape
        (nsamples, nylm) (sp.py:518-641): ymu + cho_factor(ycov) z with
        z = RandomState(seed).normal(size=(nylm, nsamples)) -- the constructor's ``seed`` when ``seed`` is None,
        which is what the reference draws on a fresh instance.  Not implemented for normalized or
        time-variable processes, as in the reference."""
        e = self._engine
        ymu, _, ycho = self._ylm_posterior(t, flux, data_cov, i, p, u, baseline_mean, baseline_var, True)
        z = self._rng(seed).normal(size=(self._nylm, int(nsamples)))
        out = e.gemm_nt(e.f64(np.ascontiguousarray(z.T)), ycho)      # (ycho z)^T
        out += ymu[None, :]
        return Eager(out.cpu().numpy())

    # -- posterior of the surface map of a time-variable process --------------------------------------
    # y(t) = mu_y + d(t) with cov(d(t), d(t')) = k(t, t', tau) Sigma_y, the model of cov() / log_likelihood on the
    # conditional branch (sp.py:696-698, 1135-1157): C = (A Sigma_y A^T) o k(t, t) + data_cov + baseline_var 1 1^T.
    # With B = A Sigma_y, alpha = C^-1 (flux - baseline_mean - A mu_y) and k_j = k(t*_j, t, tau), frame t*_j has
    # ymu_j = mu_y + B^T (k_j o alpha) and ycov_j = Sigma_y - B^T (C^-1 o k_j k_j^T) B (sp_ylm_conditional_temporal).
    def _ylm_temporal_args(self, t, flux, data_cov, t_map, baseline_mean, baseline_var, matrix_ok):
        """The checked host arguments (t [K], flux [K], data_cov, t_map [T], baseline_mean, baseline_var): every error
        of the two methods below is raised here, before any device work."""
        if self._normalized:
            raise NotImplementedError("Method not implemented when the flux is normalized.")
        if not self._time_variable:
            raise NotImplementedError("Method implemented for time-variable maps only (tau=...): use `ylm_conditional` "
                                      "for a static map.")
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1))
        K = t.shape[0]
        if K < 1:
            raise ValueError("`t` must hold at least one time")
        flux = np.asarray(flux, dtype=np.float64)
        if flux.shape != (K,):
            raise ValueError("`flux` must have one value per time: shape (%d,), not %s" % (K, flux.shape))
        if t_map is None:
            t_map = t
        else:
            t_map = np.asarray(t_map, dtype=np.float64)
            if t_map.ndim != 1:
                raise ValueError("`t_map` must be 1-D: one time per frame")
            t_map = np.ascontiguousarray(t_map)
        data_cov = np.asarray(data_cov, dtype=np.float64)
        if data_cov.ndim == 2 and not matrix_ok:
            raise ValueError("`data_cov` must be a scalar or (K,) here: the noise draw needs independent cadences")
        if data_cov.ndim > 2 or (data_cov.ndim == 1 and data_cov.shape != (K,)) or \
                (data_cov.ndim == 2 and data_cov.shape != (K, K)):
            raise ValueError("`data_cov` must be a scalar, (K,) or (K, K) with K = %d, not %s" % (K, data_cov.shape))
        bmean, bvar = np.asarray(baseline_mean, dtype=np.float64), np.asarray(baseline_var, dtype=np.float64)
        if bmean.ndim != 0 or bvar.ndim != 0:
            raise ValueError("`baseline_mean` and `baseline_var` must be scalars")
        return t, flux, data_cov, t_map, float(bmean), float(bvar)

    def _ylm_temporal_system(self, t, flux, data_cov, i, p, u, bmean, bvar):
        """(A [K, N], C [K, K], r0 [K] = flux - baseline_mean - A mu_y, Sigma_y, mu_y) on the device."""
        e, f = self._engine, self._flux
        t, i, p, u = f._ingest(t, i, p, u)
        f._bind()
        rta1 = f._rta1(u)
        mu, Sig = (e.f64(x) for x in self._moments_dev())
        A = e.design_matrix(t[None, :], make_stars(1, period=p, inc_deg=i), rta1)[0]
        C, _, _ = e.cov_conditional(t[None, :], make_stars(1, period=p, inc_deg=i, tau=self._tau), rta1,
                                    temporal=self._temporal, normalized=False)
        C = C[0]
        if data_cov.ndim == 2:
            C += e.f64(data_cov)
        else:
            C.diagonal().add_(e.f64(data_cov) if data_cov.ndim else float(data_cov))
        C += bvar
        r0 = e.f64(flux - bmean) - e.gemm_nt(mu.reshape(1, -1), A)[0]
        return A, C, r0, Sig, mu

    def ylm_conditional_temporal(self, t, flux, data_cov, t_map=None, i=defaults["i"], p=defaults["p"],
                                 u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                                 baseline_var=defaults["baseline_var"], return_cov=True):
        """Posterior of the surface map of a time-variable process at the frame times ``t_map`` (default: the observed
        times ``t``), conditioned on the observed flux: (ymu (T, nylm), ycov (T, nylm, nylm)), frame by frame the
        Gaussian of the spherical-harmonic coefficients at that time, each covariance exactly symmetric;
        ``return_cov=False`` returns ymu alone and forms nothing nylm x nylm per frame.  The reference leaves this case
        open (its sp.py:602-605); the model is that of its conditional likelihood: maps y(t) = mean_ylm + d(t) with
        cov(d(t), d(t')) = k(t, t', tau) cov_ylm.  ``data_cov`` is a scalar, (K,) or (K, K); ``baseline_var`` a scalar.
        Frames are independent marginals: for a coherent movie use ``sample_ylm_conditional_temporal``.  NaN everywhere
        if the flux covariance is not positive definite; nothing is raised.  NotImplementedError for a normalized
        process and for one without ``tau`` (use ``ylm_conditional``); ValueError for arguments of the wrong shape."""
        t, flux, data_cov, t_map, bmean, bvar = self._ylm_temporal_args(t, flux, data_cov, t_map, baseline_mean,
                                                                        baseline_var, True)
        e = self._engine
        A, C, r0, Sig, mu = self._ylm_temporal_system(t, flux, data_cov, i, p, u, bmean, bvar)
        out, ycov, _ = e.ylm_conditional_temporal(A, Sig, C, r0[None, :], t, t_map, self._tau, self._temporal,
                                                  with_cov=bool(return_cov))
        ymu = out[0] + mu[None, :]
        if not return_cov:
            return Eager(ymu.cpu().numpy())
        return Eager(ymu.cpu().numpy()), Eager(ycov.cpu().numpy())

    def sample_ylm_conditional_temporal(self, t, flux, data_cov, t_map=None, i=defaults["i"], p=defaults["p"],
                                        u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                                        baseline_var=defaults["baseline_var"], nsamples=1, seed=None):
        """Surface movies conditioned on the observed flux, shape (nsamples, T, nylm): what ``flux(y, t_map)`` and
        ``mollweide(y)`` take.  The frames of one sample are coherent in time (pathwise conditioning, Matheron's rule):
        a prior movie y0 on the union of the observed and the frame times and a noise vector eps are drawn, and the
        sample is y0(t*_j) + mean_ylm + B^T (k_j o C^-1 (flux - baseline_mean - A mean_ylm - f0 - eps)) with
        f0_k = A_k . y0(t_k), in the notation of ``ylm_conditional_temporal``, whose Gaussian every frame follows.
        ``data_cov`` is a scalar or (K,) (a matrix raises ValueError).

        The deviates come from rng = RandomState(seed) -- the constructor's ``seed`` when ``seed`` is None -- in this
        order: (1) U = rng.normal(size=(nsamples, Nu, nylm)), Nu the number of distinct values among ``t`` and
        ``t_map``, for the prior movie Lt U Ly^T on those sorted distinct times, as ``sample_ylm(t)`` forms it (zero
        mean); (2) rng.normal(size=(nsamples, K)), times sqrt(data_cov); (3) only when baseline_var > 0,
        rng.normal(size=(nsamples,)), times sqrt(baseline_var).

        If the temporal kernel's Gram matrix on the union times does not factor (the exp-squared kernel on a dense
        cadence, times that differ by rounding only) every sample is NaN, as ``sample_ylm(t)``; nothing is raised."""
        t, flux, data_cov, t_map, bmean, bvar = self._ylm_temporal_args(t, flux, data_cov, t_map, baseline_mean,
                                                                        baseline_var, False)
        import torch

        e = self._engine
        ns, K = int(nsamples), t.shape[0]
        tu = np.unique(np.concatenate([t, t_map]))
        rng = self._rng(seed)
        U = rng.normal(size=(ns, tu.shape[0], self._nylm))
        with np.errstate(invalid="ignore"):
            eps = rng.normal(size=(ns, K)) * np.sqrt(data_cov)
            if bvar > 0:
                eps = eps + (rng.normal(size=(ns,)) * np.sqrt(bvar))[:, None]
        A, C, r0, Sig, mu = self._ylm_temporal_system(t, flux, data_cov, i, p, u, bmean, bvar)
        Lt, _ = e.temporal_gram(tu, self._tau, self._temporal)
        y0 = e.ylm_temporal(Lt, self._cho_ylm_dev(), U)        # (ns, Nu, nylm); all NaN if a factorisation failed
        at_t = torch.from_numpy(np.searchsorted(tu, t)).to(e.device)
        at_map = torch.from_numpy(np.searchsorted(tu, t_map)).to(e.device)
        f0 = e.flux_rows(A, y0[:, at_t, :].contiguous())
        resid = r0[None, :] - f0 - e.f64(eps)
        out, _, _ = e.ylm_conditional_temporal(A, Sig, C, resid, t, t_map, self._tau, self._temporal, with_cov=False)
        out += y0[:, at_map, :]
        out += mu[None, None, :]
        return Eager(out.cpu().numpy())

    def _ensemble_args(self, t, flux, data_cov, i, p, u, baseline_mean, baseline_var, nobs=0):
        """Inputs of the ensemble calls, checked against flux's (S, K) shape: t (S, K) contiguous, the star records
        (period, inclination, baselines, scalar variances, limb-darkening table, nobs), the distinct limb-darkening
        sets utab and the per-cadence variances diag ((S, K) or None)."""
        flux = np.asarray(flux, dtype=np.float64)
        if flux.ndim != 2:
            raise ValueError("`flux` must be (S, K)")
        check_period_inclination(p, i)
        t, stars, utab, diag = ensemble_stars(flux.shape, t, p, i, u, self._udeg, baseline_mean, baseline_var, data_cov,
                                              tau=self._tau, nobs=nobs)
        return t, flux, stars, utab, diag

    def ylm_conditional_ensemble(self, t, flux, data_cov, i=None, p=None, u=None, baseline_mean=0.0,
                                 baseline_var=0.0, nsamples=0, seed=None):
        """Posteriors of the surface maps of S stars in one device call.

        t: (K,) or (S, K); flux: (S, K); data_cov: scalar, (S,) or (S, K); i, p: scalars or (S,);
        u: (udeg,) shared or (S, udeg); baseline_mean, baseline_var: scalars or (S,).
        Returns (ymu (S, nylm), ycov (S, nylm, nylm)) and, with nsamples > 0, samples (S, nsamples, nylm)
        drawn with z = RandomState(seed).normal(size=(S, nylm, nsamples))."""
        self._ylm_check()
        e = self._engine
        t, flux, stars, utab, diag = self._ensemble_args(t, flux, data_cov, i, p, u, baseline_mean, baseline_var)
        S = flux.shape[0]
        sinv, sinvmu = self._ylm_precision()
        rta1 = e.f64(e.rTA1L(utab))
        nsamples = int(nsamples)
        ymu, ycov, ycho, _ = e.ylm_conditional(t, flux, stars, rta1, sinv, sinvmu, diag=diag,
                                               with_cho=nsamples > 0)
        # stars with a variance <= 0 (or not a number): C = D + b 1 1^T may still be positive definite, which
        # the kernel's rule does not decide -- they take the exact route of a full data covariance
        var = diag if diag is not None else stars["data_var"][:, None]
        incs = np.broadcast_to(np.asarray(defaults["i"] if i is None else i, dtype=np.float64), (S,))
        for s_ in np.nonzero(~np.all(var > 0, axis=1))[0]:
            a = _star_fallback_args(s_, t, flux, stars, utab, diag)
            m1, c1, l1 = self._ylm_posterior(*a[:3], incs[s_], *a[3:], nsamples > 0, full=True)
            ymu[s_], ycov[s_] = m1, c1
            if ycho is not None:
                ycho[s_] = l1
        out = (Eager(ymu.cpu().numpy()), Eager(ycov.cpu().numpy()))
        if nsamples > 0:
            z = self._rng(seed).normal(size=(S, self._nylm, nsamples))
            out = out + (Eager(_affine_samples(e, ymu, ycho, z).cpu().numpy()),)
        return out

    def log_likelihood_ensemble(self, t, flux, data_cov, i=None, p=None, u=None,
                                baseline_mean=0.0, baseline_var=0.0):
        """Per-star log-likelihoods of S independent stars in one device call.

        t: (K,) or (S, K); flux: (S, K); data_cov: scalar, (S,) or (S, K);
        i, p: scalars or (S,); u: (udeg,) shared or (S, udeg).

        Ragged ensembles: ``t`` and ``flux`` may be lists of S 1-D arrays of different
        lengths (and ``data_cov`` a list of per-cadence variance vectors): the light
        curves are padded to the longest and each star is evaluated on its own cadences
        only (``sp_star.nobs``)."""
        e = self._engine
        nobs = 0
        if isinstance(flux, (list, tuple)) and len(flux) == 0:
            return Eager(np.empty(0))
        if isinstance(flux, (list, tuple)):
            S = len(flux)
            lens = np.array([np.size(x) for x in flux], dtype=np.int32)
            K = int(lens.max())
            if not isinstance(t, (list, tuple)) or len(t) != S or any(np.size(a) != n for a, n in zip(t, lens)):
                raise ValueError("ragged ensembles need one time array per light curve, of the same length")
            tp = np.empty((S, K))
            fp = np.zeros((S, K))
            for s_ in range(S):
                n_ = int(lens[s_])
                tp[s_, :n_] = np.asarray(t[s_], dtype=np.float64).reshape(-1)
                tp[s_, n_:] = tp[s_, n_ - 1]
                fp[s_, :n_] = np.asarray(flux[s_], dtype=np.float64).reshape(-1)
            if isinstance(data_cov, (list, tuple)) and np.ndim(data_cov[0]) == 1:
                dp = np.ones((S, K))
                for s_ in range(S):
                    dp[s_, : lens[s_]] = np.asarray(data_cov[s_], dtype=np.float64)
                data_cov = dp
            t, flux, nobs = tp, fp, lens
        t, flux, stars, utab, diag = self._ensemble_args(t, flux, data_cov, i, p, u, baseline_mean, baseline_var,
                                                         nobs=nobs)
        if diag is not None:
            diag = e.f64(diag)
        branch = self._branch(utab)
        out, status = e.lnlike_ensemble(e.f64(np.ascontiguousarray(t)), e.f64(flux[:, None, :]),
                                        e.stars_to_device(stars), diag=diag, **branch)
        return Eager(_neg_inf_if_nan(out.cpu().numpy()))

    # -- conditional likelihood on a grid of inclinations (calibrate/inclination.py:9-76) ------------------
    # The conditional branch (sp.py:1052-1188 with marginalize_over_inclination=False) at P inclinations in one
    # device call, whatever marginalize_over_inclination says (as ylm_conditional).  The flux covariance at one
    # inclination has rank 2 ydeg + 1 (sp_lnlike_inclinations).  What that route cannot take -- a
    # time-variable process, a full data covariance or baseline_var matrix, a variance <= 0, a star with fewer
    # distinct phases than 2 ydeg + 1 or with too little of the rotation covered (SP_STAR_NO_BASIS) -- takes the
    # dense conditional path on one system per inclination.
    def _check_inc(self, inc):
        inc = np.atleast_1d(np.asarray(inc, dtype=np.float64)).reshape(-1)
        if np.any(inc * np.pi / 180 < -1e-6) or np.any(inc * np.pi / 180 > 0.5 * np.pi + 1e-6):
            raise ValueError("inc out of bounds")
        return inc

    def _incl_dense(self, t, F, data_cov, inc, p, u, baseline_mean, baseline_var, chunk=16):
        """(P,) by the dense conditional path: sp_cov_conditional_batched on one system per inclination, then the
        data and baseline terms and sp_cholesky_lnlike_batched (log_likelihood's general path)."""
        e, f = self._engine, self._flux
        f._bind()
        K = t.shape[0]
        rta1 = f._rta1(u)
        data_cov = np.asarray(data_cov, dtype=np.float64)
        bmean, bvar = np.asarray(baseline_mean, dtype=np.float64), np.asarray(baseline_var, dtype=np.float64)
        Fd = e.f64(np.asarray(F, dtype=np.float64).reshape(-1, K))
        out = np.empty(inc.shape[0])
        for c0 in range(0, inc.shape[0], chunk):
            ii = inc[c0:c0 + chunk]
            n = ii.shape[0]
            stars = make_stars(n, period=p, inc_deg=ii, tau=self._tau)
            cov, mean, z = e.cov_conditional(np.broadcast_to(t, (n, K)), stars, rta1, temporal=self._temporal,
                                             normalized=self._normalized, norm_order=self._normN)
            if data_cov.ndim == 0:
                cov.diagonal(dim1=1, dim2=2).add_(float(data_cov))
            elif data_cov.ndim == 1:
                cov.diagonal(dim1=1, dim2=2).add_(e.f64(data_cov))
            else:
                cov += e.f64(data_cov)
            cov += e.f64(bvar) if bvar.ndim else float(bvar)
            gp = 0.0 if self._normalized else mean[:, None, None]
            resid = Fd[None, :, :] - (gp + (e.f64(bmean) if bmean.ndim else float(bmean)))
            # one residual per system: a normalised process subtracts no per-inclination mean, which leaves batch 1
            val, _ = e.cholesky_lnlike(cov, resid.expand(n, -1, -1).contiguous())
            val = val.cpu().numpy()
            if self._normalized:
                val = np.where(z.cpu().numpy() > self._normzmax, -np.inf, val)
            out[c0:c0 + n] = _neg_inf_if_nan(val)
        return out

    def _incl_basis(self, t, F, stars, utab, diag, inc):
        """(lnlike [S, P], status [S, P]) of the basis route for t [S, K], F [S, M, K]."""
        e = self._engine
        mu, cov = self._moments_dev()
        out, status = e.lnlike_inclinations(t, F, stars, e.rTA1L(utab), mu, cov, inc * (np.pi / 180), diag=diag,
                                            normalized=self._normalized, norm_order=self._normN, zmax=self._normzmax)
        return out[:, 0, :].cpu().numpy(), status[:, 0, :].cpu().numpy()

    def log_likelihood_inclinations(self, t, flux, data_cov, inc=np.linspace(0, 90, 100), p=defaults["p"],
                                    u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                                    baseline_var=defaults["baseline_var"]):
        """``log_likelihood(t, flux, data_cov, i, p, u, baseline_mean, baseline_var)`` of the conditional branch at
        every inclination of ``inc`` (degrees): shape (P,).  ``flux`` is (K,) or (M, K) light curves of one star."""
        from ._lib import SP_STAR_NO_BASIS

        f = self._flux
        inc = self._check_inc(inc)
        t, _, p, u = f._ingest(t, 60.0, p, u)
        K = t.shape[0]
        F = np.asarray(flux, dtype=np.float64).reshape(-1, K)
        data_cov = np.asarray(data_cov, dtype=np.float64)
        bmean, bvar = np.asarray(baseline_mean, dtype=np.float64), np.asarray(baseline_var, dtype=np.float64)
        fast = (not self._time_variable and data_cov.ndim <= 1 and bmean.ndim == 0 and bvar.ndim == 0
                and np.all(data_cov > 0) and np.all(np.isfinite(data_cov)))
        if fast:
            stars, diag = _one_star_noise(1, K, data_cov, period=p, baseline_var=float(bvar),
                                          baseline_mean=float(bmean))
            val, status = self._incl_basis(t[None, :], F[None, :, :], stars, u[None, :], diag, inc)
            if not np.any(status[0] & SP_STAR_NO_BASIS):
                return Eager(_neg_inf_if_nan(val[0]))
        return Eager(self._incl_dense(t, F, data_cov, inc, p, u, bmean, bvar))

    def log_likelihood_inclinations_ensemble(self, t, flux, data_cov, inc=np.linspace(0, 90, 100), p=None, u=None,
                                             baseline_mean=0.0, baseline_var=0.0):
        """``log_likelihood_inclinations`` of S stars in one device call: shape (S, P).

        t: (K,) or (S, K); flux: (S, K); data_cov: scalar, (S,) or (S, K); p: scalar or (S,);
        u: (udeg,) shared or (S, udeg); baseline_mean, baseline_var: scalars or (S,)."""
        from ._lib import SP_STAR_NO_BASIS

        inc = self._check_inc(inc)
        t, flux, stars, utab, diag = self._ensemble_args(t, flux, data_cov, None, p, u, baseline_mean, baseline_var)
        S, P = flux.shape[0], inc.shape[0]
        var = diag if diag is not None else stars["data_var"][:, None]
        dense = ~np.all((var > 0) & np.isfinite(var), axis=1)
        out = np.empty((S, P))
        if not self._time_variable:
            val, status = self._incl_basis(t, flux[:, None, :], stars, utab, diag, inc)
            out[:] = _neg_inf_if_nan(val)
            dense |= np.any(status & SP_STAR_NO_BASIS, axis=1)
        else:
            dense[:] = True
        for s_ in np.nonzero(dense)[0]:
            a = _star_fallback_args(s_, t, flux, stars, utab, diag)
            out[s_] = self._incl_dense(a[0], a[1][None, :], a[2], inc, *a[3:])
        return Eager(out)

    # -- surface maps with the inclination marginalised on a grid ------------------------------------
    # The posterior of the map when the inclination is unknown: the mixture of the conditional Gaussians of
    # ylm_conditional over the grid `inc`, weighted by pinc_j ~ prior_j exp(lnL_j) with lnL_j the value
    # log_likelihood_inclinations returns.  (As in the reference that likelihood subtracts the scalar flux mean, the
    # map posterior A mu_y; the two are kept as they are.)  One device call forms every component as a rank-(2 ydeg + 1)
    # downdate of the prior (sp_ylm_conditional_inclinations); a star that route cannot take (SP_STAR_NO_BASIS: a
    # variance <= 0, too few distinct phases, too little of the rotation covered) takes the dense route below.
    @staticmethod
    def _inc_prior_weights(inc, inc_weights):
        """Prior weight of each grid inclination (degrees): ``inc_weights`` if given (non-negative, (P,)), else
        sin(i_j) times the trapezoid width of grid point j (half intervals at the ends; 1 for a single point), which
        needs a strictly increasing grid."""
        P = inc.shape[0]
        if inc_weights is not None:
            w = np.asarray(inc_weights, dtype=np.float64).reshape(-1)
            if w.shape != (P,):
                raise ValueError("`inc_weights` must hold one weight per inclination")
            if not np.all(np.isfinite(w)) or np.any(w < 0) or not np.any(w > 0):
                raise ValueError("`inc_weights` must be finite, non-negative and not all zero")
            return w
        if P == 1:
            width = np.ones(1)
        else:
            d = np.diff(inc)
            if not np.all(d > 0):
                raise ValueError("the default prior sin(i) di needs a strictly increasing `inc`; pass `inc_weights`")
            width = np.empty(P)
            width[0], width[-1] = 0.5 * d[0], 0.5 * d[-1]
            width[1:-1] = 0.5 * (d[:-1] + d[1:])
        return np.maximum(np.sin(inc * np.pi / 180), 0.0) * width

    @staticmethod
    def _log_weights(w):
        with np.errstate(divide="ignore"):
            return np.log(w)

    @staticmethod
    def _mixture_components(pinc, u):
        """Component of each sample, pinc (S, P) and u (S, ns): searchsorted(cumsum(pinc_s), u_s) clipped to P - 1."""
        j = np.array([np.searchsorted(np.cumsum(w), x) for w, x in zip(pinc, u)]).reshape(u.shape)
        return np.minimum(j, pinc.shape[-1] - 1).astype(np.int32)

    def _marginal_deviates(self, S, nsamples, seed):
        """(u, z, e) of the mixture's samples, drawn in this order from one RandomState."""
        rs = self._rng(seed)
        u = rs.rand(S, nsamples)
        z = rs.normal(size=(S, nsamples, self._nylm))
        e = rs.normal(size=(S, nsamples, 2 * self._ydeg + 1))
        return u, z, e

    def _ylm_marginal_dense(self, t, flux, data_cov, inc, logw, p, u, baseline_mean, baseline_var, return_cov=True,
                            comp=None, z=None, chunk=16):
        """The mixture for one star by the dense route: ylm_conditional on (star x inclination) pseudo-stars in chunks,
        weights from the dense route of log_likelihood_inclinations, the mixture formed with torch on the device.
        Returns device tensors (pinc (P,), ymu (N,), ycov (N, N) or None, ymu_inc (P, N)) and, with ``comp`` (ns,) and
        ``z`` (ns, N), the samples ymu_j + cho(ycov_j) z (ns, N) as a fifth value."""
        import torch

        e = self._engine
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        K, P, N = t.shape[0], inc.shape[0], self._nylm
        data_cov = np.asarray(data_cov, dtype=np.float64)
        lnl = self._incl_dense(t, np.asarray(flux, dtype=np.float64)[None, :], data_cov, inc, p, u,
                               np.asarray(baseline_mean, dtype=np.float64), np.asarray(baseline_var, dtype=np.float64))
        lw = np.asarray(logw, dtype=np.float64) + lnl
        ok = np.isfinite(lw)
        pinc = np.zeros(P)
        if ok.any():
            pinc[ok] = np.exp(lw[ok] - lw[ok].max())
            pinc /= pinc.sum()
        else:
            pinc[:] = np.nan
        w = e.f64(pinc)
        positive = bool(np.all(data_cov > 0))

        def components(jj, with_cho):
            n = len(jj)
            if positive:
                stars, diag = _one_star_noise(n, K, data_cov, period=p, inc_deg=inc[jj],
                                              baseline_var=float(baseline_var), baseline_mean=float(baseline_mean))
                stars["table"][:] = 0
                sinv, sinvmu = self._ylm_precision()
                m, c, l, _ = e.ylm_conditional(np.broadcast_to(t, (n, K)), np.broadcast_to(flux, (n, K)), stars,
                                               self._flux._rta1(u), sinv, sinvmu, diag=diag, with_cho=with_cho)
                return m, c, l
            out = [self._ylm_posterior(t, flux, data_cov, inc[j], p, u, baseline_mean, baseline_var, with_cho, full=True)
                   for j in jj]
            return (torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out]),
                    torch.stack([o[2] for o in out]) if with_cho else None)

        ymui = e.empty(P, N)
        cbar = torch.zeros(N, N, dtype=torch.float64, device=e.device) if return_cov else None
        for c0 in range(0, P, chunk):
            jj = np.arange(c0, min(P, c0 + chunk))
            m, c, _ = components(jj, False)
            ymui[c0:c0 + len(jj)] = m
            if return_cov:
                for k, j in enumerate(jj):
                    if pinc[j] > 0:
                        cbar += w[j] * c[k]
        use = torch.nonzero(w > 0).reshape(-1)
        ymu = (w[use, None] * ymui[use]).sum(0) if ok.any() else torch.full_like(ymui[0], float("nan"))
        ycov = None
        if return_cov:
            d = ymui[use] - ymu[None, :]
            ycov = cbar + (w[use, None] * d).T @ d
            ycov = 0.5 * (ycov + ycov.T)
            if not ok.any():
                ycov = torch.full_like(ycov, float("nan"))
        out = (w, ymu, ycov, ymui)
        if comp is not None:
            comp = np.asarray(comp).reshape(-1)
            y = e.empty(comp.shape[0], N)
            zd = e.f64(z).reshape(comp.shape[0], N)
            for j in np.unique(comp):
                m, _, l = components(np.array([j]), True)
                rows = np.nonzero(comp == j)[0]
                y[rows] = m[0][None, :] + zd[rows] @ l[0].T
            out = out + (y,)
        return out

    def _ylm_marginal(self, t, flux, stars, utab, diag, inc, logw, return_cov, nsamples, seed, with_inc=False):
        """The mixtures of S stars: the basis route in one device call, the stars it flags by the dense route.
        Device tensors (pinc [S, P], ymu [S, N], ycov [S, N, N] or None, ymu_inc [S, P, N] or None), then the
        samples y [S, ns, N] (device) and their inclinations (host, degrees), or None, None."""
        from ._lib import SP_STAR_NO_BASIS

        e = self._engine
        S, P = flux.shape[0], inc.shape[0]
        mu, cov = self._moments_dev()
        pinc, ymu, ycov, ymui, status, state = e.ylm_conditional_inclinations(
            t, flux, stars, e.rTA1L(utab), mu, cov, inc * (np.pi / 180), logw, diag=diag, with_cov=return_cov,
            with_inc=with_inc, nsamples=nsamples)
        dense = np.nonzero(status.cpu().numpy() & SP_STAR_NO_BASIS)[0] if S else []

        def star_args(s_):
            a = _star_fallback_args(s_, t, flux, stars, utab, diag)
            return a[:3] + (inc, logw) + a[3:]

        for s_ in dense:
            w1, m1, c1, mi1 = self._ylm_marginal_dense(*star_args(s_), return_cov=return_cov)
            pinc[s_], ymu[s_] = w1, m1
            if return_cov:
                ycov[s_] = c1
            if with_inc:
                ymui[s_] = mi1
        if nsamples <= 0 or S == 0:
            return pinc, ymu, ycov, ymui, None, None
        u, z, dev = self._marginal_deviates(S, nsamples, seed)
        ph = pinc.cpu().numpy()
        comp = self._mixture_components(np.where(np.isfinite(ph), ph, 0.0), u)
        y = e.ylm_inclination_samples(state, self._cho_ylm_dev(), comp, z, dev)
        for s_ in dense:
            y[s_] = self._ylm_marginal_dense(*star_args(s_), return_cov=False, comp=comp[s_], z=z[s_])[4]
        return pinc, ymu, ycov, ymui, y, inc[comp]

    def _ylm_marginal_single(self, t, flux, data_cov, inc, p, u, baseline_mean, baseline_var, inc_weights, return_cov,
                             nsamples, seed):
        self._ylm_check()
        if np.ndim(data_cov) > 1 or np.ndim(baseline_var) > 0:
            raise NotImplementedError("a full data covariance is not implemented for the marginal map posterior; "
                                      "use ylm_conditional at each inclination")
        inc = self._check_inc(inc)
        logw = self._log_weights(self._inc_prior_weights(inc, inc_weights))
        t, _, p, u = self._flux._ingest(t, 60.0, p, u)
        flux = np.asarray(flux, dtype=np.float64).reshape(1, -1)
        if flux.shape[1] != t.shape[0]:
            raise ValueError("`flux` must have one value per time")
        dc = np.asarray(data_cov, dtype=np.float64)
        t, flux, stars, utab, diag = self._ensemble_args(t, flux, dc if dc.ndim == 0 else dc[None, :], None, p, u,
                                                         baseline_mean, baseline_var)
        return self._ylm_marginal(t, flux, stars, utab, diag, inc, logw, return_cov, int(nsamples), seed)

    def ylm_conditional_marginal(self, t, flux, data_cov, inc=np.linspace(0, 90, 100), p=defaults["p"],
                                 u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                                 baseline_var=defaults["baseline_var"], inc_weights=None, return_cov=True):
        """The surface map's posterior with the inclination marginalised on the grid ``inc`` (degrees): mean (nylm,),
        covariance (nylm, nylm) and ``pinc`` (P,), the posterior weight of each grid inclination (sums to 1); with
        ``return_cov=False`` only (ymu, pinc).  The posterior is the mixture of ``ylm_conditional`` over the grid:
        ymu = sum_j pinc_j ymu_j, ycov = sum_j pinc_j (ycov_j + (ymu_j - ymu)(ymu_j - ymu)^T), with
        pinc_j ~ prior_j exp(log_likelihood_inclinations_j).  The prior weight of grid point j is ``inc_weights[j]``
        (non-negative) or, by default, sin(i_j) times the trapezoid width of the point (an isotropic orientation; the
        grid must then increase strictly).  ``data_cov`` is a scalar or a vector of variances; a full matrix raises
        NotImplementedError (use ``ylm_conditional`` per inclination).  Not implemented for normalized or
        time-variable processes."""
        pinc, ymu, ycov, _, _, _ = self._ylm_marginal_single(t, flux, data_cov, inc, p, u, baseline_mean, baseline_var,
                                                             inc_weights, return_cov, 0, None)
        if return_cov:
            return Eager(ymu[0].cpu().numpy()), Eager(ycov[0].cpu().numpy()), Eager(pinc[0].cpu().numpy())
        return Eager(ymu[0].cpu().numpy()), Eager(pinc[0].cpu().numpy())

    def sample_ylm_conditional_marginal(self, t, flux, data_cov, inc=np.linspace(0, 90, 100), p=defaults["p"],
                                        u=defaults["u"][: defaults["udeg"]], baseline_mean=defaults["baseline_mean"],
                                        baseline_var=defaults["baseline_var"], inc_weights=None, nsamples=1, seed=None):
        """Samples of the surface map given the light curve with the inclination marginalised: (y (nsamples, nylm),
        inc_deg (nsamples,)), the map and the grid inclination it was drawn at.  The deviates come from one
        ``RandomState(seed)`` (the constructor's ``seed`` when None) in this order: ``u = rand(nsamples)`` chooses the
        components, j = searchsorted(cumsum(pinc), u) clipped to P - 1; ``z = normal(size=(nsamples, nylm))``;
        ``e = normal(size=(nsamples, 2 ydeg + 1))``.  Each sample is y0 + U_j^T (Z_j (hhat - B_j y0) - L_H,j^-1 e)
        with y0 = mean_ylm + cho_cov_ylm z (pathwise conditioning).  A light curve only the dense route
        can take is sampled as ymu_j + cho(ycov_j) z."""
        _, _, _, _, y, inc_s = self._ylm_marginal_single(t, flux, data_cov, inc, p, u, baseline_mean, baseline_var,
                                                         inc_weights, False, int(nsamples), seed)
        if y is None:
            return Eager(np.empty((0, self._nylm))), Eager(np.empty(0))
        return Eager(y[0].cpu().numpy()), Eager(inc_s[0])

    def ylm_conditional_marginal_ensemble(self, t, flux, data_cov, inc=np.linspace(0, 90, 100), p=None, u=None,
                                          baseline_mean=0.0, baseline_var=0.0, inc_weights=None, return_cov=True,
                                          nsamples=0, seed=None):
        """``ylm_conditional_marginal`` of S stars in one device call, one grid for all stars.

        t: (K,) or (S, K); flux: (S, K); data_cov: scalar, (S,) or (S, K); p: scalar or (S,); u: (udeg,) shared or
        (S, udeg); baseline_mean, baseline_var: scalars or (S,).
        Returns (ymu (S, nylm), ycov (S, nylm, nylm), pinc (S, P)) -- (ymu, pinc) with ``return_cov=False`` -- and, with
        nsamples > 0, also y (S, nsamples, nylm) and inc_deg (S, nsamples), drawn as sample_ylm_conditional_marginal
        does with a leading S axis on every deviate: rand(S, nsamples), normal(size=(S, nsamples, nylm)),
        normal(size=(S, nsamples, 2 ydeg + 1))."""
        self._ylm_check()
        if np.ndim(data_cov) > 2:
            raise NotImplementedError("a full data covariance is not implemented for the marginal map posterior; "
                                      "use ylm_conditional at each inclination")
        inc = self._check_inc(inc)
        logw = self._log_weights(self._inc_prior_weights(inc, inc_weights))
        t, flux, stars, utab, diag = self._ensemble_args(t, flux, data_cov, None, p, u, baseline_mean, baseline_var)
        pinc, ymu, ycov, _, y, inc_s = self._ylm_marginal(t, flux, stars, utab, diag, inc, logw, return_cov,
                                                          int(nsamples), seed)
        out = (Eager(ymu.cpu().numpy()),) + ((Eager(ycov.cpu().numpy()),) if return_cov else ())
        out = out + (Eager(pinc.cpu().numpy()),)
        if y is not None:
            out = out + (Eager(y.cpu().numpy()), Eager(inc_s))
        return out


class StarryProcessSum(StarryProcess):
    """Sum of independent processes (several spot populations on one star): the moments of
    the spherical-harmonic vectors add (sp.py:1335-1400); everything downstream -- flux mean
    and covariance, log-likelihood, prediction -- is the base class on the summed moments."""

    def __init__(self, first, second):
        if not isinstance(second, StarryProcess):
            raise AssertionError("Can only add instances of `StarryProcess` to each other.")
        for name, what in (("_ydeg", "ydeg"), ("_udeg", "udeg"), ("_normalized", "normalized"),
                           ("_marginalize_over_inclination", "marginalize_over_inclination"),
                           ("_covpts", "covpts")):
            assert getattr(first, name) == getattr(second, name), "Mismatch in `%s`." % what
        assert not first._time_variable and not second._time_variable, (
            "Sums of `StarryProcess` instances not implemented for time-variable surfaces.")
        kwargs = dict(first._kwargs)
        kwargs.pop("upstream", None)
        StarryProcess.__init__(
            self,
            mean_ylm=first._mean_ylm + second._mean_ylm,
            cov_ylm=first._cov_ylm + second._cov_ylm,
            marginalize_over_inclination=first._marginalize_over_inclination,
            normalized=first._normalized,
            covpts=first._covpts,
            **kwargs,
        )
        # hyperparameters are those of the children, not of the sum
        self._r = self._dr = self._a = self._b = self._c = self._n = None
        self._children = []
        for child in (first, second):
            self._children += getattr(child, "_children", [child])

    def log_jac(self):
        raise NotImplementedError("the latitude Jacobian is defined per child process")

    UPSTREAM_KEYS = ("epsy", "epsy15", "spts", "eps4", "smoothing", "sfac", "cutoff", "abmin", "log_alpha_max",
                     "log_beta_max")

    def log_likelihood_samples(
        self,
        t,
        flux,
        data_cov,
        samples,
        i=defaults["i"],
        p=defaults["p"],
        u=defaults["u"][: defaults["udeg"]],
        baseline_mean=defaults["baseline_mean"],
        baseline_var=defaults["baseline_var"],
        depth=6,
        out_of_bounds="raise",
        params=None,
    ):
        """``log_likelihood`` of a sum of C spot populations with THIS sum's settings at many hyperparameter vectors:
        samples (ns, 5 C [+ extras]), a block (r, a, b, c, n) per child in the order of the sum, -> (ns,) values, each
        what ``(StarryProcess(<row 1>, upstream="device") + StarryProcess(<row 2>, upstream="device") +
        ...).log_likelihood(...)`` returns.  ``params`` names the columns: by default r1, a1, b1, c1, n1, r2, ..., and in
        any order those and, each at most once, "dr1" ... "drC", "baseline_mean", "baseline_log_var", "i", "p"
        (``stars.SampleColumns(populations=C)``).  Every child keeps the dr of its own constructor unless a drK column
        overrides it.  Batched and sample-by-sample routes, ``depth`` and ``out_of_bounds`` as the base class's (the
        batched step: sp_polar_moments_samples_sum / sp_ylm_moments_samples_sum).  ValueError for a batch with the wrong
        number of columns, a child built from ``mean_ylm`` / ``cov_ylm`` (it has no hyperparameters to sample) and
        children that disagree in the upstream keywords (``epsy``, ``spts``, ...)."""
        C = len(self._children)
        if not all(ch._from_hyper for ch in self._children):
            raise ValueError("a child of this sum was built from mean_ylm / cov_ylm: it has no hyperparameters to sample")
        first = self._children[0]._kwargs
        for ch in self._children[1:]:
            for key in self.UPSTREAM_KEYS:
                if (key in first) != (key in ch._kwargs) or (key in first and first[key] != ch._kwargs[key]):
                    raise ValueError("the children of this sum disagree in the upstream keyword `%s`" % key)
        each = [ch._dr for ch in self._children]
        if params is None:
            params = SampleColumns(dr=each, populations=C).names
        cols = SampleColumns.from_params(params, self._marginalize_over_inclination, False, dr=each, populations=C)
        return self._log_likelihood_samples(cols, t, flux, data_cov, samples, i, p, u, baseline_mean, baseline_var, depth,
                                            out_of_bounds)

    def _sample_process(self, cols, hyper, dr, kw):
        """The sum of one sample's C populations, each built on the device: ``hyper`` [C, 5], ``dr`` None or [C]."""
        total = None
        for q, (r, a, b, c, n) in enumerate(hyper):
            one = dr is None or (cols.dr[q] is None)          # (a population without a spread keeps dr=None)
            child = StarryProcess(r=r, dr=None if one else dr[q], a=a, b=b, c=c, n=n, **kw)
            total = child if total is None else total + child
        return total
