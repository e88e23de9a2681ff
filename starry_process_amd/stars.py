"""
Host side of the batched calls (NumPy only): the ``sp_star`` records of an ensemble of light curves and the parameter
rows of a batch of hyperparameter samples, whose column layout ``SampleColumns`` alone knows.  Every batched front end
-- ``StarryProcess``'s ensemble methods, ``calibrate.EnsembleLogProb``, the two ensemble gradients of ``grad.py`` --
builds its records here; ``engine.py`` re-exports the names.
"""
import numpy as np

from ._lib import STAR_DTYPE
from .defaults import defaults

__all__ = ["make_stars", "ensemble_stars", "check_period_inclination", "stars_for_samples", "sample_parameters",
           "samples_in_bounds", "ipt_in_bounds", "SampleColumns"]


def make_stars(S, period=1.0, inc_deg=60.0, tau=0.0, baseline_var=0.0,
               baseline_mean=0.0, data_var=0.0, table=0, nobs=0):
    """Structured host array of ``sp_star`` (inclination converted to radians,
    flux.py:236-238).  ``nobs``: valid cadences per star for ragged ensembles (0 = all)."""
    st = np.zeros(S, dtype=STAR_DTYPE)
    st["period"] = period
    st["inc"] = np.asarray(inc_deg, dtype=float) * (np.pi / 180)
    st["tau"] = tau
    st["baseline_var"] = baseline_var
    st["baseline_mean"] = baseline_mean
    st["data_var"] = data_var
    st["table"] = table
    st["nobs"] = nobs
    return st


def check_period_inclination(p, i=None):
    """The reference's bounds on the periods and, where given, the inclinations [degrees] of an ensemble (CheckBoundsOp's
    tolerance): ValueError outside.  ``None`` stands for the default, which is inside."""
    if p is not None and np.any(np.asarray(p, dtype=np.float64) < -1e-6):
        raise ValueError("p out of bounds")
    if i is not None:
        i = np.asarray(i, dtype=np.float64)
        if np.any(i * np.pi / 180 < -1e-6) or np.any(i * np.pi / 180 > 0.5 * np.pi + 1e-6):
            raise ValueError("i out of bounds")


def ensemble_stars(flux_shape, t, p, i, u, udeg, baseline_mean, baseline_var, data_var, tau=0.0, nobs=0):
    """Inputs of the ensemble calls, checked against flux's (S, K) shape: (t (S, K) contiguous, the star records, the
    distinct limb-darkening sets utab, the per-cadence variances diag ((S, K) or None)).

    t: (K,) or (S, K); p, i [degrees], baseline_mean, baseline_var: scalars or (S,), ``None`` for p or i being the
    default; u: (udeg,) shared or (S, udeg), ``None`` the default -- the stars' ``table`` indexes the rows of utab;
    data_var: a scalar or (S,) goes to the records, (S, K) comes back as diag with the records' variance 0.  No bounds
    are checked here (``check_period_inclination``)."""
    S, K = flux_shape
    t = np.asarray(t, dtype=np.float64)
    if t.shape not in ((K,), (S, K)):
        raise ValueError("`t` must be (K,) or (S, K) like `flux` (%d, %d), not %s" % (S, K, t.shape))
    t = np.ascontiguousarray(np.broadcast_to(t, (S, K)) if t.ndim == 1 else t)

    def per(x):
        return np.broadcast_to(np.asarray(x, dtype=np.float64), (S,))

    u = np.asarray(defaults["u"][:udeg] if u is None else u, dtype=np.float64)
    if u.ndim == 1:
        utab, table = u[None, :udeg], np.zeros(S, dtype=np.int32)
    elif u.ndim == 2 and u.shape[0] == S:
        utab, table = np.unique(u[:, :udeg], axis=0, return_inverse=True)
        table = table.astype(np.int32).reshape(-1)
    else:
        raise ValueError("`u` must be (udeg,) or (S, udeg)")
    data_var = np.asarray(data_var, dtype=np.float64)
    diag = None
    dvar = 0.0
    if data_var.ndim == 2:
        if data_var.shape != (S, K):
            raise ValueError("a 2-D `data_cov` must be (S, K) like `flux` (%d, %d), not %s" % (S, K, data_var.shape))
        diag = np.ascontiguousarray(data_var)
    elif data_var.ndim <= 1 and data_var.size in (1, S):
        dvar = per(data_var.reshape(-1) if data_var.ndim else data_var)
    else:
        raise ValueError("`data_cov` must be a scalar, (S,) or (S, K)")
    stars = make_stars(S, period=per(defaults["p"] if p is None else p), inc_deg=per(defaults["i"] if i is None else i),
                       tau=tau, baseline_var=per(baseline_var), baseline_mean=per(baseline_mean), data_var=dvar,
                       table=table, nobs=nobs)
    return t, stars, utab, diag


def stars_for_samples(stars, B, ntab, baseline_mean=None, baseline_var=None, period=None, inc_deg=None, tau=None,
                      own_tables=True):
    """The sp_star array of a batch of B hyperparameter samples x S stars (sample-major: system b S + s): the S stars
    repeated B times with table = b ntab + table_s, the kernel table of sample b for the star's flux operator
    (sp_kernel_table_samples' numbering).  ``baseline_mean`` / ``baseline_var`` [B]: the baseline terms of sample b
    when they are free parameters of the samples (calibrate/log_prob.py:24-47), for every star of that sample; ``period``,
    ``inc_deg`` (degrees, stored in radians like make_stars) and ``tau`` [B] likewise: the rotation period, inclination
    and timescale of sample b.  ``own_tables=False``: every sample keeps the stars' table indices (the conditional
    branch, where ``table`` selects the flux operator and there are no per-sample tables)."""
    stars = np.ascontiguousarray(stars)
    assert stars.dtype == STAR_DTYPE
    out = np.tile(stars, int(B))
    if own_tables:
        out["table"] = (np.repeat(np.arange(int(B), dtype=np.int64), stars.shape[0]) * int(ntab)
                        + out["table"]).astype(np.int32)
    for field, val in (("baseline_mean", baseline_mean), ("baseline_var", baseline_var), ("period", period),
                       ("inc", inc_deg), ("tau", tau)):
        if val is not None:
            val = np.asarray(val, dtype=np.float64).reshape(-1)
            if val.shape[0] != int(B):
                raise ValueError("%s must have one entry per sample" % field)
            out[field] = np.repeat(val * (np.pi / 180) if field == "inc" else val, stars.shape[0])
    return out


def samples_in_bounds(samples, tol=1e-6, dr=False):
    """Boolean mask of the rows of samples [B, 5] = (r [degrees], a, b, c, n) inside the reference's bounds (r in [0, 90],
    a, b in [0, 1], n >= 0, everything finite; size.py:68, latitude.py:176-197, contrast.py:21-33 through CheckBoundsOp's
    tolerance): what ``sample_parameters`` raises ValueError for.  A sampler's walkers leave the box; the log-probability
    callables can answer -inf for such rows instead of raising (``out_of_bounds="inf"``).  ``dr=True``: rows of
    (r, dr [degrees], a, b, c, n), dr in [0, 90] (size.py:120-122)."""
    sm = np.atleast_2d(np.asarray(samples, dtype=np.float64))
    ok = np.all(np.isfinite(sm), axis=1)
    if dr:
        d = sm[:, 1] * (np.pi / 180)
        ok &= (d >= -tol) & (d <= 0.5 * np.pi + tol)
        sm = np.delete(sm, 1, axis=1)
    r, a, b, n = sm[:, 0] * (np.pi / 180), sm[:, 1], sm[:, 2], sm[:, 4]
    ok &= (r >= -tol) & (r <= 0.5 * np.pi + tol) & (a >= -tol) & (a <= 1 + tol) & (b >= -tol) & (b <= 1 + tol) & (n >= -tol)
    return ok


def ipt_in_bounds(samples, order, tol=1e-6):
    """Boolean mask of the rows whose "i", "p", "tau" columns (those that ``order`` names) lie inside the reference's
    bounds: i in [0, 90] degrees and p >= 0 through CheckBoundsOp's tolerance (flux.py:233-254), tau > 0, all finite."""
    samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
    ok = np.ones(samples.shape[0], dtype=bool)
    for q in ("i", "p", "tau"):
        if q in order:
            v = samples[:, order.index(q)]
            with np.errstate(invalid="ignore"):
                if q == "i":
                    inside = (v * (np.pi / 180) >= -tol) & (v * (np.pi / 180) <= 0.5 * np.pi + tol)
                elif q == "p":
                    inside = v >= -tol
                else:
                    inside = v > 0.0
            ok &= np.isfinite(v) & inside
    return ok


class SampleColumns(object):
    """The columns of a batch of hyperparameter samples, r[, dr], a, b, c, n[, m][, v][, i][, p][, tau]: the reference's
    order (calibrate/log_prob.py:93-102: the inclination behind the baseline terms) with dr where the constructor has it
    and the two parameters of its time-variability tutorial last.  r, dr and i are in degrees, v is the log10 of the
    baseline variance.  The one place that knows which columns there are, what they are called, how a batch is taken
    apart (``split``) and which rows lie inside the reference's bounds (``in_bounds``).

    ``dr``: None (one spot radius), a number (the same spread for every sample) or "free" (a column); ``free``: which of
    FREE are columns, in any order; ValueError for settings that name no batch.  Attributes: ``dr`` (None, the float or
    "free"), ``dr_free``, ``free`` (in column order), ``names`` (the columns as ``log_likelihood_samples``' params spell
    them) and ``columns`` (the short spelling: m, v for the baseline terms).

    ``populations`` = C > 1: a sum of C independent spot populations on one star (``StarryProcessSum``).  The
    hyperparameter block repeats per population and its names carry the population's number, r1[, dr1], a1, b1, c1, n1,
    r2, ..., followed by the free terms as above.  ``dr`` is then one setting for all populations or a sequence of C
    settings, and the attributes ``dr`` and ``dr_free`` are tuples of C."""

    FREE = ("baseline_mean", "baseline_log_var", "i", "p", "tau")
    SHORT = {"baseline_mean": "m", "baseline_log_var": "v"}
    FIELDS = {"baseline_mean": "baseline_mean", "baseline_log_var": "baseline_var", "i": "inc_deg", "p": "period",
              "tau": "tau"}          # stars_for_samples' keywords
    HYPER = ("r", "dr", "a", "b", "c", "n")

    def __init__(self, dr=None, free=(), conditional=False, temporal=None, params=None, populations=1):
        free = (free,) if isinstance(free, str) else tuple(free)
        if len(set(free)) != len(free) or any(f not in self.FREE for f in free):
            raise ValueError("free must be a subset of %r" % (self.FREE,))
        C = int(populations)
        if C < 1:
            raise ValueError("populations must be at least 1")
        if C > 1 and isinstance(dr, (list, tuple, np.ndarray)):
            if len(dr) != C:
                raise ValueError("dr must be one setting or one per population (%d)" % C)
            settings = [self._dr_setting(d) for d in dr]
        else:
            settings = [self._dr_setting(dr)] * C
        if "i" in free and not conditional:
            raise ValueError("a free inclination needs conditional=True: the marginal branch integrates over it")
        if "tau" in free and temporal is None:
            raise ValueError("a free tau needs a temporal kernel")
        self.populations = C
        if C == 1:
            self.dr, self.dr_free = settings[0], isinstance(settings[0], str)
        else:
            self.dr, self.dr_free = tuple(settings), tuple(isinstance(d, str) for d in settings)
        self.free = tuple(f for f in self.FREE if f in free)
        self.names = self.hyper_names(C, [isinstance(d, str) for d in settings]) + self.free
        self.columns = tuple(self.SHORT.get(q, q) for q in self.names)
        # (a caller's own order of the same names: samples[:, permutation] has the columns in this layout's)
        self.params = self.names if params is None else tuple(params)
        self.permutation = [self.params.index(q) for q in self.names]

    @staticmethod
    def _dr_setting(dr):
        """One population's spread: None, "free" or a number of degrees inside [0, 90] (ValueError otherwise)."""
        if isinstance(dr, str):
            if dr != "free":
                raise ValueError("dr must be None, a number or 'free'")
        elif dr is not None:
            from .ops import CheckBoundsOp

            dr = float(dr)
            CheckBoundsOp(name="dr", lower=0.0, upper=0.5 * np.pi)(dr * (np.pi / 180))
        return dr

    @classmethod
    def hyper_names(cls, populations=1, dr_free=(False,)):
        """The hyperparameter columns: r[, dr], a, b, c, n, numbered per population when there are several."""
        tag = [""] if populations == 1 else ["%d" % (k + 1) for k in range(populations)]
        return tuple(q + tag[k] for k in range(populations) for q in cls.HYPER if q != "dr" or dr_free[k])

    @classmethod
    def from_params(cls, params, marginalize_over_inclination, time_variable, dr=None, populations=1):
        """The layout that ``log_likelihood_samples``' ``params`` name, in whatever order, on a process of these two
        settings and this spot-size spread ``dr`` (None or a number: what holds where "dr" is no column); ``params`` keeps
        the caller's order and ``samples[:, permutation]`` has the columns in this layout's.  ValueError for an unknown or
        repeated name, a missing hyperparameter, "i" on a process that marginalises over the inclination, "tau" on one
        built without a temporal kernel.  ``populations`` = C > 1: the names are numbered (r1, dr1, a1, ..., r2, ...) and
        ``dr`` may be a sequence of C, one per population."""
        params = tuple(params)
        C = int(populations)
        every = cls.hyper_names(C, [True] * C)
        if (len(set(params)) != len(params) or any(q not in every + cls.FREE for q in params)
                or any(q not in params for q in cls.hyper_names(C, [False] * C))):
            if C == 1:
                raise ValueError("params must name r, a, b, c, n and, at most once each, dr, baseline_mean, "
                                 "baseline_log_var, i, p, tau")
            raise ValueError("params must name r, a, b, c, n of each of the %d populations (r1, a1, ..., n%d) and, at most "
                             "once each, dr1 ... dr%d, baseline_mean, baseline_log_var, i, p, tau" % (C, C, C))
        if "i" in params and marginalize_over_inclination:
            raise ValueError("params names i, but this process marginalises over the inclination")
        if "tau" in params and not time_variable:
            raise ValueError("params names tau, but this process was built without a temporal kernel (tau=None)")
        if C == 1:
            dr = "free" if "dr" in params else dr
        else:
            each = list(dr) if isinstance(dr, (list, tuple, np.ndarray)) else [dr] * C
            if len(each) != C:
                raise ValueError("dr must be one setting or one per population (%d)" % C)
            dr = ["free" if "dr%d" % (k + 1) in params else each[k] for k in range(C)]
        return cls(dr, [q for q in params if q in cls.FREE], params=params,
                   conditional=not marginalize_over_inclination, temporal=time_variable or None, populations=C)

    def _blocks(self):
        """(first column, whether dr is a column) of every population's hyperparameter block, then the first free column."""
        free, col, out = (self.dr_free,) if self.populations == 1 else self.dr_free, 0, []
        for f in free:
            out.append((col, f))
            col += 6 if f else 5
        return out, col

    def split(self, samples):
        """samples [B, len(names)] (float64, in this layout's order) -> (the rows (r, a, b, c, n) [B, 5], contiguous;
        dr: None, the constructor's number or the column [B]; the free terms as stars_for_samples takes them, [B] each:
        baseline_mean, baseline_var = 10 ** v, inc_deg [degrees], period, tau).  With C > 1 populations the rows are
        [B, C, 5] and dr is None when no population has a spread, else [B, C] with 0 where a population has none."""
        blocks, c1 = self._blocks()
        fields = {self.FIELDS[f]: 10.0 ** samples[:, k] if f == "baseline_log_var" else samples[:, k]
                  for k, f in enumerate(self.free, c1)}
        if self.populations == 1:
            c0 = 2 if self.dr_free else 1
            hyper = np.ascontiguousarray(np.hstack([samples[:, :1], samples[:, c0:c0 + 4]]))
            return hyper, samples[:, 1] if self.dr_free else self.dr, fields
        B = samples.shape[0]
        hyper = np.empty((B, self.populations, 5), dtype=np.float64)
        dr = None if all(d is None for d in self.dr) else np.zeros((B, self.populations), dtype=np.float64)
        for k, (col, f) in enumerate(blocks):
            hyper[:, k, 0] = samples[:, col]
            hyper[:, k, 1:] = samples[:, col + (2 if f else 1):col + (6 if f else 5)]
            if f:
                dr[:, k] = samples[:, col + 1]
            elif self.dr[k] is not None:
                dr[:, k] = self.dr[k]
        return hyper, dr, fields

    def take_dr(self, dr, index):
        """``split``'s dr for the samples ``index`` (an int or a slice), as the moment calls and the constructors take it:
        the constructor's setting (None or the number) where dr is no column of one population, else the rows -- [C] or
        [n, C] for C > 1 populations, None when no population has a spread."""
        if self.populations == 1:
            return dr[index] if self.dr_free else dr
        return None if dr is None else dr[index]

    def in_bounds(self, samples):
        """Boolean mask of the rows of samples (in this layout's order) inside the reference's bounds: samples_in_bounds
        of the hyperparameter columns (of every population), every column finite, ipt_in_bounds of i, p and tau."""
        samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
        ok = np.all(np.isfinite(samples), axis=1) & ipt_in_bounds(samples, self.names)
        for col, f in self._blocks()[0]:
            ok &= samples_in_bounds(samples[:, col:col + (6 if f else 5)], dr=f)
        return ok

    def check_ipt(self, samples):
        """ValueError unless every row's i, p and tau are inside their bounds: the three that sample_parameters, which
        raises for the hyperparameters, does not see."""
        if not ipt_in_bounds(samples, self.names).all():
            raise ValueError("samples out of bounds: i in [0, 90] degrees, p >= 0, tau > 0")


def sample_parameters(samples, dr=False, **kw):
    """samples [B, 5] = (r [degrees], a, b, c, n) -> [B, 5] = (r [radians], alpha, beta, c, n), what
    sp_polar_moments_samples takes: the reference's bounds (size.py:68, latitude.py:176-197, contrast.py:21-33 through
    CheckBoundsOp: ValueError outside, tolerance 1e-6) and its (a, b) -> (alpha, beta) map, for the whole batch at once
    (NumPy; one sample at a time ``upstream.ab_to_alphabeta`` does the same).  ``dr=True``: samples [B, 6] = (r, dr
    [degrees], a, b, c, n) -> [B, 6] = (r, dr [radians], alpha, beta, c, n), what sp_polar_moments_samples_spread takes
    (dr in [0, 90] degrees, size.py:120-122)."""
    sm = np.array(np.atleast_2d(np.asarray(samples, dtype=np.float64)), dtype=np.float64)
    if dr:
        if sm.ndim != 2 or sm.shape[1] != 6:
            raise ValueError("samples must be (B, 6): r, dr, a, b, c, n")
        from .ops import CheckBoundsOp

        d = sm[:, 1] * (np.pi / 180)
        CheckBoundsOp(name="dr", lower=0.0, upper=0.5 * np.pi)(d)
        if not np.all(np.isfinite(d)):
            raise ValueError("samples must be finite")
        out = np.empty_like(sm)
        out[:, [0, 2, 3, 4, 5]] = sample_parameters(np.delete(sm, 1, axis=1), **kw)
        out[:, 1] = np.clip(d, 0.0, None)
        return np.ascontiguousarray(out)
    if sm.ndim != 2 or sm.shape[1] != 5:
        raise ValueError("samples must be (B, 5): r, a, b, c, n")
    r, a, b, n = sm[:, 0] * (np.pi / 180), sm[:, 1], sm[:, 2], sm[:, 4]
    from .ops import CheckBoundsOp

    for name, v, lo, hi in (("r", r, 0.0, 0.5 * np.pi), ("a", a, 0.0, 1.0), ("b", b, 0.0, 1.0), ("n", n, 0.0, np.inf)):
        CheckBoundsOp(name=name, lower=lo, upper=hi)(v)
    if not np.all(np.isfinite(sm)):
        raise ValueError("samples must be finite")
    abmin = kw.get("abmin", defaults["abmin"])
    lam = kw.get("log_alpha_max", defaults["log_alpha_max"])
    lbm = kw.get("log_beta_max", defaults["log_beta_max"])
    a, b = np.maximum(a, abmin), np.maximum(b, abmin)
    out = np.empty_like(sm)
    out[:, 0] = np.clip(r, 0.0, None)
    out[:, 1] = np.exp(a * lam)
    out[:, 2] = np.exp(np.log(0.5) + b * (lbm - np.log(0.5)))
    out[:, 3] = sm[:, 3]
    out[:, 4] = np.clip(n, 0.0, None)
    return np.ascontiguousarray(out)
