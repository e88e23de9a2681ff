"""
Ensemble log-probability callable, the counterpart of the reference's
``calibrate.get_log_prob`` (calibrate/log_prob.py:7-106) --
what the dynesty / emcee drivers of the reference actually call.

    log_prob = get_log_prob(t, flux, ferr=1e-3, p=1.0)
    log_prob(r, a, b, c, n)                       # same positional order as the reference

The reference compiles a Theano function of the free scalars; here the returned
callable evaluates eagerly: hyperparameters -> (mu_y, Sigma_y) on the host
(``upstream.py``), then one batched device call for all light curves, which share
one covariance and ride along as extra rows of the same factorisation (the
multi-right-hand-side fast path of sp.py:1162-1171).  Argument order of the
callable (log_prob.py:93-102):  [flux,] r, a, b, c, n [, m] [, v] [, i].

``get_log_prob_ensemble`` is the per-star generalisation (own period /
inclination / limb darkening / noise per light curve, one covariance each),
sharded over the ranks of a ``torch.distributed`` job when one is initialised.

``compute_inclination_pdf`` is the reference's per-star inclination posterior (calibrate/inclination.py:9-76):
the conditional branch of ``get_log_prob`` at every (light curve, posterior sample, inclination) triple, in one
device call (``sp_lnlike_inclinations``).

``EnsembleLogProb`` is the same quantity for MANY hyperparameter samples at once
(the positions of all walkers / live points of an iteration -- emcee's
``vectorize=True``): the data stay on the GPU, the moments come from the device
upstream, and ``depth`` samples are kept in flight on separate streams.
"""
import numpy as np

from .calibrate_generate import draw_spots, generate
from .sp import StarryProcess
from .stars import SampleColumns

__all__ = ["get_log_prob", "get_log_prob_ensemble", "EnsembleLogProb", "SampleBatches", "MAX_STREAMS",
           "compute_inclination_pdf", "generate", "draw_spots"]

# Independent evaluations in flight on one GPU.  Four is where the throughput peaks; a fifth stream LOSES 10-25 %
# (108k against 120k evaluations/s at cfg3's shape, bench.py; EnsembleLogProb 0.584 -> 0.818 ms per sample with
# four likelihood streams + the upstream's own, tools/attic/elp_modes.py, round 5).  Callers' ``depth`` is clamped
# to it, with one warning.
MAX_STREAMS = 4
# ... except for steps that carry their upstream (SampleBatches: a third of a step's time on a stream is the samples'
# moments and tables, light kernels that leave the GPU to the other streams): 88-92k evaluations/s of one K = 1000
# light curve with four streams, 94-98k with five, 95-99k with six (round 6, one box, bench.bench_samples).
MAX_STREAMS_SAMPLES = 6
_warned_depth = [False]


def clamp_depth(depth, extra_streams=0, limit=None):
    """``depth`` likelihood streams + ``extra_streams`` others, held to MAX_STREAMS (``limit``) concurrent streams."""
    import warnings

    depth = max(1, int(depth))
    allowed = max(1, (MAX_STREAMS if limit is None else int(limit)) - int(extra_streams))
    if depth > allowed:
        if not _warned_depth[0]:
            warnings.warn("starry_process_amd: depth=%d (+%d) exceeds %d concurrent streams, beyond which the GPU's "
                          "throughput DROPS by 10-25 %% (measured); using depth=%d" % (depth, extra_streams, MAX_STREAMS,
                                                                                      allowed), RuntimeWarning, stacklevel=3)
            _warned_depth[0] = True
        depth = allowed
    return depth


def log_jac_populations(hyper):
    """The log-Jacobian of a batch of samples, hyper [B, 5] = rows of (r, a, b, c, n), or [B, C, 5] for C independent
    populations: the latitude transform is per population, so the Jacobians multiply -- the sum over the populations
    of ``upstream.log_jac_samples``.  -> [B]."""
    from .upstream import log_jac_samples

    hyper = np.asarray(hyper, dtype=np.float64)
    if hyper.ndim == 2:
        return log_jac_samples(hyper[:, 1], hyper[:, 2])
    total = log_jac_samples(hyper[:, 0, 1], hyper[:, 0, 2])
    for q in range(1, hyper.shape[1]):
        total = total + log_jac_samples(hyper[:, q, 1], hyper[:, q, 2])
    return total


class SampleBatches(object):
    """log-likelihoods of MANY hyperparameter samples for ONE planned data set, ``group`` samples per library call:

        lnl[b, s] = log_likelihood of star s under sample b = (r, a, b, c, n),        samples (ns, 5) -> (ns, S)

    The systems of a call are (sample, star) pairs, ``group`` x S of them (about 64: what fills the GPU): the samples'
    polar moments (sp_polar_moments_samples), their kernel tables (sp_kernel_table_samples) and ONE planned likelihood
    call on a replicated data plan (sp_plan_replicate) whose stars carry the table of their sample.  A single light
    curve -- how the reference is called, sp.py:1052-1062 driven by calibrate/sample.py:95-107 -- then runs at the
    rate of a 64-star ensemble instead of one latency-bound step per sample.  Marginal, normalised branch;
    consecutive groups go to the slots' streams in turn.

    ``dr``: None (one spot radius), a float (radii uniform in [r - dr, r + dr] degrees, the same for every sample:
    StarryProcess(dr=...)) or "free" (a column of the samples); ``free``: which of ("baseline_mean",
    "baseline_log_var") are columns of the samples instead of fields of ``stars`` (calibrate/log_prob.py:24-47).  The
    columns are r[, dr], a, b, c, n[, m][, v][, i][, p][, tau]: ``stars.SampleColumns`` holds that layout.  With free
    terms every group's star array goes up through the pinned staging ring into the slot's own device array (the
    likelihood step reads its stars on every call).

    ``free`` may also name "i" (inclination in degrees; conditional only), "p" (period) and "tau" (timescale; needs a
    temporal kernel), which become fields of sample b's stars.  Three routes:
      * ``conditional=True`` (the process does not marginalise over the inclination; ``normalized`` either way): the
        samples' Ylm-frame moments (sp_ylm_moments_samples), then ONE sp_lnlike_ensemble_sets call per group, system
        b S + s under set b.  No plan, no tables: the data are tiled ``group`` times once, at construction.
      * marginal with free "p" or "tau": the tables as below, then the unplanned sp_lnlike_ensemble on the tiled data
        (the plan fixes period and timescale).
      * marginal otherwise: the planned path described above, unchanged.

    ``populations`` = C > 1: the samples are those of a sum of C independent spot populations (StarryProcessSum), columns
    r1[, dr1], a1, b1, c1, n1, r2, ... and then the free terms; ``dr`` is one setting for all populations or a sequence of
    C.  All three routes then take their moments from sp_polar_moments_samples_sum / sp_ylm_moments_samples_sum;
    everything behind the moments is the same."""

    def __init__(self, slots, t_dev, flux_dev, stars, rta1_dev, covpts, diag_dev=None, temporal=None, group=None,
                 norm_order=20, zmax=0.023, upstream_kwargs=None, plan=None, dr=None, free=(), conditional=False,
                 normalized=True, populations=1):
        import torch

        self._cols = SampleColumns(dr=dr, free=free, conditional=conditional, temporal=temporal, populations=populations)
        self.columns, self._free, self._dr = self._cols.columns, self._cols.free, self._cols.dr
        self._conditional, self._normalized, self._temporal = bool(conditional), bool(normalized), temporal
        if not self._normalized and not self._conditional:
            raise ValueError("the marginal branch is batched in its normalised form only")
        # (the plan fixes every star's period and timescale: with either free, the unplanned call on tiled data)
        self._planned = not self._conditional and not ("p" in self._free or "tau" in self._free)
        if plan is not None and not self._planned:
            raise ValueError("plan= belongs to the planned route: not with conditional=True or a free p / tau")
        self._stars_host = np.ascontiguousarray(stars).copy()
        self._slots = slots
        e0 = slots[0][0]
        self.S, self.K = int(t_dev.shape[0]), int(t_dev.shape[1])
        self.M = int(flux_dev.shape[1])
        self.group = max(1, int(group) if group else -(-64 // self.S))
        self._ntab = int(rta1_dev.shape[0])
        self._rta1, self._covpts = rta1_dev, int(covpts)
        self._norm_order, self._zmax = int(norm_order), float(zmax)
        self._ukw = dict(upstream_kwargs or {})
        n = self.group * self.S
        if self._planned:
            stars_d = e0.stars_to_device(stars)
            self._base_plan = plan if plan is not None else e0.plan_data(t_dev, flux_dev, stars_d, diag=diag_dev,
                                                                          covpts=self._covpts, temporal=temporal)
            self._plan = e0.replicate_plan(self._base_plan, self.group)
        else:
            # the data of the group's systems, sample-major like the stars: S stars, ``group`` times
            self._t = t_dev.repeat(self.group, 1).contiguous()
            self._flux = flux_dev.repeat(self.group, 1, 1).contiguous()
            self._diag = None if diag_dev is None else diag_dev.repeat(self.group, 1).contiguous()
            self._select = torch.arange(self.group, dtype=torch.int32, device=e0.device).repeat_interleave(
                self.S).contiguous()
        self._stars = e0.stars_to_device(self._group_stars())
        self._buf = []
        for e, _ in slots:
            b = dict(ws=e.workspace(n, self.K, self.M))
            if self._conditional:
                b.update(mu=e.empty(self.group, e.N), cov=e.empty(self.group, e.N, e.N))
            else:
                b.update(ez=e.empty(self.group, e.N), Ez=e.empty(self.group, e.N, e.N),
                         tab=e.empty(self.group * self._ntab, 5, self._covpts + 4),
                         mv=e.empty(self.group * self._ntab, 2))
            self._buf.append(b)
            if self._free:          # (one star array per stream slot, rewritten by every group of the slot)
                self._buf[-1]["stars"] = e.stars_to_device(self._group_stars())
            e.set_size_basis(**self._ukw)
        torch.cuda.synchronize(e0.device)

    @classmethod
    def column_names(cls, dr=None, free=(), conditional=False, temporal=None, populations=1):
        """(columns, free in column order) of the samples for these settings; ValueError for settings that name no batch
        (needs no device)."""
        cols = SampleColumns(dr=dr, free=free, conditional=conditional, temporal=temporal, populations=populations)
        return cols.columns, cols.free

    def _group_stars(self, **fields):
        """The star array of one group; in the conditional branch ``table`` stays the star's flux operator."""
        from .engine import stars_for_samples

        return stars_for_samples(self._stars_host, self.group, self._ntab, own_tables=not self._conditional, **fields)

    def __call__(self, samples, out=None):
        """samples (ns, len(self.columns)) -> device tensor (ns, S); nothing is synchronised: the caller does, once."""
        import torch

        samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
        if samples.ndim != 2 or samples.shape[1] != len(self.columns):
            raise ValueError("samples must be (ns, %d): %s" % (len(self.columns), ", ".join(self.columns)))
        ns, g, S = samples.shape[0], self.group, self.S
        ngroups = -(-ns // g)
        e0 = self._slots[0][0]
        raw = e0.empty(ngroups, g * S)
        if ns < ngroups * g:          # (the last group is filled up with its own last sample; those values are dropped)
            samples = np.vstack([samples, np.repeat(samples[-1:], ngroups * g - ns, axis=0)])
        hyper, dr, fields = self._cols.split(samples)
        cur = torch.cuda.current_stream(e0.device)
        start = torch.cuda.Event()
        start.record(cur)
        # (the streams' first groups start STAGGERED, each behind the upstream of the one before: started together, six
        #  streams of equal steps stay in lockstep -- all in their light upstream phase at once, then all in their
        #  factorisations at once -- and the call runs at 71k evaluations/s instead of 90-99k, bimodally from run to run)
        stagger = None
        # (at most QUEUED groups of a stream wait behind the one that runs: a host that runs hundreds of steps ahead of
        #  the GPU ends up blocked inside the runtime's launch path -- 0.8 instead of 0.16 ms of host time per step, 52-58k
        #  evaluations/s instead of 95-100k, bimodally -- so it waits HERE, for a group of three steps back)
        QUEUED = 3
        pending = [[] for _ in self._slots]
        for gi in range(ngroups):
            k = gi % len(self._slots)
            (e, stream), b = self._slots[k], self._buf[k]
            if len(pending[k]) >= QUEUED:
                pending[k].pop(0).synchronize()
            with torch.cuda.stream(stream):
                if gi < len(self._slots):
                    stream.wait_event(start)
                    if stagger is not None:
                        stream.wait_event(stagger)
                stars_d = self._stars
                sl = slice(gi * g, (gi + 1) * g)
                drs = self._cols.take_dr(dr, sl)
                if self._cols.populations > 1:          # (a sum of populations: hyper [ns, C, 5], dr None or [ns, C])
                    if self._conditional:
                        e.ylm_moments_samples_sum(hyper[sl], mean=b["mu"], cov=b["cov"], dr=drs, **self._ukw)
                    else:
                        e.polar_moments_samples_sum(hyper[sl], ez=b["ez"], Ez=b["Ez"], dr=drs, **self._ukw)
                elif self._conditional:
                    e.ylm_moments_samples(hyper[sl], mean=b["mu"], cov=b["cov"], dr=drs, **self._ukw)
                else:
                    e.polar_moments_samples(hyper[sl], ez=b["ez"], Ez=b["Ez"], dr=drs, **self._ukw)
                if self._free:
                    stars_d = e.stars_staged(self._group_stars(**{k: v[sl] for k, v in fields.items()}), b["stars"])
                if not self._conditional:
                    e.kernel_table_samples(b["ez"], b["Ez"], self._rta1, self._covpts, tab=b["tab"], meanvar=b["mv"])
                if gi + 1 < min(ngroups, len(self._slots)):
                    stagger = torch.cuda.Event()
                    stagger.record(stream)
                if self._conditional:
                    e.lnlike_ensemble_sets(self._t, self._flux, stars_d, self._rta1, b["mu"], b["cov"], self._select,
                                           diag=self._diag, temporal=self._temporal, normalized=self._normalized,
                                           norm_order=self._norm_order, zmax=self._zmax, out=raw[gi], workspace=b["ws"])
                elif not self._planned:
                    e.lnlike_ensemble(self._t, self._flux, stars_d, diag=self._diag, covpts=self._covpts, tab=b["tab"],
                                      meanvar=b["mv"], temporal=self._temporal, norm_order=self._norm_order,
                                      zmax=self._zmax, out=raw[gi], workspace=b["ws"])
                else:
                    e.lnlike_ensemble_planned(self._plan, None, None, stars_d, b["tab"], b["mv"],
                                              norm_order=self._norm_order, zmax=self._zmax, out=raw[gi],
                                              workspace=b["ws"])
                if ngroups > QUEUED * len(self._slots):
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    pending[k].append(ev)
        for k in range(min(ngroups, len(self._slots))):
            done = torch.cuda.Event()
            done.record(self._slots[k][1])
            cur.wait_event(done)
        return raw.view(ngroups * g, S)[:ns]


def get_log_prob(
    t,
    flux=None,
    ferr=1.0e-3,
    p=1.0,
    ydeg=15,
    baseline_log_var=0.0,
    baseline_mean=0.0,
    apply_jac=True,
    normalized=True,
    marginalize_over_inclination=True,
    u=[0.0, 0.0],
    device=None,
    upstream="reference",
):
    """``upstream``: "reference" (the reference's moment algorithm on the host, ~25-75 ms per
    call) or "device" (the same integrals by quadrature of rotations on the GPU, < 1 ms;
    see upstream_device.py for how the two compare)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    K = len(t)
    free_flux = flux is None
    fixed_flux = None if free_flux else np.atleast_2d(np.asarray(flux, dtype=np.float64))

    def log_prob(*args):
        args = list(args)
        fl = np.atleast_2d(np.asarray(args.pop(0), dtype=np.float64)) if free_flux else fixed_flux
        r, a, b, c, n = (float(x) for x in args[:5])
        rest = args[5:]
        m = float(rest.pop(0)) if baseline_mean is None else float(baseline_mean)
        v = float(rest.pop(0)) if baseline_log_var is None else float(baseline_log_var)
        i = float(rest.pop(0)) if not marginalize_over_inclination else 60.0
        if rest:
            raise TypeError("too many arguments")
        sp = StarryProcess(
            ydeg=ydeg, r=r, a=a, b=b, c=c, n=n, normalized=normalized,
            marginalize_over_inclination=marginalize_over_inclination, covpts=K - 1,
            # the reference callable has no z > zmax guard (log_prob.py:53-91)
            normalization_zmax=np.inf, device=device, upstream=upstream,
        )
        ll = float(sp.log_likelihood(t, fl, ferr ** 2, i=i, p=p, u=u, baseline_mean=m,
                                     baseline_var=10.0 ** v))
        if np.isnan(ll):
            ll = -np.inf
        return ll + float(sp.log_jac()) if apply_jac else ll

    return log_prob


def get_log_prob_ensemble(
    t,
    flux,
    ferr=1.0e-3,
    p=1.0,
    i=None,
    u=None,
    ydeg=15,
    baseline_log_var=0.0,
    baseline_mean=0.0,
    apply_jac=True,
    normalized=True,
    marginalize_over_inclination=True,
    covpts=None,
    device=None,
    upstream="reference",
):
    """log_prob(r, a, b, c, n) = sum over stars of per-star log-likelihoods (+ log_jac),
    each star with its own period / inclination / limb darkening / noise:
    t (K,) or (S, K); flux (S, K); ferr, p, i scalars or (S,); u (udeg,) or (S, udeg);
    or t and flux lists of S arrays of different lengths (ragged ensemble).
    Under an initialised torch.distributed job the stars are sharded over the ranks
    (one RCCL all-gather of S doubles per call); every rank returns the same value."""
    from . import ensemble

    if not isinstance(flux, (list, tuple)):     # (lists: light curves of different lengths)
        flux = np.asarray(flux, dtype=np.float64)
    S = len(flux)
    ferr2 = np.broadcast_to(np.asarray(ferr, dtype=np.float64) ** 2, (S,))

    def log_prob(r, a, b, c, n):
        kw = {} if covpts is None else {"covpts": covpts}
        sp = StarryProcess(ydeg=ydeg, r=float(r), a=float(a), b=float(b), c=float(c), n=float(n),
                           normalized=normalized,
                           marginalize_over_inclination=marginalize_over_inclination,
                           device=device, upstream=upstream, **kw)
        lnl = ensemble.sharded_log_likelihood(sp, t, flux, ferr2, i=i, p=p, u=u,
                                              baseline_mean=baseline_mean,
                                              baseline_var=10.0 ** baseline_log_var)
        ll = float(np.sum(lnl))
        if np.isnan(ll):
            ll = -np.inf
        return ll + float(sp.log_jac()) if apply_jac else ll

    return log_prob


class EnsembleLogProb(object):
    """log_prob for a batch of hyperparameter samples, same value per sample as
    ``get_log_prob_ensemble(..., upstream="device")``.

        lp = EnsembleLogProb(t, flux, ferr=1e-3, p=periods)          # data -> GPU, once
        values = lp(samples)                                          # samples (n, 5): r, a, b, c, n

    ``baseline_mean=None`` / ``baseline_log_var=None`` make the baseline mean m / the log10 of the baseline variance v
    trailing columns of the samples, as in ``get_log_prob`` (calibrate/log_prob.py:24-47, 93-103); ``dr``: None (one
    spot radius), a float in degrees (StarryProcess(dr=...)) or "free" (a column behind r).  The columns are
    r[, dr], a, b, c, n[, m][, v] (``lp.columns``).  ``populations`` = C > 1: every star carries C independent spot
    populations (``sp1 + sp2``); the hyperparameter block repeats per population, r1[, dr1], a1, b1, c1, n1, r2, ..., ``dr``
    is one setting for all of them or a sequence of C, and the latitude Jacobians of the populations multiply.

    Per sample: moments by quadrature on the device (upstream_device.py) -> kernel table ->
    one batched likelihood call for this rank's stars; nothing is copied back or synchronised
    until every sample is enqueued, and sample k runs on stream k mod ``depth`` with its own
    library handle and workspace (engine.engine_slots), so that the latency-bound phases of
    one sample overlap the throughput-bound phases of its neighbours.  The moments of ALL samples
    are produced on one more stream with a handle of its own, ahead of the likelihood streams
    (an event per sample): the quadrature is a chain of a dozen small kernels, 0.3-0.4 ms of
    latency per sample that a likelihood stream would otherwise sit through with its share of
    the GPU idle: 0.726 -> 0.69 ms per sample with three likelihood streams + this one (a fifth stream in
    flight loses more than it hides: 0.83 -- the same cliff bench.py sees at five steps in flight; round 5, one box,
    tools/attic/elp_modes.py: 0.584 as shipped, 0.603 with the moments on the three likelihood streams themselves
    (upstream_stream=False), 0.699 on four of them, 0.818 with four + the upstream's own).  Under an initialised
    ``torch.distributed`` job the stars are sharded over the ranks and the per-sample sums are
    combined with ONE all-reduce for the whole batch."""

    def __init__(self, t, flux, ferr=1.0e-3, p=1.0, i=None, u=None, ydeg=15, baseline_log_var=0.0,
                 baseline_mean=0.0, apply_jac=True, normalized=True,
                 marginalize_over_inclination=True, covpts=None, device=None, depth=3, upstream_stream=True,
                 batch_samples=True, out_of_bounds="raise", dr=None, populations=1):
        import torch
        import torch.distributed as dist

        from . import ensemble
        from .defaults import defaults
        from .engine import engine_slots
        from .stars import check_period_inclination, ensemble_stars

        self._cols = SampleColumns(dr=dr, free=[
            name for name, val in (("baseline_mean", baseline_mean), ("baseline_log_var", baseline_log_var)) if val is None],
            populations=populations)
        self.columns, self._free, self._dr = self._cols.columns, self._cols.free, self._cols.dr
        baseline_mean = 0.0 if baseline_mean is None else baseline_mean            # (placeholders: overwritten per sample)
        baseline_log_var = 0.0 if baseline_log_var is None else baseline_log_var
        flux = np.asarray(flux, dtype=np.float64)
        if flux.ndim != 2:
            raise ValueError("flux must be (S, K); ragged ensembles: get_log_prob_ensemble")
        S, K = flux.shape
        self._dist = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if self._dist else (0, 1)
        lo, hi = ensemble.shard_bounds(S, rank, world)
        self.S, self.K, self._n_local = S, K, hi - lo
        udeg = defaults["udeg"]
        # this rank's stars: what is per star is cut to the shard [lo, hi) first, so that the limb-darkening sets (and
        # with them rta1 and the kernel tables) are those of the shard alone
        t, uu = np.asarray(t, dtype=np.float64), np.asarray(defaults["u"][:udeg] if u is None else u, dtype=np.float64)
        shard = lambda x, d: np.broadcast_to(np.asarray(d if x is None else x, dtype=np.float64), (S,))[lo:hi]  # noqa: E731
        pp, ii = shard(p, defaults["p"]), shard(i, defaults["i"])
        check_period_inclination(pp, ii)
        t, stars, utab, _ = ensemble_stars((hi - lo, K), t if t.ndim == 1 else t[lo:hi], pp, ii,
                                           uu if uu.ndim == 1 else uu[lo:hi], udeg, shard(baseline_mean, 0.0),
                                           10.0 ** baseline_log_var, shard(np.asarray(ferr, dtype=np.float64) ** 2, 1.0))
        # (depth likelihood streams + the upstream's own: never more than MAX_STREAMS concurrent streams)
        depth = clamp_depth(depth, 1)
        slots = engine_slots(ydeg, udeg, device, max(2, depth + 1))
        self._slots, self._up = slots[:-1], slots[-1]          # likelihood slots; the upstream's own engine + stream
        self._upstream_stream = bool(upstream_stream)          # False: a sample's moments on its likelihood stream
        e0 = self._slots[0][0]
        self._t = e0.f64(t)
        self._flux = e0.f64(np.ascontiguousarray(flux[lo:hi, None, :]))
        self._stars = e0.stars_to_device(stars)
        self._stars_host = stars
        self._rta1 = e0.f64(e0.rTA1L(utab))
        self._ws = [e.workspace(max(hi - lo, 1), K, 1) for e, _ in self._slots]
        self._kw = dict(conditional=not marginalize_over_inclination, normalized=bool(normalized),
                        covpts=defaults["covpts"] if covpts is None else int(covpts))
        self._marg = bool(marginalize_over_inclination)
        self._ydeg, self._apply_jac = int(ydeg), bool(apply_jac)
        # The data are fixed from here on (calibrate/log_prob.py:7-55 fixes them the same way): what depends on them
        # alone -- phases, the kernel table's weights in the covariance's sum, the sums of the flux -- is taken once
        # (sp_plan_data), and every sample goes through the planned call: no pass over the K^2 entries of every
        # star's covariance before its factorisation.  One plan, read-only, shared by the slots.
        if out_of_bounds not in ("raise", "inf"):
            raise ValueError("out_of_bounds must be 'raise' or 'inf'")
        # "inf": a sample outside the reference's bounds (which raise ValueError, ops/exceptions.py:30-48) is answered
        # with -inf and not evaluated -- what a sampler's walkers need when they step out of the prior box
        self._oob = out_of_bounds
        self._plan = self._batch = None
        if self._marg and normalized and hi - lo > 0 and K >= 2:
            from ._lib import SPError

            try:
                self._plan = e0.plan_data(self._t, self._flux, self._stars, covpts=self._kw["covpts"], workspace=self._ws[0])
            except SPError:
                # (a shape the planned step does not serve -- a lag grid beyond its LDS budget, covpts > 4794, or one
                #  whose partial tables do not fit the systems' region, covpts > 4092 at K < 64: the unplanned call
                #  takes it, its assembly reading a table that no LDS holds from memory)
                self._plan = None
        # Samples go through SampleBatches: packed ceil(64 / S) to a library call when there are fewer than 64 stars (one
        # light curve above all) -- the GPU sees 64 systems per step whatever S is --, one sample per call otherwise; either
        # way the sample's moments come from sp_polar_moments_samples, with no host arithmetic (the per-sample upstream
        # spends 0.5 ms of NumPy on the size integral and the Gauss-Jacobi rule whenever r or (a, b) change).
        if self._plan is not None and batch_samples:
            more = engine_slots(ydeg, udeg, device, 2) if len(self._slots) + 1 + 2 <= MAX_STREAMS_SAMPLES else []
            self._batch = SampleBatches(self._slots + [self._up] + more, self._t, self._flux, stars, self._rta1,
                                        self._kw["covpts"], plan=self._plan, zmax=0.023, dr=self._dr, free=self._free,
                                        populations=self._cols.populations)
        torch.cuda.synchronize(e0.device)

    def __call__(self, samples):
        import torch
        import torch.distributed as dist

        from .upstream import log_jac
        from .upstream_device import ylm_moments_device

        samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
        if samples.shape[1] != len(self.columns):
            raise ValueError("samples must be (n, %d): %s" % (len(self.columns), ", ".join(self.columns)))
        if self._oob == "inf":
            ok = self._cols.in_bounds(samples)
            if not ok.all():
                out = np.full(samples.shape[0], -np.inf)
                if ok.any():
                    out[ok] = self(samples[ok])
                return out
        ns, nl = samples.shape[0], self._n_local
        hyper, drs, fields = self._cols.split(samples)
        e0 = self._slots[0][0]
        outs = e0.empty(ns, max(nl, 1))
        torch.cuda.synchronize(e0.device)
        if nl and self._batch is not None:
            outs = self._batch(samples)
        elif nl:
            eu, su = self._up
            keep = []                                   # (the moments stay alive until the batch is done)
            C = self._cols.populations

            def moments(eng, k):
                """(mean, cov) of sample k: of its one population, or the sum over its C independent ones."""
                if C == 1:
                    r, a, b, c, n = hyper[k]
                    return ylm_moments_device(eng, r=r, dr=self._cols.take_dr(drs, k), a=a, b=b, c=c, n=n)
                mean = cov = None
                for q, (r, a, b, c, n) in enumerate(hyper[k]):
                    one = self._cols.dr[q] is None          # (a population without a spread keeps dr=None)
                    m1, c1 = ylm_moments_device(eng, r=r, dr=None if one else drs[k, q], a=a, b=b, c=c, n=n)
                    mean, cov = (m1, c1) if mean is None else (mean + m1, cov + c1)
                return mean, cov

            for k in range(ns):
                stars_d = self._stars
                if self._free:
                    st = self._stars_host.copy()
                    for field, v in fields.items():          # (baseline_mean, baseline_var: the fields' own names)
                        st[field] = v[k]
                    stars_d = eu.stars_to_device(st)
                    keep.append(stars_d)
                e, stream = self._slots[k % len(self._slots)]
                if self._upstream_stream:
                    with torch.cuda.stream(su):
                        mean, cov = moments(eu, k)
                        ready = torch.cuda.Event()
                        ready.record(su)
                    keep.append((mean, cov, ready))
                with torch.cuda.stream(stream):
                    if self._upstream_stream:
                        stream.wait_event(ready)
                    else:
                        mean, cov = moments(e, k)
                        keep.append((mean, cov))
                    e.set_moments_dev(mean, cov)
                    tab = mv = None
                    if self._marg:
                        tab, mv = e.kernel_table(self._rta1, self._kw["covpts"])
                    if self._plan is not None:
                        e.lnlike_ensemble_planned(self._plan, self._t, self._flux, stars_d, tab, mv, out=outs[k],
                                                  workspace=self._ws[k % len(self._slots)])
                    else:
                        e.lnlike_ensemble(self._t, self._flux, stars_d, tab=tab, meanvar=mv,
                                          rta1=self._rta1, out=outs[k], workspace=self._ws[k % len(self._slots)],
                                          **self._kw)
        torch.cuda.synchronize(e0.device)
        vals = outs[:, :nl]
        vals = torch.where(torch.isnan(vals), torch.full_like(vals, -float("inf")), vals)
        total = vals.sum(dim=1)
        if self._dist:
            # -inf + finite = -inf survives the sum; a NaN cannot appear (no +inf terms)
            dist.all_reduce(total, op=dist.ReduceOp.SUM)
        total = total.cpu().numpy()
        if self._apply_jac:
            total = total + log_jac_populations(hyper)
        return total


def inclination_sample_indices(nsamples, nlc, ninc_samples, weights=None, seed=None):
    """Which posterior sample each (light curve, draw) of ``compute_inclination_pdf`` uses: (equal [nsamples] or None,
    idx [nlc, ninc_samples]).  One ``RandomState(seed)``: with ``weights``, first the systematic resampling to equal
    weight (one uniform offset, the positions (offset + arange(nsamples)) / nsamples against the normalised cumulative
    weights -- what the reference takes from dynesty.utils.resample_equal), ``equal`` being the resampled rows; then
    ``randint(nsamples)`` in the reference's loop order, light curve outer, draw inner (inclination.py:65-68)."""
    rng = np.random.RandomState(seed)
    nsamples = int(nsamples)
    equal = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != nsamples:
            raise ValueError("one weight per sample")
        positions = (rng.random_sample() + np.arange(nsamples)) / nsamples
        cum = np.cumsum(w)
        cum /= cum[-1]
        equal = np.minimum(np.searchsorted(cum, positions, side="right"), nsamples - 1)
    idx = np.empty((int(nlc), int(ninc_samples)), dtype=np.int64)
    for n in range(int(nlc)):
        for j in range(int(ninc_samples)):
            idx[n, j] = rng.randint(nsamples)
    return equal, idx


def compute_inclination_pdf(t, flux, ferr, period, samples, inc=np.linspace(0, 90, 100), ninc_samples=10,
                            weights=None, seed=None, ydeg=15, u=[0.0, 0.0], baseline_mean=0.0, baseline_log_var=0.0,
                            apply_jac=True, normalized=True, upstream="device", device=None):
    """Per-star inclination posteriors (calibrate/inclination.py:9-76, without dynesty): returns
    dict(inc=inc, lp=(nlc, ninc_samples, ninc_pts)), lp[n, j, k] = get_log_prob(t, ferr=ferr, p=period, ...,
    marginalize_over_inclination=False)(flux[n], *sample, inc[k]) for the sample drawn for (n, j).

    t: (K,); flux: (nlc, K); ferr: scalar; period: scalar or (nlc,); samples: rows of (r, a, b, c, n[, m][, v]) --
    m when baseline_mean is None, v (log10 of the baseline variance) when baseline_log_var is None, as get_log_prob
    orders its free variables; weights: the samples' weights (resampled to equal weight first) or None.  The sample of
    each (n, j) comes from inclination_sample_indices.  The moments of the drawn samples are formed once each and
    every (light curve, draw, inclination) triple is ONE device call; log_jac is added when apply_jac is set and no
    zmax guard applies, as in get_log_prob."""
    from .defaults import defaults
    from .engine import get_engine, make_stars
    from .sp import StarryProcess, _neg_inf_if_nan
    from .upstream import log_jac
    from ._lib import SP_STAR_NO_BASIS

    t = np.asarray(t, dtype=np.float64).reshape(-1)
    K = t.shape[0]
    flux = np.atleast_2d(np.asarray(flux, dtype=np.float64))
    nlc = flux.shape[0]
    if flux.shape[1] != K:
        raise ValueError("`flux` must be (nlc, K) like `t`")
    inc = np.asarray(inc, dtype=np.float64).reshape(-1)
    samples = np.atleast_2d(np.asarray(samples, dtype=np.float64))
    cols = SampleColumns(free=[
        name for name, val in (("baseline_mean", baseline_mean), ("baseline_log_var", baseline_log_var)) if val is None])
    if samples.shape[1] != len(cols.columns):
        raise ValueError("samples must have %d columns: %s" % (len(cols.columns), ", ".join(cols.columns)))
    equal, idx = inclination_sample_indices(samples.shape[0], nlc, ninc_samples, weights, seed)
    if equal is not None:
        samples = samples[equal]
    used, sel = np.unique(idx.reshape(-1), return_inverse=True)
    hyper, _, fields = cols.split(samples[used])
    e = get_engine(ydeg, 2, device)
    means, covs, jac = [], [], np.zeros(used.shape[0])
    for b_, row in enumerate(hyper):
        r, a, b, c, n = (float(x) for x in row)
        if upstream == "device":
            from .upstream_device import ylm_moments_device

            mu, cov = ylm_moments_device(e, r=r, dr=defaults["dr"], a=a, b=b, c=c, n=n)
        elif upstream == "reference":
            from .upstream import ylm_moments

            mu, cov = ylm_moments(r=r, dr=defaults["dr"], a=a, b=b, c=c, n=n, ydeg=ydeg)
        else:
            raise ValueError("upstream must be 'reference' or 'device'")
        means.append(e.f64(mu).reshape(-1))
        covs.append(e.f64(cov))
        if apply_jac:
            jac[b_] = float(log_jac(a, b, ydeg=ydeg))
    import torch

    mean_ylm, cov_ylm = torch.stack(means), torch.stack(covs)
    # one system per (light curve, draw): its own baseline terms when they are free parameters
    S = nlc * int(ninc_samples)
    bm, bv = fields.get("baseline_mean"), fields.get("baseline_var")
    if bm is None:
        bm = np.full(used.shape[0], float(baseline_mean))
    if bv is None:
        bv = 10.0 ** np.full(used.shape[0], float(baseline_log_var))
    per = np.repeat(np.broadcast_to(np.asarray(period, dtype=np.float64), (nlc,)), int(ninc_samples))
    stars = make_stars(S, period=per, baseline_mean=bm[sel], baseline_var=bv[sel], data_var=float(ferr) ** 2)
    uu = np.asarray(u, dtype=np.float64).reshape(1, -1)
    fl = np.repeat(flux, int(ninc_samples), axis=0)
    out, status = e.lnlike_inclinations(np.broadcast_to(t, (S, K)), fl, stars, e.rTA1L(uu), mean_ylm, cov_ylm,
                                        inc * (np.pi / 180), select=sel.reshape(S, 1), normalized=normalized,
                                        zmax=np.inf)
    lp = _neg_inf_if_nan(out[:, 0, :].cpu().numpy())
    bad = np.nonzero(np.any(status[:, 0, :].cpu().numpy() & SP_STAR_NO_BASIS, axis=1))[0]
    for s_ in bad:
        b_ = int(sel[s_])
        sp = StarryProcess(ydeg=ydeg, mean_ylm=means[b_].cpu().numpy(), cov_ylm=covs[b_].cpu().numpy(),
                           normalized=normalized, marginalize_over_inclination=False, normalization_zmax=np.inf,
                           device=device)
        lp[s_] = np.asarray(sp.log_likelihood_inclinations(t, fl[s_], float(ferr) ** 2, inc=inc, p=per[s_], u=u,
                                                           baseline_mean=bm[sel[s_]], baseline_var=bv[sel[s_]]))
    lp = lp + jac[sel][:, None]
    return dict(inc=inc, lp=lp.reshape(nlc, int(ninc_samples), inc.shape[0]))
