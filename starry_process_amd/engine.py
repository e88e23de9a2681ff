"""
One ``Engine`` per GPU: owns the ``sp_handle`` and turns torch CUDA tensors into
the raw device pointers the C ABI takes.  PyTorch is plumbing here (HBM
buffers, streams, torch.distributed); every number is produced by the HIP
kernels in ``csrc/``.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import hostconst
from ._lib import STAR_DTYPE, TEMPORAL, SPError, c_void_p, check, hptr
from .linear import MAX_REGRESSORS
from .stars import make_stars, sample_parameters, samples_in_bounds, stars_for_samples  # noqa: F401

__all__ = ["Engine", "DataPlan", "get_engine", "make_stars", "stars_for_samples", "sample_parameters", "samples_in_bounds"]


def _torch():
    import torch

    return torch


_STAGE_BYTES, _STAGE_SLOTS = 1 << 16, 16   # pinned staging ring of Engine.dev (small uploads)

LBO_MAX_BLOCK = 64   # the widest block of lbo_ensemble: one workgroup holds a block's 64 x 64 matrix in LDS


def block_edges(block, K):
    """The partition of K cadences ``lbo_ensemble`` is given, as int32 edges 0 = e_0 < ... < e_nb = K: ``block`` an int
    b, 1 <= b <= 64 (blocks of b cadences, the last one shorter), or a 1-D integer array of edges.  Pure host code:
    ValueError for a width outside 1 .. 64, edges that do not increase strictly, do not start at 0 or do not end at K."""
    K = int(K)
    if K < 2:
        raise ValueError("leave-block-out needs at least two cadences")
    if np.ndim(block) == 0:
        if isinstance(block, (bool, np.bool_)) or int(block) != block:
            raise ValueError("`block` must be an integer width or a 1-D array of edges")
        b = int(block)
        if not 1 <= b <= LBO_MAX_BLOCK:
            raise ValueError("`block` = %d: a block holds 1 to %d cadences (wider blocks are not served)"
                             % (b, LBO_MAX_BLOCK))
        e = np.append(np.arange(0, K, b), K)
    else:
        raw = np.asarray(block)
        if raw.ndim != 1 or raw.size < 2 or not (np.issubdtype(raw.dtype, np.integer) or
                                                  np.all(raw == np.round(raw))):
            raise ValueError("`block` must be an integer width or a 1-D integer array of at least two edges")
        e = raw.astype(np.int64)
        if e[0] != 0 or e[-1] != K:
            raise ValueError("the block edges must start at 0 and end at K = %d" % K)
        w = np.diff(e)
        if np.any(w < 1):
            raise ValueError("the block edges must increase strictly")
        if np.any(w > LBO_MAX_BLOCK):
            raise ValueError("a block of %d cadences: a block holds 1 to %d (wider blocks are not served)"
                             % (int(w.max()), LBO_MAX_BLOCK))
    return np.ascontiguousarray(e, dtype=np.int32)


class Engine(object):
    def __init__(self, ydeg=15, udeg=2, device=0):
        torch = _torch()
        L = _lib.lib()
        if not torch.cuda.is_available():
            raise SPError("no MI355X visible to PyTorch: the hot path has no CPU fallback")
        self.ydeg, self.udeg, self.device_index = int(ydeg), int(udeg), int(device)
        self.device = torch.device("cuda", self.device_index)
        self.N = (self.ydeg + 1) ** 2
        self.NWIG = ((self.ydeg + 1) * (2 * self.ydeg + 1) * (2 * self.ydeg + 3)) // 3
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)  # make sure the context exists
        h = c_void_p()
        check(L.sp_create(self.ydeg, self.udeg, self.device_index, ctypes.byref(h)))
        self._h = h
        self._L = L
        wnp, Wnp = hostconst.marginal_constants(self.ydeg)
        wnp = np.ascontiguousarray(wnp)
        Wnp = np.ascontiguousarray(Wnp)
        check(L.sp_set_marginal_constants(self._h, hptr(wnp), hptr(Wnp)))
        self._moments_id = None
        self._moments_owner = None
        self._ws = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.sp_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- helpers ------------------------------------------------------------
    def _stream(self):
        return c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def dev(self, a, dtype=None):
        """Host array / tensor -> contiguous tensor on this GPU."""
        torch = _torch()
        if isinstance(a, torch.Tensor):
            # (already here, of the right type and packed: the usual case inside a chain of ops --
            #  three no-op tensor calls cost 30 us of host time, 0.3 ms per upstream evaluation)
            if a.device == self.device and (dtype is None or a.dtype == dtype) and a.is_contiguous():
                return a
            t = a.to(self.device)
            if dtype is not None:
                t = t.to(dtype)
            return t.contiguous()
        a = np.ascontiguousarray(a)
        if dtype is not None and 0 < a.nbytes <= _STAGE_BYTES and a.dtype == np.float64 and dtype == torch.float64:
            return self._upload_small(a)
        t = torch.from_numpy(a).to(self.device)
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous()

    def _upload_small(self, a, out=None):
        """Small fp64 host array -> device through a ring of pinned staging buffers: the copy is
        enqueued on the current stream and the call returns (a pageable source makes the runtime
        stage and wait: 50 us per upload, four uploads per upstream evaluation).  A slot is reused
        only after the copy that last read it has completed (its event)."""
        torch = _torch()
        ring = self.__dict__.get("_stage_ring")
        if ring is None:
            ring = self._stage_ring = {"buf": [torch.empty(_STAGE_BYTES // 8, dtype=torch.float64).pin_memory()
                                               for _ in range(_STAGE_SLOTS)],
                                       "ev": [None] * _STAGE_SLOTS, "next": 0}
        k = ring["next"]
        ring["next"] = (k + 1) % _STAGE_SLOTS
        if ring["ev"][k] is not None:
            ring["ev"][k].synchronize()
        n = a.size
        src = ring["buf"][k][:n]
        src.numpy()[...] = a.reshape(-1)
        if out is None:
            out = torch.empty(a.shape, dtype=torch.float64, device=self.device)
        out.view(-1).copy_(src, non_blocking=True)
        ev = ring["ev"][k]
        if ev is None:
            ev = ring["ev"][k] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return out

    def f64(self, a):
        return self.dev(a, _torch().float64)

    def empty(self, *shape):
        torch = _torch()
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    def _scratch(self, nbytes):
        """``nbytes`` of device scratch for one library call (a ``*_workspace_bytes`` query's answer)."""
        torch = _torch()
        return torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def _grad_scratch(self, nbytes, workspace):
        """The caller's ``workspace`` if it holds ``nbytes``, fresh scratch (kept on the engine) otherwise."""
        if workspace is None or workspace.numel() < nbytes:
            workspace = self._grad_ws = self._scratch(nbytes)
        return workspace

    def _group_scratch(self, bytes_of, S, workspace, max_workspace_bytes=None):
        """The workspace of a sweep that takes its S stars in groups: the caller's, or fresh scratch (kept on the
        engine) for all S -- ``bytes_of(n)``: the driver's ``*_workspace_bytes`` query for n stars -- or of
        ``max_workspace_bytes`` where that is less, which must hold one star."""
        if workspace is not None:
            return workspace
        need = int(bytes_of(S))
        if max_workspace_bytes is not None and int(max_workspace_bytes) < need:
            one = int(bytes_of(1))
            if int(max_workspace_bytes) < one:
                raise ValueError("max_workspace_bytes = %d holds no star: one needs %d bytes"
                                 % (int(max_workspace_bytes), one))
            need = int(max_workspace_bytes)
        self._grad_ws = self._scratch(need)
        return self._grad_ws

    def _ensemble_inputs(self, t, flux, stars, diag, rta1, conditional, what=None):
        """What the ensemble sweeps take alike, as the library wants it: t, flux [S, K] (with ``what``, the caller's
        name for itself: K >= 2), the stars' device copy, diag and rta1 (or None) in float64, ``conditional`` as int."""
        torch = _torch()
        t, flux = self.f64(t), self.f64(flux)
        if flux.dim() != 2 or t.shape != flux.shape:
            raise ValueError("t and flux must both be (S, K)")
        if what is not None and flux.shape[1] < 2:
            raise ValueError("%s needs at least two cadences" % what)
        sd = stars if isinstance(stars, torch.Tensor) else self.stars_to_device(stars)
        diag = None if diag is None else self.f64(diag)
        rta1 = None if rta1 is None else self.f64(rta1)
        return t, flux, sd, diag, rta1, int(bool(conditional))

    def _regressor_inputs(self, basis, basis_var, S, K):
        """(basis [S, q, K], basis_var [S, q], q) of the calls with regressors: float64, contiguous, shapes checked."""
        basis, basis_var = self.f64(basis), self.f64(basis_var)
        if basis.dim() != 3 or basis.shape[0] != S or basis.shape[2] != K:
            raise ValueError("`basis` must be (S, q, K)")
        q = int(basis.shape[1])
        if not 1 <= q <= MAX_REGRESSORS:
            raise ValueError("1 to %d regressors per star are served, not %d" % (MAX_REGRESSORS, q))
        if tuple(basis_var.shape) != (S, q):
            raise ValueError("`basis_var` must be (S, q)")
        return basis.contiguous(), basis_var.contiguous(), q

    def _block_edges_dev(self, edges, K, return_cov):
        """(ed, nb, bmax) of the leave-block-out calls: the edges as an int32 device tensor, the number of blocks and
        the widest block.  ``edges``: an int32 device tensor or anything ``block_edges`` takes."""
        torch = _torch()
        if isinstance(edges, torch.Tensor):
            # (a device tensor is the caller's word: the library checks it; its widest block sizes `cov`)
            ed = edges.to(device=self.device, dtype=torch.int32).contiguous()
            if ed.dim() != 1 or ed.numel() < 2:
                raise ValueError("`edges` must be a 1-D array of at least two block edges")
            bmax = int((ed[1:] - ed[:-1]).max()) if return_cov else 0
        else:
            eh = block_edges(edges, K)
            bmax = int(np.diff(eh).max())
            ed = torch.as_tensor(eh, dtype=torch.int32).to(self.device)
        return ed, int(ed.numel()) - 1, bmax

    def _out_status(self, S, out, status):
        """(out, status) of a likelihood call over S systems: the caller's tensors, or fresh ones (status zeroed)."""
        if out is None:
            out = self.empty(S)
        if status is None:
            torch = _torch()
            status = torch.zeros(S, dtype=torch.int32, device=self.device)
        return out, status

    def stars_to_device(self, stars):
        torch = _torch()
        stars = np.ascontiguousarray(stars)
        assert stars.dtype == STAR_DTYPE
        raw = torch.from_numpy(stars.view(np.uint8).reshape(-1).copy())
        return raw.to(self.device)

    def stars_staged(self, stars, out):
        """``stars`` (host sp_star array) into the device array ``out`` (of stars_to_device, same length) through the
        pinned staging ring: one copy enqueued on the current stream, nothing synchronised -- for star arrays that
        change from call to call (the free baseline terms of calibrate.SampleBatches)."""
        stars = np.ascontiguousarray(stars)
        assert stars.dtype == STAR_DTYPE and STAR_DTYPE.itemsize % 8 == 0
        assert out.numel() == stars.nbytes
        if stars.nbytes > _STAGE_BYTES:
            out.copy_(_torch().from_numpy(stars.view(np.uint8).reshape(-1).copy()))
            return out
        self._upload_small(stars.view(np.float64).reshape(-1), out=out.view(_torch().float64))
        return out

    @staticmethod
    def _p(t):
        return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)

    def synchronize(self):
        check(self._L.sp_stream_synchronize(self._h, self._stream()))

    # -- ops ------------------------------------------------------
    def Rx(self, thetas, deriv=True):
        thetas = np.ascontiguousarray(np.atleast_1d(np.asarray(thetas, dtype=np.float64)))
        n = thetas.shape[0]
        R = self.empty(n, self.NWIG)
        dR = self.empty(n, self.NWIG) if deriv else None
        check(self._L.sp_Rx(self._h, hptr(thetas), n, self._p(R), self._p(dR), self._stream()))
        return R, dR

    def dotRx(self, M, Rpacked):
        """M [rows, N] or [B, rows, N]; Rpacked [NWIG] or [B, NWIG]."""
        M = self.f64(M)
        Rpacked = self.f64(Rpacked)
        batched = M.dim() == 3
        Mb = M if batched else M.unsqueeze(0)
        B, rows, N = Mb.shape
        assert N == self.N
        strideR = self.NWIG if Rpacked.dim() == 2 else 0
        out = self.empty(B, rows, N)
        check(self._L.sp_dotRx(self._h, self._p(Mb), rows * N, N, 1, rows,
                               self._p(Rpacked), strideR, self._p(out), B, self._stream()))
        return out if batched else out[0]

    def tensordotRz(self, M, theta):
        M = self.f64(M)
        theta = self.f64(theta).reshape(-1)
        K = theta.shape[0]
        assert M.shape == (K, self.N)
        f = self.empty(K, self.N)
        check(self._L.sp_tensordotRz(self._h, self._p(M), self._p(theta), K, self._p(f), self._stream()))
        return f

    def special_tensordotRz(self, T, M, theta):
        T = self.f64(T)
        M = self.f64(M)
        theta = self.f64(theta).reshape(-1)
        assert T.shape == (self.N, self.N) and M.shape == (self.N, self.N)
        K = theta.shape[0]
        f = self.empty(K)
        check(self._L.sp_special_tensordotRz(self._h, self._p(T), self._p(M), self._p(theta), K, self._p(f), self._stream()))
        return f

    def tensordotRz_rev(self, M, theta, bf):
        """Reverse mode of tensordotRz: (bM [K, N], btheta [K])."""
        M, bf = self.f64(M), self.f64(bf)
        theta = self.f64(theta).reshape(-1)
        K = theta.shape[0]
        assert M.shape == (K, self.N) and bf.shape == (K, self.N)
        bM, bth = self.empty(K, self.N), self.empty(K)
        check(self._L.sp_tensordotRz_rev(self._h, self._p(M), self._p(theta), K, self._p(bf),
                                         self._p(bM), self._p(bth), self._stream()))
        return bM, bth

    def special_tensordotRz_rev(self, T, M, theta, bf):
        """Reverse mode of special_tensordotRz: (bM [N, N], btheta [K])."""
        T, M = self.f64(T), self.f64(M)
        theta, bf = self.f64(theta).reshape(-1), self.f64(bf).reshape(-1)
        K = theta.shape[0]
        assert T.shape == (self.N, self.N) and M.shape == (self.N, self.N) and bf.shape == (K,)
        bM, bth = self.empty(self.N, self.N), self.empty(K)
        check(self._L.sp_special_tensordotRz_rev(self._h, self._p(T), self._p(M), self._p(theta), K,
                                                 self._p(bf), self._p(bM), self._p(bth), self._stream()))
        return bM, bth

    def rTA1L_rev(self, u, bf):
        """Reverse mode of rTA1L: bu [udeg] (host)."""
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1)[: self.udeg])
        bf = np.ascontiguousarray(np.asarray(bf, dtype=np.float64).reshape(-1))
        if u.shape[0] != self.udeg or bf.shape[0] != self.N:
            raise ValueError("Vector `u` or `bf` has the wrong size.")
        bu = np.empty(self.udeg)
        check(self._L.sp_rTA1L_rev(self._h, hptr(u), hptr(bf), hptr(bu)))
        return bu

    def rTA1(self):
        out = np.empty(self.N)
        check(self._L.sp_rTA1(self._h, hptr(out)))
        return out

    def rTA1L(self, u):
        """u: (udeg,) or (nsets, udeg) -> (nsets, N); udeg = 0 gives rTA1."""
        if self.udeg == 0:
            return self.rTA1()[None, :].copy()
        u = np.asarray(u, dtype=np.float64)
        u = np.ascontiguousarray(u.reshape(-1, u.shape[-1])[:, : self.udeg])
        if u.shape[1] != self.udeg:
            raise ValueError("Vector `u` has the wrong size.")
        n = u.shape[0]
        out = np.empty((n, self.N))
        check(self._L.sp_rTA1L(self._h, hptr(u), n, hptr(out)))
        return out

    # -- moments / kernel table ------------------------------------------------
    def set_moments(self, mean_ylm, cov_ylm):
        mean_ylm = np.ascontiguousarray(np.asarray(mean_ylm, dtype=np.float64).reshape(-1))
        cov_ylm = np.ascontiguousarray(np.asarray(cov_ylm, dtype=np.float64))
        assert mean_ylm.shape == (self.N,) and cov_ylm.shape == (self.N, self.N)
        # whoever bound its moments before (flux.FluxIntegral._bind) no longer owns the resident set
        self._moments_owner = None
        check(self._L.sp_set_ylm_moments(self._h, hptr(mean_ylm), hptr(cov_ylm)))

    def set_moments_dev(self, mean_ylm, cov_ylm):
        """Same with the moments already on the device (asynchronous)."""
        assert mean_ylm.is_cuda and cov_ylm.is_cuda
        self._moments_owner = None
        check(self._L.sp_set_ylm_moments_dev(self._h, self._p(mean_ylm), self._p(cov_ylm), self._stream()))

    PROF_KINDS = {"syrk": 0, "chain": 2, "panels": 4, "panel_launch": 5, "tri1": 6, "tri2": 7}

    def profile_begin(self, max_launches, kinds=("syrk",)):
        """Bracket the factorisation's launches of the given kinds with HIP events on their stream
        ("syrk" trailing updates, "chain" / "panel_launch" every panel launch under its own pair,
        "panels" the panel launches of a super-panel under ONE pair of events)."""
        mask = 0
        for k in kinds:
            mask |= 1 << self.PROF_KINDS[k]
        check(self._L.sp_profile_begin_kinds(self._h, int(max_launches), mask))

    def profile_kind(self, kind, padded=False):
        """(launches, summed milliseconds, summed algorithmic flops) of one kind; ends the profile.  padded: a fourth
        value, the flops on the padded system the launches execute (sp_profile_kind_ex)."""
        n = ctypes.c_long()
        ms = ctypes.c_double()
        fl = ctypes.c_double()
        flp = ctypes.c_double()
        check(self._L.sp_profile_kind_ex(self._h, self.PROF_KINDS[kind], ctypes.byref(n), ctypes.byref(ms),
                                         ctypes.byref(fl), ctypes.byref(flp)))
        return (n.value, ms.value, fl.value, flp.value) if padded else (n.value, ms.value, fl.value)

    def profile_end(self):
        n = ctypes.c_long()
        ms = ctypes.c_double()
        fl = ctypes.c_double()
        check(self._L.sp_profile_end(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)))
        return n.value, ms.value, fl.value

    def polar_moments(self):
        ez = np.empty(self.N)
        Ez = np.empty((self.N, self.N))
        check(self._L.sp_get_polar_moments(self._h, hptr(ez), hptr(Ez)))
        return ez, Ez

    def kernel_table(self, rta1, covpts):
        """rta1 [ntab, N] (host or device) -> tab [ntab, 5, covpts+4], meanvar [ntab, 2]."""
        rta1 = self.f64(np.atleast_2d(rta1) if not hasattr(rta1, "dim") else rta1)
        ntab = rta1.shape[0]
        _, xp = hostconst.lag_grid(int(covpts))
        xp = np.ascontiguousarray(xp)
        assert xp.shape[0] == covpts + 4
        tab = self.empty(ntab, 5, covpts + 4)
        mv = self.empty(ntab, 2)
        check(self._L.sp_kernel_table(self._h, self._p(rta1), ntab, int(covpts), hptr(xp),
                                      self._p(tab), self._p(mv), self._stream()))
        return tab, mv

    # -- hyperparameter samples in batches (round 6) -------------------------------
    def set_size_basis(self, **kw):
        """Hands the spot profile's basis (size.py:9-47; upstream._spot_basis) to the library once per engine
        (sp_set_size_basis): what sp_polar_moments_samples integrates the sigmoid profile against."""
        from .defaults import defaults
        from .upstream import _spot_basis

        skw = {k: kw[k] for k in ("spts", "eps4", "smoothing") if k in kw}
        sfac = float(kw.get("sfac", 300))
        key = (tuple(sorted(skw.items())), sfac)
        if self.__dict__.get("_size_basis_key") == key:
            return
        theta, Bp, _ = _spot_basis(self.ydeg, **skw)
        theta, Bp = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(Bp, dtype=np.float64)
        assert Bp.shape == (self.ydeg + 1, theta.shape[0])
        check(self._L.sp_set_size_basis(self._h, hptr(theta), hptr(Bp), int(theta.shape[0]), sfac))
        self._size_basis_key = key

    def _sample_rows(self, samples, dr, **kw):
        """(rows [B, 5] or, with ``dr``, [B, 6] as the sample kernels take them, B, cutoff, epsy, epsy15):
        ``sample_parameters`` of samples [B, 5] with ``dr`` (None, a scalar or one value per sample) as their second
        column, then the three scalars the sample entry points take from ``kw``; hands the spot profile's basis to the
        library on the way (set_size_basis)."""
        from .defaults import defaults

        if dr is not None:
            sm5 = np.atleast_2d(np.asarray(samples, dtype=np.float64))
            if sm5.ndim != 2 or sm5.shape[1] != 5:
                raise ValueError("samples must be (B, 5): r, a, b, c, n")
            d = np.asarray(dr, dtype=np.float64)
            if d.ndim > 1 or (d.ndim == 1 and d.shape[0] != sm5.shape[0]):
                raise ValueError("dr must be a scalar or one value per sample")
            sm = sample_parameters(np.insert(sm5, 1, np.broadcast_to(d, (sm5.shape[0],)), axis=1), dr=True, **kw)
        else:
            sm = sample_parameters(samples, **kw)
        self.set_size_basis(**kw)
        return (sm, sm.shape[0], float(kw.get("cutoff", 1.5)), float(kw.get("epsy", defaults["epsy"])),
                float(kw.get("epsy15", defaults["epsy15"])))

    def polar_moments_samples(self, samples, ez=None, Ez=None, dr=None, **kw):
        """samples [B, 5] = (r [degrees], a, b, c, n) per row, the argument order of the reference's log-probability
        (calibrate/log_prob.py:93-102) -> (ez [B, N], Ez [B, N, N]) device tensors: the polar-frame moments of B
        hyperparameter samples in one library call (sp_polar_moments_samples).  Bounds are the reference's
        (ValueError before anything is launched).  ``dr``: None (one spot radius), or the half-width of the uniform
        law of the radii in degrees, a scalar or one value per sample (StarryProcess(dr=...), size.py:109-125): one
        call of sp_polar_moments_samples_spread; a sample with dr = 0 is the one-radius case."""
        sm, B, cutoff, epsy, epsy15 = self._sample_rows(samples, dr, **kw)
        if ez is None:
            ez = self.empty(B, self.N)
        if Ez is None:
            Ez = self.empty(B, self.N, self.N)
        assert tuple(ez.shape) == (B, self.N) and tuple(Ez.shape) == (B, self.N, self.N)
        if dr is not None:
            check(self._L.sp_polar_moments_samples_spread(self._h, B, hptr(sm), cutoff, epsy, epsy15, self._p(ez),
                                                          self._p(Ez), self._stream()))
        else:
            check(self._L.sp_polar_moments_samples(self._h, B, hptr(sm), epsy, epsy15, self._p(ez), self._p(Ez),
                                                   self._stream()))
        return ez, Ez

    def ylm_moments_samples(self, samples, mean=None, cov=None, dr=None, **kw):
        """samples [B, 5] = (r [degrees], a, b, c, n) -> (mean_ylm [B, N], cov_ylm [B, N, N]) device tensors: the
        Ylm-frame moments of B hyperparameter samples in one library call (sp_ylm_moments_samples) -- what
        ``upstream_device.ylm_moments_device`` computes one sample at a time, and what the conditional branch reads.
        Bounds, ``dr`` and the keywords are polar_moments_samples'."""
        sm, B, cutoff, epsy, epsy15 = self._sample_rows(samples, dr, **kw)
        if mean is None:
            mean = self.empty(B, self.N)
        if cov is None:
            cov = self.empty(B, self.N, self.N)
        assert tuple(mean.shape) == (B, self.N) and tuple(cov.shape) == (B, self.N, self.N)
        check(self._L.sp_ylm_moments_samples(self._h, B, hptr(sm), int(dr is not None), cutoff, epsy, epsy15,
                                             self._p(mean), self._p(cov), self._stream()))
        return mean, cov

    def _sample_rows_sum(self, samples, dr, **kw):
        """_sample_rows for samples [B, C, 5] of C populations, ``dr`` None or anything that broadcasts to [B, C]: (rows
        [B C, 5 or 6], B, C, cutoff, epsy, epsy15); the bounds are checked row by row."""
        sm = np.asarray(samples, dtype=np.float64)
        if sm.ndim != 3 or sm.shape[1] < 1 or sm.shape[2] != 5:
            raise ValueError("samples must be (B, C, 5): r, a, b, c, n of each of the C populations")
        B, C = sm.shape[:2]
        if dr is not None:
            try:
                dr = np.ascontiguousarray(np.broadcast_to(np.asarray(dr, dtype=np.float64), (B, C))).reshape(-1)
            except ValueError:
                raise ValueError("dr must be a scalar, one value per population or one per sample and population")
        rows, _, cutoff, epsy, epsy15 = self._sample_rows(sm.reshape(B * C, 5), dr, **kw)
        return rows, B, C, cutoff, epsy, epsy15

    def polar_moments_samples_sum(self, samples, ez=None, Ez=None, dr=None, **kw):
        """samples [B, C, 5]: (r [degrees], a, b, c, n) of each of C independent spot populations on one star, B samples
        -> (ez [B, N], Ez [B, N, N]) device tensors: the polar-frame moments of the SUM of the populations
        (StarryProcessSum), in one library call (sp_polar_moments_samples_sum).  ``dr``: None, or the half-widths of the
        radius laws in degrees, broadcast to [B, C] (0 where a population has one radius).  Bounds and keywords are
        polar_moments_samples'; ValueError before anything is launched."""
        sm, B, C, cutoff, epsy, epsy15 = self._sample_rows_sum(samples, dr, **kw)
        if ez is None:
            ez = self.empty(B, self.N)
        if Ez is None:
            Ez = self.empty(B, self.N, self.N)
        assert tuple(ez.shape) == (B, self.N) and tuple(Ez.shape) == (B, self.N, self.N)
        check(self._L.sp_polar_moments_samples_sum(self._h, B, C, hptr(sm), int(dr is not None), cutoff, epsy, epsy15,
                                                   self._p(ez), self._p(Ez), self._stream()))
        return ez, Ez

    def ylm_moments_samples_sum(self, samples, mean=None, cov=None, dr=None, **kw):
        """samples [B, C, 5] -> (mean_ylm [B, N], cov_ylm [B, N, N]) device tensors: the Ylm-frame moments of the sum of
        C populations, B samples in one library call (sp_ylm_moments_samples_sum) -- what the conditional branch reads.
        Arguments as polar_moments_samples_sum."""
        sm, B, C, cutoff, epsy, epsy15 = self._sample_rows_sum(samples, dr, **kw)
        if mean is None:
            mean = self.empty(B, self.N)
        if cov is None:
            cov = self.empty(B, self.N, self.N)
        assert tuple(mean.shape) == (B, self.N) and tuple(cov.shape) == (B, self.N, self.N)
        check(self._L.sp_ylm_moments_samples_sum(self._h, B, C, hptr(sm), int(dr is not None), cutoff, epsy, epsy15,
                                                 self._p(mean), self._p(cov), self._stream()))
        return mean, cov

    def kernel_table_samples(self, ez, Ez, rta1, covpts, tab=None, meanvar=None):
        """ez [B, N], Ez [B, N, N], rta1 [ntab, N] (device) -> tab [B ntab, 5, covpts + 4], meanvar [B ntab, 2]: table
        b ntab + i belongs to sample b and flux operator i (sp_kernel_table_samples)."""
        B = ez.shape[0]
        ntab = rta1.shape[0]
        xp = self.__dict__.setdefault("_xp_cache", {}).get(int(covpts))
        if xp is None:
            xp = self._xp_cache[int(covpts)] = np.ascontiguousarray(hostconst.lag_grid(int(covpts))[1])
        if tab is None:
            tab = self.empty(B * ntab, 5, covpts + 4)
        if meanvar is None:
            meanvar = self.empty(B * ntab, 2)
        check(self._L.sp_kernel_table_samples(self._h, B, self._p(ez), self._p(Ez), self._p(rta1), ntab, int(covpts),
                                              hptr(xp), self._p(tab), self._p(meanvar), self._stream()))
        return tab, meanvar

    # -- covariances -----------------------------------------------------------
    def cov_marginal(self, t, stars, covpts, tab, meanvar, temporal=None,
                     normalized=True, norm_order=20):
        t = self.f64(t)
        S, K = t.shape
        sd = self.stars_to_device(stars)
        cov = self.empty(S, K, K)
        z = self.empty(S)
        check(self._L.sp_cov_marginal_batched(
            self._h, S, K, self._p(t), self._p(sd), int(covpts), self._p(tab),
            self._p(meanvar), TEMPORAL[temporal], int(bool(normalized)), int(norm_order),
            self._p(cov), K, K * K, self._p(z), self._stream()))
        return cov, z

    def design_matrix(self, t, stars, rta1):
        t = self.f64(t)
        S, K = t.shape
        sd = self.stars_to_device(stars)
        rta1 = self.f64(rta1)
        A = self.empty(S, K, self.N)
        check(self._L.sp_design_matrix(self._h, S, K, self._p(t), self._p(sd),
                                       self._p(rta1), self._p(A), self._stream()))
        return A

    def cov_conditional(self, t, stars, rta1, temporal=None, normalized=True,
                        norm_order=20):
        t = self.f64(t)
        S, K = t.shape
        sd = self.stars_to_device(stars)
        rta1 = self.f64(rta1)
        cov = self.empty(S, K, K)
        mean = self.empty(S)
        z = self.empty(S)
        check(self._L.sp_cov_conditional_batched(
            self._h, S, K, self._p(t), self._p(sd), self._p(rta1), TEMPORAL[temporal],
            int(bool(normalized)), int(norm_order), self._p(cov), K, K * K,
            self._p(mean), self._p(z), self._stream()))
        return cov, mean, z

    # -- linear algebra ----------------------------------------------------------
    def cho_factor(self, A):
        """Lower Cholesky factor(s); A [K, K] or [B, K, K] (not modified)."""
        torch = _torch()
        A = self.f64(A).clone()
        Ab = A if A.dim() == 3 else A.unsqueeze(0)
        B, K, _ = Ab.shape
        info = torch.zeros(B, dtype=torch.int32, device=self.device)
        check(self._L.sp_cho_factor(self._h, self._p(Ab), K, K, K * K, B, self._p(info), self._stream()))
        return (Ab if A.dim() == 3 else Ab[0]), info

    def spd_inverse(self, C, workspace=None, full=True):
        """(C^-1, log det C, info) of symmetric positive definite C [K, K] or [B, K, K] by the factorisation's own
        machinery (sp_spd_inverse_batched: the identity rides through the blocked Cholesky, C^-1 = L^-T L^-1 on
        the matrix cores).  full=False returns the library's raw output: [B, Kr, Kr] (Kr = K rounded up to 64)
        with the LOWER 64 x 64 tiles valid -- what the reverse sweep of the likelihood reads (grad.py)."""
        torch = _torch()
        C = self.f64(C)
        Cb = (C if C.dim() == 3 else C.unsqueeze(0)).contiguous()
        B, K, _ = Cb.shape
        Kr = (K + 63) // 64 * 64
        nbytes = int(self._L.sp_spd_inverse_workspace_bytes(self._h, B, K))
        ws = workspace
        if ws is None or ws.numel() < nbytes:
            ws = self._scratch(nbytes)
        out = torch.zeros(B, Kr, Kr, dtype=torch.float64, device=self.device)
        logdet = self.empty(B)
        info = torch.zeros(B, dtype=torch.int32, device=self.device)
        check(self._L.sp_spd_inverse_batched(self._h, B, K, self._p(Cb), K, K * K, self._p(out), self._p(logdet),
                                             self._p(info), self._p(ws), self._stream()))
        if not full:
            return out, logdet, info
        low = torch.tril(out[:, :K, :K])
        inv = low + torch.tril(low, -1).transpose(1, 2)
        return (inv if C.dim() == 3 else inv[0]), (logdet if C.dim() == 3 else logdet[0]), info

    def cho_solve(self, L, b):
        """(L L^T)^-1 b; L [K, K] or [B, K, K]; b [K], [K, M] or [B, K, M]."""
        L = self.f64(L)
        b = self.f64(b).clone()
        Lb = L if L.dim() == 3 else L.unsqueeze(0)
        B, K, _ = Lb.shape
        shape = b.shape
        bb = b.reshape(B, K, -1).contiguous()
        nrhs = bb.shape[2]
        check(self._L.sp_cho_solve(self._h, self._p(Lb), K, K, K * K, self._p(bb), nrhs, B, self._stream()))
        return bb.reshape(shape)

    def set_lazy_cov(self, on):
        """Covariance tiles formed at first touch by the factorisation (default on; effective under
        the deferred normalisation, without a temporal kernel)."""
        check(self._L.sp_set_lazy_cov(self._h, int(bool(on))))

    def set_defer_norm(self, on):
        """True (default): normalised likelihoods assemble the raw covariance once and apply the
        normalisation's rank-2 part to the result; False: separate row-sum pass (sp_set_defer_norm).
        Invalidates the cached workspace size."""
        check(self._L.sp_set_defer_norm(self._h, int(bool(on))))
        self._ws = None

    def tri_solve(self, L, b, trans=False):
        """L^-1 b (trans False) or L^-T b (trans True); shapes as in cho_solve."""
        L = self.f64(L)
        b = self.f64(b).clone()
        Lb = L if L.dim() == 3 else L.unsqueeze(0)
        B, K, _ = Lb.shape
        shape = b.shape
        bb = b.reshape(B, K, -1).contiguous()
        check(self._L.sp_tri_solve(self._h, self._p(Lb), K, K, K * K, self._p(bb), bb.shape[2], B,
                                   int(bool(trans)), self._stream()))
        return bb.reshape(shape)

    def solve_rev(self, L, c, c_bar, trans=False):
        """Reverse mode of c = A^-1 b, A = L or L^T: returns (A_bar, b_bar)."""
        L = self.f64(L)
        Lb = (L if L.dim() == 3 else L.unsqueeze(0)).contiguous()
        B, K, _ = Lb.shape
        c = self.f64(c)
        shape = c.shape
        cb = c.reshape(B, K, -1).contiguous()
        gb = self.f64(c_bar).reshape(B, K, -1).contiguous()
        nrhs = cb.shape[2]
        Abar = self.empty(B, K, K)
        bbar = self.empty(B, K, nrhs)
        check(self._L.sp_solve_rev(self._h, self._p(Lb), K, K, K * K, self._p(cb), self._p(gb), nrhs,
                                   B, int(bool(trans)), self._p(Abar), self._p(bbar), self._stream()))
        return (Abar if L.dim() == 3 else Abar[0]), bbar.reshape(shape)

    def cholesky_rev(self, L, L_bar):
        """Reverse mode of L = cholesky(C): C_bar from L and L_bar ([K, K] or [B, K, K])."""
        L = self.f64(L)
        Lb = (L if L.dim() == 3 else L.unsqueeze(0)).contiguous()
        B, K, _ = Lb.shape
        gb = self.f64(L_bar).reshape(B, K, K).contiguous()
        out = self.empty(B, K, K)
        check(self._L.sp_cholesky_rev(self._h, self._p(Lb), K, K, K * K, self._p(gb), B, self._p(out),
                                      self._stream()))
        return out if L.dim() == 3 else out[0]

    def gemm_nt(self, A, B, C=None, alpha=1.0, lower_only=False):
        """alpha A B^T (+ C): A [M, K], B [N, K] device tensors -> [M, N] (in place on C if given)."""
        A, B = self.f64(A).contiguous(), self.f64(B).contiguous()
        M, K = A.shape
        N = B.shape[0]
        assert B.shape[1] == K
        beta = 0 if C is None else 1
        out = self.empty(M, N) if C is None else C
        check(self._L.sp_gemm_nt(self._h, self._p(A), K, 0, self._p(B), K, 0, self._p(out), N, 0, M, N,
                                 K, float(alpha), beta, int(bool(lower_only)), 1, self._stream()))
        return out

    def gemm_nt_batched(self, A, B, C, alpha=1.0, beta=0, lower_only=False):
        """C[b] = beta C[b] + alpha A[b] B[b]^T for contiguous device tensors A [b, M, K], B [b, N, K],
        C [b, M, N] (in place)."""
        b, M, K = A.shape
        N = B.shape[1]
        assert B.shape == (b, N, K) and C.shape == (b, M, N)
        assert A.is_contiguous() and B.is_contiguous() and C.is_contiguous()
        check(self._L.sp_gemm_nt(self._h, self._p(A), K, M * K, self._p(B), K, N * K, self._p(C), N, M * N,
                                 M, N, K, float(alpha), int(beta), int(bool(lower_only)), b, self._stream()))
        return C

    def gp_condition(self, Ktt, Kst, Kss, r):
        """mu = K_st K_tt^-1 r and the posterior covariance K_ss - K_st K_tt^-1 K_st^T
        (device tensors; Kss is not modified).  Returns (mu, Kpost, info)."""
        torch = _torch()
        Ktt, Kst, r = self.f64(Ktt).contiguous(), self.f64(Kst).contiguous(), self.f64(r).contiguous()
        Kpost = self.f64(Kss).clone().contiguous()
        Ks, K = Kst.shape
        mu = self.empty(Ks)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self._L.sp_gp_condition(self._h, K, Ks, self._p(Ktt), self._p(Kst), self._p(Kpost),
                                      self._p(r), self._p(mu), self._p(info), self._stream()))
        return mu, Kpost, info

    # -- conditional light curves of an ensemble (sp_predict_assemble, sp_predict_ensemble; sp.py:767-1002) ----------
    @staticmethod
    def _predict_mode(mode):
        """True (full covariance), "diag" (variances) or False (means alone) -> SP_PREDICT_COV / VAR / MEAN."""
        if mode is True:
            return 2
        if mode is False:
            return 0
        if isinstance(mode, str) and mode == "diag":
            return 1
        raise ValueError("mode must be True, False or \"diag\"")

    def _predict_call(self, fn, t, ts, flux, stars, diag, conditional, covpts, tab, meanvar, rta1, temporal, extra):
        t, flux, sd, diag, rta1, conditional = self._ensemble_inputs(t, flux, stars, diag, rta1, conditional)
        S, K = flux.shape
        ts = None if ts is None else self.f64(ts)
        if ts is not None and (ts.dim() != 2 or ts.shape[0] != S or ts.shape[1] < 1):
            raise ValueError("ts must be (S, Ks)")
        Ks = K if ts is None else int(ts.shape[1])
        ws = self._scratch(self._L.sp_predict_workspace_bytes(self._h, S, K, Ks, int(covpts)))
        out = extra(S, K, Ks)
        check(fn(self._h, S, K, Ks, self._p(t), self._p(ts), self._p(flux), self._p(diag), self._p(sd),
                 conditional, int(covpts), self._p(tab), self._p(meanvar), self._p(rta1),
                 TEMPORAL[temporal], *([x if isinstance(x, int) else self._p(x) for x in out] + [self._p(ws),
                                                                                                 self._stream()])))
        return out

    def predict_assemble(self, t, ts, flux, stars, diag=None, conditional=False, covpts=300, tab=None, meanvar=None,
                         rta1=None, temporal=None):
        """The padded systems ``predict_ensemble`` factors (sp_predict_assemble): (sys [S, Kp, Kp], mean [S]) with
        Kp = roundup(K + Ks + 1, 64).  Rows < K: the lower 64 x 64 tiles of K_tt + noise + baseline_var; rows K ..
        K + Ks - 1: K_st + baseline_var; row K + Ks: (flux - baseline_mean) - mean; the tiles above the diagonal
        are left zero.  Arguments as ``predict_ensemble``."""
        torch = _torch()

        def extra(S, K, Ks):
            Kp = (K + Ks + 1 + 63) // 64 * 64
            return [torch.zeros(S, Kp, Kp, dtype=torch.float64, device=self.device), self.empty(S)]

        sys, mean = self._predict_call(self._L.sp_predict_assemble, t, ts, flux, stars, diag, conditional, covpts, tab,
                                       meanvar, rta1, temporal, extra)
        return sys, mean

    def predict_ensemble(self, t, ts, flux, stars, diag=None, conditional=False, covpts=300, tab=None, meanvar=None,
                         rta1=None, temporal=None, mode=True):
        """Conditional light curves of S stars of an un-normalised process (sp_predict_ensemble): device tensors in,
        device tensors out, nothing crosses to the host in between.

        t, flux [S, K]; ts [S, Ks] or None (predict at t); stars: host sp_star records or their device copy
        (period, inc, tau, table, baseline_mean, baseline_var, data_var); diag [S, K] per-cadence variances or
        None.  Marginal branch: tab, meanvar from ``kernel_table(rta1, covpts)``; conditional branch: rta1 and the
        moments set on this engine.  mode True: (mu [S, Ks], cov [S, Ks, Ks], info [S]); "diag": (mu,
        var [S, Ks], info); False: (mu, None, info).  A star with info != 0 (K_tt not positive definite)
        has NaN outputs."""
        torch = _torch()
        m = self._predict_mode(mode)

        def extra(S, K, Ks):
            return [m, self.empty(S, Ks), self.empty(S, Ks) if m == 1 else None,
                    self.empty(S, Ks, Ks) if m == 2 else None, torch.zeros(S, dtype=torch.int32, device=self.device)]

        _, mu, var, cov, info = self._predict_call(self._L.sp_predict_ensemble, t, ts, flux, stars, diag, conditional,
                                                   covpts, tab, meanvar, rta1, temporal, extra)
        return mu, (cov if m == 2 else var), info

    def predict_linear_workspace(self, S, K, Ks, q, covpts=300):
        """Device scratch of ``predict_linear`` (sp_predict_linear_workspace_bytes): it stops growing with S where a
        pass of stars is full."""
        return self._scratch(self._L.sp_predict_linear_workspace_bytes(self._h, int(S), int(K), int(Ks), int(q),
                                                                       int(covpts)))

    def predict_linear(self, t, ts, flux, stars, basis, basis_var, basis_sample=None, diag=None, conditional=False,
                       covpts=300, tab=None, meanvar=None, rta1=None, temporal=None, mode=True, workspace=None):
        """``predict_ensemble`` with q linear regressors per star marginalised out (sp_predict_linear): the model of
        ``lnlike_linear``, flux = process + U w + noise, w ~ N(0, diag(basis_var)).  The arguments of
        ``predict_ensemble``, and basis [S, q, K], basis_var [S, q] as ``lnlike_linear`` takes them; basis_sample
        [S, Ks, q]: the regressors at the sample times, or None -- the process alone, the trend removed, the
        uncertainty of the weights still carried.  Returns (mu [S, Ks], cov [S, Ks, Ks] / var [S, Ks] / None by
        ``mode``, info [S], w_mean [S, q], lnlike [S], lnlike0 [S], status [S]) on the device.  A star whose
        covariance does not factor (info != 0, SP_STAR_NOT_PD) or that holds a NaN (SP_STAR_NAN) has NaN outputs.
        workspace: a byte tensor (``predict_linear_workspace``); a smaller one makes the passes of stars shorter."""
        torch = _torch()
        m = self._predict_mode(mode)
        t, flux, sd, diag, rta1, conditional = self._ensemble_inputs(t, flux, stars, diag, rta1, conditional)
        S, K = flux.shape
        ts = None if ts is None else self.f64(ts)
        if ts is not None and (ts.dim() != 2 or ts.shape[0] != S or ts.shape[1] < 1):
            raise ValueError("ts must be (S, Ks)")
        Ks = K if ts is None else int(ts.shape[1])
        basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        if basis_sample is not None:
            basis_sample = self.f64(basis_sample)
            if tuple(basis_sample.shape) != (S, Ks, q):
                raise ValueError("`basis_sample` must be (S, Ks, q)")
            basis_sample = basis_sample.contiguous()
        mu = self.empty(S, Ks)
        var = self.empty(S, Ks) if m == 1 else None
        cov = self.empty(S, Ks, Ks) if m == 2 else None
        info = torch.zeros(S, dtype=torch.int32, device=self.device)
        wmean, lnlike, lnlike0 = self.empty(S, q), self.empty(S), self.empty(S)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S > 0:
            if workspace is None:
                workspace = self.predict_linear_workspace(S, K, Ks, q, covpts)
            check(self._L.sp_predict_linear(
                self._h, S, K, Ks, q, self._p(t), self._p(ts), self._p(flux), self._p(diag), self._p(sd),
                self._p(basis), self._p(basis_sample), self._p(basis_var), conditional, int(covpts), self._p(tab),
                self._p(meanvar), self._p(rta1), TEMPORAL[temporal], m, self._p(mu), self._p(var), self._p(cov),
                self._p(info), self._p(wmean), self._p(lnlike), self._p(lnlike0), self._p(status),
                self._p(workspace), int(workspace.numel()), self._stream()))
        return mu, (cov if m == 2 else var), info, wmean, lnlike, lnlike0, status

    def ylm_precision(self, mean_ylm, cov_ylm):
        """(Sigma_y^-1, Sigma_y^-1 mu_y) the way the reference forms them (sp.py:267-271: cho_factor, then
        cho_solve against I and mu_y), on the device.  NaN if Sigma_y is not positive definite."""
        torch = _torch()
        L, _ = self.cho_factor(cov_ylm)
        sinv = self.cho_solve(L, torch.eye(self.N, dtype=torch.float64, device=self.device))
        sinvmu = self.cho_solve(L, self.f64(mean_ylm).reshape(-1))
        return sinv, sinvmu

    def _ylm_buffers(self, S, K, with_cho):
        torch = _torch()
        ws = self._scratch(self._L.sp_ylm_conditional_workspace_bytes(self._h, S, K))
        ymu, ycov = self.empty(S, self.N), self.empty(S, self.N, self.N)
        ycho = self.empty(S, self.N, self.N) if with_cho else None
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        return ws, ymu, ycov, ycho, status

    def ylm_conditional(self, t, flux, stars, rta1, sinv, sinvmu, diag=None, with_cho=True):
        """Posterior of the Ylm map of S stars given their light curves (sp_ylm_conditional_batched):
        t, flux [S, K]; stars (host sp_star records: period, inc, table, baseline_mean, baseline_var, data_var);
        diag [S, K] per-cadence variances or None; sinv, sinvmu from ylm_precision.
        Returns (ymu [S, N], ycov [S, N, N], ycho [S, N, N] or None, status [S])."""
        t, flux = self.f64(t), self.f64(flux)
        S, K = flux.shape
        sd = self.stars_to_device(stars)
        diag = None if diag is None else self.f64(diag)
        # (held until the call is enqueued: an upload that is dropped at once gives its block to the next one)
        rta1, sinv, sinvmu = self.f64(rta1), self.f64(sinv), self.f64(sinvmu)
        ws, ymu, ycov, ycho, status = self._ylm_buffers(S, K, with_cho)
        check(self._L.sp_ylm_conditional_batched(
            self._h, S, K, self._p(t), self._p(flux), self._p(diag), self._p(sd), self._p(rta1),
            self._p(sinv), self._p(sinvmu), self._p(ymu), self._p(ycov), self._p(ycho),
            self._p(status), self._p(ws), self._stream()))
        return ymu, ycov, ycho, status

    def ylm_conditional_whitened(self, B, r, sinv, sinvmu, with_cho=True):
        """The same posterior for whitened data (sp_ylm_conditional_whitened): B [S, K, N] = L^-1 A,
        r [S, K] = L^-1 (flux - baseline_mean) for a full data covariance C = L L^T."""
        B, r = self.f64(B), self.f64(r)
        S, K, _ = B.shape
        sinv, sinvmu = self.f64(sinv), self.f64(sinvmu)
        ws, ymu, ycov, ycho, status = self._ylm_buffers(S, K, with_cho)
        check(self._L.sp_ylm_conditional_whitened(
            self._h, S, K, self._p(B), self._p(r), self._p(sinv), self._p(sinvmu),
            self._p(ymu), self._p(ycov), self._p(ycho), self._p(status), self._p(ws), self._stream()))
        return ymu, ycov, ycho, status

    # -- pixel space (sp_pixel_*; sp.py:443-487, 1199-1235) ------------------------------
    def pixel_transform(self, xyz):
        """M [npts, N] = pi pT(x, y, z) A1, the Ylm -> intensity transform at the points xyz [3, npts] of the unit
        sphere (sp_pixel_transform; NaN rows where z is NaN)."""
        xyz = self.f64(xyz)
        if xyz.dim() != 2 or xyz.shape[0] != 3 or xyz.shape[1] < 1:
            raise ValueError("xyz must be (3, npts)")
        npts = int(xyz.shape[1])
        ws = self._scratch(self._L.sp_pixel_transform_workspace_bytes(self._h, npts))
        M = self.empty(npts, self.N)
        check(self._L.sp_pixel_transform(self._h, npts, self._p(xyz), self._p(M), self.N, self._p(ws),
                                         self._stream()))
        return M

    def pixel_cov(self, M, cov):
        """(M cov) M^T, exactly symmetric (sp_pixel_cov_batched): cov [N, N] -> [npts, npts], or a stack of S
        covariances [S, N, N] -> [S, npts, npts] in one call.  M [npts, N] from pixel_transform."""
        M, cov = self.f64(M), self.f64(cov)
        npts, N = M.shape
        assert N == self.N and cov.shape[-2:] == (N, N)
        single = cov.dim() == 2
        cov = cov.reshape(-1, N, N).contiguous()
        S = int(cov.shape[0])
        out = self.empty(S, npts, npts)
        ws = self._scratch(self._L.sp_pixel_cov_workspace_bytes(self._h, S, npts))
        check(self._L.sp_pixel_cov_batched(self._h, S, npts, self._p(M), N, self._p(cov), N * N, self._p(out), npts,
                                           npts * npts, self._p(ws), self._stream()))
        return out[0] if single else out

    PIXEL_VAR_BATCH = 65535    # covariances per sp_pixel_var_batched call (a grid dimension)
    PIXEL_VAR_MAX_YDEG = 20    # SP_PIXEL_VAR_MAX_YDEG: the kernel keeps a row block of M in LDS

    def pixel_var(self, M, cov):
        """Per-pixel variances diag(M cov M^T) (sp_pixel_var_batched): cov [N, N] -> [npts], or a stack [..., N, N]
        -> [..., npts] in one call, with neither M cov nor the npts x npts covariance formed in memory.  cov is read
        as given (both triangles); a tensor on the device is used where it is.  M [npts, N] from pixel_transform.
        An empty stack [0, N, N] gives an empty result.  ValueError for operands of the wrong shape and for an engine
        of ydeg > 20 (PIXEL_VAR_MAX_YDEG): the kernel's row block of M does not fit LDS beyond that; the diagonal of
        pixel_cov serves those degrees."""
        if self.ydeg > self.PIXEL_VAR_MAX_YDEG:
            raise ValueError("pixel_var serves ydeg <= %d (its row block of M must fit LDS); this engine has ydeg %d: "
                             "take the diagonal of pixel_cov instead" % (self.PIXEL_VAR_MAX_YDEG, self.ydeg))
        M, cov = self.f64(M), self.f64(cov)
        N = self.N
        if M.dim() != 2 or M.shape[1] != N or M.shape[0] < 1 or cov.dim() < 2 or tuple(cov.shape[-2:]) != (N, N):
            raise ValueError("cov must be (..., %d, %d) and M (npts, %d) with npts >= 1" % (N, N, N))
        npts = int(M.shape[0])
        lead = tuple(cov.shape[:-2])
        S = int(np.prod(lead, dtype=np.int64))
        cov = cov.reshape(S, N, N).contiguous()
        out = self.empty(S, npts)
        for s0 in range(0, S, self.PIXEL_VAR_BATCH):
            n = min(self.PIXEL_VAR_BATCH, S - s0)
            check(self._L.sp_pixel_var_batched(self._h, n, npts, self._p(M), N, self._p(cov[s0:]), N * N,
                                               self._p(out[s0:]), npts, self._stream()))
        return out.reshape(lead + (npts,))

    def pixel_render(self, M, y, unit_background=True):
        """Images M y (sp_pixel_render): y [..., N] -> [..., npix]; unit_background adds 1 to y_0 first, i.e. the
        column M[:, 0] (1 on a grid, NaN off it).  M [npix, N] from pixel_transform."""
        M, y = self.f64(M), self.f64(y)
        npix, N = M.shape
        if y.dim() < 1 or y.shape[-1] != N:
            raise ValueError("the last dimension of y must be the number of Ylm coefficients (%d)" % N)
        lead = tuple(y.shape[:-1])
        y2 = y.reshape(-1, N).contiguous()
        out = self.empty(*(lead + (npix,)))
        check(self._L.sp_pixel_render(self._h, int(y2.shape[0]), npix, self._p(y2), self._p(M), N,
                                      int(bool(unit_background)), self._p(out), self._stream()))
        return out

    # -- time-variable surface maps (sp_temporal_gram, sp_ylm_temporal, sp_flux_rows; sp.py:489-516, 1237-1282) ------
    def temporal_gram(self, t, tau, temporal):
        """(Lt [Nt, Nt], info [1]): the lower Cholesky factor of the temporal kernel k(t, t, tau) with no jitter,
        temporal "matern32" or "expsquared"; all NaN and info 1 if it is not positive definite."""
        torch = _torch()
        t = self.f64(t).reshape(-1)
        Nt = int(t.shape[0])
        if Nt < 1:
            raise ValueError("t must hold at least one time")
        Lt = self.empty(Nt, Nt)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self._L.sp_temporal_gram(self._h, Nt, self._p(t), float(tau), TEMPORAL[temporal], self._p(Lt), Nt,
                                       self._p(info), self._stream()))
        return Lt, info

    def ylm_temporal(self, Lt, Ly, U, status=None):
        """Y[n] = Lt U[n] Ly^T (sp_ylm_temporal): Lt [Nt, Nt], Ly [N, N] (lower triangles read), U [ns, Nt, N] ->
        Y [ns, Nt, N]; all NaN if a factor's diagonal is not finite (then status [1], if given, gets 1)."""
        Lt, Ly, U = self.f64(Lt), self.f64(Ly), self.f64(U)
        if U.dim() != 3 or Lt.dim() != 2 or Lt.shape[0] != Lt.shape[1] or Lt.shape[0] != U.shape[1] or \
                Ly.shape != (self.N, self.N) or U.shape[2] != self.N:
            raise ValueError("need Lt [Nt, Nt], Ly [N, N] and U [ns, Nt, N] with N = %d" % self.N)
        ns, Nt = int(U.shape[0]), int(U.shape[1])
        Y = self.empty(ns, Nt, self.N)
        ws = self._scratch(self._L.sp_ylm_temporal_workspace_bytes(self._h, ns, Nt))
        check(self._L.sp_ylm_temporal(self._h, ns, Nt, self._p(Lt), Nt, self._p(Ly), self.N, self._p(U), self._p(Y),
                                      self._p(ws), self._p(status), self._stream()))
        return Y

    def flux_rows(self, A, y, normalized=False):
        """F[..., k] = A[k, :] . y[..., k, :] (sp_flux_rows): A [Nt, N], y [..., Nt, N] -> [..., Nt]; normalized maps
        every row to (1 + F) / mean(1 + F) - 1."""
        A, y = self.f64(A), self.f64(y)
        if A.dim() != 2 or A.shape[1] != self.N or y.dim() < 2 or tuple(y.shape[-2:]) != tuple(A.shape):
            raise ValueError("y must have shape (..., %d, %d)" % (int(A.shape[0]), self.N))
        Nt = int(A.shape[0])
        lead = tuple(y.shape[:-2])
        y2 = y.reshape(-1, Nt, self.N)
        out = self.empty(*(lead + (Nt,)))
        check(self._L.sp_flux_rows(self._h, int(y2.shape[0]), Nt, self._p(A), self.N, self._p(y2),
                                   int(bool(normalized)), self._p(out), self._stream()))
        return out

    # -- posterior maps of a time-variable process (sp_ylm_conditional_temporal) -------------------------
    def ylm_conditional_temporal(self, A, cov_ylm, C, resid, t, t_map, tau, temporal, with_cov=True):
        """Posterior maps of one star at the frame times ``t_map`` [T]: device tensors in, device tensors out, nothing
        crosses to the host in between.  A [K, N] the design matrix at the observed times t [K]; cov_ylm [N, N];
        C [K, K] = (A Sigma_y A^T) o k(t, t) + data covariance + baseline_var; resid [R, K] residual vectors.
        Returns (out [R, T, N] = B^T (k_j o C^-1 resid_r) with B = A Sigma_y, ycov [T, N, N] = Sigma_y - B^T (C^-1 o
        k_j k_j^T) B or None, info [1]): C^-1 by ``spd_inverse``, its products with the residuals by ``gemm_nt``, the
        frames by sp_ylm_conditional_temporal.  info != 0 (C not positive definite): every output is NaN."""
        torch = _torch()
        A, Sig, C = self.f64(A), self.f64(cov_ylm), self.f64(C)
        resid, t, t_map = self.f64(resid), self.f64(t).reshape(-1), self.f64(t_map).reshape(-1)
        K, T, R = int(t.shape[0]), int(t_map.shape[0]), int(resid.shape[0])
        if A.shape != (K, self.N) or Sig.shape != (self.N, self.N) or C.shape != (K, K) or resid.dim() != 2 or \
                resid.shape[1] != K or K < 1:
            raise ValueError("need A [K, N], cov_ylm [N, N], C [K, K] and resid [R, K] with N = %d, K = %d" % (self.N, K))
        out = self.empty(R, T, self.N)
        ycov = self.empty(T, self.N, self.N) if with_cov else None
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        if T == 0 or R == 0:
            return out, ycov, info
        low, _, info = self.spd_inverse(C, full=False)          # [1, Kr, Kr]: the lower 64 x 64 tiles of C^-1
        low = torch.tril(low[0])
        Cinv = (low + torch.tril(low, -1).T).contiguous()       # full and exactly symmetric, zero beyond K
        Kr = int(Cinv.shape[0])
        Rp = torch.zeros(R, Kr, dtype=torch.float64, device=self.device)
        Rp[:, :K] = resid
        Z = self.gemm_nt(Rp, Cinv)                              # rows (C^-1 resid_r)^T, [R, Kr]
        ws = self._scratch(self._L.sp_ylm_conditional_temporal_workspace_bytes(self._h, K, T, R, int(bool(with_cov))))
        check(self._L.sp_ylm_conditional_temporal(
            self._h, K, T, R, self._p(A), self.N, self._p(Sig), self.N, self._p(Cinv), self._p(Z), Kr, self._p(t),
            self._p(t_map), float(tau), TEMPORAL[temporal], self._p(info), self._p(out), self._p(ycov), self._p(ws),
            self._stream()))
        return out, ycov, info

    # -- synthetic ensembles (sp_generate_*; calibrate/generate.py) -------------------------------------------------
    GEN_ROWS, GEN_DEPTH = 128, 32   # padding of the projection's operands (rows, pixels): sp_generate_paint

    def generate_setup(self, nlon, eps=1e-12):
        """(WPT, L) of the reference's nlon x nlon // 2 lat/lon grid: WPT [roundup(N, 128), ldp] = (P^T W) zero-padded,
        P = M / pi the intensity design matrix, and L = cho_factor((W P)^T (W P) + eps I) [N, N] (sp_generate_gram).
        Formed once per (nlon, eps) and kept on the engine (one grid at a time)."""
        torch = _torch()
        key = (int(nlon), float(eps))
        cache = self.__dict__.get("_gen_setup")
        if cache is not None and cache[0] == key:
            return cache[1]
        self._gen_setup = None
        from .calibrate_generate import grid

        lat, lon, w, xyz = grid(nlon)
        npix = lat.size * lon.size
        M = self.pixel_transform(xyz)
        ldp = (npix + self.GEN_DEPTH - 1) // self.GEN_DEPTH * self.GEN_DEPTH
        Np = (self.N + self.GEN_ROWS - 1) // self.GEN_ROWS * self.GEN_ROWS
        WPT = torch.empty(Np, ldp, dtype=torch.float64, device=self.device)
        L = self.empty(self.N, self.N)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = self._scratch(self._L.sp_generate_gram_workspace_bytes(self._h))
        wd = self.f64(np.repeat(w, lon.size))   # (every uploaded operand stays referenced until the call returns)
        check(self._L.sp_generate_gram(self._h, npix, self._p(M), self.N, self._p(wd), float(eps), self._p(WPT), ldp,
                                       self._p(L), self.N, self._p(info), self._p(ws), self._stream()))
        del M
        if int(info.cpu()[0]):
            raise SPError("the projection's Gram matrix is not positive definite (nlon %d, eps %g)" % key)
        self._gen_setup = (key, (WPT, L))
        return WPT, L

    def generate_paint(self, nlon, spots, offsets, linear=True, intensities=False):
        """(X [S, npix] or None, WX [roundup(S, 128), ldwx]): the stars of the spot table spots [nspots, 4] (lon, lat,
        radius, contrast), star s owning rows offsets[s] .. offsets[s + 1] - 1, painted on the nlon grid
        (sp_generate_paint).  WX = w X zero-padded is what generate_project reads."""
        torch = _torch()
        from .calibrate_generate import grid

        lat, lon, w, _ = grid(nlon, xyz=False)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        S = int(offsets.shape[0]) - 1
        spots = np.ascontiguousarray(spots, dtype=np.float64).reshape(-1, 4)
        if S < 0 or offsets[0] != 0 or offsets[-1] != spots.shape[0] or np.any(np.diff(offsets) < 0):
            raise ValueError("offsets must rise from 0 to the number of spots")
        npix = lat.size * lon.size
        ldwx = (npix + self.GEN_DEPTH - 1) // self.GEN_DEPTH * self.GEN_DEPTH
        rows = max(1, (S + self.GEN_ROWS - 1) // self.GEN_ROWS) * self.GEN_ROWS
        X = self.empty(S, npix) if intensities else None
        WX = torch.empty(rows, ldwx, dtype=torch.float64, device=self.device)
        sp = self.f64(spots) if spots.size else None
        latd, lond, wd, offd = self.f64(lat), self.f64(lon), self.f64(w), self.dev(offsets)
        check(self._L.sp_generate_paint(self._h, S, lat.size, lon.size, self._p(latd), self._p(lond), self._p(wd),
                                        self._p(sp), self._p(offd), int(bool(linear)), self._p(X), self._p(WX), ldwx,
                                        self._stream()))
        return X, WX

    def generate_project(self, WPT, L, WX, S, smoothing):
        """y [S, N] = s_l . G^-1 (W P)^T (W X[s]) (sp_generate_project), WPT / L from generate_setup, WX from
        generate_paint."""
        ldp, ldwx = int(WPT.shape[1]), int(WX.shape[1])
        if int(WX.shape[0]) < max(1, (S + self.GEN_ROWS - 1) // self.GEN_ROWS) * self.GEN_ROWS or \
                int(WPT.shape[0]) < (self.N + self.GEN_ROWS - 1) // self.GEN_ROWS * self.GEN_ROWS:
            raise ValueError("WX must come from generate_paint of the same S stars, WPT from generate_setup")
        y = self.empty(S, self.N)
        ws = self._scratch(self._L.sp_generate_project_workspace_bytes(self._h, S))
        check(self._L.sp_generate_project(self._h, int(S), ldp, self._p(WPT), ldp, self._p(L), self.N, self._p(WX),
                                          ldwx, float(smoothing), self._p(y), self._p(ws), self._stream()))
        return y

    GEN_NORM = {None: 0, "mean": 1, "median": 2}

    def generate_flux(self, t, stars, rta1, y, noise, ferr, normalization=None):
        """(flux0, flux) [S, K] (sp_generate_flux): flux0[s] = A_s y[s] at the shared times t [K], A_s the design
        matrix of stars[s]; flux = flux0 (normalization None) or its mean / median normalisation, plus ferr noise."""
        t, y, noise = self.f64(t).reshape(-1), self.f64(y), self.f64(noise)
        S, K = int(y.shape[0]), int(t.shape[0])
        if y.shape != (S, self.N) or noise.shape != (S, K) or len(stars) != S:
            raise ValueError("need y [S, %d], noise [S, K] and S stars" % self.N)
        flux0, flux = self.empty(S, K), self.empty(S, K)
        ws = self._scratch(self._L.sp_generate_flux_workspace_bytes(self._h, S, K))
        sd, rta1 = self.stars_to_device(stars), self.f64(rta1)
        check(self._L.sp_generate_flux(self._h, S, K, self._p(t), self._p(sd), self._p(rta1), self._p(y),
                                       self._p(noise), float(ferr), self.GEN_NORM[normalization], self._p(flux0),
                                       self._p(flux), self._p(ws), self._stream()))
        return flux0, flux

    # -- conditional likelihoods on a grid of inclinations (sp_lnlike_inclinations) ---------------
    def lnlike_inclinations(self, t, flux, stars, rta1, mean_ylm, cov_ylm, inc_rad, select=None, diag=None,
                            normalized=True, norm_order=20, zmax=0.023):
        """Conditional-branch log-likelihoods of S stars x J moment sets x P inclinations in one call:
        t [S, K], flux [S, M, K] (or [S, K]), stars (host sp_star records; inc is not read), rta1 [ntab, N],
        mean_ylm [B, N], cov_ylm [B, N, N], inc_rad [P], select [S, J] indices of the moment sets (None: J = B,
        every set for every star), diag [S, K] per-cadence variances or None.
        Returns (lnlike [S, J, P], status [S, J, P]); SP_STAR_NO_BASIS marks stars the basis cannot take."""
        torch = _torch()
        t, flux = self.f64(t), self.f64(flux)
        if flux.dim() == 2:
            flux = flux[:, None, :].contiguous()
        S, M, K = flux.shape
        sd = self.stars_to_device(stars)
        rta1 = self.f64(rta1).reshape(-1, self.N)
        mean_ylm = self.f64(mean_ylm).reshape(-1, self.N)
        cov_ylm = self.f64(cov_ylm).reshape(-1, self.N, self.N)
        B, ntab = int(mean_ylm.shape[0]), int(rta1.shape[0])
        if cov_ylm.shape[0] != B:
            raise ValueError("mean_ylm and cov_ylm hold different numbers of moment sets")
        inc = self.f64(np.asarray(inc_rad, dtype=np.float64).reshape(-1))
        P = int(inc.shape[0])
        if select is None:
            J, sel = B, None
        else:
            select = np.array(np.broadcast_to(np.asarray(select, dtype=np.int32), (S, np.shape(select)[-1])))
            if select.size and (select.min() < 0 or select.max() >= B):
                raise ValueError("select holds an index outside the %d moment sets" % B)
            J, sel = int(select.shape[1]), self.dev(select)
        diag = None if diag is None else self.f64(diag)
        out = self.empty(S, J, P)
        status = torch.zeros(S, J, P, dtype=torch.int32, device=self.device)
        if S == 0 or J == 0 or P == 0:
            return out, status
        ws = self._scratch(self._L.sp_lnlike_inclinations_workspace_bytes(self._h, S, M, ntab, B, P))
        check(self._L.sp_lnlike_inclinations(
            self._h, S, K, M, self._p(t), self._p(flux), self._p(diag), self._p(sd), self._p(rta1), ntab, B,
            self._p(mean_ylm), self._p(cov_ylm), J, self._p(sel), P, self._p(inc), int(bool(normalized)),
            int(norm_order), float(zmax), self._p(out), self._p(status), self._p(ws), self._stream()))
        return out, status

    # -- the grid with derivatives and its mixture (sp_lnlike_inclinations_grad) ---------------
    def incl_plan_data(self, t, flux, stars_dev, diag=None):
        """The per-star plan of the inclination grid for one light curve per star (sp_incl_plan_data): t, flux
        [S, K], stars_dev (device records), diag [S, K] or None -> (plan, status [S]: SP_STAR_NO_BASIS or 0)."""
        torch = _torch()
        t, flux = self.f64(t), self.f64(flux)
        S, K = flux.shape
        diag = None if diag is None else self.f64(diag)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        plan = self._scratch(max(int(self._L.sp_incl_plan_bytes(self._h, S, 1)), 1))
        if S == 0:
            return plan, status
        check(self._L.sp_incl_plan_data(self._h, S, K, 1, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev),
                                        self._p(plan), self._p(status), self._stream()))
        return plan, status

    def incl_plan_tangent(self, t, flux, stars_dev, plan, diag=None):
        """The plan's derivative with respect to each star's period (sp_incl_plan_tangent), from the inputs of
        ``incl_plan_data`` and its plan: per star Ldot [n, n], wdot, g0dot, T0dot [n], rhodot and W = L_G^-1 Ldot [n, n];
        NaN for a star the plan flagged.  Once per data set; ``lnlike_inclinations_grad(star_tangent=...)`` reads it."""
        t, flux = self.f64(t), self.f64(flux)
        S, K = flux.shape
        diag = None if diag is None else self.f64(diag)
        ptan = self._scratch(max(int(self._L.sp_incl_plan_tangent_bytes(self._h, S)), 1))
        if S == 0:
            return ptan
        if int(plan.numel()) < int(self._L.sp_incl_plan_bytes(self._h, S, 1)):
            raise ValueError("the plan does not hold %d stars" % S)
        check(self._L.sp_incl_plan_tangent(self._h, S, K, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev),
                                           self._p(plan), self._p(ptan), self._stream()))
        return ptan

    def lnlike_inclinations_grad(self, plan, stars, rta1, mean_ylm, cov_ylm, dmu, dsig, inc_rad, logw=None,
                                 normalized=True, norm_order=20, zmax=0.023, star_tangent=None, star_mask=0):
        """The grid of ``lnlike_inclinations`` for one moment set with its derivatives along Pd directions of the
        moments, and its mixture over the grid: plan (``incl_plan_data``), stars (host sp_star records or their device copy), rta1
        [ntab, N], mean_ylm [N], cov_ylm [N, N], dmu [Pd, N], dsig [Pd, N, N] (symmetric, 1 <= Pd <= 8), inc_rad [P],
        logw [P] log prior weights or None.  Returns (lnlike [S, P], dlnlike [S, P, Pd], lnmix [S], dlnmix [S, Pd],
        pinc [S, P], status [S, P]); lnmix, dlnmix and pinc are None without logw.

        star_mask: bit k asks for slot k of each star's own derivatives (period, baseline_mean, baseline_var, log_var;
        sp_lnlike_inclinations_grad_stars); star_tangent: the plan's ``incl_plan_tangent``, needed with bit 0.  The return
        then ends with (dstar [S, P, 4], dstarmix [S, 4] or None without logw); a slot that was not asked for holds NaN.
        The other outputs have the bits of the call without."""
        torch = _torch()
        N = self.N
        if isinstance(stars, np.ndarray):
            stars = self.stars_to_device(stars)
        S = int(stars.numel()) // STAR_DTYPE.itemsize
        rta1 = self.f64(rta1).reshape(-1, N)
        ntab = int(rta1.shape[0])
        mean_ylm, cov_ylm = self.f64(mean_ylm).reshape(N), self.f64(cov_ylm).reshape(N, N)
        dmu = self.f64(dmu).reshape(-1, N)
        Pd = int(dmu.shape[0])
        dsig = self.f64(dsig)
        if not 1 <= Pd <= 8 or tuple(dsig.shape) != (Pd, N, N):
            raise ValueError("need dmu [Pd, %d] and dsig [Pd, %d, %d] with 1 <= Pd <= 8" % (N, N, N))
        vec = lambda x: self.f64(x if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)).reshape(-1)  # noqa: E731
        inc = vec(inc_rad)
        P = int(inc.shape[0])
        if P < 1:
            raise ValueError("at least one inclination")
        lw = None
        if logw is not None:
            lw = vec(logw)
            if lw.shape[0] != P:
                raise ValueError("logw must hold one value per inclination")
        lnl, dlnl = self.empty(S, P), self.empty(S, P, Pd)
        status = torch.zeros(S, P, dtype=torch.int32, device=self.device)
        mix = (self.empty(S), self.empty(S, Pd), self.empty(S, P)) if lw is not None else (None, None, None)
        star_mask = int(star_mask)
        if not 0 <= star_mask <= 15:
            raise ValueError("star_mask: bits 0-3 (period, baseline_mean, baseline_var, log_var)")
        if star_mask & 1:
            if star_tangent is None:
                raise ValueError("star_mask asks for the period: star_tangent (incl_plan_tangent) is needed")
            if S > 0 and int(star_tangent.numel()) < int(self._L.sp_incl_plan_tangent_bytes(self._h, S)):
                raise ValueError("star_tangent does not hold %d stars" % S)
        if S > 0 and int(plan.numel()) < int(self._L.sp_incl_plan_bytes(self._h, S, 1)):
            raise ValueError("the plan does not hold %d stars" % S)
        if star_mask:
            nan = float("nan")
            dstar = torch.full((S, P, 4), nan, dtype=torch.float64, device=self.device)
            dstarmix = torch.full((S, 4), nan, dtype=torch.float64, device=self.device) if lw is not None else None
            if S > 0:
                ws = self._scratch(self._L.sp_lnlike_inclinations_grad_workspace_bytes(self._h, S, ntab, P, Pd))
                check(self._L.sp_lnlike_inclinations_grad_stars(
                    self._h, S, self._p(plan), self._p(stars), self._p(rta1), ntab, self._p(mean_ylm), self._p(cov_ylm),
                    Pd, self._p(dmu), self._p(dsig), P, self._p(inc), self._p(lw), int(bool(normalized)),
                    int(norm_order), float(zmax), self._p(lnl), self._p(dlnl), self._p(mix[0]), self._p(mix[1]),
                    self._p(mix[2]), self._p(status), self._p(star_tangent), star_mask, self._p(dstar),
                    self._p(dstarmix), self._p(ws), self._stream()))
            return (lnl, dlnl) + mix + (status, dstar, dstarmix)
        if S > 0:
            ws = self._scratch(self._L.sp_lnlike_inclinations_grad_workspace_bytes(self._h, S, ntab, P, Pd))
            check(self._L.sp_lnlike_inclinations_grad(
                self._h, S, self._p(plan), self._p(stars), self._p(rta1), ntab, self._p(mean_ylm), self._p(cov_ylm), Pd,
                self._p(dmu), self._p(dsig), P, self._p(inc), self._p(lw), int(bool(normalized)), int(norm_order),
                float(zmax), self._p(lnl), self._p(dlnl), self._p(mix[0]), self._p(mix[1]), self._p(mix[2]),
                self._p(status), self._p(ws), self._stream()))
        return (lnl, dlnl) + mix + (status,)

    # -- surface-map posteriors with the inclination marginalised (sp_ylm_conditional_inclinations) ------
    def ylm_conditional_inclinations(self, t, flux, stars, rta1, mean_ylm, cov_ylm, inc_rad, logprior, diag=None,
                                     with_cov=True, with_inc=False, nsamples=0):
        """Mixture over P grid inclinations of the map posteriors of S stars, one device call: t, flux [S, K], stars
        (host sp_star records; inc is not read), rta1 [ntab, N], mean_ylm [N], cov_ylm [N, N], inc_rad [P],
        logprior [P] (log prior weight of each grid point; -inf: weight 0), diag [S, K] or None.
        Returns (pinc [S, P], ymu [S, N], ycov [S, N, N] or None, ymu_inc [S, P, N] or None, status [S], state);
        ``state`` is what ylm_inclination_samples needs for up to ``nsamples`` draws per star."""
        torch = _torch()
        t, flux = self.f64(t), self.f64(flux)
        S, K = flux.shape
        sd = self.stars_to_device(stars)
        rta1 = self.f64(rta1).reshape(-1, self.N)
        ntab = int(rta1.shape[0])
        mean_ylm = self.f64(mean_ylm).reshape(self.N)
        cov_ylm = self.f64(cov_ylm).reshape(self.N, self.N)
        inc = self.f64(np.asarray(inc_rad, dtype=np.float64).reshape(-1))
        lp = self.f64(np.asarray(logprior, dtype=np.float64).reshape(-1))
        P, ns = int(inc.shape[0]), int(nsamples)
        if lp.shape[0] != P:
            raise ValueError("logprior must hold one value per inclination")
        diag = None if diag is None else self.f64(diag)
        pinc, ymu = self.empty(S, P), self.empty(S, self.N)
        ycov = self.empty(S, self.N, self.N) if with_cov else None
        ymui = self.empty(S, P, self.N) if with_inc else None
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S == 0:
            return pinc, ymu, ycov, ymui, status, None
        nbytes = self._L.sp_ylm_conditional_inclinations_workspace_bytes(self._h, S, ntab, P, int(bool(with_cov)), ns)
        ws = self._scratch(max(int(nbytes), 1))
        check(self._L.sp_ylm_conditional_inclinations(
            self._h, S, K, self._p(t), self._p(flux), self._p(diag), self._p(sd), self._p(rta1), ntab,
            self._p(mean_ylm), self._p(cov_ylm), P, self._p(inc), self._p(lp), self._p(pinc), self._p(ymu),
            self._p(ycov), self._p(ymui), self._p(status), ns, self._p(ws), self._stream()))
        state = {"ws": ws, "S": S, "ntab": ntab, "P": P, "ns": ns, "stars": sd, "mean_ylm": mean_ylm}
        return pinc, ymu, ycov, ymui, status, state

    def ylm_inclination_samples(self, state, cho_ylm, comp, z, e):
        """Samples of the mixture by pathwise conditioning (sp_ylm_inclination_samples): ``state`` from
        ylm_conditional_inclinations, cho_ylm [N, N] the lower factor of Sigma_y, comp [S, ns] the component of each
        sample, z [S, ns, N] and e [S, ns, 2 ydeg + 1] standard normal deviates.  Returns y [S, ns, N]."""
        S, n = state["S"], 2 * self.ydeg + 1
        comp = self.dev(np.ascontiguousarray(np.asarray(comp, dtype=np.int32).reshape(S, -1)))
        ns = int(comp.shape[1])
        if ns > state["ns"]:
            raise ValueError("the posterior was computed for at most %d samples per star" % state["ns"])
        z, e = self.f64(z).reshape(S, ns, self.N), self.f64(e).reshape(S, ns, n)
        cho_ylm = self.f64(cho_ylm)
        y = self.empty(S, ns, self.N)
        check(self._L.sp_ylm_inclination_samples(
            self._h, S, state["ntab"], state["P"], ns, self._p(state["stars"]), self._p(state["mean_ylm"]),
            self._p(cho_ylm), self._p(comp), self._p(z), self._p(e), self._p(y), self._p(state["ws"]),
            self._stream()))
        return y

    # -- fused likelihood ----------------------------------------------------------
    def workspace(self, S, K, M):
        nbytes = self._L.sp_lnlike_workspace_bytes(self._h, S, K, M)
        if nbytes < 0:
            check(int(nbytes))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = self._scratch(nbytes)
        return self._ws

    def lnlike_ensemble(self, t, flux, stars_dev, diag=None, conditional=False,
                        covpts=300, tab=None, meanvar=None, rta1=None, temporal=None,
                        normalized=True, norm_order=20, zmax=0.023, out=None,
                        status=None, workspace=None):
        """All arguments already on the device (torch tensors); t [S,K],
        flux [S,M,K], stars_dev from stars_to_device().  Returns (lnlike, status)."""
        S, K = t.shape
        M = flux.shape[1]
        ws = workspace if workspace is not None else self.workspace(S, K, M)
        out, status = self._out_status(S, out, status)
        check(self._L.sp_lnlike_ensemble(
            self._h, S, K, M, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev),
            int(bool(conditional)), int(covpts), self._p(tab), self._p(meanvar),
            self._p(rta1), TEMPORAL[temporal], int(bool(normalized)), int(norm_order),
            float(zmax), self._p(ws), self._p(out), self._p(status), self._stream()))
        return out, status

    def lnlike_ensemble_sets(self, t, flux, stars_dev, rta1, mean_ylm, cov_ylm, select, diag=None, temporal=None,
                             normalized=True, norm_order=20, zmax=0.023, out=None, status=None, workspace=None):
        """The conditional branch of lnlike_ensemble with one moment set per system (sp_lnlike_ensemble_sets): system
        s is evaluated under (mean_ylm[select[s]], cov_ylm[select[s]]).  t [S, K], flux [S, M, K], stars_dev, rta1
        [ntab, N], mean_ylm [B, N], cov_ylm [B, N, N] on the device; ``select`` [S]: a host array of indices (checked
        here: ValueError outside [0, B)) or an int32 device tensor (taken as it is).  The engine's own moments are not
        touched.  Returns (lnlike, status)."""
        torch = _torch()
        S, K = t.shape
        M = flux.shape[1]
        B = int(mean_ylm.shape[0])
        if tuple(mean_ylm.shape) != (B, self.N) or tuple(cov_ylm.shape) != (B, self.N, self.N):
            raise ValueError("mean_ylm must be (B, N) and cov_ylm (B, N, N)")
        if not isinstance(select, torch.Tensor):
            sel = np.ascontiguousarray(np.asarray(select).reshape(-1), dtype=np.int32)
            if sel.shape[0] != S:
                raise ValueError("select must hold one index per system")
            if sel.size and (sel.min() < 0 or sel.max() >= B):
                raise ValueError("select holds an index outside the %d moment sets" % B)
            select = torch.from_numpy(sel).to(self.device)
        elif select.dtype != torch.int32 or select.numel() != S or not select.is_contiguous() or not select.is_cuda:
            raise ValueError("a device select must be a contiguous int32 tensor with one index per system")
        ws = workspace if workspace is not None else self.workspace(S, K, M)
        out, status = self._out_status(S, out, status)
        check(self._L.sp_lnlike_ensemble_sets(
            self._h, S, K, M, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), self._p(rta1), B,
            self._p(mean_ylm), self._p(cov_ylm), self._p(select), TEMPORAL[temporal], int(bool(normalized)),
            int(norm_order), float(zmax), self._p(ws), self._p(out), self._p(status), self._stream()))
        return out, status

    def plan_data(self, t, flux, stars_dev, diag=None, covpts=300, temporal=None, workspace=None):
        """What depends on the data alone, once per data set (sp_plan_data): phases, the weights of the kernel
        table in the covariance's sum, sums of the flux and of the variances.  t [S,K], flux [S,M,K] device
        tensors, stars_dev from stars_to_device().  The plan fixes the stars' period, nobs and tau; it may be
        shared by every engine of this GPU.  Returns a ``DataPlan``."""
        S, K = t.shape
        M = flux.shape[1]
        ws = workspace if workspace is not None else self.workspace(S, K, M)
        p = c_void_p()
        check(self._L.sp_plan_data(self._h, S, K, M, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev),
                                   int(covpts), TEMPORAL[temporal], self._p(ws), self._stream(), ctypes.byref(p)))
        # (the plan records the data pointers: the tensors must outlive it)
        return DataPlan(self._L, p, S, K, M, int(covpts), temporal, diag is not None, keep=(t, flux, diag))

    def replicate_plan(self, plan, B):
        """B copies of a planned data set as one batch of B S systems (sp_plan_replicate): system b S + s is star s under
        hyperparameter sample b.  The replica owns its data; evaluate it with ``lnlike_ensemble_planned(plan, None, None,
        stars_for_samples(...), ...)``."""
        p = c_void_p()
        check(self._L.sp_plan_replicate(self._h, plan.ptr, int(B), self._stream(), ctypes.byref(p)))
        return DataPlan(self._L, p, plan.S * int(B), plan.K, plan.M, plan.covpts, plan.temporal, plan.has_diag)

    def lnlike_ensemble_planned(self, plan, t, flux, stars_dev, tab, meanvar, diag=None, norm_order=20,
                                zmax=0.023, out=None, status=None, workspace=None):
        """``lnlike_ensemble(conditional=False, normalized=True)`` on planned data (sp_lnlike_ensemble_planned):
        the same values to rounding, without the per-sample pass over the covariance's entries."""
        S, K, M = plan.S, plan.K, plan.M
        # (t = flux = diag = None: the plan's own arrays -- a replica's copies, or the tensors of plan time)
        assert (t is None and flux is None and diag is None) or (tuple(t.shape) == (S, K) and tuple(flux.shape) == (S, M, K))
        ws = workspace if workspace is not None else self.workspace(S, K, M)
        out, status = self._out_status(S, out, status)
        check(self._L.sp_lnlike_ensemble_planned(
            self._h, plan.ptr, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), self._p(tab),
            self._p(meanvar), int(norm_order), float(zmax), self._p(ws), self._p(out), self._p(status),
            self._stream()))
        return out, status

    def lnlike_grad_marginal(self, t, flux, stars_dev, tab, meanvar, diag=None, covpts=300, temporal=None,
                             normalized=True, norm_order=20, zmax=0.023, workspace=None):
        """Device half of the ensemble gradient (sp_lnlike_grad_marginal_multi): t [S, K], flux [S, K] or [S, M, K]
        (M light curves per star on one covariance) -> (lnlike [S], ybar [S, covpts + 4], meanbar [S], status [S]):
        the log-likelihoods (summed over a star's light curves) and their derivatives with respect to each star's
        kernel table and flux mean (grad.py chains them to the hyperparameters)."""
        torch = _torch()
        S, K = t.shape
        flux = flux.reshape(S, -1, K)
        M = flux.shape[1]
        nbytes = int(self._L.sp_lnlike_grad_workspace_bytes_multi(self._h, S, K, M, int(covpts)))
        ws = self._grad_scratch(nbytes, workspace)
        out, ybar, mbar = self.empty(S), self.empty(S, covpts + 4), self.empty(S)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        check(self._L.sp_lnlike_grad_marginal_multi(
            self._h, S, K, M, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), int(covpts), self._p(tab),
            self._p(meanvar), TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), self._p(ws),
            self._p(out), self._p(ybar), self._p(mbar), self._p(status), self._stream()))
        return out, ybar, mbar, status

    def lnlike_grad_marginal_stars(self, t, flux, stars_dev, tab, meanvar, diag=None, covpts=300, temporal=None,
                                   normalized=True, norm_order=20, zmax=0.023, workspace=None):
        """``lnlike_grad_marginal`` and, from the same sweep, the derivatives with respect to each star's own
        parameters (sp_lnlike_grad_marginal_stars) -> (lnlike [S], ybar [S, covpts + 4], meanbar [S], starbar [S, 6],
        status [S]); starbar[s] = d lnL_s / d (period, tau, baseline_mean, baseline_var, log of a common factor on the
        star's data variances, reserved 0)."""
        torch = _torch()
        S, K = t.shape
        flux = flux.reshape(S, -1, K)
        M = flux.shape[1]
        nbytes = int(self._L.sp_lnlike_grad_workspace_bytes_multi(self._h, S, K, M, int(covpts)))
        ws = self._grad_scratch(nbytes, workspace)
        out, ybar, mbar, sbar = self.empty(S), self.empty(S, covpts + 4), self.empty(S), self.empty(S, 6)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        check(self._L.sp_lnlike_grad_marginal_stars(
            self._h, S, K, M, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), int(covpts), self._p(tab),
            self._p(meanvar), TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), self._p(ws),
            self._p(out), self._p(ybar), self._p(mbar), self._p(status), self._p(sbar), self._stream()))
        return out, ybar, mbar, sbar, status

    def lnlike_grad_conditional(self, t, flux, stars_dev, rta1, diag=None, temporal=None, normalized=True,
                                norm_order=20, zmax=0.023, workspace=None):
        """Device half of the CONDITIONAL branch's ensemble gradient (sp_lnlike_grad_conditional), at the engine's
        current moments: t [S, K], flux [S, K], stars_dev (each star's inclination in sp_star.inc, radians), rta1
        [ntab, N] -> (lnlike [S], mubar [S, N], sigbar [S, N, N], starbar [S, 6], status [S]); starbar[s] = d lnL_s / d
        (period, inclination per radian, baseline_mean, baseline_var, log of a common factor on the star's data
        variances, 0)."""
        torch = _torch()
        S, K = t.shape
        assert tuple(flux.shape) == (S, K)
        N = self.N
        out, mubar, sigbar, sbar = self.empty(S), self.empty(S, N), self.empty(S, N, N), self.empty(S, 6)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S == 0:
            return out, mubar, sigbar, sbar, status
        nbytes = int(self._L.sp_lnlike_grad_conditional_workspace_bytes(self._h, S, K))
        ws = self._grad_scratch(nbytes, workspace)
        check(self._L.sp_lnlike_grad_conditional(
            self._h, S, K, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), self._p(rta1),
            TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), self._p(ws), self._p(out),
            self._p(mubar), self._p(sigbar), self._p(sbar), self._p(status), self._stream()))
        return out, mubar, sigbar, sbar, status

    def fisher_workspace(self, S, K, P, covpts):
        """Device scratch that holds ``S`` stars of ``fisher_marginal`` at once (sp_fisher_workspace_bytes)."""
        return self._scratch(self._L.sp_fisher_workspace_bytes(self._h, int(S), int(K), int(P), int(covpts)))

    def fisher_linear_workspace(self, S, K, P, q, covpts):
        """Device scratch that holds ``S`` stars of ``fisher_marginal(basis=...)`` at once
        (sp_fisher_linear_workspace_bytes)."""
        return self._scratch(self._L.sp_fisher_linear_workspace_bytes(self._h, int(S), int(K), int(P), int(q),
                                                                      int(covpts)))

    def fisher_marginal(self, t, stars_dev, tab, meanvar, dyp, dmean, diag=None, covpts=300, temporal=None,
                        normalized=True, norm_order=20, zmax=0.023, workspace=None, return_tangents=False, basis=None,
                        basis_var=None):
        """Device half of the ensemble's Fisher information (sp_fisher_marginal): t [S, K], the kernel tables of the
        engine's last ``kernel_table`` (tab [ntab, 5, covpts + 4], meanvar [ntab, 2]) and the tangents of their first
        rows and of the flux means with respect to P parameters (dyp [P, ntab, covpts + 4], dmean [P, ntab]) ->
        (fisher [S, P, P], status [S]) and, with ``return_tangents``, dcov [S, P, K, K]: the tangents of the stars'
        covariances.  workspace: a byte tensor (``fisher_workspace``); one that holds fewer than S stars makes the call
        work through the stars in groups, with the same bits.  basis [S, q, K], basis_var [S, q]: q linear regressors
        per star marginalised out (sp_fisher_marginal_linear; the workspace is then ``fisher_linear_workspace``'s)."""
        torch = _torch()
        S, K = t.shape
        P = int(dyp.shape[0])
        assert tuple(dyp.shape) == (P, tab.shape[0], covpts + 4) and tuple(dmean.shape) == (P, tab.shape[0])
        if basis is None and basis_var is not None:
            raise ValueError("`basis_var` needs a `basis`")
        if basis is not None:
            basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        fisher = self.empty(S, P, P)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        dcov = self.empty(S, P, K, K) if return_tangents else None
        if S > 0 and basis is not None:
            workspace = self._group_scratch(
                lambda n: self._L.sp_fisher_linear_workspace_bytes(self._h, n, K, P, q, int(covpts)), S, workspace)
            check(self._L.sp_fisher_marginal_linear(
                self._h, S, K, P, q, self._p(t), self._p(diag), self._p(stars_dev), self._p(basis), self._p(basis_var),
                int(covpts), self._p(tab), self._p(meanvar), self._p(dyp.contiguous()), self._p(dmean.contiguous()),
                TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), self._p(fisher), self._p(dcov),
                self._p(status), self._p(workspace), int(workspace.numel()), self._stream()))
        elif S > 0:
            workspace = self._group_scratch(
                lambda n: self._L.sp_fisher_workspace_bytes(self._h, n, K, P, int(covpts)), S, workspace)
            check(self._L.sp_fisher_marginal(
                self._h, S, K, P, self._p(t), self._p(diag), self._p(stars_dev), int(covpts), self._p(tab),
                self._p(meanvar), self._p(dyp.contiguous()), self._p(dmean.contiguous()), TEMPORAL[temporal],
                int(bool(normalized)), int(norm_order), float(zmax), self._p(fisher), self._p(dcov), self._p(status),
                self._p(workspace), int(workspace.numel()), self._stream()))
        return (fisher, status, dcov) if return_tangents else (fisher, status)

    def fisher_conditional_workspace(self, S, K, P):
        """Device scratch that holds ``S`` stars of ``fisher_conditional`` at once (sp_fisher_conditional_workspace_bytes)."""
        return self._scratch(self._L.sp_fisher_conditional_workspace_bytes(self._h, int(S), int(K), int(P)))

    def fisher_conditional_linear_workspace(self, S, K, P, q):
        """Device scratch that holds ``S`` stars of ``fisher_conditional(basis=...)`` at once
        (sp_fisher_conditional_linear_workspace_bytes)."""
        return self._scratch(self._L.sp_fisher_conditional_linear_workspace_bytes(self._h, int(S), int(K), int(P),
                                                                                  int(q)))

    def fisher_conditional(self, t, stars_dev, rta1, dmu, dsig, star_params=("i", "p"), diag=None, temporal=None,
                           normalized=True, norm_order=20, zmax=0.023, workspace=None, return_tangents=False, basis=None,
                           basis_var=None):
        """Device half of the conditional branch's Fisher information (sp_fisher_conditional), at the engine's current
        moments: t [S, K], stars_dev (each star's inclination in sp_star.inc, radians), rta1 [ntab, N] and the moments'
        tangents with respect to Ph shared hyperparameters (dmu [Ph, N], dsig [Ph, N, N]; None for Ph = 0) ->
        (fisher [S, P, P], status [S]) and, with ``return_tangents``, dcov [S, P, K, K].  The rows of a star's block: the
        Ph hyperparameters, then its inclination (per RADIAN) when "i" is in ``star_params``, then its period when "p"
        is.  workspace: a byte tensor (``fisher_conditional_workspace``); one that holds fewer than S stars makes the
        call work through the stars in groups, with the same bits.  basis [S, q, K], basis_var [S, q]: q linear
        regressors per star marginalised out (sp_fisher_conditional_linear; the workspace is then
        ``fisher_conditional_linear_workspace``'s)."""
        torch = _torch()
        S, K = t.shape
        N = self.N
        if basis is None and basis_var is not None:
            raise ValueError("`basis_var` needs a `basis`")
        if basis is not None:
            basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        Ph = 0 if dmu is None else int(dmu.shape[0])
        mask = (1 if "i" in star_params else 0) | (2 if "p" in star_params else 0)
        P = Ph + (mask & 1) + (mask >> 1)
        if Ph:
            assert tuple(dmu.shape) == (Ph, N) and tuple(dsig.shape) == (Ph, N, N)
            dmu, dsig = dmu.contiguous(), dsig.contiguous()
        else:
            dmu = dsig = None
        fisher = self.empty(S, P, P)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        dcov = self.empty(S, P, K, K) if return_tangents else None
        if S > 0 and basis is not None:
            workspace = self._group_scratch(
                lambda n: self._L.sp_fisher_conditional_linear_workspace_bytes(self._h, n, K, P, q), S, workspace)
            check(self._L.sp_fisher_conditional_linear(
                self._h, S, K, Ph, mask, q, self._p(t), self._p(diag), self._p(stars_dev), self._p(basis),
                self._p(basis_var), self._p(rta1), self._p(dmu), self._p(dsig), TEMPORAL[temporal],
                int(bool(normalized)), int(norm_order), float(zmax), self._p(fisher), self._p(dcov), self._p(status),
                self._p(workspace), int(workspace.numel()), self._stream()))
        elif S > 0:
            workspace = self._group_scratch(
                lambda n: self._L.sp_fisher_conditional_workspace_bytes(self._h, n, K, P), S, workspace)
            check(self._L.sp_fisher_conditional(
                self._h, S, K, Ph, mask, self._p(t), self._p(diag), self._p(stars_dev), self._p(rta1), self._p(dmu),
                self._p(dsig), TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), self._p(fisher),
                self._p(dcov), self._p(status), self._p(workspace), int(workspace.numel()), self._stream()))
        return (fisher, status, dcov) if return_tangents else (fisher, status)

    def loo_workspace(self, S, K, covpts=300, conditional=False):
        """Device scratch that holds ``S`` stars of ``loo_ensemble`` at once (sp_loo_workspace_bytes)."""
        return self._scratch(self._L.sp_loo_workspace_bytes(self._h, int(S), int(K), int(covpts),
                                                            int(bool(conditional))))

    def loo_ensemble(self, t, flux, stars, diag=None, conditional=False, covpts=300, tab=None, meanvar=None, rta1=None,
                     temporal=None, normalized=True, norm_order=20, zmax=0.023, workspace=None,
                     max_workspace_bytes=None):
        """Leave-one-out predictive checks of S light curves (sp_loo_ensemble): t, flux [S, K]; stars: host sp_star
        records or their device copy; diag [S, K] per-cadence variances or None.  Marginal branch: tab, meanvar from
        ``kernel_table(rta1, covpts)``; conditional branch: rta1 and the moments set on this engine.  Returns
        (loo [S, 5, K], lnlike [S], status [S]) on the device; the rows of loo: mu_loo, var_loo, the standardised
        residual z, the log predictive density, and the whitened residual L^-1 r.  A star whose covariance does not
        factor, or a ragged one, holds NaN; a normalised star with z > zmax has lnlike = -inf and finite rows.
        workspace: a byte tensor (``loo_workspace``); ``max_workspace_bytes`` caps the scratch allocated here
        instead.  A workspace that holds fewer than S stars makes the call work through them in groups, with the
        same bits."""
        torch = _torch()
        t, flux, sd, diag, rta1, conditional = self._ensemble_inputs(t, flux, stars, diag, rta1, conditional,
                                                                     "leave-one-out")
        S, K = flux.shape
        loo, lnlike = self.empty(S, 5, K), self.empty(S)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S > 0:
            workspace = self._group_scratch(
                lambda n: self._L.sp_loo_workspace_bytes(self._h, n, K, int(covpts), conditional), S, workspace,
                max_workspace_bytes)
            check(self._L.sp_loo_ensemble(
                self._h, S, K, self._p(t), self._p(flux), self._p(diag), self._p(sd), conditional, int(covpts),
                self._p(tab), self._p(meanvar), self._p(rta1), TEMPORAL[temporal], int(bool(normalized)),
                int(norm_order), float(zmax), self._p(loo), self._p(lnlike), self._p(status), self._p(workspace),
                int(workspace.numel()), self._stream()))
        return loo, lnlike, status

    def lbo_workspace(self, S, K, covpts=300, conditional=False, nblocks=1):
        """Device scratch that holds ``S`` stars of ``lbo_ensemble`` at once (sp_lbo_workspace_bytes)."""
        return self._scratch(self._L.sp_lbo_workspace_bytes(self._h, int(S), int(K), int(covpts),
                                                            int(bool(conditional)), int(nblocks)))

    def lbo_ensemble(self, t, flux, stars, edges, diag=None, conditional=False, covpts=300, tab=None, meanvar=None,
                     rta1=None, temporal=None, normalized=True, norm_order=20, zmax=0.023, return_cov=False,
                     workspace=None, max_workspace_bytes=None):
        """Leave-block-out predictive checks of S light curves (sp_lbo_ensemble): t, flux [S, K]; stars: host sp_star
        records or their device copy; edges [nblocks + 1]: a partition of the cadence indices into blocks of 1 to 64
        (``block_edges``), an int32 device tensor or anything ``block_edges`` takes; the other arguments as
        ``loo_ensemble``.  Returns (rows [S, 4, K], lpd [S, nblocks], cov [S, nblocks, bmax, bmax] or None, lnlike [S],
        status [S]) on the device; the rows: the blocks' predictive means, variances and whitened residuals u, and
        the whitened residual L^-1 r of the whole light curve.  A star whose covariance does not factor, or a ragged
        one, holds NaN; a normalised star with z > zmax has lnlike = -inf and finite rows.  workspace: a byte tensor
        (``lbo_workspace``); ``max_workspace_bytes`` caps the scratch allocated here instead.  A workspace that holds
        fewer than S stars makes the call work through them in groups, with the same bits."""
        torch = _torch()
        t, flux, sd, diag, rta1, conditional = self._ensemble_inputs(t, flux, stars, diag, rta1, conditional,
                                                                     "leave-block-out")
        S, K = flux.shape
        ed, nb, bmax = self._block_edges_dev(edges, K, return_cov)
        rows, lpd, lnlike = self.empty(S, 4, K), self.empty(S, nb), self.empty(S)
        cov = self.empty(S, nb, bmax, bmax) if return_cov else None
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S > 0:
            workspace = self._group_scratch(
                lambda n: self._L.sp_lbo_workspace_bytes(self._h, n, K, int(covpts), conditional, nb), S, workspace,
                max_workspace_bytes)
            check(self._L.sp_lbo_ensemble(
                self._h, S, K, self._p(t), self._p(flux), self._p(diag), self._p(sd), conditional, int(covpts),
                self._p(tab), self._p(meanvar), self._p(rta1), TEMPORAL[temporal], int(bool(normalized)),
                int(norm_order), float(zmax), nb, self._p(ed), self._p(rows), self._p(lpd), self._p(cov),
                self._p(lnlike), self._p(status), self._p(workspace), int(workspace.numel()), self._stream()))
        return rows, lpd, cov, lnlike, status

    def lnlike_linear_workspace(self, S, K, q, covpts=300, conditional=False):
        """Device scratch that holds ``S`` stars of ``lnlike_linear`` at once (sp_lnlike_linear_workspace_bytes)."""
        return self._scratch(self._L.sp_lnlike_linear_workspace_bytes(self._h, int(S), int(K), int(q), int(covpts),
                                                                      int(bool(conditional))))

    def lnlike_linear(self, t, flux, stars, basis, basis_var, diag=None, conditional=False, covpts=300, tab=None,
                      meanvar=None, rta1=None, temporal=None, normalized=True, norm_order=20, zmax=0.023,
                      return_cov=True, workspace=None, max_workspace_bytes=None):
        """The likelihood of S light curves with q linear regressors per star marginalised out (sp_lnlike_linear):
        t, flux [S, K]; stars: host sp_star records or their device copy; basis [S, q, K]: regressor j of star s along
        row j; basis_var [S, q]: the prior variances of the weights, >= 0; diag [S, K] per-cadence variances or None.
        Marginal branch: tab, meanvar from ``kernel_table(rta1, covpts)``; conditional branch: rta1 and the moments
        set on this engine.  Returns (lnlike [S], lnlike0 [S], w_mean [S, q], w_cov [S, q, q] or None, status [S]) on
        the device: the likelihood with and without the regressors and the posterior of their weights.  A star whose
        covariance does not factor, or a ragged one, holds NaN; a normalised star with z > zmax has lnlike = lnlike0 =
        -inf and finite weights.  workspace: a byte tensor (``lnlike_linear_workspace``); ``max_workspace_bytes``
        caps the scratch allocated here instead.  A workspace that holds fewer than S stars makes the call work
        through them in groups, with the same bits."""
        torch = _torch()
        t, flux, sd, diag, rta1, conditional = self._ensemble_inputs(t, flux, stars, diag, rta1, conditional,
                                                                     "the likelihood with regressors")
        S, K = flux.shape
        basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        lnlike, lnlike0, wmean = self.empty(S), self.empty(S), self.empty(S, q)
        wcov = self.empty(S, q, q) if return_cov else None
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S > 0:
            workspace = self._group_scratch(
                lambda n: self._L.sp_lnlike_linear_workspace_bytes(self._h, n, K, q, int(covpts), conditional), S,
                workspace, max_workspace_bytes)
            check(self._L.sp_lnlike_linear(
                self._h, S, K, q, self._p(t), self._p(flux), self._p(diag), self._p(sd), self._p(basis),
                self._p(basis_var), conditional, int(covpts), self._p(tab), self._p(meanvar), self._p(rta1),
                TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), self._p(lnlike),
                self._p(lnlike0), self._p(wmean), self._p(wcov), self._p(status), self._p(workspace),
                int(workspace.numel()), self._stream()))
        return lnlike, lnlike0, wmean, wcov, status

    def lbo_linear_workspace(self, S, K, q, covpts=300, conditional=False, nblocks=1):
        """Device scratch that holds ``S`` stars of ``lbo_linear`` at once (sp_lbo_linear_workspace_bytes)."""
        return self._scratch(self._L.sp_lbo_linear_workspace_bytes(self._h, int(S), int(K), int(q), int(covpts),
                                                                   int(bool(conditional)), int(nblocks)))

    def lbo_linear(self, t, flux, stars, edges, basis, basis_var, diag=None, conditional=False, covpts=300, tab=None,
                   meanvar=None, rta1=None, temporal=None, normalized=True, norm_order=20, zmax=0.023,
                   return_cov=False, workspace=None, max_workspace_bytes=None):
        """Leave-block-out predictive checks of S light curves with q linear regressors per star marginalised out
        (sp_lbo_linear): ``lbo_ensemble`` for the model of ``lnlike_linear``.  t, flux, stars, edges, diag and the
        branch arguments as ``lbo_ensemble``; basis [S, q, K] and basis_var [S, q] as ``lnlike_linear``.  Returns
        (rows [S, 4, K], lpd [S, nblocks], cov [S, nblocks, bmax, bmax] or None, lnlike [S], lnlike0 [S], w_mean
        [S, q], status [S]) on the device; the rows: the blocks' predictive means, variances and whitened residuals u
        -- the uncertainty of the weights included -- and the whitened DETRENDED residual L^-1 (r - U w_mean) of the
        whole light curve.  lnlike, lnlike0 and w_mean are ``lnlike_linear``'s.  A star whose covariance does not
        factor, a ragged one, or one with a variance that is negative or not finite holds NaN; a normalised star with
        z > zmax has lnlike = lnlike0 = -inf and finite rows.  workspace: a byte tensor (``lbo_linear_workspace``);
        ``max_workspace_bytes`` caps the scratch allocated here instead.  A workspace that holds fewer than S stars
        makes the call work through them in groups, with the same bits."""
        torch = _torch()
        t, flux, sd, diag, rta1, conditional = self._ensemble_inputs(t, flux, stars, diag, rta1, conditional,
                                                                     "leave-block-out with regressors")
        S, K = flux.shape
        basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        ed, nb, bmax = self._block_edges_dev(edges, K, return_cov)
        rows, lpd = self.empty(S, 4, K), self.empty(S, nb)
        lnlike, lnlike0, wmean = self.empty(S), self.empty(S), self.empty(S, q)
        cov = self.empty(S, nb, bmax, bmax) if return_cov else None
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S > 0:
            workspace = self._group_scratch(
                lambda n: self._L.sp_lbo_linear_workspace_bytes(self._h, n, K, q, int(covpts), conditional, nb), S,
                workspace, max_workspace_bytes)
            check(self._L.sp_lbo_linear(
                self._h, S, K, q, self._p(t), self._p(flux), self._p(diag), self._p(sd), self._p(basis),
                self._p(basis_var), conditional, int(covpts), self._p(tab), self._p(meanvar), self._p(rta1),
                TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax), nb, self._p(ed), self._p(rows),
                self._p(lpd), self._p(cov), self._p(lnlike), self._p(lnlike0), self._p(wmean), self._p(status),
                self._p(workspace), int(workspace.numel()), self._stream()))
        return rows, lpd, cov, lnlike, lnlike0, wmean, status

    def grad_linear_workspace(self, S, K, q, covpts=300):
        """Device scratch of ``lnlike_grad_linear`` (sp_lnlike_grad_linear_workspace_bytes)."""
        return self._scratch(self._L.sp_lnlike_grad_linear_workspace_bytes(self._h, int(S), int(K), int(q), int(covpts)))

    def lnlike_grad_linear(self, t, flux, stars_dev, basis, basis_var, tab, meanvar, diag=None, covpts=300,
                           temporal=None, normalized=True, norm_order=20, zmax=0.023, workspace=None):
        """Device half of the ensemble gradient with q linear regressors per star marginalised out
        (sp_lnlike_grad_linear): t, flux [S, K]; basis [S, q, K], regressor j of star s along row j; basis_var [S, q],
        the prior variances of the weights -> (lnlike [S], ybar [S, covpts + 4], meanbar [S], starbar [S, 6],
        lambar [S, q], w_mean [S, q], status [S]): ``lnlike_linear``'s likelihood, its derivatives with respect to each
        star's kernel table, flux mean and own parameters as ``lnlike_grad_marginal_stars`` returns them, with respect
        to the prior variances themselves, and the posterior mean of the weights."""
        torch = _torch()
        S, K = t.shape
        if tuple(flux.shape) != (S, K):
            raise ValueError("`flux` must be (S, K): one light curve per star")
        basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        nbytes = int(self._L.sp_lnlike_grad_linear_workspace_bytes(self._h, S, K, q, int(covpts)))
        ws = self._grad_scratch(nbytes, workspace)
        out, ybar, mbar, sbar = self.empty(S), self.empty(S, covpts + 4), self.empty(S), self.empty(S, 6)
        lbar, wmean = self.empty(S, q), self.empty(S, q)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        check(self._L.sp_lnlike_grad_linear(
            self._h, S, K, q, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), self._p(basis),
            self._p(basis_var), int(covpts), self._p(tab), self._p(meanvar), TEMPORAL[temporal], int(bool(normalized)),
            int(norm_order), float(zmax), self._p(ws), self._p(out), self._p(ybar), self._p(mbar), self._p(status),
            self._p(sbar), self._p(lbar), self._p(wmean), self._stream()))
        return out, ybar, mbar, sbar, lbar, wmean, status

    def grad_conditional_workspace(self, S, K):
        return self._scratch(self._L.sp_lnlike_grad_conditional_workspace_bytes(self._h, S, K))

    def grad_conditional_linear_workspace(self, S, K, q):
        """Device scratch of ``lnlike_grad_conditional_linear`` (sp_lnlike_grad_conditional_linear_workspace_bytes)."""
        return self._scratch(self._L.sp_lnlike_grad_conditional_linear_workspace_bytes(self._h, int(S), int(K), int(q)))

    def lnlike_grad_conditional_linear(self, t, flux, stars_dev, basis, basis_var, rta1, diag=None, temporal=None,
                                       normalized=True, norm_order=20, zmax=0.023, workspace=None):
        """Device half of the CONDITIONAL branch's ensemble gradient with q linear regressors per star marginalised out
        (sp_lnlike_grad_conditional_linear), at the engine's current moments: t, flux [S, K]; basis [S, q, K], regressor
        j of star s along row j; basis_var [S, q], the prior variances of the weights; rta1 [ntab, N] -> (lnlike [S],
        mubar [S, N], sigbar [S, N, N], starbar [S, 6], lambar [S, q], w_mean [S, q], status [S]):
        ``lnlike_linear(conditional=True)``'s likelihood, its derivatives as ``lnlike_grad_conditional`` returns them,
        with respect to the prior variances themselves, and the posterior mean of the weights."""
        torch = _torch()
        S, K = t.shape
        if tuple(flux.shape) != (S, K):
            raise ValueError("`flux` must be (S, K): one light curve per star")
        basis, basis_var, q = self._regressor_inputs(basis, basis_var, S, K)
        N = self.N
        out, mubar, sigbar, sbar = self.empty(S), self.empty(S, N), self.empty(S, N, N), self.empty(S, 6)
        lbar, wmean = self.empty(S, q), self.empty(S, q)
        status = torch.zeros(S, dtype=torch.int32, device=self.device)
        if S == 0:
            return out, mubar, sigbar, sbar, lbar, wmean, status
        nbytes = int(self._L.sp_lnlike_grad_conditional_linear_workspace_bytes(self._h, S, K, q))
        ws = self._grad_scratch(nbytes, workspace)
        check(self._L.sp_lnlike_grad_conditional_linear(
            self._h, S, K, q, self._p(t), self._p(flux), self._p(diag), self._p(stars_dev), self._p(basis),
            self._p(basis_var), self._p(rta1), TEMPORAL[temporal], int(bool(normalized)), int(norm_order), float(zmax),
            self._p(ws), self._p(out), self._p(mubar), self._p(sigbar), self._p(sbar), self._p(lbar), self._p(wmean),
            self._p(status), self._stream()))
        return out, mubar, sigbar, sbar, lbar, wmean, status

    def grad_workspace(self, S, K, covpts, M=1):
        return self._scratch(self._L.sp_lnlike_grad_workspace_bytes_multi(self._h, S, K, int(M), int(covpts)))

    def cholesky_lnlike(self, cov, resid):
        """cov [S,K,K] (noise included), resid [S,M,K] -> (lnlike [S], status [S])."""
        cov = self.f64(cov)
        resid = self.f64(resid)
        S, K, _ = cov.shape
        M = resid.shape[1]
        ws = self.workspace(S, K, M)
        out, status = self._out_status(S, None, None)
        check(self._L.sp_cholesky_lnlike_batched(self._h, S, K, M, self._p(cov), self._p(resid),
                                                 self._p(ws), self._p(out), self._p(status), self._stream()))
        return out, status


class DataPlan(object):
    """Owner of an ``sp_plan`` (include/starry_process_amd.h: sp_plan_data)."""

    def __init__(self, L, ptr, S, K, M, covpts, temporal, has_diag, keep=None):
        self._L, self.ptr = L, ptr
        self.S, self.K, self.M, self.covpts, self.temporal, self.has_diag = S, K, M, covpts, temporal, has_diag
        self._keep = keep

    def wbar(self):
        """[S, covpts + 4] host copy of the table's weights in the covariance's sum."""
        out = np.empty((self.S, self.covpts + 4))
        check(self._L.sp_plan_get_wbar(self.ptr, hptr(out)))
        return out

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                self._L.sp_plan_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


_engines = {}


def engine_slots(ydeg=15, udeg=2, device=None, depth=3):
    """``depth`` independent (Engine, torch.cuda.Stream) pairs on one GPU, for keeping several
    INDEPENDENT evaluations in flight (the walkers / live points a sampler evaluates per
    iteration): run evaluation i inside ``with torch.cuda.stream(stream_i)`` on ``engine_i``,
    each with its own workspace and outputs.  One evaluation alone leaves most of the GPU idle
    during its latency-bound phases (the chain of diagonal blocks); with three in flight those
    overlap the neighbours' assembly and trailing updates: 0.95 -> 0.66 ms per 64-star step
    (bench.py).  FOUR is where it peaks: a fifth stream in flight loses 10-25 % (108k against 120k
    evaluations/s at cfg3's shape; calibrate.MAX_STREAMS, to which the callers' ``depth`` is clamped -- this function
    gives what it is asked for, bench.py measures the cliff with it).  A handle is not re-entrant, hence one per slot (fresh handles; the
    process-wide engine of ``get_engine`` is left as it is, and is what depth = 1 returns)."""
    torch = _torch()
    depth = max(1, int(depth))
    first = get_engine(ydeg, udeg, device)
    if depth == 1:
        return [(first, torch.cuda.Stream(device=first.device))]
    out = []
    for k in range(depth):
        e = Engine(first.ydeg, first.udeg, first.device_index)
        out.append((e, torch.cuda.Stream(device=e.device)))
    return out


def get_engine(ydeg=15, udeg=2, device=None):
    """Process-wide engine cache keyed by (ydeg, udeg, device)."""
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    key = (int(ydeg), int(udeg), int(device))
    if key not in _engines:
        _engines[key] = Engine(*key)
    return _engines[key]
