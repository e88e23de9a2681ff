"""
The surface-map posterior (csrc/sp_ylm.hip: sp_ylm_conditional_batched, sp_ylm_conditional_whitened) at its layout
edges, against the long-double arbiter of tests/ylm_arbiter.py.

tests/test_gpu_ylm_conditional.py pins this family to the executed reference at 1e-6 posterior standard deviations:
with the real moments cond(W) is about 1e9, and no float64 evaluation agrees with another more closely.  Here the
prior precision is an input of our own making (ya.prior_precision: cond_2(W) <= 1e3, asserted on the device's matrix),
so the same kernels can be held to rounding: ya.star_bound = 10 x the error of a float64 SciPy restatement against
the arbiter, and never more than 32 (K + N) u cond_2(W) at the star's own cond_2(W) (ya.YARDSTICK, measured on the CPU
by tests/test_ylm_arbiter_host.py, which also shows that a subtly wrong kernel exceeds the bound by orders of
magnitude).  The arbiter runs on the design matrix downloaded from the device
(itself checked against the oracle), so sp_ylm.hip, the Gram product and the N x N solves are what is under test.

Shapes: ya.SWEEP -- N below one tile (4, 9), ragged (36, 441), exactly one 64-tile (64) and an exact multiple (256);
K on either side of every multiple of 32 up to 129, and 257; K < N and K > N.

Measured on an MI355X, largest over each degree's cases (ymu / ycov / ycho ycho^T in sd, the bound, worst cond_2(W)):
    ydeg  1   1.1e-14 / 2.4e-15 / 2.5e-15   1.1e-13    10.3    (K = 1, star 1: 6e-16 against the model's 7.1e-14)
    ydeg  2   2.4e-14 / 3.0e-15 / 2.9e-15   6.9e-14    11.5
    ydeg  5   1.9e-13 / 2.3e-14 / 2.3e-14   3.6e-13    37.1
    ydeg  7   1.5e-13 / 3.5e-14 / 3.5e-14   2.5e-13    69.7
    ydeg 15   2.2e-13 / 1.5e-13 / 1.5e-13   3.2e-13   261.4
    ydeg 20   6.5e-14 / 4.4e-14 / 4.4e-14   3.0e-13   446.2
    whitened, ydeg  5   7.6e-15 / 1.2e-15 / 1.3e-15;   ydeg 15   2.3e-14 / 1.3e-14 / 1.3e-14
The float64 NumPy form of the kernel's own algebra reaches 1.8e-13 at ydeg 5 and 1.5e-13 at ydeg 15 on the CPU: ymu's
share is |ymu| / sd (up to 20) times the rounding of W^-1 rhs, the rest the cancellation in G - c g g^T.

What the sweep found: Engine.ylm_conditional, given sinv, sinvmu and rta1 as host arrays, uploaded each inside the
argument list and dropped the tensor at once, so the allocator gave rta1's block to sinvmu (same size) before the call
was enqueued: the design matrix was built from Sigma^-1 mu.  Errors of 0.02 to 16 sd and SP_STAR_NOT_PD at every shape
with K > 2; the kernels were right.
"""
import ctypes

import numpy as np
import pytest

import ylm_arbiter as ya
from conftest import golden

pytestmark = pytest.mark.gpu

MARK = -1234.5678125                       # sentinel of the memory outside a written region
MARK_I32 = 0x5A5A5A5A
MARK_U8 = 0xA5


def _torch():
    import torch

    return torch


def _engine(ydeg):
    from starry_process_amd.engine import get_engine

    return get_engine(ydeg, 2)


def _host(x):
    return x.detach().cpu().numpy()


def _stars(noise, order=None):
    from starry_process_amd.engine import make_stars

    o = np.arange(ya.S) if order is None else np.asarray(order)
    return make_stars(len(o), period=ya.PERIOD[o], inc_deg=ya.INC_DEG[o], baseline_var=ya.BASELINE_VAR[o],
                      baseline_mean=ya.BASELINE_MEAN[o], data_var=ya.DATA_VAR[o] if noise == "scalar" else 0.0)


def _device_design(ydeg, t, check=True):
    """The device's own design matrices of the sweep's three stars [S, K, N], checked against the oracle at
    test_cov_conditional's tolerances."""
    e = _engine(ydeg)
    A = _host(e.design_matrix(t, _stars("scalar"), e.rTA1L(ya.LIMB)))
    if check:
        ref = ya.oracle_design(ydeg, t)
        tol = 3e-10 if ydeg == 20 else 4e-12
        for s in range(ya.S):
            assert np.max(np.abs(A[s] - ref[s])) < tol * np.max(np.abs(ref[s])), s
    return A


def _assert_posterior(x, ymu, ycov, ycho, ydeg, K, what):
    """The sweep's metrics of one star against the arbiter's x, printed, then held to ya.star_bound: 10 x the
    yardstick, and never more than 32 (K + N) u cond_2(W) at the star's own cond_2(W)."""
    e_mu, e_cov, e_cho = ya.errors(x, ymu, ycov, ycho)
    cw = ya.cond2(x["W"])
    bound = ya.star_bound(ydeg, K, cw)
    print("%s: ymu %.2e ycov %.2e ycho %.2e sd (bound %.2e), cond2(W) %.1f" % (what, e_mu, e_cov, e_cho, bound, cw))
    assert cw <= ya.COND_CAP
    assert np.all(np.triu(ycho, 1) == 0)
    assert e_mu <= bound, what
    assert e_cov <= bound, what
    assert e_cho <= bound, what


# ---- 1. the sweep --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg,K,noise", ya.sweep_cases(), ids=["L%d-K%d-%s" % c for c in ya.sweep_cases()])
def test_edges_against_arbiter(ydeg, K, noise):
    """S = 3 stars per call and one call per star's prior precision (the kernel takes one per call): that star is
    checked."""
    e = _engine(ydeg)
    t, flux, d = ya.case_inputs(ydeg, K, noise)
    A = _device_design(ydeg, t)
    stars = _stars(noise)
    rta1 = e.rTA1L(ya.LIMB)
    diag = None if noise == "scalar" else d
    print()
    for q in ya.star_problems(ydeg, K, noise, A=A):
        s = q["s"]
        out = e.ylm_conditional(t, flux, stars, rta1, q["sinv"], q["sinvmu"], diag=diag, with_cho=True)
        ymu, ycov, ycho, status = (_host(o) for o in out)
        assert status.tolist() == [0] * ya.S
        x = ya.arbiter(q["A"], q["r"], q["C"], q["sinv"], q["sinvmu"])
        _assert_posterior(x, ymu[s], ycov[s], ycho[s], ydeg, K, "L%d K%d %s star %d" % (ydeg, K, noise, s))
        # without the factor of ycov: the same bits of ymu and ycov, for every star of the call
        m0, c0, none, st0 = e.ylm_conditional(t, flux, stars, rta1, q["sinv"], q["sinvmu"], diag=diag, with_cho=False)
        assert none is None and _host(st0).tolist() == [0] * ya.S
        assert np.array_equal(_host(m0), ymu) and np.array_equal(_host(c0), ycov)


def test_host_arrays_and_device_tensors_agree():
    """The wrappers take sinv, sinvmu and rta1 from the host or from the device: the same bits either way."""
    ydeg, K = 5, 33
    e = _engine(ydeg)
    t, flux, d = ya.case_inputs(ydeg, K, "vector")
    A = _device_design(ydeg, t, check=False)
    sinv, sinvmu = ya.prior_precision(A[1], 1.0 / d[1], ya.prior_seed(ydeg, K, 1))
    stars, rta1 = _stars("vector"), e.rTA1L(ya.LIMB)
    host = [_host(o) for o in e.ylm_conditional(t, flux, stars, rta1, sinv, sinvmu, diag=d)]
    rd, si, sm = e.f64(rta1), e.f64(sinv), e.f64(sinvmu)
    dev = [_host(o) for o in e.ylm_conditional(t, flux, stars, rd, si, sm, diag=d)]
    assert host[3].tolist() == [0] * ya.S
    for h, g in zip(host, dev):
        assert np.array_equal(h, g)
    B, rw = A / np.sqrt(d)[:, :, None], flux / np.sqrt(d)
    host = [_host(o) for o in e.ylm_conditional_whitened(B, rw, sinv, sinvmu)]
    dev = [_host(o) for o in e.ylm_conditional_whitened(e.f64(B), e.f64(rw), si, sm)]
    for h, g in zip(host, dev):
        assert np.array_equal(h, g)


# ---- 2. the whitened entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [5, 15])
@pytest.mark.parametrize("K", [1, 33, 65, 129])
def test_whitened_against_arbiter(ydeg, K):
    """A full data covariance of golden case c's form, whitened in long double on the host and rounded: the kernel
    alone is under test, and the arbiter runs on the rounded B and r_w."""
    e = _engine(ydeg)
    t, flux, _ = ya.case_inputs(ydeg, K, "scalar")
    A = _device_design(ydeg, t)
    rng = np.random.RandomState(77 * ydeg + K)
    B, rw = np.empty_like(A), np.empty_like(flux)
    for s in range(ya.S):
        B[s], rw[s] = ya.whiten(ya.correlated_cov(t[s], rng), A[s], flux[s] - ya.BASELINE_MEAN[s])
    print()
    for s in range(ya.S):
        sinv, sinvmu = ya.prior_precision(B[s], np.ones(K), ya.prior_seed(ydeg, K, s) + 5)
        out = e.ylm_conditional_whitened(B, rw, sinv, sinvmu, with_cho=True)
        ymu, ycov, ycho, status = (_host(o) for o in out)
        assert status.tolist() == [0] * ya.S
        x = ya.arbiter(B[s], rw[s], None, sinv, sinvmu)
        _assert_posterior(x, ymu[s], ycov[s], ycho[s], ydeg, K, "whitened L%d K%d star %d" % (ydeg, K, s))
        m0, c0, none, _ = e.ylm_conditional_whitened(B, rw, sinv, sinvmu, with_cho=False)
        assert none is None and np.array_equal(_host(m0), ymu) and np.array_equal(_host(c0), ycov)


# ---- 3. sentinels around every buffer the library writes -----------------------------------------------------------
def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def _sentinel_buffers(e, K):
    """Outputs with room for S + 1 stars, and the workspace at exactly its queried size inside a marked byte tensor."""
    torch = _torch()
    N, S = e.N, ya.S
    dev = e.device
    out = dict(ymu=torch.full(((S + 1) * N,), MARK, dtype=torch.float64, device=dev),
               ycov=torch.full(((S + 1) * N * N,), MARK, dtype=torch.float64, device=dev),
               ycho=torch.full(((S + 1) * N * N,), MARK, dtype=torch.float64, device=dev),
               status=torch.full((S + 1,), MARK_I32, dtype=torch.int32, device=dev))
    nbytes = int(e._L.sp_ylm_conditional_workspace_bytes(e._h, S, K))
    assert nbytes > 0
    head = 4096
    arena = torch.full((head + nbytes + (1 << 20),), MARK_U8, dtype=torch.uint8, device=dev)
    return out, arena, head, nbytes


def _check_sentinels(e, out, arena, head, nbytes):
    """What lies behind each buffer kept its bits; returns the S stars' (ymu, ycov, ycho, status)."""
    N, S = e.N, ya.S
    _torch().cuda.synchronize()
    ymu, ycov, ycho, status = (_host(out[k]) for k in ("ymu", "ycov", "ycho", "status"))
    mark = np.array([MARK]).view(np.uint64)[0]
    assert np.all(ymu[S * N:].view(np.uint64) == mark)
    assert np.all(ycov[S * N * N:].view(np.uint64) == mark)
    assert np.all(ycho[S * N * N:].view(np.uint64) == mark)
    assert status[S:].tolist() == [MARK_I32]
    a = _host(arena)
    assert np.all(a[:head] == MARK_U8) and np.all(a[head + nbytes:] == MARK_U8)
    return ymu[:S * N].reshape(S, N), ycov[:S * N * N].reshape(S, N, N), ycho[:S * N * N].reshape(S, N, N), status[:S]


@pytest.mark.parametrize("ydeg,K", [(5, 33), (5, 65), (7, 64), (20, 1)])
@pytest.mark.parametrize("noise", ya.NOISE)
def test_sentinels_batched(ydeg, K, noise):
    """sp_ylm_conditional_batched through ctypes: nothing behind ymu, ycov, ycho, status or the workspace is written,
    and the result is the engine wrapper's, bit for bit."""
    e = _engine(ydeg)
    t, flux, d = ya.case_inputs(ydeg, K, noise)
    A = _device_design(ydeg, t, check=False)
    sinv, sinvmu = ya.prior_precision(A[1], 1.0 / d[1], ya.prior_seed(ydeg, K, 1))
    stars, rta1 = _stars(noise), e.rTA1L(ya.LIMB)
    diag = None if noise == "scalar" else d
    ref = [_host(o) for o in e.ylm_conditional(t, flux, stars, rta1, sinv, sinvmu, diag=diag, with_cho=True)]
    out, arena, head, nbytes = _sentinel_buffers(e, K)
    td, fd, sd, rd, si, sm = e.f64(t), e.f64(flux), e.stars_to_device(stars), e.f64(rta1), e.f64(sinv), e.f64(sinvmu)
    dd = None if diag is None else e.f64(diag)
    rc = e._L.sp_ylm_conditional_batched(e._h, ya.S, K, _ptr(td), _ptr(fd), _ptr(dd) if dd is not None else None,
                                         _ptr(sd), _ptr(rd), _ptr(si), _ptr(sm), _ptr(out["ymu"]), _ptr(out["ycov"]),
                                         _ptr(out["ycho"]), _ptr(out["status"]), _ptr(arena, head), e._stream())
    assert rc == 0
    got = _check_sentinels(e, out, arena, head, nbytes)
    assert got[3].tolist() == [0] * ya.S
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    # the inputs are read only
    assert np.array_equal(_host(td), t) and np.array_equal(_host(fd), flux) and np.array_equal(_host(si), sinv)


@pytest.mark.parametrize("ydeg,K", [(5, 33), (5, 65), (7, 64), (20, 1)])
def test_sentinels_whitened(ydeg, K):
    """sp_ylm_conditional_whitened through ctypes, the same way (the design matrix stands in for L^-1 A)."""
    e = _engine(ydeg)
    t, flux, d = ya.case_inputs(ydeg, K, "scalar")
    B = _device_design(ydeg, t, check=False) / np.sqrt(d)[:, :, None]
    rw = flux / np.sqrt(d)
    sinv, sinvmu = ya.prior_precision(B[1], np.ones(K), ya.prior_seed(ydeg, K, 1))
    ref = [_host(o) for o in e.ylm_conditional_whitened(B, rw, sinv, sinvmu, with_cho=True)]
    out, arena, head, nbytes = _sentinel_buffers(e, K)
    Bd, rd, si, sm = e.f64(B), e.f64(rw), e.f64(sinv), e.f64(sinvmu)
    rc = e._L.sp_ylm_conditional_whitened(e._h, ya.S, K, _ptr(Bd), _ptr(rd), _ptr(si), _ptr(sm), _ptr(out["ymu"]),
                                          _ptr(out["ycov"]), _ptr(out["ycho"]), _ptr(out["status"]),
                                          _ptr(arena, head), e._stream())
    assert rc == 0
    got = _check_sentinels(e, out, arena, head, nbytes)
    assert got[3].tolist() == [0] * ya.S
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    assert np.array_equal(_host(Bd), B) and np.array_equal(_host(rd), rw)


# ---- 4. position in the batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg,K", [(5, 65), (15, 129)])
@pytest.mark.parametrize("noise", ya.NOISE)
def test_position_in_the_batch(ydeg, K, noise):
    """A star alone, then first, middle and last of S = 5: ymu, ycov and ycho keep their bits.  No kernel of the
    chain (prep, Gram, epilogue, sp_cho_factor, sp_cho_solve) orders its sums by the batch."""
    e = _engine(ydeg)
    t, flux, d = ya.case_inputs(ydeg, K, noise)
    rta1 = e.rTA1L(ya.LIMB)
    A = _device_design(ydeg, t, check=False)
    probe = 1
    sinv, sinvmu = ya.prior_precision(A[probe], 1.0 / d[probe], ya.prior_seed(ydeg, K, probe))

    def run(order):
        o = np.asarray(order)
        diag = None if noise == "scalar" else d[o]
        out = e.ylm_conditional(t[o], flux[o], _stars(noise, order=o), rta1, sinv, sinvmu, diag=diag, with_cho=True)
        return [_host(x) for x in out]

    alone = run([probe])
    assert alone[3].tolist() == [0]
    for pos, order in ((0, [1, 0, 2, 0, 2]), (2, [0, 2, 1, 2, 0]), (4, [2, 0, 0, 2, 1])):
        got = run(order)
        assert got[3].tolist() == [0] * 5
        for name, a, g in zip(("ymu", "ycov", "ycho"), alone, got):
            diff = np.max(np.abs(a[0] - g[pos]))
            print("L%d K%d %s position %d: max |%s - alone| = %.2e" % (ydeg, K, noise, pos, name, diff))
            assert np.array_equal(a[0], g[pos]), (name, pos)


# ---- 5. the real moments -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ydeg", ya.PRECISION_SETS, ids=["%s-L%d" % c for c in ya.PRECISION_SETS])
def test_ylm_precision_against_long_double(name, ydeg):
    """Engine.ylm_precision against a long-double inverse of Sigma_y; bound: 10 x the float64 SciPy cho_solve error
    against the same arbiter (ya.PRECISION_YARDSTICK).  Measured on an MI355X (sinv, sinvmu; the bounds):
        default ydeg  5   1.1e-13, 8.4e-17   (1.3e-12, 6.6e-16)
        default ydeg 15   2.6e-09, 5.7e-12   (2.0e-08, 8.4e-11)
        default ydeg 20   1.0e-08, 1.1e-11   (4.0e-08, 6.1e-11)
        hilat   ydeg 15   1.3e-07, 1.6e-08   (3.4e-07, 7.2e-08)
        spread  ydeg 15   8.0e-08, 9.1e-09   (4.9e-07, 1.7e-08)"""
    mom = golden("moments_L%d" % ydeg)
    mu, Sig = mom[name + "_mean_ylm"], mom[name + "_cov_ylm"]
    sinv, sinvmu = (_host(x) for x in _engine(ydeg).ylm_precision(mu, Sig))
    e_s, e_m = ya.precision_errors(*ya.precision_arbiter(mu, Sig), mu, sinv, sinvmu)
    y_s, y_m = ya.PRECISION_YARDSTICK[(name, ydeg)]
    print("\n%s L%d: sinv %.2e (bound %.2e), sinvmu %.2e (bound %.2e)"
          % (name, ydeg, e_s, ya.BOUND_FACTOR * y_s, e_m, ya.BOUND_FACTOR * y_m))
    assert e_s <= ya.BOUND_FACTOR * y_s
    assert e_m <= ya.BOUND_FACTOR * y_m


@pytest.mark.parametrize("ydeg,K", [(5, 65), (15, 129)])
@pytest.mark.parametrize("route", ["sherman_morrison", "whitened"])
def test_facade_against_arbiter(ydeg, K, route):
    """sp.ylm_conditional with the real moments (cond(W) about 1e9) against the arbiter fed with the device's own
    Sigma_y^-1 and design matrix; bound: 10 x the float64 Cholesky restatement's error at the same inputs.  `whitened`:
    one variance is 0 with baseline_var > 0, which the facade factors as a full C.  Measured on an MI355X, ymu and
    ycov in sd (the restatement's own error at the same inputs, a tenth of the bound):
        ydeg  5, K  65   sherman_morrison 2.6e-11 (1.5e-11), 4.3e-12 (2.8e-12)
                         whitened         2.4e-11 (3.1e-11), 1.0e-11 (3.3e-12)
        ydeg 15, K 129   sherman_morrison 6.8e-09 (3.6e-09), 1.3e-09 (1.3e-09)
                         whitened         8.4e-09 (3.8e-09), 3.1e-09 (2.3e-09)"""
    from starry_process_amd import StarryProcess

    mom = golden("moments_L%d" % ydeg)
    sp = StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], normalized=False)
    t, flux, d = ya.case_inputs(ydeg, K, "vector")
    s = 1
    kw = dict(i=ya.INC_DEG[s], p=ya.PERIOD[s], u=ya.LIMB, baseline_mean=ya.BASELINE_MEAN[s])
    b = ya.BASELINE_VAR[s]
    dv = d[s].copy()
    if route == "whitened":
        dv[K // 3] = 0.0
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional(t[s], flux[s], dv, baseline_var=b, **kw))
    A = np.array(sp._flux.design_matrix(t[s], kw["i"], kw["p"], kw["u"]))
    sinv, sinvmu = (_host(x) for x in sp._ylm_precision())
    sinv = np.tril(sinv) + np.tril(sinv, -1).T          # the triangle the kernel reads
    r = flux[s] - kw["baseline_mean"]
    C = ya.data_cov(dv, b, K)
    x = ya.arbiter(A, r, C, sinv, sinvmu)
    y_mu, y_cov, _ = ya.errors(x, *ya.restatement(A, r, C, sinv, sinvmu)[:2])
    e_mu, e_cov, _ = ya.errors(x, ymu, ycov)
    print("\nfacade L%d K%d %s: ymu %.2e (restatement %.2e), ycov %.2e (restatement %.2e) sd"
          % (ydeg, K, route, e_mu, y_mu, e_cov, y_cov))
    assert e_mu <= ya.BOUND_FACTOR * y_mu
    assert e_cov <= ya.BOUND_FACTOR * y_cov
