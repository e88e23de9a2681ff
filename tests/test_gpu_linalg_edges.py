"""
The general-purpose fp64 linear algebra of the C ABI at its layout edges: sp_gemm_nt on each of its three kernels,
sp_cho_factor at every remainder size of the blocked factorisation, the triangular solves and their reverse modes,
sp_gp_condition with many riding rows, sp_spd_inverse_batched on strided input.

The entry points are called through ctypes wherever the engine's wrappers cannot express a case (leading dimensions,
batch strides, pointer offsets).  Every buffer the library writes to is larger than the region it may write, and is
pre-filled with a marked value: everything outside that region must keep its bits.  The references are NumPy / SciPy
in float64, np.longdouble where the point is precision; every input is seeded.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg

from conftest import golden
from oracle import sp_oracle as orc

pytestmark = pytest.mark.gpu

U = np.finfo(np.float64).eps / 2          # unit roundoff
MARK = -1234.5678125                       # sentinel of the memory outside a written region
SP_OK, SP_ERR_INVALID = 0, -1


def _e():
    from starry_process_amd.engine import get_engine

    return get_engine(5, 2)


def _torch():
    import torch

    return torch


def _up(a):
    """Host array -> device float64 tensor (exact copy)."""
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(_e().device)


def _down(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _i32(n, fill=0):
    torch = _torch()
    return torch.full((n,), fill, dtype=torch.int32, device=_e().device)


def _p(t, off=0):
    """Device pointer to element `off` of tensor t."""
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * off)


def _call(name, *args):
    """sp_<name>(handle, *args, stream): the raw status."""
    e = _e()
    rc = getattr(e._L, name)(e._h, *args, e._stream())
    _torch().cuda.synchronize()
    return rc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _strided(mats, ld, stride, off=0, fill=MARK):
    """Flat buffer holding mats [b, r, c] at element off + b stride + i ld + j, `fill` everywhere else (plus a tail),
    and the mask of the places the matrices occupy."""
    b, r, c = mats.shape
    n = off + (b - 1) * stride + (r - 1) * ld + c + 37 if b else 37
    buf = np.full(n, fill)
    mask = np.zeros(n, dtype=bool)
    for s in range(b):
        for i in range(r):
            o = off + s * stride + i * ld
            buf[o:o + c] = mats[s, i]
            mask[o:o + c] = True
    return buf, mask


def _unstride(buf, shape, ld, stride, off=0):
    b, r, c = shape
    out = np.empty(shape)
    for s in range(b):
        for i in range(r):
            o = off + s * stride + i * ld
            out[s, i] = buf[o:o + c]
    return out


def _spd(rng, K):
    """Well-conditioned SPD matrix (condition ~5)."""
    B = rng.randn(K, K)
    return B.dot(B.T) + K * np.eye(K)


# ---------------------------------------------------------------------------------------------------------------------
# 1. sp_gemm_nt:  C[b] = beta C[b] + alpha A[b] B[b]^T
# launch_gemm (csrc/sp_gemm.hip) takes
#   MM2<128, 128>   M, N multiples of 128, K a multiple of 32, even lda / ldb / strides, 16-byte aligned A and B,
#                   not lower_only;
#   MM2<64, 64>     the other such calls with M, N multiples of 64, and every such lower_only call;
#   gemm_nt_kernel  everything else (K = 0, K % 32 != 0, odd lda, misaligned A, ragged M or N).
# Each MM2 has an alpha = +-1 instantiation (accumulators start from +-C) and one for any other alpha.
# ---------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [
    # (id, M, N, K, lda, ldb, offA, batch, lower_only allowed)
    ("mm128", 256, 256, 256, 258, 256, 0, 3, True),       # MM2<128,128>; lower_only -> MM2<64,64>
    ("mm64_m64", 64, 256, 256, 256, 260, 0, 9, False),    # MM2<64,64>: M = 64 is not a multiple of 128
    ("mm64_m192", 192, 256, 96, 96, 96, 0, 17, False),    # MM2<64,64>: M = 192
    ("mm64_lower", 192, 192, 64, 64, 66, 0, 1, True),     # MM2<64,64> (lower_only) / MM2<64,64> (not: 192 % 128)
    ("gen_k100", 128, 128, 100, 100, 100, 0, 3, True),    # generic: K % 32 != 0
    ("gen_odd_lda", 128, 128, 64, 65, 64, 0, 9, True),    # generic: odd lda
    ("gen_offA", 128, 256, 64, 64, 64, 1, 3, False),      # generic: A one double past 16-byte alignment
    ("gen_1x63", 1, 63, 40, 40, 41, 0, 17, False),        # generic: ragged M, N
    ("gen_65x129", 65, 129, 33, 33, 33, 0, 3, False),     # generic: ragged
    ("gen_129x65", 129, 65, 64, 64, 64, 0, 1, False),     # generic: ragged (K fine, M, N not)
    ("gen_lower65", 65, 65, 31, 31, 31, 0, 9, True),      # generic: ragged lower_only
    ("gen_lower129", 129, 129, 96, 96, 97, 0, 3, True),   # generic: ragged lower_only
    ("k0", 64, 64, 0, 0, 0, 0, 3, True),                  # generic: K = 0 (C = beta C)
]


def _gemm_run(A, B, C0, alpha, beta, lower, lda, ldb, offA):
    """One sp_gemm_nt call on strided copies of A [b,M,K], B [b,N,K], C0 [b,M,N] (beta = 1; NaN where beta = 0).
    The gaps of A and B hold NaN (never read), C lives at ldc = N + 3 / strideC = M ldc + 5 inside MARK.
    Checks the operands and everything around C, returns C [b,M,N]."""
    b, M, K = A.shape
    N = B.shape[1]
    sA, sB = M * lda + 2 * (lda % 2 == 0) + (lda % 2), N * ldb + 2 * (ldb % 2 == 0) + (ldb % 2)
    ldc = N + 3
    sC = M * ldc + 5
    Ah, _ = _strided(A, lda, sA, offA, fill=np.nan)
    Bh, _ = _strided(B, ldb, sB, 0, fill=np.nan)
    Cin = C0 if beta else np.full_like(C0, np.nan)
    Ch, cmask = _strided(Cin, ldc, sC)
    Ad, Bd, Cd = _up(Ah), _up(Bh), _up(Ch)
    rc = _call("sp_gemm_nt", _p(Ad, offA), lda, sA, _p(Bd), ldb, sB, _p(Cd), ldc, sC, M, N, K, float(alpha),
               int(beta), int(lower), b)
    assert rc == SP_OK
    # the operands are read only
    assert np.array_equal(_bits(_down(Ad)), _bits(Ah)) and np.array_equal(_bits(_down(Bd)), _bits(Bh))
    Cout = _down(Cd)
    # nothing outside the matrices changes: the ldc gaps, the space between batches, the tail
    assert np.array_equal(_bits(Cout[~cmask]), _bits(Ch[~cmask]))
    Cm = _unstride(Cout, (b, M, N), ldc, sC)
    if lower:
        # strictly-upper 64 x 64 tiles keep their bits
        ti, tj = np.arange(M)[:, None] // 64, np.arange(N)[None, :] // 64
        up = np.broadcast_to(tj > ti, Cm.shape)
        assert np.array_equal(_bits(Cm[up]), _bits(Cin[up]))
    return Cm


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_nt_exact(case):
    """Integer entries in [-4, 4], integer C0 and dyadic alpha: every product and partial sum is exact in fp64, so
    the result must equal the host product bit for bit whatever the summation order -- any indexing, tile-map,
    accumulator-layout or dropped-slice error shows."""
    _, M, N, K, lda, ldb, offA, batch, lower_ok = case
    rng = np.random.RandomState(M * 7 + N * 3 + K)
    A = rng.randint(-4, 5, (batch, M, K)).astype(np.float64)
    B = rng.randint(-4, 5, (batch, N, K)).astype(np.float64)
    C0 = rng.randint(-50, 51, (batch, M, N)).astype(np.float64)
    P = A @ B.transpose(0, 2, 1)                 # exact: integers far below 2^53
    ti, tj = np.arange(M)[:, None] // 64, np.arange(N)[None, :] // 64
    for lower in ((0, 1) if lower_ok else (0,)):
        for alpha in (1.0, -1.0, 0.375):
            for beta in (0, 1):
                C = _gemm_run(A, B, C0, alpha, beta, lower, lda, ldb, offA)
                ref = alpha * P + beta * C0
                sel = np.broadcast_to(tj <= ti, C.shape) if lower else np.ones(C.shape, bool)
                assert not np.isnan(C[sel]).any(), (lower, alpha, beta)     # beta = 0 reads no C
                assert np.array_equal(C[sel], ref[sel]), (lower, alpha, beta)


@pytest.mark.parametrize("M,N,K,lower", [(256, 256, 512, 0),   # MM2<128,128>
                                         (64, 256, 288, 0),    # MM2<64,64>
                                         (192, 192, 160, 1),   # MM2<64,64>, lower_only
                                         (100, 70, 333, 0),    # generic
                                         (129, 129, 64, 1)])   # generic, lower_only
def test_gemm_nt_precision(M, N, K, lower):
    """Normal inputs against a long-double product: |C - C_ref| <= 2 K u (|alpha| |A| |B|^T + beta |C0|) elementwise.
    Catches fp32 intermediates and lost FMAs, which the integer test cannot see."""
    rng = np.random.RandomState(M + N + K)
    batch = 2
    A, B, C0 = rng.randn(batch, M, K), rng.randn(batch, N, K), rng.randn(batch, M, N)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    P = np.einsum("bik,bjk->bij", Al, Bl)
    absP = np.abs(A) @ np.abs(B).transpose(0, 2, 1)
    ti, tj = np.arange(M)[:, None] // 64, np.arange(N)[None, :] // 64
    sel = np.broadcast_to(tj <= ti, (batch, M, N)) if lower else np.ones((batch, M, N), bool)
    for alpha in (1.0, -1.0, 0.3):
        for beta in (0, 1):
            C = _gemm_run(A, B, C0, alpha, beta, lower, K, K, 0)
            ref = np.longdouble(alpha) * P + beta * C0.astype(np.longdouble)
            err = np.abs((C.astype(np.longdouble) - ref).astype(np.float64))
            bound = 2 * K * U * (abs(alpha) * absP + beta * np.abs(C0))
            assert np.all(err[sel] <= bound[sel]), (alpha, beta, np.max(err[sel] / bound[sel]))


_processes = {}


def _SP15(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _processes:
        from starry_process_amd import StarryProcess

        mom = golden("moments_L15")
        _processes[key] = StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"],
                                        normalized=False, **kw)
    return _processes[key]


@pytest.mark.parametrize("nsamples", [1, 63, 64, 128, 129])
def test_sample_ylm_conditional_product(nsamples):
    """sample_ylm_conditional = ymu + (ycho z)^T: at ydeg 15, nsamples 64 runs MM2<64,64> and 128 runs MM2<128,128>
    through sp_gemm_nt, the others the generic kernel.  Against the host product on the same ycho and deviates, to
    1e-12 posterior standard deviations (plus the rounding of adding ymu)."""
    sp = _SP15(marginalize_over_inclination=False)
    rng = np.random.RandomState(nsamples)
    K = 300
    t = np.linspace(0, 3, K)
    flux = 1e-3 * np.sin(2 * np.pi * t / 0.9) + 1e-3 * rng.randn(K)
    kw = dict(i=60.0, p=0.9, u=[0.3, 0.1], baseline_mean=1e-4, baseline_var=1e-6)
    smp = np.array(sp.sample_ylm_conditional(t, flux, 1e-6, nsamples=nsamples, seed=5, **kw))
    ymu, ycov, ycho = (x.cpu().numpy() for x in sp._ylm_posterior(t, flux, 1e-6, with_cho=True, **kw))
    z = np.random.RandomState(5).normal(size=(256, nsamples))
    ref = ymu[None, :] + (ycho @ z).T
    sd = np.sqrt(np.diag(ycov))
    assert smp.shape == (nsamples, 256)
    assert np.all(np.abs(smp - ref) <= 1e-12 * sd[None, :] + 4 * U * np.abs(ymu)[None, :])


def test_ylm_conditional_ensemble_product():
    """ylm_conditional_ensemble's samples with nsamples = 64: one batched sp_gemm_nt on MM2<64,64> over 9 stars (not a
    multiple of the 8 XCDs), against the host product with each star's own factor."""
    sp = _SP15()
    S, K, nsm = 9, 200, 64
    rng = np.random.RandomState(17)
    t = np.linspace(0, 3, K)
    p, inc = 0.6 + rng.rand(S), 20 + 65 * rng.rand(S)
    flux = 1e-3 * np.sin(2 * np.pi * t[None, :] / p[:, None]) + 1e-3 * rng.randn(S, K)
    dcov = 1e-6 * (1 + rng.rand(S))
    ymu, ycov, smp = (np.array(x) for x in sp.ylm_conditional_ensemble(t, flux, dcov, i=inc, p=p, u=[0.3, 0.1],
                                                                       nsamples=nsm, seed=3))
    # the same device posterior (every variance > 0: one call, no per-star fallback)
    e = sp._engine
    tt, fl, stars, utab, diag = sp._ensemble_args(t, flux, dcov, inc, p, [0.3, 0.1], 0.0, 0.0)
    sinv, sinvmu = sp._ylm_precision()
    m, c, ycho, _ = e.ylm_conditional(tt, fl, stars, e.f64(e.rTA1L(utab)), sinv, sinvmu, diag=diag, with_cho=True)
    m, ycho = m.cpu().numpy(), ycho.cpu().numpy()
    assert np.array_equal(m, ymu)
    z = np.random.RandomState(3).normal(size=(S, 256, nsm))
    for s in range(S):
        sd = np.sqrt(np.diag(ycov[s]))
        ref = ymu[s][None, :] + (ycho[s] @ z[s]).T
        assert np.all(np.abs(smp[s] - ref) <= 1e-12 * sd[None, :] + 4 * U * np.abs(ymu[s])[None, :]), s


# ---------------------------------------------------------------------------------------------------------------------
# 2. sp_cho_factor at every remainder size.  csrc/sp_cholesky.hip: super-panels of 4 panels below 16 pivot steps, 8
# from 16 on (960 -> 961); a partial last pivot block; trailing remainders of 17 or more 64-blocks on syrk128_kernel
# (csrc/sp_gemm.hip, sp_launch_syrk_diag): K = 1600 (Kp = 1600, first remainder 1600 - 512 = 17 blocks) and K = 2100
# (Kp = 2112: remainders of 25 and 17 blocks, then 9).
# ---------------------------------------------------------------------------------------------------------------------
K_SWEEP = sorted({1, 2, 7, 960, 961, 1600, 2100} |
                 {64 * n + d for n in (1, 2, 4, 5, 8, 9, 15, 16, 17) for d in (-1, 0, 1)})


def _factor(A, lda=None, stride=None, info_fill=0):
    """sp_cho_factor on A [b,K,K] at (lda, stride) inside MARK; returns (L [b,K,K], info, buffer out, buffer in,
    mask)."""
    b, K, _ = A.shape
    lda = K if lda is None else lda
    stride = K * lda if stride is None else stride
    h, mask = _strided(A, lda, stride)
    d = _up(h)
    info = _i32(b, info_fill)
    assert _call("sp_cho_factor", _p(d), K, lda, stride, b, _p(info)) == SP_OK
    out = _down(d)
    return _unstride(out, A.shape, lda, stride), _down(info), out, h, mask


def _cov(K, seed):
    """The library's own marginal covariance of a synthetic light curve plus its data variance (what the likelihood
    factors: ill-conditioned)."""
    from starry_process_amd.synthetic import synthetic_star

    st = synthetic_star(seed, K)
    C = np.array(_SP15().cov(st["t"], p=st["p"]))
    return C + st["data_cov"] * np.eye(K)


@pytest.mark.parametrize("K", K_SWEEP)
def test_cho_factor_sweep(K):
    """Forward error on a well-conditioned matrix (within 5e-14 of max |L| of LAPACK's factor), backward error on an
    ill-conditioned covariance (condition up to 1e6: |A - L L^T| <= 32 K u |L| |L^T| elementwise; the residual is formed
    in fp64, and the rows below a pivot block are products with the block's explicit inverse, which is not
    componentwise stable -- the worst K of the sweep measured 9.5 K u), and an exactly zero strict upper triangle.
    A factor wrong in its tenth digit is 13x over the bound at K = 2100."""
    rng = np.random.RandomState(K)
    C = _spd(rng, K)
    Cv = _cov(K, K % 7) if K > 1 else np.array([[2.5e-6]])
    L, info, _, _, _ = _factor(np.stack([C, Cv]))
    assert not info.any()
    assert np.array_equal(np.triu(L[0], 1), np.zeros((K, K))) and np.array_equal(np.triu(L[1], 1), np.zeros((K, K)))
    ref = np.linalg.cholesky(C)
    assert np.abs(L[0] - ref).max() < 5e-14 * np.abs(ref).max()
    Lv = L[1]
    res = np.abs(Cv - Lv @ Lv.T)
    bound = 32 * K * U * (np.abs(Lv) @ np.abs(Lv).T)
    il = np.tril_indices(K)
    ratio = np.max(res[il] / bound[il])
    ev = np.linalg.eigvalsh(Cv)
    print("K = %d: condition %.2g, backward error / (32 K u |L| |L^T|) = %.3g" % (K, ev[-1] / ev[0], ratio))
    assert ratio <= 1.0, ratio


def _bad_at(C, p):
    """C with its leading p x p block intact and pivot p equal to -1 (not positive definite exactly there)."""
    L = np.linalg.cholesky(C)
    B = C.copy()
    B[p, p] -= L[p, p] ** 2 + 1.0
    return B


@pytest.mark.parametrize("K", [1100, 200])
def test_cho_factor_batch_isolation(K):
    """Matrices that fail at chosen pivots -- in the first block, inside a later super-panel, in the partial last
    block and at pivot K - 1 -- are flagged alone and come back all NaN; the other matrices of the batch have the
    bits they have in a batch without them."""
    rng = np.random.RandomState(K + 1)
    g = [_spd(rng, K) for _ in range(3)]
    # K = 1100: 18 pivot steps, super-panels of 8 (blocks 0-7, 8-15, 16-17), last block 12 columns wide
    # K = 200: 4 pivot steps, one super-panel of 4, last block 8 columns wide
    pivots = [5, 64 * 9 + 10, K - 6, K - 1] if K > 1000 else [5, 64 * 2 + 3, K - 6, K - 1]
    bad = [_bad_at(g[k % 3], p) for k, p in enumerate(pivots)]
    Lg, info_g, _, _, _ = _factor(np.stack(g))
    assert not info_g.any()
    mats = [g[0], bad[0], bad[1], g[1], bad[2], g[2], bad[3]]
    L, info, _, _, _ = _factor(np.stack(mats))
    assert info.tolist() == [0, 1, 1, 0, 1, 0, 1]
    for k in (1, 2, 4, 6):
        assert np.isnan(L[k]).all(), k
    for k, j in ((0, 0), (3, 1), (5, 2)):
        assert np.array_equal(_bits(L[k]), _bits(Lg[j])), k


def test_cho_factor_batch_zero_touches_nothing():
    K = 70
    A = _spd(np.random.RandomState(0), K)
    d = _up(A)
    info = _i32(1, 7)
    assert _call("sp_cho_factor", _p(d), K, K, K * K, 0, _p(info)) == SP_OK
    assert np.array_equal(_bits(_down(d)), _bits(A)) and _down(info).tolist() == [7]


@pytest.mark.parametrize("K", [1, 63, 65, 200, 961])
def test_cho_factor_layout(K):
    """lda = K + 3 and strideA > K lda: the same bits as the contiguous call, and every gap keeps its bits."""
    rng = np.random.RandomState(K + 2)
    A = np.stack([_spd(rng, K) for _ in range(3)])
    L0, info0, _, _, _ = _factor(A)
    lda = K + 3
    L1, info1, out, h, mask = _factor(A, lda, K * lda + 11)
    assert not info0.any() and not info1.any()
    assert np.array_equal(_bits(L1), _bits(L0))
    assert np.array_equal(_bits(out[~mask]), _bits(h[~mask]))


@pytest.mark.parametrize("K", [7, 65, 961, 1600])
def test_cho_factor_upper_triangle(K):
    """Only the lower triangle enters the factor (LAPACK potrf('L')): a finite asymmetric strict upper triangle gives
    the bits of the matrix mirrored from its lower triangle.  A NaN or inf in the strict upper triangle gives the
    reference's answer: scipy's check_finite raises, math.py:83-91 returns NaN -- all NaN and info 1."""
    rng = np.random.RandomState(K + 3)
    C = _spd(rng, K)
    asym = np.tril(C) + np.triu(rng.randn(K, K) * K, 1)
    Lsym, info_s, _, _, _ = _factor(C[None])
    Lasym, info_a, _, _, _ = _factor(asym[None])
    assert not info_s.any() and not info_a.any()
    assert np.array_equal(_bits(Lasym), _bits(Lsym))
    for bad in (np.nan, np.inf, -np.inf):
        X = C.copy()
        X[K // 3, K - 1] = bad                       # strict upper triangle (K // 3 < K - 1 for K > 1)
        L, info, _, _, _ = _factor(np.stack([C, X]))
        assert info.tolist() == [0, 1], bad
        assert np.isnan(L[1]).all(), bad
        assert np.array_equal(_bits(L[0]), _bits(Lsym[0])), bad
        assert np.isnan(orc.cho_factor(X)).all()     # the reference's semantics


# ---------------------------------------------------------------------------------------------------------------------
# 3. Triangular solves and their reverse modes.  L lives at ldl = K + 5 with NaN in the gap; the solves (which read
# the lower triangle only) also get NaN in the strict upper triangle, sp_cholesky_rev (which needs zeros there) not.
# ---------------------------------------------------------------------------------------------------------------------
K_SOLVE = [1, 7, 63, 64, 65, 127, 129, 255, 257, 511, 513, 961, 1025]


def _L_buffer(Ls, upper_nan):
    b, K, _ = Ls.shape
    ldl = K + 5
    sL = K * ldl + 7
    M = np.array(Ls)
    if upper_nan:
        iu = np.triu_indices(K, 1)
        for s in range(b):
            M[s][iu] = np.nan
    h, _ = _strided(M, ldl, sL, fill=np.nan)
    return _up(h), ldl, sL


@pytest.mark.parametrize("K", K_SOLVE)
def test_solves(K):
    """sp_cho_solve and sp_tri_solve (both directions) against SciPy, relative 1e-12, for nrhs 0 .. 300."""
    rng = np.random.RandomState(K + 4)
    b = 2
    Ls = np.stack([np.linalg.cholesky(_spd(rng, K)) for _ in range(b)])
    Ld, ldl, sL = _L_buffer(Ls, upper_nan=True)
    for nrhs in (0, 1, 63, 64, 65, 300):
        rhs = rng.randn(b, K, nrhs)
        for what in ("cho", 0, 1):
            bd = _up(rhs if nrhs else np.full(4, MARK))     # (nrhs = 0: a real pointer, which must stay untouched)
            if what == "cho":
                rc = _call("sp_cho_solve", _p(Ld), K, ldl, sL, _p(bd), nrhs, b)
            else:
                rc = _call("sp_tri_solve", _p(Ld), K, ldl, sL, _p(bd), nrhs, b, what)
            assert rc == SP_OK
            x = _down(bd)
            if nrhs == 0:
                assert (x == MARK).all()
                continue
            for s in range(b):
                if what == "cho":
                    ref = scipy.linalg.cho_solve((Ls[s], True), rhs[s])
                else:
                    ref = scipy.linalg.solve_triangular(Ls[s], rhs[s], lower=True, trans=what)
                assert np.abs(x[s] - ref).max() <= 1e-12 * np.abs(ref).max(), (what, nrhs, s)


@pytest.mark.parametrize("K", [1, 63, 65, 129, 257, 513, 961])
def test_reverse_modes(K):
    """sp_solve_rev (both directions) and sp_cholesky_rev on strided L against the oracle's solve_L_op and
    cholesky_L_op, 1e-12 of the largest entry."""
    rng = np.random.RandomState(K + 5)
    b = 2
    Ls = np.stack([np.linalg.cholesky(_spd(rng, K)) for _ in range(b)])
    Ld, ldl, sL = _L_buffer(Ls, upper_nan=False)
    for nrhs in (1, 65):
        c, cbar = rng.randn(b, K, nrhs), rng.randn(b, K, nrhs)
        cd, cbd = _up(c), _up(cbar)
        for trans in (0, 1):
            Abar, bbar = _up(np.zeros((b, K, K))), _up(np.zeros((b, K, nrhs)))
            assert _call("sp_solve_rev", _p(Ld), K, ldl, sL, _p(cd), _p(cbd), nrhs, b, trans,
                         _p(Abar), _p(bbar)) == SP_OK
            Abar, bbar = _down(Abar), _down(bbar)
            for s in range(b):
                Am = Ls[s].T if trans else Ls[s]
                rA, rb = orc.solve_L_op(Am, None, c[s], cbar[s], not trans)
                assert np.abs(Abar[s] - rA).max() <= 1e-12 * np.abs(rA).max(), (nrhs, trans, s)
                assert np.abs(bbar[s] - rb).max() <= 1e-12 * np.abs(rb).max(), (nrhs, trans, s)
    Lbar = np.tril(rng.randn(b, K, K))
    Cbar, Lbd = _up(np.zeros((b, K, K))), _up(Lbar)
    assert _call("sp_cholesky_rev", _p(Ld), K, ldl, sL, _p(Lbd), b, _p(Cbar)) == SP_OK
    Cbar = _down(Cbar)
    for s in range(b):
        ref = orc.cholesky_L_op(Ls[s], Lbar[s])
        assert np.abs(Cbar[s] - ref).max() <= 1e-12 * np.abs(ref).max(), s


def test_solve_limits():
    """The documented limits: sp_cho_solve caps nrhs and batch at 65535, sp_tri_solve and sp_cholesky_rev cap batch;
    SP_ERR_INVALID and nothing written.  sp_tri_solve takes any nrhs (checked at 70 000 against SciPy)."""
    big = 65536
    L1 = _up(np.full(big, 2.0))                         # K = 1 factors, strideL = 1
    b0 = np.arange(big, dtype=np.float64)
    for args in (("sp_cho_solve", _p(L1), 1, 1, 1, None, big, 1),
                 ("sp_cho_solve", _p(L1), 1, 1, 1, None, 1, big),
                 ("sp_tri_solve", _p(L1), 1, 1, 1, None, 1, big, 0)):
        bd = _up(b0)
        args = tuple(_p(bd) if a is None else a for a in args)
        assert _call(*args) == SP_ERR_INVALID, args[0]
        assert np.array_equal(_bits(_down(bd)), _bits(b0)), args[0]
    cbar, lbar = _up(np.full(big, MARK)), _up(np.ones(big))
    assert _call("sp_cholesky_rev", _p(L1), 1, 1, 1, _p(lbar), big, _p(cbar)) == SP_ERR_INVALID
    assert (_down(cbar) == MARK).all()
    # nrhs above 65535 on sp_tri_solve
    rng = np.random.RandomState(6)
    K, nrhs = 3, 70000
    L = np.linalg.cholesky(_spd(rng, K))
    rhs = rng.randn(K, nrhs)
    for trans in (0, 1):
        bd, Ld = _up(rhs), _up(L)
        assert _call("sp_tri_solve", _p(Ld), K, K, K * K, _p(bd), nrhs, 1, trans) == SP_OK
        ref = scipy.linalg.solve_triangular(L, rhs, lower=True, trans=trans)
        assert np.abs(_down(bd) - ref).max() <= 1e-12 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------------
# 4. sp_gp_condition: K_tt factored with K_st and r riding as Ks + 1 rows below it (Kp = roundup(K + Ks + 1, 64)),
# then mu = Y w and K_ss -= Y Y^T through sp_gemm_nt at row stride Kp.
# ---------------------------------------------------------------------------------------------------------------------
GP_CASES = [(1, 1), (10, 1000),       # ten pivots, 1001 riding rows: many more riding rows than pivots
            (63, 1), (64, 64),
            (100, 29),                # K + Ks + 1 = 130: the riding rows cross a tile boundary
            (960, 64), (961, 63),     # super-panel width switch; riding rows in the partial last block
            (1000, 1000),             # the realistic predict shape: 1001 riding rows across super-panels
            (1024, 128)]              # K % 32 == 0, Ks % 128 == 0: K_ss -= Y Y^T on MM2<128,128> (mu: N = 1, generic)


def _gp(Ktt, Kst, Kss, r):
    K, Ks = Ktt.shape[0], Kss.shape[0]
    d = [_up(x) for x in (Ktt, Kst, Kss, r)]
    mu = _up(np.full(Ks, MARK))
    info = _i32(1, 0)
    assert _call("sp_gp_condition", K, Ks, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(mu), _p(info)) == SP_OK
    for x, h in ((d[0], Ktt), (d[1], Kst), (d[3], r)):
        assert np.array_equal(_bits(_down(x)), _bits(h))      # inputs are not modified
    return _down(mu), _down(d[2]), int(_down(info)[0])


@pytest.mark.parametrize("K,Ks", GP_CASES)
def test_gp_condition(K, Ks):
    """mu = K_st K_tt^-1 r and K_ss - K_st K_tt^-1 K_st^T against a host float64 Cholesky, 1e-12 of the scale."""
    rng = np.random.RandomState(K * 3 + Ks)
    Ktt = _spd(rng, K)
    Kst = rng.randn(Ks, K)
    Kss = _spd(rng, Ks) / Ks
    r = rng.randn(K)
    mu, Kpost, info = _gp(Ktt, Kst, Kss, r)
    assert info == 0
    Lh = np.linalg.cholesky(Ktt)
    Y = scipy.linalg.solve_triangular(Lh, Kst.T, lower=True)
    w = scipy.linalg.solve_triangular(Lh, r, lower=True)
    mu_ref, Q = Y.T @ w, Y.T @ Y
    assert np.abs(mu - mu_ref).max() <= 1e-12 * np.abs(mu_ref).max()
    scale = max(np.abs(Kss).max(), np.abs(Q).max())
    assert np.abs(Kpost - (Kss - Q)).max() <= 1e-12 * scale
    if (K, Ks) == (100, 29):
        bad = Ktt.copy()
        bad[50, 50] = -1.0
        assert _gp(bad, Kst, Kss, r)[2] == 1


@pytest.mark.parametrize("tau", [None, 2.0])
def test_predict_realistic(tau):
    """StarryProcess.predict with 1000 observed cadences and 1000 sample times (marginal; time-variable with tau)
    against the reference's algebra (its sp.py:767-903) restated in NumPy on the library's own covariance blocks,
    to 1e-9 of the prior scale like tests/test_gpu_facade.py."""
    from starry_process_amd.defaults import defaults

    kw = {} if tau is None else dict(tau=tau)
    sp = _SP15(marginalize_over_inclination=True, **kw)
    rng = np.random.RandomState(8)
    K, Ks = 1000, 1000
    t = np.linspace(0, 4, K)
    ts = np.linspace(-0.5, 4.5, Ks)
    flux = 1e-2 * np.sin(2 * np.pi * t / 0.9) + 1e-3 * rng.randn(K)
    dcov, bmean, bvar = 1e-6, 1e-4, 1e-6
    kw = dict(p=0.9, u=[0.3, 0.1])
    mu, Kp = (np.array(x) for x in sp.predict(t, flux, dcov, t_sample=ts, baseline_mean=bmean, baseline_var=bvar,
                                               **kw))
    _, cov, fmean = sp._device_cov(np.concatenate([ts, t]), defaults["i"], kw["p"], kw["u"])
    cov, mean = cov.cpu().numpy(), float(fmean)
    K_ts_ts = cov[:Ks, :Ks] + bvar
    K_ts_t = cov[:Ks, Ks:] + bvar
    K_t_t = cov[Ks:, Ks:] + dcov * np.eye(K) + bvar
    cho = scipy.linalg.cho_factor(K_t_t, lower=True)
    mu_ref = mean + K_ts_t @ scipy.linalg.cho_solve(cho, flux - bmean - mean)
    K_ref = K_ts_ts - K_ts_t @ scipy.linalg.cho_solve(cho, K_ts_t.T)
    scale = np.abs(K_ts_ts).max()
    assert np.abs(mu - mu_ref).max() < 1e-9 * np.abs(mu_ref).max() + 1e-12
    assert np.abs(Kp - K_ref).max() < 1e-9 * scale


# ---------------------------------------------------------------------------------------------------------------------
# 5. sp_spd_inverse_batched on strided input (the K sweep is in tests/test_gpu_linalg_rev.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 961])
def test_spd_inverse_strided(K):
    """ldc = K + 3, strideC > K ldc, NaN in every gap: the bits of the contiguous call."""
    e = _e()
    rng = np.random.RandomState(K + 9)
    S = 2
    A = rng.randn(S, K, K)
    C = A @ A.transpose(0, 2, 1) / K + 0.5 * np.eye(K)[None]
    Kr = (K + 63) // 64 * 64
    ws = _torch().empty(int(e._L.sp_spd_inverse_workspace_bytes(e._h, S, K)), dtype=_torch().uint8,
                        device=e.device)

    def run(ldc, stride):
        h, _ = _strided(C, ldc, stride, fill=np.nan)
        hd, out, logdet, info = _up(h), _up(np.zeros((S, Kr, Kr))), _up(np.zeros(S)), _i32(S)
        assert _call("sp_spd_inverse_batched", S, K, _p(hd), ldc, stride, _p(out), _p(logdet), _p(info),
                     _p(ws)) == SP_OK
        return _down(out), _down(logdet), _down(info)

    i0, l0, f0 = run(K, K * K)
    i1, l1, f1 = run(K + 3, K * (K + 3) + 5)
    assert not f0.any() and not f1.any()
    assert np.array_equal(_bits(i1), _bits(i0)) and np.array_equal(_bits(l1), _bits(l0))
    low = np.tril(i1[:, :K, :K])
    inv = low + np.tril(low, -1).transpose(0, 2, 1)
    ref = np.linalg.inv(C)
    assert np.abs(inv - ref).max() < 1e-10 * np.abs(ref).max()
