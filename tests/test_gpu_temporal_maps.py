"""
GPU checks of the time-variable surface maps (sp_temporal_gram, sp_ylm_temporal, sp_flux_rows; reference
sp.py:489-516, 1237-1282): parity with the reference's recorded samples and light curves, the triangular products
against NumPy with an element-wise rounding bound, batch independence, an exact tie of the whole chain to the
covariance of the process, and the tutorial's flow on the public class.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS = np.finfo(np.float64).eps
KERNELS = {1: "Matern32Kernel", 2: "ExpSquaredKernel"}
I, P, U = 65.0, 0.8, [0.2, 0.1]


def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _engine(ydeg):
    from starry_process_amd.engine import get_engine

    return get_engine(ydeg, 2, 0)


def _process(case, **kw):
    from starry_process_amd import StarryProcess, temporal

    g = _golden("temporal")
    kind, tau, ydeg = g[case + "_scalars"][:3]
    mom = _golden("moments_L%d" % int(ydeg))
    sp = StarryProcess(ydeg=int(ydeg), tau=float(tau), temporal_kernel=getattr(temporal, KERNELS[int(kind)]),
                       mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)
    return sp, g


# ---- parity with the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_sample_ylm_matches_the_reference(case):
    sp, g = _process(case, normalized=False)
    ns, seed = int(g[case + "_scalars"][3]), int(g[case + "_scalars"][4])
    Y = np.array(sp.sample_ylm(g[case + "_t"], nsamples=ns, seed=seed))
    ref = g[case + "_Y"]
    assert Y.shape == ref.shape
    assert np.max(np.abs(Y - ref)) <= 1e-10 * np.max(np.abs(ref))


@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("normalized", [False, True])
def test_flux_matches_the_reference(case, normalized):
    sp, g = _process(case, normalized=normalized)
    t, Y = g[case + "_t"], g[case + "_Y"]
    sfx = "n" if normalized else ""
    for y, key in ((Y, "_flux3"), (Y[0], "_flux2")):
        ref = g[case + key + sfx]
        got = np.array(sp.flux(y, t, i=I, p=P, u=U))
        assert got.shape == ref.shape
        assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))


def test_singular_temporal_kernel_gives_nan_and_raises_nothing():
    for normalized in (False, True):
        sp, g = _process("d", normalized=normalized)
        t = g["d_t"]
        ns, seed = int(g["d_scalars"][3]), int(g["d_scalars"][4])
        Y = np.array(sp.sample_ylm(t, nsamples=ns, seed=seed))
        assert Y.shape == g["d_Y"].shape and np.isnan(Y).all()
        F = np.array(sp.flux(Y, t, i=I, p=P, u=U))
        assert F.shape == (ns, t.shape[0]) and np.isnan(F).all()
    e = _engine(5)
    Lt, info = e.temporal_gram(t, 25.0, "expsquared")
    assert int(info[0].item()) == 1 and bool(Lt.isnan().all())
    import torch

    status = torch.zeros(1, dtype=torch.int32, device=e.device)
    Ly = torch.eye(e.N, dtype=torch.float64, device=e.device)
    Y = e.ylm_temporal(Lt, Ly, np.ones((2, t.shape[0], e.N)), status=status)
    assert int(status[0].item()) == 1 and bool(Y.isnan().all())


def test_time_independent_process_refuses_times():
    from starry_process_amd import StarryProcess

    mom = _golden("moments_L5")
    sp = StarryProcess(ydeg=5, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"])
    with pytest.raises(NotImplementedError):
        sp.sample_ylm(np.linspace(0, 1, 10))


def test_flux_checks_the_shape_of_y():
    sp, g = _process("b", normalized=False)
    t = g["b_t"]
    with pytest.raises(ValueError):
        sp.flux(np.zeros((3, t.shape[0] + 1, 36)), t)
    with pytest.raises(ValueError):
        sp.flux(np.zeros((3, 36)), t)
    with pytest.raises(ValueError):
        sp.flux(np.zeros(36), t)


# ---- the kernel against NumPy -----------------------------------------------------------------------------------
def _factors(Nt, N, rs):
    Lt = np.tril(rs.randn(Nt, Nt)) + 2 * np.eye(Nt)
    Ly = np.tril(rs.randn(N, N)) + 2 * np.eye(N)
    return Lt, Ly


@pytest.mark.parametrize("ydeg", [1, 5, 15, 20])
@pytest.mark.parametrize("Nt", [1, 2, 63, 64, 65, 129, 1000])
def test_ylm_temporal_against_numpy(Nt, ydeg):
    e = _engine(ydeg)
    N = e.N
    rs = np.random.RandomState(Nt * 100 + ydeg)
    Lt, Ly = _factors(Nt, N, rs)
    ns = 2
    Uh = rs.randn(ns, Nt, N)
    Y = e.ylm_temporal(Lt, Ly, Uh).cpu().numpy()
    assert Y.shape == (ns, Nt, N)
    for n in range(ns):
        ref = Lt @ Uh[n] @ Ly.T
        bound = 8 * (Nt + N) * EPS * (np.abs(Lt) @ np.abs(Uh[n]) @ np.abs(Ly).T)
        assert np.all(np.abs(Y[n] - ref) <= bound)
    # the strict upper triangles are never read
    nan_up = np.triu(np.full((Nt, Nt), np.nan), 1) + Lt, np.triu(np.full((N, N), np.nan), 1) + Ly
    Y2 = e.ylm_temporal(nan_up[0], nan_up[1], Uh).cpu().numpy()
    assert np.array_equal(Y.view(np.uint64), Y2.view(np.uint64))


def test_ylm_temporal_zero_samples():
    e = _engine(5)
    Y = e.ylm_temporal(np.eye(4), np.eye(e.N), np.zeros((0, 4, e.N)))
    assert tuple(Y.shape) == (0, 4, e.N)
    assert int(e._L.sp_ylm_temporal_workspace_bytes(e._h, 0, 4)) == 0


# ---- batch independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg, Nt, ns", [(5, 65, 5), (20, 1500, 13)])
def test_ylm_temporal_batch_independence(ydeg, Nt, ns):
    e = _engine(ydeg)
    rs = np.random.RandomState(7)
    Lt, Ly = _factors(Nt, e.N, rs)
    Uh = rs.randn(ns, Nt, e.N)
    Y = e.ylm_temporal(Lt, Ly, Uh).cpu().numpy()
    for n in (0, ns // 2, ns - 1):
        Yn = e.ylm_temporal(Lt, Ly, Uh[n:n + 1]).cpu().numpy()[0]
        assert np.array_equal(Y[n].view(np.uint64), Yn.view(np.uint64))


@pytest.mark.parametrize("normalized", [False, True])
def test_flux_rows_batch_independence(normalized):
    e = _engine(15)
    rs = np.random.RandomState(3)
    Nt = 300
    A = rs.randn(Nt, e.N)
    y = 1e-3 * rs.randn(2, 3, Nt, e.N)
    F = e.flux_rows(A, y, normalized=normalized).cpu().numpy()
    assert F.shape == (2, 3, Nt)
    ref = np.einsum("kj,abkj->abk", A, y)
    if normalized:
        ref = (1 + ref) / np.mean(1 + ref, axis=-1, keepdims=True) - 1
    assert np.max(np.abs(F - ref)) <= 1e-12 * np.max(np.abs(ref))
    yf = y.reshape(6, Nt, e.N)
    for r in (0, 4, 5):
        Fr = e.flux_rows(A, yf[r:r + 1], normalized=normalized).cpu().numpy()[0]
        assert np.array_equal(F.reshape(6, Nt)[r].view(np.uint64), Fr.view(np.uint64))


# ---- exact tie to the covariance of the process --------------------------------------------------------------------
def test_identity_basis_reproduces_the_covariance():
    """With U running over the identity basis e_a e_b^T (ns = Nt N), sum_n F_n F_n^T = K_t o (A Sigma_y A^T), the
    conditional covariance of a time-variable process (reference sp.py:698)."""
    from starry_process_amd import StarryProcess
    from starry_process_amd.temporal import Matern32Kernel

    mom = _golden("moments_L5")
    sp = StarryProcess(ydeg=5, tau=3.0, temporal_kernel=Matern32Kernel, normalized=False,
                       marginalize_over_inclination=False, mean_ylm=mom["default_mean_ylm"],
                       cov_ylm=mom["default_cov_ylm"])
    e = sp._engine
    Nt, N = 24, 36
    t = np.linspace(0, 10, Nt)
    Lt, info = e.temporal_gram(t, 3.0, "matern32")
    assert int(info[0].item()) == 0
    Ub = np.eye(Nt * N).reshape(Nt * N, Nt, N)
    Y = e.ylm_temporal(Lt, sp._cho_ylm_dev(), Ub)
    F = np.array(sp.flux(Y.cpu().numpy(), t, i=I, p=P, u=U))
    assert F.shape == (Nt * N, Nt)
    cov = np.array(sp.cov(t, i=I, p=P, u=U))
    assert np.max(np.abs(F.T @ F - cov)) <= 1e-12 * np.max(np.abs(cov))


# ---- the tutorial's flow ----------------------------------------------------------------------------------------------
def test_tutorial_flow():
    from starry_process_amd import StarryProcess

    sp = StarryProcess(tau=25.0)
    t = np.linspace(0, 50, 1000)
    y = np.array(sp.sample_ylm(t))
    assert y.shape == (1, 1000, 256) and np.isfinite(y).all()
    flux = np.array(sp.flux(y, t))
    assert flux.shape == (1, 1000) and np.isfinite(flux).all()
    img = np.array(sp.mollweide(y[:, ::100]))
    assert img.shape == (1, 10, 150, 300)


def test_seeds():
    sp, g = _process("b", normalized=False, seed=17)
    t = g["b_t"]
    a = np.array(sp.sample_ylm(t, nsamples=2))
    b = np.array(sp.sample_ylm(t, nsamples=2, seed=17))
    c = np.array(sp.sample_ylm(t, nsamples=2, seed=17))
    d = np.array(sp.sample_ylm(t, nsamples=2, seed=18))
    assert np.array_equal(a, b) and np.array_equal(b, c)
    assert not np.array_equal(c, d)
