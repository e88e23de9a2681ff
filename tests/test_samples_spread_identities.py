"""
CPU checks of what the batched spread path (sp_polar_moments_samples_spread, csrc/sp_samples.hip) relies on -- no GPU:

  * the identity that spares the matrix square root.  The reference rotates the columns of eigE, eigE eigE^T = Etilde
    (size.py:63-89, integrals.py:109-156); every column is zonal, so (col_j Rx(phi) Rx(pi/2))[(l, m)] = col_j[l]
    rho_phi(l, m) with rho_phi the rotated all-ones zonal vector, and
        sum_k w_k sum_j (col_j R_k)^T (col_j R_k) = Etilde[l, l'] * (sum_k w_k rho_k rho_k^T)[(l, m), (l', m')];
  * Etilde formed the way sm_spread_kernel forms it (rows of C0 one by one, never stored; strips of 128 rows added in
    order; symmetrised; divided by 2 dr sfac at the end) against upstream.size_moments' eigE eigE^T;
  * the host helpers: the dr column of the parameter map and of the bounds mask, per-sample baseline terms of the
    (sample, star) systems, kernel_id on its own ids.
"""
import numpy as np
import pytest

from starry_process_amd import upstream

PAIRS = [(20.0, 5.0), (10.0, 10.0), (30.0, 2.0), (45.0, 44.0), (15.0, 1e-3)]


def etilde_by_strips(r_deg, dr_deg, ydeg, sfac=300.0, cutoff=1.5, strip=128):
    """Etilde [ydeg + 1, ydeg + 1] in sm_spread_kernel's order of operations."""
    theta, Bp, _ = upstream._spot_basis(ydeg)
    r, dr = r_deg * np.pi / 180, dr_deg * np.pi / 180
    kmax = int(np.argmax(theta / (r + dr) > cutoff))
    nl = ydeg + 1
    X = np.zeros((nl, nl))
    t = theta[:kmax]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        chim, chip = np.exp(sfac * (r - dr - t)), np.exp(sfac * (r + dr - t))
        term = np.log(1 + chim) - np.log(1 + chip)
        diag = 1 / (1 + chip) + chim / (1 + chim) - term - 1
        for j0 in range(0, kmax, strip):
            j1 = min(kmax, j0 + strip)
            V = np.zeros((j1 - j0, nl))
            for j in range(j0, j1):
                x = np.exp(sfac * (t - t[j]))
                row = (x * term - term[j]) / (1 - x + 1.0e-15)
                row[j] = diag[j]
                V[j - j0] = Bp[:, :kmax] @ row
            X += Bp[:, j0:j1] @ V
    return 0.5 * (X + X.T) / (2 * dr * sfac), kmax


@pytest.mark.parametrize("ydeg", [5, 15])
@pytest.mark.parametrize("pair", PAIRS)
def test_second_moment_is_etilde_times_the_unit_coefficient_product(ydeg, pair):
    from oracle import sp_oracle as orc

    r, dr = pair
    N = (ydeg + 1) ** 2
    e, eigE = upstream.size_moments(r, dr, ydeg)
    idx = np.arange(ydeg + 1) * (np.arange(ydeg + 1) + 1)
    l_of = np.floor(np.sqrt(np.arange(N))).astype(int)
    Et = (eigE @ eigE.T)[np.ix_(idx, idx)]
    ones = np.zeros(N)
    ones[idx] = 1.0
    alpha, beta = upstream.ab_to_alphabeta(0.4, 0.27)
    t, w = orc.gauss_jacobi(ydeg + 2, beta - 1.0, alpha - 1.0)
    x = 0.5 * (1.0 + t)
    phis = np.concatenate([np.arccos(x), -np.arccos(x)])
    wphi = 0.5 * np.concatenate([w, w])
    Rp = orc.Rx(ydeg, 0.5 * np.pi)[0]
    cols = np.ascontiguousarray(eigE.T[np.abs(eigE).sum(axis=0) > 0.0])
    lhs, G = np.zeros((N, N)), np.zeros((N, N))
    for ph, wk in zip(phis, wphi):
        Rk = orc.Rx(ydeg, ph)[0]
        U = orc.dotRx(ydeg, orc.dotRx(ydeg, cols, Rk), Rp)               # every column of eigE, rotated
        lhs += wk * (U.T @ U)
        rho = orc.dotRx(ydeg, orc.dotRx(ydeg, ones[None, :], Rk), Rp)[0]
        G += wk * np.outer(rho, rho)
    rhs = Et[np.ix_(l_of, l_of)] * G
    # 1e-13 of the largest entry: the square root reproduces Etilde to 4e-15, the rotations and products add the rest
    err = np.abs(lhs - rhs).max() / np.abs(lhs).max()
    print("ydeg %d (r, dr) = %r: identity to %.2e" % (ydeg, pair, err))
    assert err < 1e-13, (ydeg, pair, err)


@pytest.mark.parametrize("ydeg", [5, 15])
@pytest.mark.parametrize("pair", PAIRS)
def test_etilde_in_row_strips_equals_the_square_of_the_reference_factor(ydeg, pair):
    r, dr = pair
    _, eigE = upstream.size_moments(r, dr, ydeg)
    idx = np.arange(ydeg + 1) * (np.arange(ydeg + 1) + 1)
    ref = (eigE @ eigE.T)[np.ix_(idx, idx)]
    Et, kmax = etilde_by_strips(r, dr, ydeg)
    assert kmax > 0 and np.all(np.isfinite(Et))
    assert np.array_equal(Et, Et.T)
    # (the eigen square root zeroes eigenvalues below 1e-15: absolute, far below 1e-13 of the largest entry)
    assert np.abs(Et - ref).max() < 1e-13 * np.abs(ref).max(), (ydeg, pair)
    assert np.linalg.eigvalsh(Et).min() > -1e-13 * np.abs(Et).max()


@pytest.mark.parametrize("hyper", [(20.0, 5.0, 0.4, 0.27, 0.1, 10.0), (12.0, 9.0, 0.9, 0.05, 0.2, 3.0), (5.0, 10.0, 1.0, 1.0, 0.05, 1.0)])
def test_spread_polar_moments_are_the_quadrature_of_rotations(hyper):
    """(ez, Ez) the way sp_polar_moments_samples_spread forms them -- unit-coefficient rows, the projection, Etilde at the
    finish, e1 from the first moment -- against the per-sample route: every column of eigE rotated, then polar_moments."""
    from oracle import sp_oracle as orc

    ydeg = 6
    r, dr, a, b, c, n = hyper
    N = (ydeg + 1) ** 2
    idx = np.arange(ydeg + 1) * (np.arange(ydeg + 1) + 1)
    q, eigE = upstream.size_moments(r, dr, ydeg)
    cols = np.ascontiguousarray(eigE.T[np.abs(eigE).sum(axis=0) > 0.0])
    alpha, beta = upstream.ab_to_alphabeta(a, b)
    mu, Sig = orc.ylm_moments_quadrature(q, cols, alpha, beta, c, n, ydeg)
    ez, Ez = orc.polar_moments(ydeg, mu, Sig)
    # the batched form
    Et, _ = etilde_by_strips(r, dr, ydeg)
    t, w = orc.gauss_jacobi(ydeg + 2, beta - 1.0, alpha - 1.0)
    x = 0.5 * (1.0 + t)
    phis = np.concatenate([np.arccos(x), -np.arccos(x)])
    wphi = 0.5 * np.concatenate([w, w])
    Rp = orc.Rx(ydeg, 0.5 * np.pi)[0]
    tabs = orc.index_tables(ydeg)
    m_of, mirror = tabs["m_of"], tabs["mirror"]
    l_of = np.floor(np.sqrt(np.arange(N))).astype(int)
    ones = np.zeros(N)
    ones[idx] = 1.0
    g = np.pi * c * np.sqrt(n)
    M, e1 = np.zeros((N, N)), np.zeros(N)
    for ph, wk in zip(phis, wphi):
        rho = orc.dotRx(ydeg, orc.dotRx(ydeg, ones[None, :], orc.Rx(ydeg, ph)[0]), Rp)[0]
        M += wk * np.outer(rho, rho)
        e1 += g * wk * np.where(m_of == 0, rho, 0.0) * q[idx][l_of]
    Mm = M[np.ix_(mirror, mirror)]
    same = m_of[:, None] == m_of[None, :]
    opp = (m_of[:, None] == -m_of[None, :]) & (m_of[:, None] != 0)
    G = (np.where(same, 0.5 * (M + Mm), 0.0) + np.where(opp, 0.5 * (M - Mm), 0.0)) * Et[np.ix_(l_of, l_of)]
    lam = np.ones(N) * 1e-12
    lam[15 ** 2:] = 1e-9
    ez2, Ez2 = np.sqrt(n) * e1, g * g * G + (n - 1.0) * np.outer(e1, e1) + np.diag(lam)
    assert np.abs(ez.ravel() - ez2).max() < 1e-13 * np.abs(ez).max()
    assert np.abs(Ez - Ez2).max() < 1e-13 * np.abs(Ez).max()


def test_no_grid_point_beyond_the_cutoff_gives_kmax_zero():
    """r + dr above 120 degrees: theta / (r + dr) never exceeds 1.5, argmax of all-false is 0 and Etilde vanishes."""
    Et, kmax = etilde_by_strips(80.0, 45.0, 5)
    assert kmax == 0 and not Et.any()
    _, eigE = upstream.size_moments(80.0, 45.0, 5)
    assert not eigE.any()


def test_parameter_map_and_bounds_with_a_dr_column():
    from starry_process_amd.engine import sample_parameters, samples_in_bounds

    rows = np.array([[20.0, 5.0, 0.4, 0.27, 0.1, 10.0], [12.0, 0.0, 0.9, 0.05, 0.2, 3.0]])
    p = sample_parameters(rows, dr=True)
    q = sample_parameters(np.delete(rows, 1, axis=1))
    assert p.shape == (2, 6) and np.array_equal(p[:, [0, 2, 3, 4, 5]], q)
    assert np.array_equal(p[:, 1], rows[:, 1] * (np.pi / 180))
    for bad in ([20.0, -1.0, 0.4, 0.27, 0.1, 10.0], [20.0, 95.0, 0.4, 0.27, 0.1, 10.0], [20.0, np.nan, 0.4, 0.27, 0.1, 10.0],
                [95.0, 5.0, 0.4, 0.27, 0.1, 10.0]):
        with pytest.raises(ValueError):
            sample_parameters([bad], dr=True)
        assert not samples_in_bounds([bad], dr=True)[0]
    with pytest.raises(ValueError):
        sample_parameters(np.zeros((2, 5)), dr=True)
    assert list(samples_in_bounds(rows, dr=True)) == [True, True]
    assert list(samples_in_bounds(np.delete(rows, 1, axis=1))) == [True, True]


def test_stars_of_a_batch_take_per_sample_baseline_terms():
    from starry_process_amd.engine import make_stars, stars_for_samples

    stars = make_stars(2, period=[1.0, 2.0], baseline_mean=[0.1, 0.2], baseline_var=0.5, table=[0, 1])
    plain = stars_for_samples(stars, 3, 2)
    rep = stars_for_samples(stars, 3, 2, baseline_var=[1.0, 2.0, 3.0])
    assert np.array_equal(rep["baseline_var"], [1.0, 1.0, 2.0, 2.0, 3.0, 3.0])
    for f in ("period", "baseline_mean", "table", "inc", "tau", "data_var", "nobs"):
        assert np.array_equal(rep[f], plain[f])
    rep = stars_for_samples(stars, 3, 2, baseline_mean=[-1.0, 0.0, 1.0], baseline_var=[1.0, 2.0, 3.0])
    assert np.array_equal(rep["baseline_mean"], [-1.0, -1.0, 0.0, 0.0, 1.0, 1.0])
    assert np.array_equal(rep["table"], [0, 1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        stars_for_samples(stars, 3, 2, baseline_mean=[0.0, 1.0])


def test_kernel_id_accepts_its_own_ids():
    from starry_process_amd.temporal import ExpSquaredKernel, Matern32Kernel, kernel_id

    assert kernel_id("matern32") == kernel_id(Matern32Kernel) == "matern32"
    assert kernel_id("expsquared") == kernel_id(ExpSquaredKernel) == "expsquared"
    with pytest.raises(NotImplementedError):
        kernel_id("periodic")


def test_the_new_entry_point_refuses_a_handle_without_a_device():
    from starry_process_amd import _lib

    import ctypes

    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))        # a host-only handle
    x = np.zeros(8)
    assert L.sp_polar_moments_samples_spread(h, 1, _lib.hptr(x), 1.5, 1e-12, 1e-9, _lib.hptr(x), _lib.hptr(x), None) == -3
    L.sp_destroy(h)
