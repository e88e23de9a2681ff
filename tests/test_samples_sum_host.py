"""
Batched samples of a sum of spot populations (``StarryProcessSum``), the host side -- no GPU:

  * the column layout ``stars.SampleColumns(populations=C)``: names, ``split``, a mixed ``dr`` sequence, ``from_params``
    in any order and its errors, ``in_bounds`` per population; ``populations=1`` is today's object;
  * the identity sp_polar_moments_samples_sum relies on: with independent children the polar-frame moments of the sum are
        ez = sum_c ez_c,    Ez = sum_c Ez_c + sum_{c < d} (ez_c ez_d^T + ez_d ez_c^T),
    against ``oracle.polar_moments`` of the summed Ylm moments (sp.py:1380-1382 of the reference);
  * the log-Jacobian of several populations is the sum of theirs.
"""
import numpy as np
import pytest

from starry_process_amd import stars, upstream
from starry_process_amd.stars import SampleColumns


def rows(ns, seed, cmax, nmax):
    """ns rows (r, a, b, c, n) of one population: one RandomState, the columns drawn in this order."""
    rng = np.random.RandomState(seed)
    out = np.empty((ns, 5))
    out[:, 0] = rng.uniform(10.0, 30.0, ns)
    out[:, 1] = rng.uniform(0.2, 0.6, ns)
    out[:, 2] = rng.uniform(0.1, 0.5, ns)
    out[:, 3] = rng.uniform(0.03, cmax, ns)
    out[:, 4] = rng.uniform(1.0, nmax, ns)
    return out


def populations(ns, C, cmax=0.1, nmax=10):
    """[ns, C, 5]: population k (1-based) from seed 20 + k."""
    return np.stack([rows(ns, 21 + k, cmax, nmax) for k in range(C)], axis=1)


def combine(ezc, Ezc):
    """The moments of the sum from the children's ezc [C, N], Ezc [C, N, N], in the order sm_combine_kernel adds them;
    also the sum of the terms' magnitudes per entry (what a rounding bound scales with)."""
    C = ezc.shape[0]
    Ez, mag = Ezc[0].copy(), np.abs(Ezc[0])
    for c in range(1, C):
        Ez, mag = Ez + Ezc[c], mag + np.abs(Ezc[c])
    for c in range(C):
        for d in range(c + 1, C):
            t, u = np.outer(ezc[c], ezc[d]), np.outer(ezc[d], ezc[c])
            Ez, mag = Ez + (t + u), mag + np.abs(t) + np.abs(u)
    return ezc.sum(axis=0), Ez, mag


@pytest.mark.parametrize("C", [2, 3])
def test_names_and_split(C):
    cols = SampleColumns(populations=C, free=("baseline_log_var", "baseline_mean"))
    block = lambda k: tuple(q + str(k) for q in ("r", "a", "b", "c", "n"))          # noqa: E731
    hyper_names = sum((block(k + 1) for k in range(C)), ())
    assert cols.populations == C and cols.dr == (None,) * C and cols.dr_free == (False,) * C
    assert cols.names == hyper_names + ("baseline_mean", "baseline_log_var")
    assert cols.columns == hyper_names + ("m", "v") and cols.params == cols.names
    assert cols.permutation == list(range(5 * C + 2))
    B = 4
    samples = 0.25 + 0.125 * np.arange(B * len(cols.names), dtype=np.float64).reshape(B, len(cols.names))
    before = samples.copy()
    hyper, dr, fields = cols.split(samples)
    assert np.array_equal(samples, before) and dr is None
    assert hyper.shape == (B, C, 5) and hyper.dtype == np.float64 and hyper.flags["C_CONTIGUOUS"]
    assert np.array_equal(hyper, samples[:, :5 * C].reshape(B, C, 5))
    assert list(fields) == ["baseline_mean", "baseline_var"]
    assert np.array_equal(fields["baseline_mean"], samples[:, 5 * C])
    assert np.array_equal(fields["baseline_var"], 10.0 ** samples[:, 5 * C + 1])
    # one number for every population
    cols = SampleColumns(populations=C, dr=4.0)
    assert cols.dr == (4.0,) * C and cols.names == hyper_names
    hyper, dr, fields = cols.split(samples[:, :5 * C])
    assert dr.shape == (B, C) and np.all(dr == 4.0) and fields == {}
    # the batch builder takes the pieces of a sum as it takes one population's
    cols = SampleColumns(populations=C, free=("i", "p"), conditional=True)
    _, _, fields = cols.split(samples)
    st = stars.stars_for_samples(stars.make_stars(2), B, 1, **fields)
    assert np.array_equal(st["inc"], np.repeat(samples[:, 5 * C] * (np.pi / 180), 2))
    assert np.array_equal(st["period"], np.repeat(samples[:, 5 * C + 1], 2))


def test_a_mixed_dr_sequence():
    cols = SampleColumns(populations=3, dr=[None, "free", 5.0], free=("p",))
    assert cols.dr == (None, "free", 5.0) and cols.dr_free == (False, True, False)
    assert cols.names == ("r1", "a1", "b1", "c1", "n1", "r2", "dr2", "a2", "b2", "c2", "n2", "r3", "a3", "b3", "c3", "n3", "p")
    B = 3
    samples = 1.0 + np.arange(B * 17, dtype=np.float64).reshape(B, 17)
    col = {q: samples[:, k] for k, q in enumerate(cols.names)}
    hyper, dr, fields = cols.split(samples)
    for k in range(3):
        assert np.array_equal(hyper[:, k], np.stack([col[q + str(k + 1)] for q in ("r", "a", "b", "c", "n")], axis=1))
    assert dr.shape == (B, 3) and np.all(dr[:, 0] == 0.0) and np.array_equal(dr[:, 1], col["dr2"]) and np.all(dr[:, 2] == 5.0)
    assert list(fields) == ["period"] and np.array_equal(fields["period"], col["p"])
    # no population with a spread: no dr at all
    assert SampleColumns(populations=3, dr=[None, None, None]).split(samples[:, :15])[1] is None
    for bad in (dict(dr=[None, 5.0]), dict(dr=[None, "fixed", None]), dict(dr=[None, 91.0, None]), dict(dr=-1.0)):
        with pytest.raises(ValueError):
            SampleColumns(populations=3, **bad)
    with pytest.raises(ValueError):
        SampleColumns(populations=0)


def test_from_params_in_any_order_and_its_errors():
    params = ("p", "n2", "c2", "b2", "a2", "r2", "dr1", "r1", "a1", "b1", "c1", "n1", "i")
    cols = SampleColumns.from_params(params, False, False, dr=[3.0, 7.0], populations=2)
    assert cols.params == params
    assert cols.names == ("r1", "dr1", "a1", "b1", "c1", "n1", "r2", "a2", "b2", "c2", "n2", "i", "p")
    assert cols.dr == ("free", 7.0) and cols.dr_free == (True, False)
    assert cols.permutation == [7, 6, 8, 9, 10, 11, 5, 4, 3, 2, 1, 12, 0]
    row = np.arange(13.0)[None, :]
    hyper, dr, fields = cols.split(row[:, cols.permutation])
    assert hyper.tolist() == [[[7.0, 8.0, 9.0, 10.0, 11.0], [5.0, 4.0, 3.0, 2.0, 1.0]]]
    assert dr.tolist() == [[6.0, 7.0]] and {k: v.tolist() for k, v in fields.items()} == {"inc_deg": [12.0], "period": [0.0]}
    # one setting for every population; the default order
    cols = SampleColumns.from_params(SampleColumns(populations=2).names, True, False, dr=None, populations=2)
    assert cols.names == ("r1", "a1", "b1", "c1", "n1", "r2", "a2", "b2", "c2", "n2") and cols.dr == (None, None)
    ten = SampleColumns(populations=2).names
    with pytest.raises(ValueError, match="populations"):
        SampleColumns.from_params(("r", "a", "b", "c", "n"), True, False, populations=2)          # (one population's names)
    with pytest.raises(ValueError, match="populations"):
        SampleColumns.from_params(ten[:-1], True, False, populations=2)                            # (n2 is missing)
    with pytest.raises(ValueError, match="populations"):
        SampleColumns.from_params(ten + ("r3",), True, False, populations=2)
    with pytest.raises(ValueError, match="populations"):
        SampleColumns.from_params(ten + ("dr2", "dr2"), True, False, populations=2)
    with pytest.raises(ValueError, match="marginalises"):
        SampleColumns.from_params(ten + ("i",), True, False, populations=2)
    with pytest.raises(ValueError, match="tau"):
        SampleColumns.from_params(ten + ("tau",), False, False, populations=2)
    with pytest.raises(ValueError):
        SampleColumns.from_params(ten, True, False, dr=[1.0, 2.0, 3.0], populations=2)


def test_in_bounds_per_population():
    cols = SampleColumns(populations=2, dr=[None, "free"], free=("p",))
    j = {q: k for k, q in enumerate(cols.names)}
    good = [20.0, 0.4, 0.27, 0.1, 10.0, 15.0, 5.0, 0.5, 0.3, 0.05, 4.0, 1.0]
    batch = np.tile(good, (10, 1))
    batch[1, j["a1"]] = 1.0 + 1e-3
    batch[2, j["a2"]] = 1.2
    batch[3, j["r2"]] = 90.0 + 1e-3
    batch[4, j["dr2"]] = -1e-3
    batch[5, j["n1"]] = -1.0
    batch[6, j["c2"]] = np.nan
    batch[7, j["p"]] = -1e-3
    batch[8, j["b2"]], batch[8, j["dr2"]] = 1.0, 90.0          # (on the box's edge: inside)
    assert cols.in_bounds(batch).tolist() == [True, False, False, False, False, False, False, False, True, True]
    cols.check_ipt(batch[:7])
    with pytest.raises(ValueError, match="out of bounds"):
        cols.check_ipt(batch)
    # each population against the one-population mask of its own block
    one, spread = SampleColumns(), SampleColumns(dr="free")
    assert np.array_equal(cols.in_bounds(batch), one.in_bounds(batch[:, :5]) & spread.in_bounds(batch[:, 5:11])
                          & stars.ipt_in_bounds(batch, cols.names))


def test_one_population_is_todays_object():
    for kw in (dict(), dict(dr=7.0), dict(dr="free", free=("p", "baseline_mean")),
               dict(free=SampleColumns.FREE, conditional=True, temporal="matern32")):
        a, b = SampleColumns(**kw), SampleColumns(populations=1, **kw)
        assert vars(a) == vars(b)
        free = tuple(f for f in SampleColumns.FREE if f in kw.get("free", ()))
        dr = kw.get("dr")
        names = ("r",) + (("dr",) if dr == "free" else ()) + ("a", "b", "c", "n") + free
        assert vars(a) == dict(populations=1, dr=dr, dr_free=dr == "free", free=free, names=names,
                               columns=tuple(SampleColumns.SHORT.get(q, q) for q in names), params=names,
                               permutation=list(range(len(names))))
        samples = 0.5 + np.arange(3.0 * len(names)).reshape(3, len(names))
        hyper, d, fields = b.split(samples)
        assert hyper.shape == (3, 5) and (d is dr if dr != "free" else np.array_equal(d, samples[:, 1]))
    cols = SampleColumns.from_params(("tau", "i", "r", "a", "b", "c", "n", "p"), False, True, dr=5.0, populations=1)
    assert cols.names == ("r", "a", "b", "c", "n", "i", "p", "tau") and cols.dr == 5.0 and cols.dr_free is False


@pytest.mark.parametrize("ydeg, ns, C", [(5, 8, 2), (5, 4, 3), (15, 2, 2)])
def test_polar_moments_of_a_sum_from_the_childrens(ydeg, ns, C):
    """Both sides are the same polynomial in the children's Ylm moments, ez = R^T mu and Ez = R^T (Sigma + mu mu^T) R
    with mu = sum mu_c, Sigma = sum Sigma_c; they differ by the rounding of rotations of N terms, N 2^-53 of the largest
    entry each (6e-14 at ydeg 15): 1e-13, the bound of tests/test_samples_identities.py for the same rotations."""
    from oracle import sp_oracle as orc

    sm = populations(ns, C)
    for k in range(ns):
        mus, Sigs = [], []
        for r, a, b, c, n in sm[k]:
            s1, _ = upstream.size_moments(r, None, ydeg)
            alpha, beta = upstream.ab_to_alphabeta(a, b)
            mu, Sig = orc.ylm_moments_quadrature(s1, s1[None, :], alpha, beta, c, n, ydeg)
            mus.append(np.asarray(mu).ravel())
            Sigs.append(np.asarray(Sig))
        child = [orc.polar_moments(ydeg, mu, Sig) for mu, Sig in zip(mus, Sigs)]
        ez, Ez, _ = combine(np.array([e.ravel() for e, _ in child]), np.array([E for _, E in child]))
        ez_ref, Ez_ref = orc.polar_moments(ydeg, sum(mus), sum(Sigs))
        assert np.abs(ez - ez_ref.ravel()).max() <= 1e-13 * np.abs(ez_ref).max()
        assert np.abs(Ez - Ez_ref).max() <= 1e-13 * np.abs(Ez_ref).max()


def test_log_jac_of_populations_is_the_sum():
    from starry_process_amd.calibrate import log_jac_populations

    sm = populations(6, 3)
    got = log_jac_populations(sm)
    want = [sum(float(upstream.log_jac(a, b)) for _, a, b, _, _ in row) for row in sm]
    assert got.shape == (6,) and np.allclose(got, want, rtol=1e-14, atol=0.0)
    assert np.array_equal(log_jac_populations(sm[:, :2]),
                          upstream.log_jac_samples(sm[:, 0, 1], sm[:, 0, 2]) + upstream.log_jac_samples(sm[:, 1, 1], sm[:, 1, 2]))
    assert np.array_equal(log_jac_populations(sm[:, 0]), upstream.log_jac_samples(sm[:, 0, 1], sm[:, 0, 2]))
