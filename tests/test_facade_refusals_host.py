"""
The host side of the facade's ensemble methods (starry_process_amd/sp.py): what they refuse, word for word, and how
they open the device work.  No GPU and no library call: the process is made with ``object.__new__`` and given by hand
only the attributes a method reads before the engine.

  * CALLS / EXPECTED: (method, arguments) -> (exception type, full message) for loo, lbo, log_likelihood_linear and the
    ensemble forms loo_ensemble, lbo_ensemble, log_likelihood_linear_ensemble, predict_ensemble, sample_conditional_ensemble --
    ragged input, a 1-D flux, (K, K) and 3-D ``data_cov`` (S = K, which is (S, K) variances, is served), a matrix
    ``baseline_var``, K = 1, ``basis_var`` without ``basis``, a bad partition.  The strings were recorded from the
    methods as they stood before the shared pieces (_dense_ensemble_input, _one_curve, _branch) existed and are compared
    with ``==``.  A call that passes every check meets the missing engine next: AttributeError, nothing else first.
  * the opening: a stub engine and a stub flux object record what a method calls, in order, and the keywords of the
    final engine call; the expected sequences and keyword sets are read off the same earlier code.  ``_bind`` comes
    first, ``kernel_table`` only on the marginal branch, and the predict calls take no normalisation keywords.
"""
import numpy as np
import pytest

S, K, Q = 3, 20, 4
T = np.linspace(0, 1, K)
FLUX = np.zeros((S, K))
U = np.ones((K, Q))
RAGGED_T = [T, T[:10], T]
RAGGED_F = [FLUX[0], FLUX[1][:10], FLUX[2]]
EYE = np.eye(K) * 1e-6
CUBE = np.full((S, K, K), 1e-6)
BVAR2 = np.zeros((S, S))
LIN = dict(basis=U, basis_var=1e-4)


def _process(**attrs):
    """A StarryProcess with nothing behind it but ``attrs``: touching the engine is an AttributeError."""
    from starry_process_amd import StarryProcess

    sp = object.__new__(StarryProcess)
    # (what the methods read on the host: predict's refusal of a normalised process, the star records' udeg and tau)
    sp.__dict__.update(dict(_normalized=False, _udeg=2, _tau=0.0), **attrs)
    return sp


def _variant(method, k=K):
    """(method name, trailing positional arguments, keywords) of the call variant ``method`` ("name" or "name+basis")
    for light curves of k cadences."""
    name, _, basis = method.partition("+")
    Uk = np.ones((k, Q))
    if name.startswith("log_likelihood_linear"):
        return name, (Uk, 1e-4), {}
    return name, ((4,) if name.startswith("lbo") else ()), (dict(basis=Uk, basis_var=1e-4) if basis else {})


# name of a call -> (method, positional arguments, keywords); the table of expected refusals uses the same names
CALLS = {}
for _m in ("loo_ensemble", "loo_ensemble+basis", "lbo_ensemble", "lbo_ensemble+basis", "log_likelihood_linear_ensemble",
           "predict_ensemble", "predict_ensemble+basis", "sample_conditional_ensemble",
           "sample_conditional_ensemble+basis"):
    _n, _x, _kw = _variant(_m)
    _, _xs, _kws = _variant(_m, S)
    _, _x1, _kw1 = _variant(_m, 1)
    CALLS.update({
        _m + ":ragged": (_n, (RAGGED_T, RAGGED_F, 1e-6) + _x, _kw),
        _m + ":flux-1d": (_n, (T, FLUX[0], 1e-6) + _x, _kw),
        _m + ":data_cov-KK": (_n, (T, FLUX, EYE) + _x, _kw),
        _m + ":data_cov-3d": (_n, (T, FLUX, CUBE) + _x, _kw),
        _m + ":data_cov-SK-with-S=K": (_n, (T[:S], FLUX[:, :S], np.full((S, S), 1e-6)) + _xs, _kws),
        _m + ":baseline_var-matrix": (_n, (T, FLUX, 1e-6) + _x, dict(_kw, baseline_var=BVAR2)),
        _m + ":K=1": (_n, (T[:1], FLUX[:, :1], 1e-6) + _x1, _kw1),
        _m + ":passes": (_n, (T, FLUX, 1e-6) + _x, _kw),
    })
for _m in ("loo", "loo+basis", "lbo", "lbo+basis", "log_likelihood_linear"):
    _n, _x, _kw = _variant(_m)
    _, _x1, _kw1 = _variant(_m, 1)
    CALLS.update({
        _m + ":ragged": (_n, (T, [[1.0, 2.0], [3.0]], 1e-6) + _x, _kw),
        _m + ":flux-2d": (_n, (T, FLUX, 1e-6) + _x, _kw),
        _m + ":data_cov-KK": (_n, (T, FLUX[0], EYE) + _x, _kw),
        _m + ":data_cov-3d": (_n, (T, FLUX[0], CUBE) + _x, _kw),
        _m + ":baseline_var-vector": (_n, (T, FLUX[0], 1e-6) + _x, dict(_kw, baseline_var=np.zeros(K))),
        _m + ":baseline_var-matrix": (_n, (T, FLUX[0], 1e-6) + _x, dict(_kw, baseline_var=np.zeros((K, K)))),
        _m + ":K=1": (_n, (T[:1], FLUX[0, :1], 1e-6) + _x1, _kw1),
        _m + ":passes": (_n, (T, FLUX[0], np.full(K, 1e-6)) + _x, _kw),
    })
CALLS.update({
    # one of the pair of regressor arguments without the other, and regressors of the wrong shape
    "loo_ensemble:basis_var-alone": ("loo_ensemble", (T, FLUX, 1e-6), dict(basis_var=1e-4)),
    "lbo_ensemble:basis_var-alone": ("lbo_ensemble", (T, FLUX, 1e-6, 4), dict(basis_var=1e-4)),
    "loo:basis_var-alone": ("loo", (T, FLUX[0], 1e-6), dict(basis_var=1e-4)),
    "lbo:basis_var-alone": ("lbo", (T, FLUX[0], 1e-6, 4), dict(basis_var=1e-4)),
    "predict_ensemble:basis_var-alone": ("predict_ensemble", (T, FLUX, 1e-6), dict(basis_var=1e-4)),
    "predict_ensemble:basis_sample-alone": ("predict_ensemble", (T, FLUX, 1e-6), dict(basis_sample=U)),
    "sample_conditional_ensemble:basis_var-alone": ("sample_conditional_ensemble", (T, FLUX, 1e-6),
                                                    dict(basis_var=1e-4)),
    "loo_ensemble:basis-alone": ("loo_ensemble", (T, FLUX, 1e-6), dict(basis=U)),
    "lbo_ensemble:basis-alone": ("lbo_ensemble", (T, FLUX, 1e-6, 4), dict(basis=U)),
    "predict_ensemble:basis-alone": ("predict_ensemble", (T, FLUX, 1e-6), dict(basis=U)),
    "log_likelihood_linear_ensemble:no-basis": ("log_likelihood_linear_ensemble", (T, FLUX, 1e-6, None, 1e-4), {}),
    "log_likelihood_linear_ensemble:no-basis_var": ("log_likelihood_linear_ensemble", (T, FLUX, 1e-6, U, None), {}),
    "log_likelihood_linear:no-basis": ("log_likelihood_linear", (T, FLUX[0], 1e-6, None, 1e-4), {}),
    "log_likelihood_linear:no-basis_var": ("log_likelihood_linear", (T, FLUX[0], 1e-6, U, None), {}),
    "log_likelihood_linear:basis-1d": ("log_likelihood_linear", (T, FLUX[0], 1e-6, U[:, 0], 1e-4), {}),
    "log_likelihood_linear:basis-3d": ("log_likelihood_linear", (T, FLUX[0], 1e-6, U[None], 1e-4), {}),
    "log_likelihood_linear:basis_var-2d": ("log_likelihood_linear", (T, FLUX[0], 1e-6, U, np.ones((1, Q))), {}),
    "loo:basis-1d": ("loo", (T, FLUX[0], 1e-6), dict(basis=U[:, 0], basis_var=1e-4)),
    "lbo:basis_var-2d": ("lbo", (T, FLUX[0], 1e-6, 4), dict(basis=U, basis_var=np.ones((1, Q)))),
    # partitions
    "lbo_ensemble:block-65": ("lbo_ensemble", (T, FLUX, 1e-6, 65), {}),
    "lbo_ensemble:block-0": ("lbo_ensemble", (T, FLUX, 1e-6, 0), {}),
    "lbo_ensemble:block-2.5": ("lbo_ensemble", (T, FLUX, 1e-6, 2.5), {}),
    "lbo_ensemble:edges-repeat": ("lbo_ensemble", (T, FLUX, 1e-6, [0, 5, 5, K]), {}),
    "lbo_ensemble:edges-short": ("lbo_ensemble", (T, FLUX, 1e-6, [0, 5, K - 1]), {}),
    "lbo_ensemble:edges-wide": ("lbo_ensemble", (np.linspace(0, 1, 70), np.zeros((S, 70)), 1e-6, [0, 65, 70]), {}),
    "lbo_ensemble+basis:block-65": ("lbo_ensemble", (T, FLUX, 1e-6, 65), LIN),
    "lbo:block-65": ("lbo", (T, FLUX[0], 1e-6, 65), {}),
    "lbo:edges-repeat": ("lbo", (T, FLUX[0], 1e-6, [0, 5, 5, K]), {}),
    # predict's own
    "predict_ensemble:return_cov": ("predict_ensemble", (T, FLUX, 1e-6), dict(return_cov="full")),
    "predict_ensemble:t_sample-shape": ("predict_ensemble", (T, FLUX, 1e-6), dict(t_sample=np.zeros((S + 1, 5)))),
    "predict_ensemble+basis:basis_sample-shape": ("predict_ensemble", (T, FLUX, 1e-6),
                                                  dict(LIN, basis_sample=np.ones((K, Q + 1)))),
    "sample_conditional_ensemble:t_sample-shape": ("sample_conditional_ensemble", (T, FLUX, 1e-6),
                                                   dict(t_sample=np.zeros((S + 1, 5)))),
})

ENGINE = "'StarryProcess' object has no attribute '_engine'"

# name of the call -> (exception type, str(exception)), recorded from the methods before they shared their refusals;
# None where the words are NumPy's own (predict's ensemble calls leave ragged input and a matrix `baseline_var` to it)
EXPECTED = {
    "lbo+basis:K=1": ("ValueError", "leave-block-out needs at least two cadences"),
    "lbo+basis:baseline_var-matrix":
        ("NotImplementedError", "lbo does not serve a matrix `baseline_var`: pass a scalar"),
    "lbo+basis:baseline_var-vector":
        ("NotImplementedError", "lbo does not serve a matrix `baseline_var`: pass a scalar"),
    "lbo+basis:data_cov-3d":
        ("NotImplementedError", "lbo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "lbo+basis:data_cov-KK":
        ("NotImplementedError", "lbo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "lbo+basis:flux-2d": ("ValueError", "`basis` must be (K, q) or (S, K, q) with S = 1, K = 60, not (1, 20, 4)"),
    "lbo+basis:passes": ("AttributeError", ENGINE),
    "lbo+basis:ragged": ("ValueError", "`flux` must be one light curve of K cadences"),
    "lbo:K=1": ("ValueError", "leave-block-out needs at least two cadences"),
    "lbo:baseline_var-matrix": ("NotImplementedError", "lbo does not serve a matrix `baseline_var`: pass a scalar"),
    "lbo:baseline_var-vector": ("NotImplementedError", "lbo does not serve a matrix `baseline_var`: pass a scalar"),
    "lbo:basis_var-2d": ("ValueError", "`basis_var` must be a scalar or (q,)"),
    "lbo:basis_var-alone": ("ValueError", "`basis_var` needs a `basis`"),
    "lbo:block-65": ("ValueError", "`block` = 65: a block holds 1 to 64 cadences (wider blocks are not served)"),
    "lbo:data_cov-3d":
        ("NotImplementedError", "lbo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "lbo:data_cov-KK":
        ("NotImplementedError", "lbo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "lbo:edges-repeat": ("ValueError", "the block edges must increase strictly"),
    "lbo:flux-2d": ("ValueError", "`t` must be (K,) or (S, K) like `flux` (1, 60), not (20,)"),
    "lbo:passes": ("AttributeError", ENGINE),
    "lbo:ragged": ("ValueError", "`flux` must be one light curve of K cadences"),
    "lbo_ensemble+basis:K=1": ("ValueError", "leave-block-out needs at least two cadences"),
    "lbo_ensemble+basis:baseline_var-matrix":
        ("NotImplementedError", "lbo_ensemble does not serve a matrix `baseline_var`: pass a scalar or (S,)"),
    "lbo_ensemble+basis:block-65":
        ("ValueError", "`block` = 65: a block holds 1 to 64 cadences (wider blocks are not served)"),
    "lbo_ensemble+basis:data_cov-3d":
        ("NotImplementedError", "lbo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "lbo_ensemble+basis:data_cov-KK":
        ("NotImplementedError", "lbo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "lbo_ensemble+basis:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "lbo_ensemble+basis:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "lbo_ensemble+basis:passes": ("AttributeError", ENGINE),
    "lbo_ensemble+basis:ragged":
        ("ValueError", "lbo_ensemble does not serve ragged input (lists of light curves of different lengths): "
         "pass `t` and `flux` as (S, K) arrays"),
    "lbo_ensemble:K=1": ("ValueError", "leave-block-out needs at least two cadences"),
    "lbo_ensemble:baseline_var-matrix":
        ("NotImplementedError", "lbo_ensemble does not serve a matrix `baseline_var`: pass a scalar or (S,)"),
    "lbo_ensemble:basis-alone": ("ValueError", "`basis` needs a `basis_var`"),
    "lbo_ensemble:basis_var-alone": ("ValueError", "`basis_var` needs a `basis`"),
    "lbo_ensemble:block-0": ("ValueError", "`block` = 0: a block holds 1 to 64 cadences (wider blocks are not served)"),
    "lbo_ensemble:block-2.5": ("ValueError", "`block` must be an integer width or a 1-D array of edges"),
    "lbo_ensemble:block-65":
        ("ValueError", "`block` = 65: a block holds 1 to 64 cadences (wider blocks are not served)"),
    "lbo_ensemble:data_cov-3d":
        ("NotImplementedError", "lbo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "lbo_ensemble:data_cov-KK":
        ("NotImplementedError", "lbo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "lbo_ensemble:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "lbo_ensemble:edges-repeat": ("ValueError", "the block edges must increase strictly"),
    "lbo_ensemble:edges-short": ("ValueError", "the block edges must start at 0 and end at K = 20"),
    "lbo_ensemble:edges-wide":
        ("ValueError", "a block of 65 cadences: a block holds 1 to 64 (wider blocks are not served)"),
    "lbo_ensemble:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "lbo_ensemble:passes": ("AttributeError", ENGINE),
    "lbo_ensemble:ragged":
        ("ValueError", "lbo_ensemble does not serve ragged input (lists of light curves of different lengths): "
         "pass `t` and `flux` as (S, K) arrays"),
    "log_likelihood_linear:K=1": ("ValueError", "the likelihood with regressors needs at least two cadences"),
    "log_likelihood_linear:baseline_var-matrix":
        ("NotImplementedError", "log_likelihood_linear does not serve a matrix `baseline_var`: pass a scalar, and the "
         "structured part as `basis`, `basis_var`"),
    "log_likelihood_linear:baseline_var-vector":
        ("NotImplementedError", "log_likelihood_linear does not serve a matrix `baseline_var`: pass a scalar, and the "
         "structured part as `basis`, `basis_var`"),
    "log_likelihood_linear:basis-1d": ("ValueError", "`basis` must be (K, q)"),
    "log_likelihood_linear:basis-3d": ("ValueError", "`basis` must be (K, q)"),
    "log_likelihood_linear:basis_var-2d": ("ValueError", "`basis_var` must be a scalar or (q,)"),
    "log_likelihood_linear:data_cov-3d":
        ("NotImplementedError", "log_likelihood_linear does not serve a full-matrix `data_cov`: pass a scalar or (K,) "
         "variances"),
    "log_likelihood_linear:data_cov-KK":
        ("NotImplementedError", "log_likelihood_linear does not serve a full-matrix `data_cov`: pass a scalar or (K,) "
         "variances"),
    "log_likelihood_linear:flux-2d":
        ("ValueError", "`basis` must be (K, q) or (S, K, q) with S = 1, K = 60, not (1, 20, 4)"),
    "log_likelihood_linear:no-basis": ("ValueError", "`basis` must be (K, q)"),
    "log_likelihood_linear:no-basis_var": ("ValueError", "`basis_var` must be finite and >= 0"),
    "log_likelihood_linear:passes": ("AttributeError", ENGINE),
    "log_likelihood_linear:ragged": ("ValueError", "`flux` must be one light curve of K cadences"),
    "log_likelihood_linear_ensemble:K=1": ("ValueError", "the likelihood with regressors needs at least two cadences"),
    "log_likelihood_linear_ensemble:baseline_var-matrix":
        ("NotImplementedError", "log_likelihood_linear_ensemble does not serve a matrix `baseline_var`: pass a scalar "
         "or (S,), and the structured part as `basis`, `basis_var`"),
    "log_likelihood_linear_ensemble:data_cov-3d":
        ("NotImplementedError", "log_likelihood_linear_ensemble does not serve a full-matrix `data_cov`: pass a "
         "scalar, (S,) or (S, K) variances"),
    "log_likelihood_linear_ensemble:data_cov-KK":
        ("NotImplementedError", "log_likelihood_linear_ensemble does not serve a full-matrix `data_cov`: pass a "
         "scalar, (S,) or (S, K) variances"),
    "log_likelihood_linear_ensemble:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "log_likelihood_linear_ensemble:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "log_likelihood_linear_ensemble:no-basis":
        ("ValueError", "`basis` must be (K, q) or (S, K, q) with S = 3, K = 20, not ()"),
    "log_likelihood_linear_ensemble:no-basis_var": ("ValueError", "`basis_var` must be finite and >= 0"),
    "log_likelihood_linear_ensemble:passes": ("AttributeError", ENGINE),
    "log_likelihood_linear_ensemble:ragged":
        ("ValueError", "log_likelihood_linear_ensemble does not serve ragged input (lists of light curves of "
         "different lengths): pass `t` and `flux` as (S, K) arrays"),
    "loo+basis:K=1": ("ValueError", "leave-block-out needs at least two cadences"),
    "loo+basis:baseline_var-matrix":
        ("NotImplementedError", "loo does not serve a matrix `baseline_var`: pass a scalar"),
    "loo+basis:baseline_var-vector":
        ("NotImplementedError", "loo does not serve a matrix `baseline_var`: pass a scalar"),
    "loo+basis:data_cov-3d":
        ("NotImplementedError", "loo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "loo+basis:data_cov-KK":
        ("NotImplementedError", "loo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "loo+basis:flux-2d": ("ValueError", "`basis` must be (K, q) or (S, K, q) with S = 1, K = 60, not (1, 20, 4)"),
    "loo+basis:passes": ("AttributeError", ENGINE),
    "loo+basis:ragged": ("ValueError", "`flux` must be one light curve of K cadences"),
    "loo:K=1": ("ValueError", "leave-one-out needs at least two cadences"),
    "loo:baseline_var-matrix": ("NotImplementedError", "loo does not serve a matrix `baseline_var`: pass a scalar"),
    "loo:baseline_var-vector": ("NotImplementedError", "loo does not serve a matrix `baseline_var`: pass a scalar"),
    "loo:basis-1d": ("ValueError", "`basis` must be (K, q)"),
    "loo:basis_var-alone": ("ValueError", "`basis_var` needs a `basis`"),
    "loo:data_cov-3d":
        ("NotImplementedError", "loo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "loo:data_cov-KK":
        ("NotImplementedError", "loo does not serve a full-matrix `data_cov`: pass a scalar or (K,) variances"),
    "loo:flux-2d": ("ValueError", "`t` must be (K,) or (S, K) like `flux` (1, 60), not (20,)"),
    "loo:passes": ("AttributeError", ENGINE),
    "loo:ragged": ("ValueError", "`flux` must be one light curve of K cadences"),
    "loo_ensemble+basis:K=1": ("ValueError", "leave-block-out needs at least two cadences"),
    "loo_ensemble+basis:baseline_var-matrix":
        ("NotImplementedError", "loo_ensemble does not serve a matrix `baseline_var`: pass a scalar or (S,)"),
    "loo_ensemble+basis:data_cov-3d":
        ("NotImplementedError", "loo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "loo_ensemble+basis:data_cov-KK":
        ("NotImplementedError", "loo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "loo_ensemble+basis:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "loo_ensemble+basis:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "loo_ensemble+basis:passes": ("AttributeError", ENGINE),
    "loo_ensemble+basis:ragged":
        ("ValueError", "loo_ensemble does not serve ragged input (lists of light curves of different lengths): "
         "pass `t` and `flux` as (S, K) arrays"),
    "loo_ensemble:K=1": ("ValueError", "leave-one-out needs at least two cadences"),
    "loo_ensemble:baseline_var-matrix":
        ("NotImplementedError", "loo_ensemble does not serve a matrix `baseline_var`: pass a scalar or (S,)"),
    "loo_ensemble:basis-alone": ("ValueError", "`basis` needs a `basis_var`"),
    "loo_ensemble:basis_var-alone": ("ValueError", "`basis_var` needs a `basis`"),
    "loo_ensemble:data_cov-3d":
        ("NotImplementedError", "loo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "loo_ensemble:data_cov-KK":
        ("NotImplementedError", "loo_ensemble does not serve a full-matrix `data_cov`: pass a scalar, (S,) or (S, K) "
         "variances"),
    "loo_ensemble:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "loo_ensemble:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "loo_ensemble:passes": ("AttributeError", ENGINE),
    "loo_ensemble:ragged":
        ("ValueError", "loo_ensemble does not serve ragged input (lists of light curves of different lengths): "
         "pass `t` and `flux` as (S, K) arrays"),
    "predict_ensemble+basis:K=1": ("AttributeError", ENGINE),
    "predict_ensemble+basis:baseline_var-matrix": ("ValueError", None),
    "predict_ensemble+basis:basis_sample-shape":
        ("ValueError", "`basis_sample` must be (Ks, q) or (S, Ks, q) with S = 3, Ks = 20, q = 4, not (20, 5)"),
    "predict_ensemble+basis:data_cov-3d": ("ValueError", "`data_cov` must be a scalar, (S,) or (S, K)"),
    "predict_ensemble+basis:data_cov-KK":
        ("ValueError", "a 2-D `data_cov` must be (S, K) like `flux` (3, 20), not (20, 20)"),
    "predict_ensemble+basis:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "predict_ensemble+basis:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "predict_ensemble+basis:passes": ("AttributeError", ENGINE),
    "predict_ensemble+basis:ragged": ("ValueError", None),
    "predict_ensemble:K=1": ("AttributeError", ENGINE),
    "predict_ensemble:baseline_var-matrix": ("ValueError", None),
    "predict_ensemble:basis-alone": ("ValueError", "`basis` needs a `basis_var`"),
    "predict_ensemble:basis_sample-alone": ("ValueError", "`basis_var` and `basis_sample` need a `basis`"),
    "predict_ensemble:basis_var-alone": ("ValueError", "`basis_var` and `basis_sample` need a `basis`"),
    "predict_ensemble:data_cov-3d": ("ValueError", "`data_cov` must be a scalar, (S,) or (S, K)"),
    "predict_ensemble:data_cov-KK": ("ValueError", "a 2-D `data_cov` must be (S, K) like `flux` (3, 20), not (20, 20)"),
    "predict_ensemble:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "predict_ensemble:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "predict_ensemble:passes": ("AttributeError", ENGINE),
    "predict_ensemble:ragged": ("ValueError", None),
    "predict_ensemble:return_cov": ("ValueError", '`return_cov` must be True, False or "diag"'),
    "predict_ensemble:t_sample-shape": ("ValueError", "`t_sample` must be (Ks,) or (S, Ks) with S = 3, not (4, 5)"),
    "sample_conditional_ensemble+basis:K=1": ("AttributeError", ENGINE),
    "sample_conditional_ensemble+basis:baseline_var-matrix": ("ValueError", None),
    "sample_conditional_ensemble+basis:data_cov-3d": ("ValueError", "`data_cov` must be a scalar, (S,) or (S, K)"),
    "sample_conditional_ensemble+basis:data_cov-KK":
        ("ValueError", "a 2-D `data_cov` must be (S, K) like `flux` (3, 20), not (20, 20)"),
    "sample_conditional_ensemble+basis:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "sample_conditional_ensemble+basis:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "sample_conditional_ensemble+basis:passes": ("AttributeError", ENGINE),
    "sample_conditional_ensemble+basis:ragged": ("ValueError", None),
    "sample_conditional_ensemble:K=1": ("AttributeError", ENGINE),
    "sample_conditional_ensemble:baseline_var-matrix": ("ValueError", None),
    "sample_conditional_ensemble:basis_var-alone": ("ValueError", "`basis_var` and `basis_sample` need a `basis`"),
    "sample_conditional_ensemble:data_cov-3d": ("ValueError", "`data_cov` must be a scalar, (S,) or (S, K)"),
    "sample_conditional_ensemble:data_cov-KK":
        ("ValueError", "a 2-D `data_cov` must be (S, K) like `flux` (3, 20), not (20, 20)"),
    "sample_conditional_ensemble:data_cov-SK-with-S=K": ("AttributeError", ENGINE),
    "sample_conditional_ensemble:flux-1d": ("ValueError", "`flux` must be (S, K)"),
    "sample_conditional_ensemble:passes": ("AttributeError", ENGINE),
    "sample_conditional_ensemble:ragged": ("ValueError", None),
    "sample_conditional_ensemble:t_sample-shape":
        ("ValueError", "`t_sample` must be (Ks,) or (S, Ks) with S = 3, not (4, 5)"),
}


def _outcome(sp, name):
    method, args, kw = CALLS[name]
    try:
        getattr(sp, method)(*args, **kw)
    except Exception as exc:       # noqa: BLE001 -- the type is part of what is compared
        return type(exc).__name__, (None if EXPECTED[name][1] is None else str(exc))
    return None, None


def test_the_table_covers_every_call():
    assert sorted(EXPECTED) == sorted(CALLS)
    for method in ("loo", "lbo", "log_likelihood_linear", "loo_ensemble", "lbo_ensemble",
                   "log_likelihood_linear_ensemble", "predict_ensemble", "sample_conditional_ensemble"):
        kinds = {EXPECTED[k][0] for k in CALLS if CALLS[k][0] == method}
        assert "AttributeError" in kinds and len(kinds) >= 2, method         # (a call that passes, and refusals)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_refusals_word_for_word(name):
    """Type and full text of every refusal; a call that passes every check meets the missing engine next."""
    assert _outcome(_process(), name) == EXPECTED[name]


def test_a_normalized_process_is_refused_by_predict_before_anything_else():
    sp = _process(_normalized=True)
    for name in ("predict_ensemble:flux-1d", "predict_ensemble:passes", "sample_conditional_ensemble+basis:passes"):
        assert _outcome(sp, name) == ("NotImplementedError", "Method not implemented when the flux is normalized.")


# ---- the opening of the device work, against a recording stub ------------------------------------------------------
class Reached(Exception):
    """The final engine call was made."""


class StubFlux:
    def __init__(self, log):
        self.log = log

    def _bind(self):
        self.log.append("_bind")


class StubEngine:
    FINAL = ("loo_ensemble", "lbo_ensemble", "lbo_linear", "lnlike_linear", "predict_ensemble", "predict_linear",
             "lnlike_ensemble")

    def __init__(self, log):
        self.log = log
        self.final = None

    def rTA1L(self, utab):
        self.log.append("rTA1L")
        return "rTA1L(utab)"

    def f64(self, x):
        self.log.append("f64")
        return "RTA1" if isinstance(x, str) and x == "rTA1L(utab)" else ("f64", x)

    def kernel_table(self, rta1, covpts):
        self.log.append("kernel_table")
        assert rta1 == "RTA1" and covpts == 123
        return "TAB", "MV"

    def stars_to_device(self, stars):
        self.log.append("stars_to_device")
        return stars

    def __getattr__(self, name):
        if name not in self.FINAL:
            raise AssertionError("the opening calls Engine.%s" % name)

        def final(*args, **kw):
            self.log.append(name)
            self.final = (name, args, kw)
            raise Reached(name)

        return final


def _stubbed(marginal, normalized):
    log = []
    sp = _process(_covpts=123, _normN=7, _normzmax=0.011, _temporal="matern32", _tau=2.0, _udeg=2,
                  _normalized=normalized, _marginalize_over_inclination=marginal, _flux=StubFlux(log),
                  _engine=StubEngine(log))
    return sp, log


DIAG = np.full((S, K), 1e-6)
OPEN = ["_bind", "rTA1L", "f64"]
# (method, arguments, keywords, the calls after the opening -- the final one last --, its own keywords, predict?)
OPENINGS = {
    "loo_ensemble": ("loo_ensemble", (T, FLUX, DIAG), dict(max_workspace_bytes=1 << 20), ["loo_ensemble"],
                     dict(max_workspace_bytes=1 << 20), False),
    "loo_ensemble+basis": ("loo_ensemble", (T, FLUX, DIAG), dict(LIN, max_workspace_bytes=1 << 20),
                           ["f64", "lbo_linear"], dict(return_cov=False, max_workspace_bytes=1 << 20), False),
    "lbo_ensemble": ("lbo_ensemble", (T, FLUX, DIAG, 7), dict(return_cov=True), ["lbo_ensemble"],
                     dict(return_cov=True, max_workspace_bytes=None), False),
    "lbo_ensemble+basis": ("lbo_ensemble", (T, FLUX, DIAG, 7), dict(LIN, max_workspace_bytes=4096),
                           ["f64", "lbo_linear"], dict(return_cov=False, max_workspace_bytes=4096), False),
    "log_likelihood_linear_ensemble": ("log_likelihood_linear_ensemble", (T, FLUX, DIAG, U, 1e-4),
                                       dict(return_cov=False), ["f64", "lnlike_linear"],
                                       dict(return_cov=False, max_workspace_bytes=None), False),
    "log_likelihood_ensemble": ("log_likelihood_ensemble", (T, FLUX, DIAG), {},
                                ["f64", "f64", "stars_to_device", "lnlike_ensemble"], {}, False),
    "predict_ensemble": ("predict_ensemble", (T, FLUX, DIAG), dict(return_cov="diag"), ["predict_ensemble"],
                         dict(mode="diag"), True),
    "predict_ensemble+basis": ("predict_ensemble", (T, FLUX, DIAG), dict(LIN, basis_sample=U),
                               ["f64", "f64", "predict_linear"], dict(mode=True), True),
    "sample_conditional_ensemble": ("sample_conditional_ensemble", (T, FLUX, DIAG), {}, ["predict_ensemble"],
                                    dict(mode=True), True),
    "sample_conditional_ensemble+basis": ("sample_conditional_ensemble", (T, FLUX, DIAG), LIN,
                                          ["f64", "predict_linear"], dict(mode=True), True),
}


@pytest.mark.parametrize("normalized", (False, True))
@pytest.mark.parametrize("marginal", (False, True))
@pytest.mark.parametrize("name", sorted(OPENINGS))
def test_the_opening_and_the_keywords_of_the_engine_call(name, marginal, normalized):
    method, args, kw, after, own, predict = OPENINGS[name]
    sp, log = _stubbed(marginal, normalized)
    if predict and normalized:
        with pytest.raises(NotImplementedError):
            getattr(sp, method)(*args, **kw)
        assert log == []
        return
    with pytest.raises(Reached):
        getattr(sp, method)(*args, **kw)
    # log_likelihood_ensemble uploads the per-cadence variances before it binds; nothing else precedes _bind
    before = ["f64"] if name == "log_likelihood_ensemble" else []
    assert log == before + OPEN + (["kernel_table"] if marginal else []) + after
    final, _, got = sp._engine.final
    assert final == after[-1]
    tab, mv = ("TAB", "MV") if marginal else (None, None)
    want = dict(conditional=not marginal, covpts=123, tab=tab, meanvar=mv, rta1="RTA1", temporal="matern32")
    if not predict:
        want.update(normalized=normalized, norm_order=7, zmax=0.011)
    want.update(own)
    diag = got.pop("diag")
    if name == "log_likelihood_ensemble":
        assert diag[0] == "f64"
        diag = diag[1]
    assert np.array_equal(diag, DIAG)
    assert got == want
    if predict:
        assert not {"normalized", "norm_order", "zmax"} & set(got)


def test_a_scalar_variance_gives_no_diag():
    sp, _ = _stubbed(True, True)
    with pytest.raises(Reached):
        sp.lbo_ensemble(T, FLUX, 1e-6, 4)
    assert sp._engine.final[2]["diag"] is None
