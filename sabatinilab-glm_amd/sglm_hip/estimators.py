"""sklearn-protocol estimators backed by the MI355X engine.

``GLM.__init__`` (backend/sglm.py:95-130) picks an estimator class from the family and the
kwargs and calls ``Base(*args, **kwargs)``; it then uses ``.fit(X, y)``, ``.predict(X)``,
``.score(X, y)``, ``.coef_``, ``.intercept_`` (backend/sglm.py:184, 241, 347).  These
classes keep the constructor signatures and defaults of the scikit-learn estimators the
reference selects, so keyword errors surface the same way (``TypeError`` on unknown
kwargs), and replace their numerics with the batched IRLS engine:

  LinearRegression  min ||y - Xw - b||^2                      -> squared loss, lam = 0
  Ridge(alpha)      ||y - Xw - b||^2 + alpha ||w||^2          -> squared loss, lam = alpha
  TweedieRegressor  mean loss + alpha/2 ||w||^2                -> lam = alpha * n_train
                    (power 0 identity -> squared loss; power >= 1 log link -> Tweedie-log)
  Lasso/ElasticNet  1/(2n)||.||^2 + a rho |w|_1 + a(1-rho)/2 ||w||^2 -> Gram-space CD
  GroupLasso        1/(2n)||.||^2 + a rho sum_g sqrt(k_g)|w_g|_2 + a(1-rho)/2 ||w||^2
                    -> Gram-space block descent (glasso.py)
  TweedieRegressor(l1_ratio=rho > 0), log link:
                    mean loss + a rho |w|_1 + a(1-rho)/2 ||w||^2 -> proximal Newton (pn.py)
  BinomialRegressor mean [softplus(eta) - y eta] + alpha/2 ||w||^2, y in {0, 1}, logit link
                    (sklearn's HalfBinomialLoss in the TweedieRegressor objective; the GLM
                    'Binomial' name) -> lam = alpha * n_train
  NegativeBinomialRegressor
                    mean [(y + 1/kappa) log(1 + kappa e^eta) - y eta] + alpha/2 ||w||^2, y >= 0,
                    log link, dispersion kappa fixed or estimated by maximum likelihood
                    (kappa='ml', nb2.py) (NB2; the GLM 'NegativeBinomial' / 'NB2' names)
                    -> lam = alpha * n_train
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import engine as E


class NotYetImplementedError(NotImplementedError):
    """Defined here (the reference raises this name without defining it, sglm.py:126)."""


@dataclass
class Objective:
    kind: str          # 'irls' | 'cd' | 'pn' (log link with an L1 term: pn.prox_newton)
                       # | 'gcd' (group lasso: glasso block descent, ``groups`` set)
    family: int
    power: float
    alpha: float
    lam_scale: str     # 'abs' -> lam = alpha ; 'n' -> lam = alpha * n_train
    fit_intercept: bool
    max_iter: int
    l1_ratio: float = 0.0
    tol: float = 1e-4
    groups: tuple = None   # 'gcd': the group id of every column, as a tuple of ints

    def lam(self, n_train: float) -> float:
        return self.alpha * n_train if self.lam_scale == "n" else self.alpha

    def l1(self, n_train: float) -> float:
        """L1 penalty of a 'pn' objective in the engine's sum scaling (alpha rho n)."""
        return self.alpha * self.l1_ratio * n_train

    def l2(self, n_train: float) -> float:
        """L2 penalty of a 'pn' objective in the engine's sum scaling (alpha (1 - rho) n)."""
        return self.alpha * (1.0 - self.l1_ratio) * n_train


def _check_y_range(power: float, y: np.ndarray):
    """``in_y_true_range`` of the half-Tweedie losses (sklearn glm.py:231-235)."""
    if power == 0:
        return
    bad = np.any(y < 0) if 0 < power < 2 else np.any(y <= 0)
    if power < 0:
        bad = False
    if bad:
        name = {1: "HalfPoissonLoss", 2: "HalfGammaLoss"}.get(power, "HalfTweedieLoss")
        raise ValueError(f"Some value(s) of y are out of the valid range of the loss {name!r}.")


def check_binomial_y(y) -> np.ndarray:
    """The response of a Binomial fit as float64: bool / int / float values that are exactly 0
    or 1 on every row (host check, before any device work)."""
    y = np.asarray(y)
    if y.dtype == object:
        y = y.astype(np.float64)
    if not np.all((y == 0) | (y == 1)):
        raise ValueError("Binomial responses must be 0 or 1")
    return y.astype(np.float64).reshape(-1)


def host_matrix(X):
    """Host numeric values of a design given as a DataFrame / array-like.  A frame of numpy
    numeric columns converts as ``.values`` does; a frame with pandas nullable columns (what
    ``df.convert_dtypes()`` makes: Int64 / Float64 / boolean -- the production driver converts its
    frame before fitting, sglm_cb_concat_make_design_mat.py:244) converts per column block to
    float64 with pd.NA as NaN, where ``.values`` would build an object array that sklearn
    converts element by element; an object array converts to float64."""
    import pandas as pd
    if isinstance(X, pd.DataFrame):
        if all(isinstance(dt, np.dtype) and dt.kind in "fiub" for dt in X.dtypes):
            return X.values
        return X.to_numpy(dtype=np.float64, na_value=np.nan)
    if hasattr(X, "values") and not isinstance(X, np.ndarray):
        X = X.values
    X = np.asarray(X)
    if X.dtype == object:
        X = np.where(pd.isna(X), np.nan, X).astype(np.float64)
    return X


def _as2d(X):
    from .lagframe import LagFrame
    if isinstance(X, LagFrame):             # device-resident lagged frame: no host values
        if len(X.shape) != 2:
            raise ValueError("Expected 2D array")
        return X
    X = host_matrix(X)
    if X.ndim == 1:
        raise ValueError("Expected 2D array, got 1D array instead")
    return X


# Outside fit_set, the designs packed for the last DESIGN_CACHE_ENTRIES numpy arrays (any
# estimator; DESIGN_CACHE_MAX_BYTES of device memory in total) are kept and reused when a call
# on the same device passes an array with the same shape, dtype and bytes -- an xxh3-128
# digest of the whole buffer, so an array modified in place is packed again,
# as sklearn would read it again.  The digest runs at host memory speed; the pack it saves is a
# PCIe upload plus the device pack and bit-plane passes.  Designs above DESIGN_CACHE_MAX_BYTES
# of device memory are not kept (the reference keeps every fold's model alive).
DESIGN_CACHE_ENTRIES = 2
DESIGN_CACHE_MAX_BYTES = 1 << 30
_DESIGN_CACHE = __import__("collections").OrderedDict()
_DESIGN_CACHE_LOCK = __import__("threading").Lock()


def _cached_design(Xa):
    E.require_gpu()
    key = _digest(Xa)
    if key is not None:
        with _DESIGN_CACHE_LOCK:
            d = _DESIGN_CACHE.get(key)
            if d is not None:
                _DESIGN_CACHE.move_to_end(key)
                return d
    d = E.Design.from_host(Xa)
    nbytes = _design_bytes(d)
    if key is not None and nbytes <= DESIGN_CACHE_MAX_BYTES:
        with _DESIGN_CACHE_LOCK:
            _DESIGN_CACHE[key] = d
            # bounded by entry count AND by the device bytes the kept designs hold
            while len(_DESIGN_CACHE) > DESIGN_CACHE_ENTRIES or (
                    len(_DESIGN_CACHE) > 1 and
                    sum(_design_bytes(v) for v in _DESIGN_CACHE.values()) > DESIGN_CACHE_MAX_BYTES):
                _DESIGN_CACHE.popitem(last=False)
    return d


def _design_bytes(d) -> int:
    # d._xb: the dense copy only if it was built (reading d.xb would build it)
    return sum(t.numel() * t.element_size() for t in (d._xb, d.xf, d.xbits, d.rbits, d._cbits)
               if t is not None)


def clear_design_cache():
    """Drop the designs kept for predict / score (frees their device memory)."""
    with _DESIGN_CACHE_LOCK:
        _DESIGN_CACHE.clear()


def _digest(X):
    """(device, shape, dtype, xxh3-128 of the bytes) of a C-contiguous numpy array, else
    None: a design packed on another device, or an array whose bytes differ, never matches."""
    if not isinstance(X, np.ndarray) or not X.flags.c_contiguous or X.dtype == object:
        return None
    try:
        import torch
        import xxhash
    except ImportError:                       # pragma: no cover - part of the image
        return None
    return (torch.cuda.current_device(), X.shape, X.dtype.str,
            xxhash.xxh3_128_intdigest(memoryview(X).cast("B")))


class _EngineRegressor:
    _params: tuple = ()

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    # ---- sklearn-ish plumbing
    def get_params(self, deep=True):
        return {k: getattr(self, k) for k in self._params}

    def set_params(self, **kw):
        for k, v in kw.items():
            if k not in self._params:
                raise ValueError(f"Invalid parameter {k!r} for estimator {type(self).__name__}")
            setattr(self, k, v)
        return self

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self._params) + ") [sglm_hip]"

    # ---- objective
    def objective(self) -> Objective:  # pragma: no cover - abstract
        raise NotImplementedError

    def _objective(self) -> Objective:
        """The objective fit / predict use (NegativeBinomialRegressor(kappa='ml') has one only
        once fitted: at ``kappa_``)."""
        return self.objective()

    def _warm(self):
        if getattr(self, "warm_start", False) and hasattr(self, "coef_"):
            c = np.asarray(self.coef_, dtype=np.float64).reshape(-1)
            b = float(np.asarray(getattr(self, "intercept_", 0.0)).reshape(-1)[0]) if \
                np.ndim(getattr(self, "intercept_", 0.0)) else float(getattr(self, "intercept_", 0.0))
            return c, b
        return None, None

    # Designs already resident for this estimator, keyed by id() of the host array they were
    # packed from (set only for the duration of GLM.fit_set, which uses each of X / X_test
    # two or three times; outside it every call packs its X, as sklearn does).
    _resident = None

    def _design(self, X):
        res = self._resident
        if res is not None and id(X) in res and res[id(X)][0] is X:
            return res[id(X)][1]
        from .lagframe import LagFrame
        if isinstance(X, LagFrame):
            return X.design()
        return _cached_design(_as2d(X))

    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotYetImplementedError("sample_weight is not used by the reference path")
        Xh = X
        X = _as2d(X)
        obj = self.objective()
        if obj.family == E.FAM_BINOMIAL_LOGIT:
            y = check_binomial_y(y)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if X.shape[0] != y.shape[0]:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: "
                             f"[{X.shape[0]}, {y.shape[0]}]")
        # (NB2 takes Poisson's range: y >= 0)
        _check_y_range(obj.power if obj.family == E.FAM_TWEEDIE_LOG
                       else 1 if obj.family == E.FAM_NB2_LOG else 0, y)
        d = self._design(Xh)
        prob = E.Problem(d, [y], [np.ones(X.shape[0], np.uint8)])
        c0, b0 = self._warm()
        if c0 is not None and c0.shape[0] != X.shape[1]:
            c0, b0 = None, None
        if obj.kind == "cd":
            from . import cd
            res = cd.enet_fit(prob, [obj], [0], [0], coef0=[c0])[0]
        elif obj.kind == "gcd":
            from . import cd
            res = cd.enet_fit(prob, [obj], [0], [0], groups=obj.groups)[0]
        elif obj.kind == "pn":
            from . import pn
            nt = X.shape[0]
            req = E.FitReq(obj.family, obj.power, obj.l2(nt), 0, 0, obj.fit_intercept,
                           obj.max_iter, c0, b0, l1=obj.l1(nt))
            (res,), _ = pn.prox_newton(prob, [req])
        else:
            req = E.FitReq(obj.family, obj.power, obj.lam(X.shape[0]), 0, 0, obj.fit_intercept,
                           obj.max_iter, c0, b0)
            (res,), _ = E.irls(prob, [req])
        self._set_fitted(res.coef, res.intercept, res.n_iter)
        return self

    def _set_fitted(self, coef, intercept, n_iter):
        self.coef_ = np.asarray(coef, dtype=np.float64)
        self.intercept_ = float(intercept)
        self.n_iter_ = int(n_iter)
        self.n_features_in_ = self.coef_.shape[0]

    def _linear_predictor(self, X):
        import torch
        Xh = X
        X = _as2d(X)
        if X.shape[1] != self.coef_.shape[0]:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.coef_.shape[0]} features as input.")
        d = self._design(Xh)
        beta = np.zeros((1, d.P), dtype=np.float32)
        beta[0, : d.p] = self.coef_
        beta[0, d.p] = self.intercept_
        eta = d.eta(torch.from_numpy(beta).to(d.device))
        return eta[0, : d.n].double().cpu().numpy()

    def predict(self, X):
        eta = self._linear_predictor(X)
        obj = self._objective()
        if obj.family == E.FAM_BINOMIAL_LOGIT:
            return sigmoid_np(eta)
        return np.exp(eta) if obj.family in (E.FAM_TWEEDIE_LOG, E.FAM_NB2_LOG) else eta

    def inference(self, X, y, **kw):
        """Standard errors, z-tests, scale and (with ``groups=``) per-group Wald tests of this
        fitted model on the design ``X`` it was fitted on: ``inference.infer(X, y, self, **kw)``
        (``cov_type='cluster', clusters=ids`` for the covariance clustered by trial or session)."""
        from . import inference
        return inference.infer(X, y, self, **kw)

    def predict_bands(self, X, y, X_new=None, **kw):
        """Pointwise confidence bands of this fitted model's trace (``eta``, ``mean``, their
        standard errors, ``lo`` / ``hi``) on the rows of ``X_new`` (default: the design ``X`` it
        was fitted on), with ``groups=`` each group's share of the predictor and its band:
        ``inference.predict_bands(X, y, self, X_new, **kw)`` (``rows``, ``level`` and
        ``inference``'s ``cov_type``, ``scale``, ``clusters``)."""
        from . import inference
        return inference.predict_bands(X, y, self, X_new, **kw)

    def score(self, X, y, sample_weight=None):
        """R^2 (Gaussian estimators, sklearn RegressorMixin.score)."""
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        pred = self.predict(X)
        ssr = float(np.sum((y - pred) ** 2))
        sst = float(np.sum((y - y.mean()) ** 2))
        if sst == 0.0:
            return 1.0 if ssr == 0.0 else 0.0
        return 1.0 - ssr / sst


class LinearRegression(_EngineRegressor):
    _params = ("fit_intercept", "copy_X", "tol", "n_jobs", "positive")

    def __init__(self, *, fit_intercept=True, copy_X=True, tol=1e-6, n_jobs=None, positive=False):
        if positive:
            raise NotYetImplementedError("positive=True is not supported by the engine")
        super().__init__(fit_intercept=fit_intercept, copy_X=copy_X, tol=tol, n_jobs=n_jobs,
                         positive=positive)

    def objective(self):
        return Objective("irls", E.FAM_SQUARED, 0.0, 0.0, "abs", self.fit_intercept, 100)


class Ridge(_EngineRegressor):
    _params = ("alpha", "fit_intercept", "copy_X", "max_iter", "tol", "solver", "positive",
               "random_state")

    def __init__(self, alpha=1.0, *, fit_intercept=True, copy_X=True, max_iter=None, tol=1e-4,
                 solver="auto", positive=False, random_state=None):
        if positive:
            raise NotYetImplementedError("positive=True is not supported by the engine")
        super().__init__(alpha=alpha, fit_intercept=fit_intercept, copy_X=copy_X,
                         max_iter=max_iter, tol=tol, solver=solver, positive=positive,
                         random_state=random_state)

    def objective(self):
        if np.ndim(self.alpha) or self.alpha < 0:
            raise ValueError(f"The 'alpha' parameter of Ridge must be a float in the range [0.0, inf). Got {self.alpha!r} instead.")
        return Objective("irls", E.FAM_SQUARED, 0.0, float(self.alpha), "abs", self.fit_intercept, 100)


class ElasticNet(_EngineRegressor):
    _params = ("alpha", "l1_ratio", "fit_intercept", "precompute", "max_iter", "copy_X", "tol",
               "warm_start", "positive", "random_state", "selection")

    def __init__(self, alpha=1.0, *, l1_ratio=0.5, fit_intercept=True, precompute=False,
                 max_iter=1000, copy_X=True, tol=1e-4, warm_start=False, positive=False,
                 random_state=None, selection="cyclic"):
        if positive:
            raise NotYetImplementedError("positive=True is not supported by the engine")
        super().__init__(alpha=alpha, l1_ratio=l1_ratio, fit_intercept=fit_intercept,
                         precompute=precompute, max_iter=max_iter, copy_X=copy_X, tol=tol,
                         warm_start=warm_start, positive=positive, random_state=random_state,
                         selection=selection)

    def objective(self):
        return Objective("cd", E.FAM_SQUARED, 0.0, float(self.alpha), "abs", self.fit_intercept,
                         int(self.max_iter), float(self.l1_ratio), float(self.tol))


class Lasso(ElasticNet):
    _params = ("alpha", "fit_intercept", "precompute", "copy_X", "max_iter", "tol", "warm_start",
               "positive", "random_state", "selection")

    def __init__(self, alpha=1.0, *, fit_intercept=True, precompute=False, copy_X=True,
                 max_iter=1000, tol=1e-4, warm_start=False, positive=False, random_state=None,
                 selection="cyclic"):
        super().__init__(alpha=alpha, l1_ratio=1.0, fit_intercept=fit_intercept,
                         precompute=precompute, max_iter=max_iter, copy_X=copy_X, tol=tol,
                         warm_start=warm_start, positive=positive, random_state=random_state,
                         selection=selection)


class GroupLasso(_EngineRegressor):
    """Group lasso in sklearn ElasticNet's scaling,
    1/(2n)|y - Xw - b|^2 + alpha rho sum_g sqrt(k_g) |w_g|_2 + alpha (1 - rho)/2 |w|^2 with
    rho = l1_ratio in (0, 1]: ``groups`` gives one integer id per column, equal ids form a
    group of k_g columns (the ids themselves are arbitrary), and a group's coefficients are
    all in the model or all exactly zero.  With every column its own group this is ElasticNet;
    ``alpha == 0`` is LinearRegression's objective.  No warm start along a path yet
    (``warm_start`` is accepted and not used)."""
    _params = ("alpha", "groups", "l1_ratio", "fit_intercept", "max_iter", "tol", "warm_start")

    def __init__(self, alpha=1.0, *, groups, l1_ratio=1.0, fit_intercept=True, max_iter=1000,
                 tol=1e-4, warm_start=False):
        super().__init__(alpha=alpha, groups=groups, l1_ratio=l1_ratio,
                         fit_intercept=fit_intercept, max_iter=max_iter, tol=tol,
                         warm_start=warm_start)

    def objective(self):
        if np.ndim(self.alpha) or self.alpha < 0:
            raise ValueError(f"The 'alpha' parameter of GroupLasso must be a float in the range "
                             f"[0.0, inf). Got {self.alpha!r} instead.")
        rho = float(self.l1_ratio)
        if not 0.0 < rho <= 1.0:
            raise ValueError(f"The 'l1_ratio' parameter of GroupLasso must be a float in the "
                             f"range (0.0, 1.0]. Got {self.l1_ratio!r} instead.")
        if self.alpha == 0:
            return LinearRegression(fit_intercept=self.fit_intercept).objective()
        ids = np.asarray(self.groups).reshape(-1)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise TypeError("groups: integer group ids, one per column")
        return Objective("gcd", E.FAM_SQUARED, 0.0, float(self.alpha), "abs", self.fit_intercept,
                         int(self.max_iter), rho, float(self.tol),
                         groups=tuple(int(v) for v in ids))

    def fit(self, X, y, sample_weight=None):
        if self.alpha != 0 and np.asarray(self.groups).reshape(-1).shape[0] != _as2d(X).shape[1]:
            raise ValueError(f"groups has {np.asarray(self.groups).reshape(-1).shape[0]} entries, "
                             f"X has {_as2d(X).shape[1]} columns")
        return super().fit(X, y, sample_weight)


class TweedieRegressor(_EngineRegressor):
    _params = ("power", "alpha", "fit_intercept", "link", "solver", "max_iter", "tol",
               "warm_start", "verbose", "l1_ratio")

    def __init__(self, *, power=0.0, alpha=1.0, fit_intercept=True, link="auto", solver="lbfgs",
                 max_iter=100, tol=1e-4, warm_start=False, verbose=0, l1_ratio=0.0):
        super().__init__(power=power, alpha=alpha, fit_intercept=fit_intercept, link=link,
                         solver=solver, max_iter=max_iter, tol=tol, warm_start=warm_start,
                         verbose=verbose, l1_ratio=l1_ratio)

    def _log_link(self):
        if self.link == "auto":
            return self.power > 0
        if self.link not in ("log", "identity"):
            raise ValueError(f"The 'link' parameter of TweedieRegressor must be a str among "
                             f"{{'auto', 'identity', 'log'}}. Got {self.link!r} instead.")
        return self.link == "log"

    def objective(self):
        p = float(self.power)
        if 0 < p < 1:
            raise ValueError("Tweedie power between 0 and 1 is not a valid distribution")
        log = self._log_link()
        if log and p >= 1:
            fam = E.FAM_TWEEDIE_LOG
        elif not log and p == 0:
            fam = E.FAM_SQUARED
        else:
            raise NotYetImplementedError(f"TweedieRegressor(power={p}, link={self.link!r}) "
                                         "is outside the engine's families")
        if self.alpha < 0:
            raise ValueError("alpha must be >= 0")
        rho = float(self.l1_ratio)
        if not 0.0 <= rho <= 1.0:
            raise ValueError(f"The 'l1_ratio' parameter of {type(self).__name__} must be a float "
                             f"in the range [0.0, 1.0]. Got {self.l1_ratio!r} instead.")
        if rho > 0.0 and self.alpha > 0:
            if fam == E.FAM_SQUARED:
                # power 0 with the identity link is sklearn's ElasticNet objective itself
                return ElasticNet(alpha=self.alpha, l1_ratio=rho,
                                  fit_intercept=self.fit_intercept).objective()
            return Objective("pn", fam, p, float(self.alpha), "n", self.fit_intercept,
                             int(self.max_iter), rho)
        return Objective("irls", fam, p if fam == E.FAM_TWEEDIE_LOG else 0.0, float(self.alpha),
                         "n", self.fit_intercept, int(self.max_iter))

    def score(self, X, y, sample_weight=None):
        """D^2, fraction of deviance explained (sklearn glm.py:371-444)."""
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        obj = self.objective()
        eta = self._linear_predictor(X)
        if obj.family == E.FAM_SQUARED:            # D^2 of the squared loss == R^2
            ssr = float(np.sum((y - eta) ** 2))
            sst = float(np.sum((y - y.mean()) ** 2))
            return (1.0 if ssr == 0 else 0.0) if sst == 0 else 1.0 - ssr / sst
        _check_y_range(obj.power, y)
        dev = np.mean(half_loss_np(obj.power, y, eta))
        ym = y.mean()
        dev0 = np.mean(half_loss_np(obj.power, y, np.full_like(y, math.log(ym))))
        const = np.mean(loss_constant_np(obj.power, y))
        return 1.0 - (dev + const) / (dev0 + const)


class PoissonRegressor(TweedieRegressor):
    _params = ("alpha", "fit_intercept", "solver", "max_iter", "tol", "warm_start", "verbose",
               "l1_ratio")

    def __init__(self, *, alpha=1.0, fit_intercept=True, solver="lbfgs", max_iter=100, tol=1e-4,
                 warm_start=False, verbose=0, l1_ratio=0.0):
        super().__init__(power=1.0, alpha=alpha, fit_intercept=fit_intercept, link="log",
                         solver=solver, max_iter=max_iter, tol=tol, warm_start=warm_start,
                         verbose=verbose, l1_ratio=l1_ratio)


class BinomialRegressor(_EngineRegressor):
    """Bernoulli GLM with the logit link in TweedieRegressor's mean-scaled objective,
    mean_i [softplus(eta_i) - y_i eta_i] + alpha/2 |w|^2 (unpenalised intercept): the minimiser
    of sklearn LogisticRegression(C = 1 / (alpha n)).  Responses are exactly 0 or 1."""
    _params = ("alpha", "fit_intercept", "solver", "max_iter", "tol", "warm_start", "verbose",
               "l1_ratio")

    def __init__(self, *, alpha=1.0, fit_intercept=True, solver="lbfgs", max_iter=100, tol=1e-4,
                 warm_start=False, verbose=0, l1_ratio=0.0):
        super().__init__(alpha=alpha, fit_intercept=fit_intercept, solver=solver,
                         max_iter=max_iter, tol=tol, warm_start=warm_start, verbose=verbose,
                         l1_ratio=l1_ratio)

    def objective(self):
        if self.alpha < 0:
            raise ValueError("alpha must be >= 0")
        rho = float(self.l1_ratio)
        if not 0.0 <= rho <= 1.0:
            raise ValueError(f"The 'l1_ratio' parameter of {type(self).__name__} must be a float "
                             f"in the range [0.0, 1.0]. Got {self.l1_ratio!r} instead.")
        if rho > 0.0 and self.alpha > 0:
            raise NotYetImplementedError("BinomialRegressor(l1_ratio > 0): elastic-net penalties "
                                         "on the logit link")
        return Objective("irls", E.FAM_BINOMIAL_LOGIT, 0.0, float(self.alpha), "n",
                         self.fit_intercept, int(self.max_iter))

    def decision_function(self, X):
        """The linear predictor eta = X w + b."""
        return self._linear_predictor(X)

    def score(self, X, y, sample_weight=None):
        """D^2, the fraction of binomial deviance explained (as TweedieRegressor.score; the
        loss constant of 0/1 labels is 0)."""
        y = check_binomial_y(y)
        dev = np.sum(binomial_loss_np(y, self._linear_predictor(X)))
        dev0 = binomial_null_np(float(y.size), float(y.mean()))
        return 1.0 - dev / dev0 if dev0 > 0 else (1.0 if dev == 0 else 0.0)


def nb2_kappa(kappa) -> float:
    """The dispersion every layer uses: ``kappa`` rounded to float32 once (the C ABI carries it in
    the float ``power`` argument of the row passes), as a Python float.  The kernels, the host
    scores, the null deviance and the saturated constant all take this one value."""
    k = float(kappa)
    if not (math.isfinite(k) and k > 0.0):
        raise ValueError(f"kappa must be a finite float > 0. Got {kappa!r} instead.")
    with np.errstate(over="ignore", under="ignore"):
        k32 = float(np.float32(k))
    if not (math.isfinite(k32) and k32 > 0.0 and math.isfinite(1.0 / k32)):
        raise ValueError(f"kappa = {kappa!r} is outside the float32 range")
    return k32


class NegativeBinomialRegressor(_EngineRegressor):
    """Negative-binomial GLM (NB2: Var y = mu + kappa mu^2) with the log link and a fixed
    dispersion ``kappa > 0``, in TweedieRegressor's mean-scaled objective,
    mean_i [(y_i + 1/kappa) log(1 + kappa e^eta_i) - y_i eta_i] + alpha/2 |w|^2 (unpenalised
    intercept): statsmodels' ``NegativeBinomial(alpha=kappa)`` family, pyglmnet's
    ``'neg-binomial'`` with a fixed theta.  kappa -> 0 is PoissonRegressor.  Responses are >= 0
    (non-integers accepted, as for Poisson).

    ``kappa`` is rounded to float32 once (``nb2_kappa``: the C ABI carries it in a float) and
    that value is the dispersion of the fit, of ``score`` and of the grid's scores;
    ``get_params`` returns what was given.

    ``kappa='ml'`` estimates the dispersion by maximum likelihood (integer counts required):
    ``fit`` alternates the fixed-kappa fit with ``nb2.profile`` (the likelihood's maximiser in
    kappa at that fit's predictor) from the moment estimate (s^2 - ybar) / ybar^2 clipped to
    [2^-6, 2^6], each round warm-started from the last, until |d ln kappa| <= 2^-20 (at most
    ``ML_MAX_ROUNDS`` rounds).  ``kappa_`` is the float32 value the returned coefficients were
    fitted at (``coef_`` is exactly the fixed-kappa fit at ``kappa_``), with ``kappa_n_rounds_``,
    ``kappa_converged_``, ``kappa_at_bound_`` and ``n_iter_`` (the IRLS iterations of all
    rounds); ``score`` and ``predict`` use ``kappa_``.  Counts without over-dispersion end at
    the lower bound 2^-20 with a ``UserWarning`` (the Poisson limit).  ``objective()`` has no
    value before the fit, so the CV grids refuse ``'ml'``: put kappa on the parameter grid with
    ``score_method='ll'`` there.
    Elastic-net and group penalties and drop sets are not implemented."""
    ML_MAX_ROUNDS = 25
    ML_TOL = 2.0 ** -20
    _params = ("kappa", "alpha", "fit_intercept", "solver", "max_iter", "tol", "warm_start",
               "verbose", "l1_ratio")

    def __init__(self, *, kappa=1.0, alpha=1.0, fit_intercept=True, solver="lbfgs", max_iter=100,
                 tol=1e-4, warm_start=False, verbose=0, l1_ratio=0.0):
        super().__init__(kappa=kappa, alpha=alpha, fit_intercept=fit_intercept, solver=solver,
                         max_iter=max_iter, tol=tol, warm_start=warm_start, verbose=verbose,
                         l1_ratio=l1_ratio)

    def _is_ml(self) -> bool:
        return isinstance(self.kappa, str) and self.kappa == "ml"

    def _kappa(self) -> float:
        """The dispersion of predict / score: the given one, or the fitted ``kappa_``."""
        if not self._is_ml():
            return nb2_kappa(self.kappa)
        if not hasattr(self, "kappa_"):
            raise AttributeError("NegativeBinomialRegressor(kappa='ml') is not fitted yet: "
                                 "kappa_ is set by fit")
        return float(self.kappa_)

    def objective(self):
        if self._is_ml():
            raise NotYetImplementedError(
                "NegativeBinomialRegressor(kappa='ml') has no objective before it is fitted, and "
                "a CV grid solves one (family, kappa) per launch: put kappa on the parameter "
                "grid with score_method='ll' instead")
        return self._objective_at(nb2_kappa(self.kappa))

    def _objective(self):
        return self._objective_at(self._kappa())

    def _objective_at(self, kappa):
        if self.alpha < 0:
            raise ValueError("alpha must be >= 0")
        rho = float(self.l1_ratio)
        if not 0.0 <= rho <= 1.0:
            raise ValueError(f"The 'l1_ratio' parameter of {type(self).__name__} must be a float "
                             f"in the range [0.0, 1.0]. Got {self.l1_ratio!r} instead.")
        if rho > 0.0 and self.alpha > 0:
            raise NotYetImplementedError("NegativeBinomialRegressor(l1_ratio > 0): elastic-net "
                                         "penalties on the NB2 family")
        return Objective("irls", E.FAM_NB2_LOG, kappa, float(self.alpha), "n",
                         self.fit_intercept, int(self.max_iter))

    def fit(self, X, y, sample_weight=None):
        if not self._is_ml():
            return super().fit(X, y, sample_weight)
        import warnings
        from . import nb2
        if sample_weight is not None:
            raise NotYetImplementedError("sample_weight is not used by the reference path")
        obj = self._objective_at(1.0)                       # validates alpha / l1_ratio
        Xh = X
        X = _as2d(X)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if X.shape[0] != y.shape[0]:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: "
                             f"[{X.shape[0]}, {y.shape[0]}]")
        _check_y_range(1, y)
        y = nb2.check_counts(y)
        d = self._design(Xh)
        n = X.shape[0]
        prob = E.Problem(d, [y], [np.ones(n, np.uint8)])
        tails = nb2.count_tails(prob)
        c0, b0 = self._warm()
        if c0 is not None and c0.shape[0] != X.shape[1]:
            c0, b0 = None, None
        kappa = nb2.moment_kappa(tails[0, 0], float(n))
        n_iter, converged, at_bound = 0, False, False
        for rnd in range(1, self.ML_MAX_ROUNDS + 1):
            kfit = nb2_kappa(kappa)
            req = E.FitReq(obj.family, kfit, obj.lam(n), 0, 0, obj.fit_intercept, obj.max_iter,
                           c0, b0)
            (res,), eta = E.irls(prob, [req])
            n_iter += res.n_iter
            ks, ab, _ = nb2.profile(prob, eta, [0], [0], [0], tails, start=[kfit])
            kappa, at_bound = float(ks[0]), bool(ab[0])
            if abs(math.log(kappa) - math.log(kfit)) <= self.ML_TOL:
                converged = True
                break
            c0, b0 = res.coef, (res.intercept if obj.fit_intercept else None)
        self._set_fitted(res.coef, res.intercept, n_iter)
        self.kappa_ = kfit
        self.kappa_n_rounds_ = rnd
        self.kappa_converged_ = converged
        self.kappa_at_bound_ = at_bound
        if at_bound and kappa == nb2.KAPPA_LO:
            warnings.warn("NegativeBinomialRegressor(kappa='ml'): the likelihood has no "
                          "over-dispersion to fit (the Poisson limit); fitted at the lower bound "
                          "kappa = 2^-20 -- PoissonRegressor is the model for these counts",
                          UserWarning, stacklevel=2)
        elif at_bound:
            warnings.warn("NegativeBinomialRegressor(kappa='ml'): the likelihood still rises at "
                          "the upper bound kappa = 2^10", UserWarning, stacklevel=2)
        elif not converged:
            warnings.warn(f"NegativeBinomialRegressor(kappa='ml'): kappa did not settle within "
                          f"{self.ML_MAX_ROUNDS} rounds (last |d ln kappa| = "
                          f"{abs(math.log(kappa) - math.log(kfit)):.3g})", UserWarning,
                          stacklevel=2)
        return self

    def score(self, X, y, sample_weight=None):
        """D^2, the fraction of NB2 deviance explained at the fit's kappa:
        1 - (sum loss + sum c) / (null + sum c), c the saturated constant."""
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        _check_y_range(1, y)
        kappa = self._kappa()
        dev = float(np.sum(nb2_loss_np(kappa, y, self._linear_predictor(X))))
        const = float(np.sum(nb2_constant_np(kappa, y)))
        dev0 = nb2_null_np(kappa, float(y.size), float(y.sum()))
        den = dev0 + const
        return 1.0 - (dev + const) / den if den > 0 else (1.0 if dev + const <= 0 else 0.0)


class LogisticRegression:
    """Out of scope: the reference's Logistic/Multinomial path."""

    def __init__(self, *a, **k):
        raise NotYetImplementedError("Logistic/Multinomial GLMs are outside the MI355X engine's "
                                     "scope (SURVEY.md §8(a) A2)")


def half_loss_np(power, y, eta):
    """Host float64 half-Tweedie loss (log link) for scores only."""
    if power == 1:
        return np.exp(eta) - y * eta
    if power == 2:
        return eta + y * np.exp(-eta)
    return np.exp((2 - power) * eta) / (2 - power) - y * np.exp((1 - power) * eta) / (1 - power)


def sigmoid_np(eta):
    """Host float64 logistic function, no overflow."""
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def binomial_loss_np(y, eta):
    """Host float64 half-binomial loss softplus(eta) - y eta (logit link) for scores only."""
    return np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))) - y * eta


def binomial_null_np(cnt: float, ym: float) -> float:
    """Summed loss of 0/1 labels with mean ``ym`` over ``cnt`` rows at eta = logit(ym), in closed
    form: -cnt (ym ln ym + (1 - ym) ln(1 - ym)); 0 when every label is the same."""
    if not 0.0 < ym < 1.0:
        return 0.0
    return -cnt * (ym * math.log(ym) + (1.0 - ym) * math.log1p(-ym))


def nb2_loss_np(kappa, y, eta):
    """Host float64 NB2 loss (y + 1/kappa) softplus(eta + ln kappa) - y eta (log link): the
    negative log-likelihood up to terms free of eta.  For scores only."""
    z = eta + math.log(kappa)
    return (y + 1.0 / kappa) * (np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))) - y * eta


def nb2_constant_np(kappa, y):
    """The NB2 saturated constant c(y) = y ln y - (y + 1/kappa) ln(1 + kappa y), 0 at y = 0:
    loss + c >= 0, 0 at mu = y."""
    y = np.asarray(y, dtype=np.float64)
    pos = y > 0
    ys = np.where(pos, y, 1.0)
    return np.where(pos, ys * np.log(ys) - (ys + 1.0 / kappa) * np.log1p(kappa * ys), 0.0)


def nb2_null_np(kappa: float, cnt: float, sy: float) -> float:
    """Summed NB2 loss of ``cnt`` rows with sum ``sy`` at the null optimum eta = log(mean y), in
    closed form: (sy + cnt/kappa) log(1 + kappa ybar) - sy log ybar (0 rows or ybar = 0: 0)."""
    if cnt <= 0 or sy <= 0:
        return 0.0
    ym = sy / cnt
    return (sy + cnt / kappa) * math.log1p(kappa * ym) - sy * math.log(ym)


def loss_constant_np(power, y):
    if power == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0)), 0.0) - y
    if power == 2:
        return -np.log(y) - 1
    return np.power(np.maximum(y, 0), 2 - power) / (1 - power) / (2 - power)


def objective_for(Base, kwargs) -> Objective:
    """Construct the estimator (validating kwargs exactly as GLM would) and return its objective."""
    return Base(**kwargs).objective()
