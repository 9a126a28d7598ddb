"""The negative-binomial (NB2, log link) family without a GPU: the loss against scipy's pmf, the
float64 Newton oracle of tests/nb2_cases.py against scipy.optimize and the Poisson limit, the D^2
helpers, the host surface (dispatch, kappa's float32 rounding, refusals) and the synthetic
counts."""
import math

import numpy as np
import pytest
import scipy.optimize
import scipy.special
import scipy.stats

import nb2_cases as nc


@pytest.mark.parametrize("kappa", [0.25, 1.0, nc.k32(0.3), 8.0, 2.0 ** -10])
def test_loss_is_the_negative_log_pmf_up_to_eta_free_terms(kappa):
    """l(y, eta) - [lgamma(y + 1) + lgamma(1/kappa) - lgamma(y + 1/kappa) - y ln kappa]
    = -nbinom.logpmf(y, 1/kappa, 1/(1 + kappa mu)) on integer y, to 1e-12 relative."""
    rng = np.random.default_rng(5)
    y = rng.integers(0, 40, 400).astype(np.float64)
    eta = rng.normal(0.5, 1.5, 400)
    r = 1.0 / kappa
    free = (scipy.special.gammaln(y + 1) + scipy.special.gammaln(r)
            - scipy.special.gammaln(y + r) - y * math.log(kappa))
    ref = -scipy.stats.nbinom.logpmf(y, r, 1.0 / (1.0 + kappa * np.exp(eta)))
    got = nc.loss(kappa, y, eta) + free
    # relative to the terms that are added: |l| and each lgamma on its own (at small kappa
    # lgamma(1/kappa) and lgamma(y + 1/kappa) are thousands and cancel to tens, so each side
    # carries their rounding, not that of their difference)
    scale = (np.abs(nc.loss(kappa, y, eta)) + scipy.special.gammaln(y + 1)
             + np.abs(scipy.special.gammaln(r)) + np.abs(scipy.special.gammaln(y + r))
             + np.abs(y * math.log(kappa)))
    assert np.max(np.abs(got - ref) / scale) <= 1e-12


def test_loss_tends_to_poisson():
    y = np.array([0.0, 1.0, 3.0, 7.5])
    eta = np.array([-2.0, 0.3, 1.0, 2.0])
    assert np.max(np.abs(nc.loss(2.0 ** -30, y, eta) - (np.exp(eta) - y * eta))) < 1e-7


def _minimize(X, y, alpha, kappa, fit_intercept):
    n, p = X.shape
    f = y + 1.0 / kappa
    lk = math.log(kappa)

    def fun(c):
        w, b = c[:p], (c[p] if fit_intercept else 0.0)
        eta = X @ w + b
        r = f * nc.sigmoid(eta + lk) - y
        g = np.concatenate([X.T @ r / n + alpha * w, [r.mean()] if fit_intercept else []])
        return nc.loss(kappa, y, eta).mean() + 0.5 * alpha * w @ w, g
    c0 = np.zeros(p + int(fit_intercept))
    if fit_intercept:
        c0[p] = math.log(y.mean())
    return scipy.optimize.minimize(fun, c0, jac=True, method="L-BFGS-B",
                                   options=dict(maxiter=5000, ftol=1e-15, gtol=1e-10,
                                                maxcor=30)).fun


@pytest.mark.parametrize("fi", [True, False])
@pytest.mark.parametrize("kappa", nc.KAPPAS_A)
@pytest.mark.parametrize("alpha", nc.ALPHAS_A)
def test_oracle_case_a_is_stationary_and_not_above_lbfgs(alpha, kappa, fi):
    _, X, y = nc.case_a()
    k = nc.k32(kappa)
    w, b = nc.oracle("A", alpha, kappa, fi)
    assert nc.gradient(k, X, y, alpha, w, b, fi) <= 1e-10
    f_ref = _minimize(X, y, alpha, k, fi)
    assert nc.objective(k, X, y, alpha, w, b) <= f_ref + 1e-15 * abs(f_ref)


def test_oracle_case_t_reaches_the_saturated_tail():
    _, X, y = nc.case_t()
    w, b = nc.oracle("T", nc.ALPHA_T, nc.KAPPA_T)
    assert nc.gradient(nc.KAPPA_T, X, y, nc.ALPHA_T, w, b) <= 1e-10
    km = nc.KAPPA_T * np.exp(X @ w + b)
    assert km.max() >= 100 and np.sum(km >= 100) >= 5
    f_ref = _minimize(X, y, nc.ALPHA_T, nc.KAPPA_T, True)
    assert nc.objective(nc.KAPPA_T, X, y, nc.ALPHA_T, w, b) <= f_ref + 1e-15 * abs(f_ref)


def test_oracle_case_z_is_the_poisson_limit():
    from oracle import glm_ref
    _, X, y = nc.case_a()
    w, b = nc.oracle("Z", nc.ALPHA_Z, nc.KAPPA_Z)
    assert nc.gradient(nc.KAPPA_Z, X, y, nc.ALPHA_Z, w, b) <= 1e-10
    wp, bp = glm_ref.fit_tweedie_newton(X, y, nc.ALPHA_Z, 1.0)
    scale = np.max(np.abs(wp))
    assert np.max(np.abs(w - wp)) <= 1e-3 * scale and abs(b - bp) <= 1e-3 * scale
    wm, bm = nc.oracle("M", nc.ALPHA_M, nc.KAPPA_M)
    Xm, ym = nc.case_mixed()
    assert nc.gradient(nc.KAPPA_M, Xm, ym, nc.ALPHA_M, wm, bm) <= 1e-10


@pytest.mark.parametrize("kappa", [0.25, nc.k32(0.3), 8.0, 2.0 ** -16])
def test_d2_helpers(kappa):
    """loss + c >= 0, 0 at mu = y; the closed-form null loss is the loss at log(mean y); the
    estimators' host helpers are the cases' own."""
    from sglm_hip import estimators as est
    rng = np.random.default_rng(8)
    y = np.concatenate([[0.0, 0.0, 1.0, 2.5], rng.integers(0, 60, 200).astype(np.float64)])
    eta = rng.normal(0.5, 2.0, y.size)
    dev = nc.loss(kappa, y, eta) + nc.constant(kappa, y)
    scale = np.abs(nc.loss(kappa, y, eta)) + np.abs(nc.constant(kappa, y))
    assert np.all(dev >= -4e-16 * scale)
    pos = y > 0
    at = nc.loss(kappa, y[pos], np.log(y[pos])) + nc.constant(kappa, y[pos])
    sc = (y[pos] + 1.0 / kappa) * np.log1p(kappa * y[pos]) + np.abs(y[pos] * np.log(y[pos]))
    assert np.max(np.abs(at) / sc) <= 1e-14
    assert np.all(nc.constant(kappa, np.zeros(3)) == 0)
    # y = 0: the loss tends to 0 as eta -> -inf, never below
    assert np.all(nc.loss(kappa, 0.0, np.array([-50.0, -5.0, 0.0])) > 0)
    ref = float(np.sum(nc.loss(kappa, y, np.full(y.size, math.log(y.mean())))))
    assert abs(nc.null_loss(kappa, y) - ref) <= 1e-13 * abs(ref)
    assert abs(est.nb2_null_np(kappa, float(y.size), float(y.sum())) - ref) <= 1e-13 * abs(ref)
    assert est.nb2_null_np(kappa, 0.0, 0.0) == 0.0 and est.nb2_null_np(kappa, 5.0, 0.0) == 0.0
    assert np.array_equal(est.nb2_loss_np(kappa, y, eta), nc.loss(kappa, y, eta))
    assert np.array_equal(est.nb2_constant_np(kappa, y), nc.constant(kappa, y))
    assert abs(nc.d2(kappa, y, np.full(y.size, math.log(y.mean())))) < 1e-12
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        big = est.nb2_loss_np(kappa, np.array([0.0, 3.0]), np.array([-800.0, 800.0]))
    assert np.all(np.isfinite(big))


def test_dispatch_params_and_kappa_rounding():
    import sglm
    import sglm_
    from sglm.models import sglm as models_sglm
    from sglm_hip import engine as E, estimators as est
    assert E.FAM_NB2_LOG == 3
    assert sglm_.NegativeBinomialRegressor is est.NegativeBinomialRegressor
    assert models_sglm.NegativeBinomialRegressor is est.NegativeBinomialRegressor
    for name in ("NegativeBinomial", "NB2"):
        g = sglm.GLM(name, alpha=0.5, kappa=0.3)
        assert type(g.model) is est.NegativeBinomialRegressor
        assert g.model.get_params() == dict(kappa=0.3, alpha=0.5, fit_intercept=True,
                                            solver="lbfgs", max_iter=100, tol=1e-4,
                                            warm_start=False, verbose=0, l1_ratio=0.0)
        o = g.model.objective()
        assert (o.kind, o.family, o.alpha, o.lam_scale) == ("irls", 3, 0.5, "n")
        # kappa is rounded to float32 once: that value is the dispersion of every layer
        assert o.power == float(np.float32(0.3)) != 0.3
        assert o.lam(200.0) == 100.0
    d = est.NegativeBinomialRegressor()
    assert d.kappa == 1.0 and d.alpha == 1.0 and d.objective().power == 1.0
    assert est.nb2_kappa(2.0 ** -16) == 2.0 ** -16
    m = est.NegativeBinomialRegressor(kappa=0.25)
    m.set_params(kappa=2.0)
    assert m.objective().power == 2.0 and "kappa=2.0" in repr(m)
    # the existing names dispatch as they did
    assert type(sglm.GLM("Poisson", alpha=0.1).model) is est.TweedieRegressor
    assert type(sglm.GLM("Binomial", alpha=0.1).model) is est.BinomialRegressor
    with pytest.raises(est.NotYetImplementedError):
        sglm.GLM("NegBin")


@pytest.mark.parametrize("kappa", [0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60])
def test_bad_kappa_is_refused(kappa):
    import sglm
    from sglm_hip import estimators as est
    with pytest.raises(ValueError, match="kappa"):
        est.NegativeBinomialRegressor(kappa=kappa).objective()
    with pytest.raises(ValueError, match="kappa"):
        sglm.GLM("NB2", alpha=0.1, kappa=kappa).fit(np.zeros((4, 2)), np.array([0, 1, 0, 2.]))


def test_refusals_on_the_host():
    import sglm
    from sglm_hip import estimators as est, grid
    X, y = np.zeros((4, 2)), np.array([0, 1, 0, 3.0])
    with pytest.raises(est.NotYetImplementedError):
        sglm.GLM("NegativeBinomial", alpha=.1, kappa=.5, l1_ratio=.5).model.objective()
    with pytest.raises(est.NotYetImplementedError):
        sglm.GLM("NB2", alpha=.1, l1_ratio=.5).fit(X, y)
    with pytest.raises(ValueError):
        est.NegativeBinomialRegressor(l1_ratio=1.5).objective()
    with pytest.raises(ValueError):
        est.NegativeBinomialRegressor(alpha=-1.0).objective()
    # alpha = 0 carries no L1 term whatever l1_ratio says (as TweedieRegressor)
    assert est.NegativeBinomialRegressor(alpha=0.0, l1_ratio=.5).objective().kind == "irls"
    for name in ("NegativeBinomial", "NB2"):
        with pytest.raises(est.NotYetImplementedError, match="groups"):
            sglm.GLM(name, alpha=.1, groups=[0, 1])
    # y < 0: Poisson's ValueError, before any device work
    with pytest.raises(ValueError, match="out of the valid range"):
        sglm.GLM("NB2", alpha=.1).fit(X, np.array([0, 1, -1, 2.0]))
    with pytest.raises(ValueError, match="out of the valid range"):
        est.NegativeBinomialRegressor().score(X, np.array([0, 1, -1, 2.0]))
    obj = est.NegativeBinomialRegressor(alpha=.1, kappa=.5).objective()
    groups = [{"cv_idx": [], "objectives": [obj], "rolls": [0]}]
    with pytest.raises(est.NotYetImplementedError, match="drop sets"):
        grid.check_drop_sets([[], [0]], 2, groups)
    assert grid.check_drop_sets([[]], 2, groups) == [[]]


def test_synth_nb2_counts_and_other_families_unchanged():
    """Gamma-Poisson counts: mean mu and variance mu + kappa mu^2 within sampling error at a fixed
    seed; the draws are rng(seed + 2)'s Gamma then Poisson streams; the other families' streams
    stay where tests/test_binomial_cpu.py pins them."""
    from sglm_hip import synth
    kappa = 0.5
    kw = dict(N=200000, m=2, L=2, rho=0.05, seed=21, beta_scale=0.0)
    s = synth.make(family="nb2", kappa=kappa, intercept=math.log(3.0), **kw)
    assert s.family == "nb2" and np.all(s.y >= 0) and np.all(s.y == np.round(s.y))
    mu, n = 3.0, kw["N"]
    var = mu + kappa * mu * mu
    # the mean's standard error, and the sample variance's from the fourth central moment
    # (bounded by 60 var^2 for this NB2: kurtosis = 3 + 6 kappa + 1 / var < 8)
    assert abs(s.y.mean() - mu) <= 5 * math.sqrt(var / n)
    assert abs(s.y.var() - var) <= 5 * var * math.sqrt(8.0 / n)
    assert s.y.var() > 1.5 * mu                                  # over-dispersed
    rng2 = np.random.default_rng(kw["seed"] + 2)
    g = rng2.gamma(1.0 / kappa, kappa, size=n)
    assert np.array_equal(s.y, rng2.poisson(mu * g).astype(np.float64))
    assert synth.make(N=50, m=2, L=2, family="nb2").intercept == -1.0
    with pytest.raises(ValueError):
        synth.make(N=50, m=2, L=2, family="nb2", kappa=0.0)
    kw = dict(N=3000, m=5, L=3, rho=0.05, seed=9, beta_scale=0.4)
    p = synth.make(family="poisson", **kw)
    q = synth.make(family="nb2", **kw)
    assert np.array_equal(p.E, q.E) and np.array_equal(p.beta, q.beta) and p.intercept == -1.0
    eta = np.full(kw["N"], -1.0)
    B = p.beta.reshape(len(p.shifts), kw["m"])
    for bi, sh in enumerate(p.shifts):
        r0 = p.L - 1 - sh
        eta += p.E[r0:r0 + kw["N"]].astype(np.float64) @ B[bi]
    assert np.array_equal(p.y, np.random.default_rng(kw["seed"] + 2).poisson(np.exp(eta))
                          .astype(np.float64))
