"""NB2 dispersion by maximum likelihood and the log-likelihood score without a GPU: the oracle of
tests/nb2ml_cases.py against scipy, finite differences and mpmath; the product's stop rule against
the exact alternation; the host surface (kappa='ml' parameters and refusals, score_method='ll'
refusals, GLM.log_likelihood, the host tail sums of sglm_hip.nb2) and the margin of the kappa
grid that the GPU score test uses."""
import math

import numpy as np
import pytest
import scipy.stats

import nb2_cases as nc
import nb2ml_cases as mc

LD = np.longdouble


def _case_a_eta():
    _, X, y = nc.case_a()
    w, b = nc.oracle("A", 1e-2, 0.25)
    return y, X @ w + b


# ------------------------------------------------------------------------------ likelihood forms
@pytest.mark.parametrize("kappa", [2.0 ** -16, 0.25, 8.0])
def test_tail_likelihood_equals_scipy(kappa):
    """-sum l_k + sum_j T[j] (log1p(k j) - ln(j + 1)) is the summed nbinom.logpmf.  Bound 1e-8
    relative: scipy's form adds lgamma(y + 1/k) - lgamma(1/k) and (1/k) log p, terms of size
    (1/k) ln(1/k) = 7e5 at k = 2^-16 that cancel to O(1) per row, so scipy itself carries about
    7e5 * 2^-53 * 3 = 2e-10 per row; the tail form has no such cancellation."""
    y, eta = _case_a_eta()
    ref = float(np.sum(mc.ll_nb2_rows(kappa, y, eta)))
    got = mc.ll_nb2_tail(kappa, y, eta)
    assert abs(got - ref) <= 1e-8 * abs(ref)
    m = np.random.default_rng(1).integers(0, 4, y.size)
    ref = float(np.sum(m * mc.ll_nb2_rows(kappa, y, eta)))
    assert abs(mc.ll_nb2_tail(kappa, y, eta, m) - ref) <= 1e-8 * abs(ref)


def test_poisson_tail_likelihood_equals_scipy():
    y, eta = _case_a_eta()
    ref = float(np.sum(mc.ll_poisson_rows(y, eta)))
    assert abs(mc.ll_poisson_tail(y, eta) - ref) <= 1e-12 * abs(ref)


def test_tail_is_the_count_of_larger_values():
    y = np.array([0, 3, 1, 3, 0, 7])
    m = np.array([1, 2, 0, 1, 3, 1])
    T = mc.tail(y, m)
    assert T.tolist() == [float(np.sum(m * (y > j))) for j in range(7)]


# ------------------------------------------------------------------------------ the score
@pytest.mark.parametrize("kappa", [2.0 ** -16, 0.25, 8.0])
def test_score_equals_central_difference(kappa):
    """Central difference of the longdouble tail likelihood with h = 1e-4 kappa: truncation
    h^2 |f'''| / 6 ~ 1e-8 relative, rounding 2^-64 |ll| / h far below.  Bound 1e-6 of the summed
    magnitudes of the score's terms."""
    y, eta = _case_a_eta()

    def ll(k):
        T = mc.tail(y).astype(LD)
        j = np.arange(T.size, dtype=LD)
        return mc.eta_sums(k, y, eta)[0][0] + (T * np.log1p(LD(k) * j)).sum()
    h = 1e-4 * kappa
    fd = (ll(kappa + h) - ll(kappa - h)) / (2 * LD(h))
    T = mc.tail(y)
    scale = float(np.sum(T * np.arange(T.size) / (1 + kappa * np.arange(T.size)))
                  + mc.eta_sums(kappa, y, eta)[1][1])
    assert abs(float(fd - mc.score(kappa, y, eta))) <= 1e-6 * scale


def test_mpmath_confirms_the_longdouble_score_at_the_poisson_end():
    """At kappa = 2^-20 on 400 rows of Case A: the longdouble cancellation-free score equals the
    50-digit digamma form to 1e-15 of the terms' magnitudes, where the float64 digamma form is
    off by orders more."""
    y, eta = _case_a_eta()
    y, eta = y[:400], eta[:400]
    k = 2.0 ** -20
    ref = mc.score_mp(k, y, eta)
    got = mc.score(k, y, eta)
    T = mc.tail(y)
    scale = float(np.sum(T * np.arange(T.size)) + mc.eta_sums(k, y, eta)[1][1])
    import mpmath
    hi = float(got)                                   # the longdouble value as two doubles
    err = abs(float(ref - (mpmath.mpf(hi) + mpmath.mpf(float(got - LD(hi))))))
    assert err <= 1e-15 * scale
    naive = abs(mc.score_digamma(k, y, eta) - float(got))
    assert naive > 100 * err


def test_profile_is_a_root_of_the_score():
    y, eta = _case_a_eta()
    k, at_bound = mc.kappa_profile(y, eta)
    assert not at_bound and abs(k - 0.5380) < 5e-4
    assert float(mc.score(k * (1 - 1e-9), y, eta)) > 0 > float(mc.score(k * (1 + 1e-9), y, eta))


# ------------------------------------------------------------------------------ the stop rule
@pytest.mark.parametrize("name", ["A0", "A2", "A1", "T", "L"])
def test_product_stop_rule_is_within_1e6_of_the_exact_alternation(name):
    ex, pr = mc.ml_oracle(name, True), mc.ml_oracle(name, False)
    assert ex["converged"] and pr["converged"] and not pr["at_bound"]
    assert pr["kappa"] == nc.k32(pr["kappa"]) and pr["rounds"] >= 2
    err = abs(math.log(pr["kappa"]) - math.log(ex["kappa"]))
    print(f"{name}: kappa {ex['kappa']:.9g}, product rule {pr['kappa']:.9g} after "
          f"{pr['rounds']} rounds, |d ln kappa| = {err:.3g}")
    assert err <= 1e-6


def test_poisson_counts_end_at_the_lower_bound():
    pr = mc.ml_oracle("P", False)
    assert pr["at_bound"] and pr["converged"] and pr["kappa"] == 2.0 ** -20


# ------------------------------------------------------------------------------ host surface
def test_ml_keeps_params_and_refuses_objective():
    from sglm_hip.estimators import NegativeBinomialRegressor, NotYetImplementedError
    import sglm
    ref = NegativeBinomialRegressor(kappa=1.0)
    m = NegativeBinomialRegressor(kappa="ml", alpha=0.5)
    assert set(m.get_params()) == set(ref.get_params())
    assert m.get_params()["kappa"] == "ml"
    with pytest.raises(NotYetImplementedError, match="score_method='ll'"):
        m.objective()
    g = sglm.GLM("NB2", kappa="ml", alpha=0.1)
    assert g.model.get_params()["kappa"] == "ml"
    with pytest.raises(NotYetImplementedError, match="kappa"):
        g.model.objective()
    with pytest.raises(AttributeError, match="kappa_"):
        m.score(np.zeros((3, 2)), np.zeros(3))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e50])
def test_numeric_kappa_is_validated_as_before(bad):
    from sglm_hip.estimators import NegativeBinomialRegressor
    with pytest.raises(ValueError, match="kappa"):
        NegativeBinomialRegressor(kappa=bad).objective()


@pytest.mark.parametrize("name,kw", [("Normal", {}), ("Gaussian", {"alpha": 1.0}), ("Gamma", {}),
                                     ("Tweedie", {"power": 1.5})])
def test_ll_score_refuses_other_families(name, kw):
    import sglm
    with pytest.raises(sglm.NotYetImplementedError, match=name):
        sglm.GLM(name, score_method="ll", **kw)


@pytest.mark.parametrize("name,kw", [("Poisson", {}), ("Tweedie", {"power": 1}), ("NB2", {}),
                                     ("NegativeBinomial", {"kappa": "ml"}), ("Binomial", {})])
def test_ll_score_accepts_the_count_families(name, kw):
    import sglm
    g = sglm.GLM(name, score_method="ll", **kw)
    assert g.score == g.ll_score


def test_run_multi_refuses_ll_on_normal_and_gamma_before_any_device_work():
    from sglm_hip import grid
    from sglm_hip.estimators import NotYetImplementedError, Ridge, TweedieRegressor
    X, y = np.zeros((8, 2)), np.ones(8)
    for est, name in ((Ridge(alpha=1.0), "Normal"), (TweedieRegressor(power=2.0), "Gamma")):
        with pytest.raises(NotYetImplementedError, match=name):
            grid.run(X, y, [(np.arange(4), np.arange(4, 8))], [est.objective()], [0],
                     score_method="ll")


def test_log_likelihood_equals_scipy():
    import sglm
    rng = np.random.default_rng(9)
    eta = rng.normal(0.4, 1.0, 500)
    mu = np.exp(eta)
    y = rng.poisson(mu * rng.gamma(2.0, 0.5, 500)).astype(np.float64)

    def close(a, b):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)
    close(sglm.GLM("Poisson").log_likelihood(mu, y), np.sum(scipy.stats.poisson.logpmf(y, mu)))
    for kappa in (0.25, 8.0):
        close(sglm.GLM("NB2", kappa=kappa).log_likelihood(mu, y),
              np.sum(scipy.stats.nbinom.logpmf(y, 1 / kappa, 1 / (1 + kappa * mu))))
    g = sglm.GLM("NegativeBinomial", kappa="ml")
    g.model.kappa_ = 0.5                              # as a fit leaves it
    close(g.log_likelihood(mu, y), np.sum(scipy.stats.nbinom.logpmf(y, 2.0, 1 / (1 + 0.5 * mu))))
    p = 1 / (1 + np.exp(-eta))
    yb = (rng.random(500) < p).astype(np.float64)
    close(sglm.GLM("Binomial").log_likelihood(p, yb), np.sum(scipy.stats.bernoulli.logpmf(yb, p)))
    # the Gaussian branch is what it was
    r = sglm.GLM("Normal").log_likelihood(eta, eta + 0.5 * rng.normal(size=500))
    assert np.isfinite(r)
    with pytest.raises(sglm.NotYetImplementedError):
        sglm.GLM("Gamma").log_likelihood(mu, y + 1)


def test_non_integer_counts_are_refused():
    import sglm
    from sglm_hip import nb2
    mu = np.ones(4)
    for y in ([0.0, 1.5, 2.0, 1.0], [0.0, -1.0, 2.0, 1.0], [0.0, np.nan, 2.0, 1.0]):
        with pytest.raises(ValueError, match="integer counts"):
            sglm.GLM("Poisson").log_likelihood(mu, np.array(y))
        with pytest.raises(ValueError, match="integer counts"):
            nb2.check_counts(y)
    with pytest.raises(sglm.NotYetImplementedError, match="2\\^20"):
        nb2.check_counts([0.0, 2.0 ** 20])


def test_host_tail_sums_match_the_oracle():
    from sglm_hip import engine as E, nb2
    y, eta = _case_a_eta()
    m = np.random.default_rng(2).integers(0, 3, y.size)
    T = nb2.tail_np(y, m)
    assert np.array_equal(T, mc.tail(y, m))
    for kappa in (2.0 ** -16, 0.25, 8.0):
        ref = float(np.sum(m * mc.ll_nb2_rows(kappa, y, eta)))
        got = -float(np.sum(m * nc.loss(kappa, y, eta))) + nb2.ll_const(T, E.FAM_NB2_LOG, kappa)
        assert abs(got - ref) <= 1e-8 * abs(ref)
        j = np.arange(T.size)
        s1, s2 = nb2.tail_score(T, kappa)
        assert abs(s1 - np.sum(T * j / (1 + kappa * j))) <= 1e-13 * s1
        h = 1e-6 * kappa
        fd = (nb2.tail_score(T, kappa + h)[0] - nb2.tail_score(T, kappa - h)[0]) / (2 * h)
        assert abs(s2 - fd) <= 1e-5 * abs(s2)
    assert nb2.ll_const(T, E.FAM_BINOMIAL_LOGIT) == 0.0
    ref = float(np.sum(m * mc.ll_poisson_rows(y, eta)))
    got = -float(np.sum(m * (np.exp(eta) - y * eta))) + nb2.ll_const(T, E.FAM_TWEEDIE_LOG)
    assert abs(got - ref) <= 1e-12 * abs(ref)
    assert nb2.moment_kappa(nb2.tail_np(y), float(y.size)) == pytest.approx(mc.moment_kappa(y),
                                                                          rel=1e-12)


# ------------------------------------------------------------------------------ grid margin
def test_kappa_grid_has_a_clear_winner():
    """The GPU 'll' grid test holds every score to 1e-6 relative and then asks for the oracle's
    best kappa: the oracle's best mean test log-likelihood beats the runner-up by at least
    100 x that bar, and Poisson scores below every NB2 value near the optimum."""
    means = {k: float(np.mean(mc.grid_oracle(k)[1])) for k in mc.GRID_KAPPAS}
    order = sorted(means, key=means.get, reverse=True)
    best, second = order[0], order[1]
    assert means[best] - means[second] >= 100 * 1e-6 * abs(means[best])
    assert best == 0.5
    assert float(np.mean(mc.grid_oracle(None)[1])) < means[best] - 100 * 1e-6 * abs(means[best])
