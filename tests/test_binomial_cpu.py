"""The Binomial (logit link) family off the device: the float64 Newton oracle of
tests/binomial_cases.py against the sklearn golden, and the host surface -- GLM dispatch, the
objective, the 0/1 label check, the refusals, and synth's Bernoulli draws."""
import os

import numpy as np
import pytest

import binomial_cases as bc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binomial.npz")


def test_oracle_matches_sklearn_golden():
    """The damped-Newton oracle and LogisticRegression(newton-cholesky, tol 1e-12, C = 1 / (alpha
    N)) reach the same minimiser: coefficients and intercepts within 1e-8 absolute on cases A
    (every alpha) and S, and the scores recorded from the sklearn fit within 1e-8."""
    g = np.load(GOLDEN)
    assert tuple(g["A_alphas"]) == bc.ALPHAS_A
    _, X, y = bc.case_a()
    assert X.shape == (6000, 48) and set(np.unique(y)) == {0.0, 1.0}
    for j, a in enumerate(bc.ALPHAS_A):
        w, b = bc.oracle("A", a)
        err = max(np.max(np.abs(w - g[f"A{j}_coef"])), abs(b - float(g[f"A{j}_intercept"])))
        print(f"case A alpha {a:g}: oracle - sklearn {err:.2e}")
        assert err <= 1e-8, a
        eta = X @ w + b
        assert abs(bc.d2(y, eta) - float(g[f"A{j}_d2"])) <= 1e-8
        assert abs(bc.neg_mse(y, eta) - float(g[f"A{j}_neg_mse"])) <= 1e-8
    _, X, y = bc.case_s()
    assert X.shape == (4000, 48)
    w, b = bc.oracle("S", bc.ALPHA_S)
    err = max(np.max(np.abs(w - g["S_coef"])), abs(b - float(g["S_intercept"])))
    print(f"case S: oracle - sklearn {err:.2e}")
    assert err <= 1e-8
    eta = X @ w + b
    e = np.exp(-np.abs(eta))
    # the separable labels drive the weights towards zero
    assert np.max(np.abs(eta)) > 12 and np.min(e / (1 + e) ** 2) < 1e-5


def test_glm_binomial_dispatch_and_objective():
    import sglm
    import sglm_
    from sglm.models import sglm as models_sglm
    from sglm_hip import engine, estimators as est
    assert engine.FAM_BINOMIAL_LOGIT == 2
    glm = sglm.GLM("Binomial", alpha=.5)
    assert isinstance(glm.model, est.BinomialRegressor)
    o = glm.model.objective()
    assert (o.kind, o.family, o.lam_scale, o.l1_ratio) == ("irls", 2, "n", 0.0)
    assert o.lam(1000) == 500 and o.fit_intercept and o.max_iter == 100
    assert sglm.BinomialRegressor is est.BinomialRegressor is sglm_.BinomialRegressor
    assert models_sglm.BinomialRegressor is est.BinomialRegressor
    m = est.BinomialRegressor()
    assert m.get_params() == dict(alpha=1.0, fit_intercept=True, solver="lbfgs", max_iter=100,
                                  tol=1e-4, warm_start=False, verbose=0, l1_ratio=0.0)
    with pytest.raises(TypeError):
        est.BinomialRegressor(power=1)
    with pytest.raises(ValueError):
        est.BinomialRegressor(alpha=-1.0).objective()
    # alpha = 0 carries no L1 term whatever l1_ratio says (as TweedieRegressor)
    assert est.BinomialRegressor(alpha=0.0, l1_ratio=.5).objective().kind == "irls"
    # the sklearn LogisticRegression surface stays refused
    for name in ("Logistic", "Multinomial"):
        with pytest.raises(est.NotYetImplementedError):
            sglm.GLM(name)


def test_l1_ratio_is_refused():
    import sglm
    from sglm_hip import estimators as est
    with pytest.raises(est.NotYetImplementedError):
        sglm.GLM("Binomial", alpha=.1, l1_ratio=.5).model.objective()
    with pytest.raises(est.NotYetImplementedError):
        sglm.GLM("Binomial", alpha=.1, l1_ratio=.5).fit(np.zeros((4, 2)), np.array([0, 1, 0, 1.]))
    with pytest.raises(ValueError):
        est.BinomialRegressor(l1_ratio=1.5).objective()


@pytest.mark.parametrize("y", [np.array([0, 1, 2, 0]), np.array([0.0, 0.5, 1.0, 1.0]),
                               np.array([0.0, 1.0, np.nan, 1.0]), np.array([-1, 0, 1, 1])])
def test_labels_outside_01_raise_on_the_host(y):
    """Checked before any device work: no GPU is needed to be refused."""
    import sglm
    from sglm_hip import estimators as est, grid
    X = np.zeros((4, 2))
    with pytest.raises(ValueError, match="Binomial responses must be 0 or 1"):
        sglm.GLM("Binomial", alpha=.1).fit(X, y)
    obj = est.BinomialRegressor(alpha=.1).objective()
    with pytest.raises(ValueError, match="Binomial responses must be 0 or 1"):
        grid.run(X, y, [(np.array([0, 1]), np.array([2, 3]))], [obj], [0])
    with pytest.raises(ValueError, match="Binomial responses must be 0 or 1"):
        est.BinomialRegressor().score(X, y)


def test_label_dtypes_are_accepted():
    from sglm_hip import estimators as est
    for y in (np.array([True, False, True]), np.array([1, 0, 1], dtype=np.int8),
              np.array([1.0, 0.0, 1.0], dtype=np.float32), [1, 0, 1]):
        out = est.check_binomial_y(y)
        assert out.dtype == np.float64 and out.tolist() == [1.0, 0.0, 1.0]


def test_host_loss_helpers():
    """sigmoid / loss helpers of the estimators: overflow-free and equal to the cases' own."""
    from sglm_hip import estimators as est
    eta = np.array([-800.0, -30.0, -1.0, -0.0, 0.0, 2.5, 40.0, 800.0])
    y = np.array([0, 1, 0, 1, 0, 1, 0, 1.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        mu = est.sigmoid_np(eta)
        l = est.binomial_loss_np(y, eta)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(l)) and mu[0] == 0 and mu[-1] == 1
    assert np.array_equal(mu, bc.sigmoid(eta)) and np.array_equal(l, bc.loss(y, eta))
    assert abs(mu[2] - 1 / (1 + np.e)) < 1e-16
    yy = np.array([0, 0, 1, 1, 1.0])
    assert abs(est.binomial_null_np(5.0, 0.6) - bc.null_deviance(yy)) < 1e-14
    assert abs(bc.null_deviance(yy) - bc.deviance(yy, np.full(5, np.log(0.6 / 0.4)))) < 1e-13
    assert est.binomial_null_np(5.0, 1.0) == 0.0


def test_synth_binomial_and_other_families_unchanged():
    from sglm_hip import synth
    kw = dict(N=3000, m=5, L=3, rho=0.05, seed=9, beta_scale=0.4)
    s = synth.make(family="binomial", intercept=-0.3, **kw)
    assert set(np.unique(s.y)) == {0.0, 1.0} and s.family == "binomial"
    assert 0.2 < s.y.mean() < 0.6
    # the draws are one uniform per row of rng(seed + 2) against sigma(eta)
    def eta_of(b):                        # the predictor as synth.make accumulates it
        eta = np.full(kw["N"], b, dtype=np.float64)
        B = s.beta.reshape(len(s.shifts), kw["m"])
        for bi, sh in enumerate(s.shifts):
            r0 = s.L - 1 - sh
            eta += s.E[r0:r0 + kw["N"]].astype(np.float64) @ B[bi]
        return eta
    u = np.random.default_rng(kw["seed"] + 2).random(kw["N"])
    assert np.array_equal(s.y, (u < 1.0 / (1.0 + np.exp(-eta_of(-0.3)))).astype(np.float64))
    # the other families for the same seed: the same events and coefficients, and the draws
    # their own branches made before the Binomial one existed
    p = synth.make(family="poisson", **kw)
    g = synth.make(family="gamma", **kw)
    z = synth.make(family="gaussian", **kw)
    assert np.array_equal(p.E, s.E) and np.array_equal(p.beta, s.beta)
    assert (p.intercept, g.intercept, z.intercept) == (-1.0, 0.5, 0.5)
    rng2 = np.random.default_rng(kw["seed"] + 2)
    assert np.array_equal(p.y, rng2.poisson(np.exp(eta_of(-1.0))).astype(np.float64))
    rng2 = np.random.default_rng(kw["seed"] + 2)
    assert np.array_equal(g.y, rng2.gamma(2.0, np.exp(eta_of(0.5)) / 2.0))
    rng2 = np.random.default_rng(kw["seed"] + 2)
    assert np.array_equal(z.y, eta_of(0.5) + rng2.normal(0.0, 1.0, kw["N"]))
