"""The oracles of tests/cd_cases.py held to something independent of them, the cases' own
claims (a fit that is all zero, a fit with zero and non-zero coefficients, no sweep count that
hangs on rounding), and the fits-per-workgroup table of sglm_enet_cd_fits_per_wg.  No GPU."""
import numpy as np
import pytest

import cd_cases as C


@pytest.mark.parametrize("p", [5, 40])
def test_converged_oracle_satisfies_kkt(p):
    Qs, fit_q, q, l1, l2 = C.cd_case(p)
    mixed = 0
    for m in range(Qs.shape[0]):
        sel = np.flatnonzero(fit_q == m)
        w, sweeps, _ = C.cd_oracle(Qs[m], q[sel], l1[sel], l2[sel], 20000, 1e-12)
        assert sweeps.max() < 20000
        for i, f in enumerate(sel):
            assert C.kkt_violation(Qs[m], q[f], l1[f], l2[f], w[i]) <= 1e-9, (p, f)
            if l1[f] > np.abs(q[f]).max():
                assert not w[i].any() and sweeps[i] == 1
            mixed += bool((w[i] == 0).any() and (w[i] != 0).any())
    assert mixed > 0


def test_cases_are_deterministic():
    for p in (7, 513):
        a = C.cd_case(p)
        C.cd_case.cache_clear()
        C.gram.cache_clear()
        b = C.cd_case(p)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for f in (C.center_case, C.gram_ss_case):
        a = f(33)
        f.cache_clear()
        b = f(33)
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("p,S", [(1, 3), (7, 1), (7, 3), (513, 1), (513, 3)])
def test_fixed_sweep_cases_exercise_the_threshold(p, S):
    """What the GPU tests rely on: a fit with l1 > max|q| is all zero after exactly one sweep,
    some fit has zero and non-zero coefficients, the dead column is exactly zero, and no sweep
    count hangs on rounding."""
    Qs, fit_q, q, l1, l2 = C.cd_case(p)
    w, sweeps, ratios = C.cd_reference(p, S)
    zero = l1 > np.abs(q).max(axis=1)
    assert zero.any() and not w[zero].any() and (sweeps[zero] == 1).all()
    dc = C.dead_column(p)
    if p == 1:
        # exact arithmetic: the second sweep moves nothing, in any precision
        assert (sweeps[~zero] == min(S, 2)).all()
        assert all(r in ([1.0], [1.0, 0.0]) for i, r in enumerate(ratios) if not zero[i])
        return
    assert Qs[0][dc, dc] == 0 and not w[:, dc].any()
    assert any((w[i] == 0).sum() > 1 and (w[i] != 0).any() for i in range(len(l1)))
    assert (sweeps[~zero] == S).all()
    for i in np.flatnonzero(~zero):
        assert len(ratios[i]) == S and min(ratios[i]) > 1e-6, (i, ratios[i])


def test_layouts():
    fit_q = C.cd_case(7)[1]
    rows, spare = C.fit_rows(len(fit_q))
    assert len(set(rows) | set(spare)) == len(fit_q) + 2
    for fpw, sparse, nwg in ((8, True, 11), (8, False, 3), (4, True, 11), (4, False, 6)):
        wg_fits, wg_q = C.layout(fit_q, rows, fpw, sparse)
        assert wg_fits.shape == (nwg, fpw)
        assert (np.diff(wg_q) < 0).any()                    # not sorted by workgroup
        named = wg_fits[wg_fits >= 0]
        assert sorted(named) == sorted(rows)
        for m in (0, 1):
            last = wg_fits[np.flatnonzero(wg_q == m)]
            assert (last[:, -1] == -1).any()                # a padded workgroup for each Q
        for k in range(nwg):
            own = wg_fits[k][wg_fits[k] >= 0]
            assert all(fit_q[list(rows).index(f)] == wg_q[k] for f in own)


def test_center_oracle_is_the_centred_gram():
    """Q of the oracle is X_c^T X_c of the design the counts came from (float64 rounding of a
    direct computation: 1e-10 of the diagonal)."""
    p = 37
    rng = np.random.default_rng(300 + p)
    X = np.ones((5000, p + 1))
    X[:, :p] = rng.random((5000, p)) < rng.uniform(0.02, 0.6, p)[None, :]
    H = C.center_case(p)
    Qr, bound = C.center_oracle(H, p, C.CG_GRAM_OF, 1)
    Xc = X[:, :p] - X[:, :p].mean(0)
    direct = Xc.T @ Xc
    assert np.abs(Qr[0].astype(np.float64) - direct).max() <= 1e-10 * direct.diagonal().max()
    assert np.array_equal(Qr[0], Qr[2]) and not Qr[1].any()          # slot 0: the empty mask
    assert bound.max() < 1e-11 and np.array_equal(Qr[0], Qr[0].T)
    Q0, _ = C.center_oracle(H, p, C.CG_GRAM_OF, 0)
    assert np.array_equal(Q0[0].astype(np.float64), (X.T @ X)[:p, :p])


def test_gram_ss_oracle_is_the_residual_sum():
    """yy - 2 beta.c + beta^T G beta with yy = |y|^2 and c = X^T y is |y - X beta|^2."""
    pa = 33
    H, grp_off, fits, beta, c, cidx, yy, w1 = C.gram_ss_case(pa)
    raw, bound = C.gram_ss_oracle(H, pa, grp_off, fits, beta, c, cidx, yy)
    assert raw[w1] == -1 and (np.delete(raw, w1) > 0).all()
    assert bound.max() < 1e-7
    rng = np.random.default_rng(500 + pa)
    X = np.ones((400, pa))
    X[:, :pa - 1] = rng.random((400, pa - 1)) < 0.2         # slot 0's design, as gram_ss_case
    y = np.random.default_rng(1).normal(size=400)
    g = int(np.flatnonzero(C.GS_SLOT == 0)[0])
    w = int(grp_off[g])
    c2 = np.zeros((C.GS_NC, C.GS_P))
    c2[cidx[w], :pa] = X.T @ y
    yy2 = yy.copy()
    yy2[w] = y @ y
    raw2, _ = C.gram_ss_oracle(H, pa, grp_off, fits, beta, c2, cidx, yy2)
    direct = np.sum((y - X @ beta[fits[w], :pa]) ** 2)
    assert abs(float(raw2[w]) - direct) <= 1e-11 * direct


def test_fits_per_workgroup_table(monkeypatch):
    from sglm_hip import _lib
    lib = _lib.load()
    monkeypatch.delenv("SGLM_CD_FPW", raising=False)
    for p, (unset, _) in C.FPW_TABLE.items():
        assert lib.sglm_enet_cd_fits_per_wg(p) == unset, p
    monkeypatch.setenv("SGLM_CD_FPW", "4")
    for p, (_, four) in C.FPW_TABLE.items():
        assert lib.sglm_enet_cd_fits_per_wg(p) == four, p
    # the table is (2 f + 1) * 8 p <= 160 KiB - 1 KiB past the register forms' p <= 2048:
    # f = 8 would need p <= 1196, so the eight-fit LDS form is never chosen
    for p in (2049, 2261, 2262, 4070, 4071):
        f = next((f for f in (8, 4, 2) if (2 * f + 1) * 8 * p <= 160 * 1024 - 1024), 1)
        assert f == C.FPW_TABLE[p][0] and f < 8
