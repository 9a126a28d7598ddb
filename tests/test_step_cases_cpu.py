"""The oracles and cases of tests/step_cases.py held to independent statements of the same
operations, and the cases' own claims: every branch of the Anderson accept rule is taken with a
clear margin, every outcome of the Newton decisions occurs.  No GPU."""
import numpy as np
import pytest

import step_cases as C


@pytest.mark.parametrize("power", C.MS_POWERS)
def test_mask_stats_oracle(power):
    """against a weighted np.bincount-style statement in float64 on the repeated rows"""
    n = 255
    M, Y, K = C.mask_stats_case(n, power >= 2)
    ref, mag = C.mask_stats_oracle(M, Y, K, n, power)
    assert (M[:, n:] == 1).all() and set(np.unique(M[1, :n])) == {0, 2, 3}
    assert ref[0, 2, 0] == 0 and np.isposinf(ref[0, 2, 4]) and not ref[:, 2, 1:4].any()
    assert ref[1, 3, 0] == 1 and ref[1, 3, 4] == Y[1, n - 1]
    for r in range(2):
        for f in (0, 1):
            rows = np.repeat(np.arange(n), M[f, :n])       # a row of multiplicity m, m times
            y = Y[r, rows]
            assert ref[r, f, 0] == rows.size and ref[r, f, 4] == y.min()
            assert abs(float(ref[r, f, 1]) - np.sum(y - K[r])) <= 1e-12 * float(mag[r, f, 0])
            assert abs(float(ref[r, f, 2]) - np.sum((y - K[r]) ** 2)) <= 1e-12 * float(mag[r, f, 1])
            if power < 0:
                assert ref[r, f, 3] == 0
            elif power == 1:
                c = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0)), 0.0) - y
                assert abs(float(ref[r, f, 3]) - c.sum()) <= 1e-12 * float(mag[r, f, 2])
            elif power == 3:
                assert abs(float(ref[r, f, 3]) - np.sum(0.5 / y)) <= 1e-12 * float(mag[r, f, 2])
    if power < 2:
        assert (Y[1] == 0).any() and (Y[1] >= 0).all()
    else:
        assert (Y > 0).all()


def test_eta_axpy_oracle():
    for n in C.EA_N[:2]:
        ld, eta, deta, M = C.eta_axpy_case(n)
        e64, bound, dmax = C.eta_axpy_oracle(n, eta, deta, M)
        assert ld > n and np.isnan(deta[:, n:]).all()
        assert np.array_equal(e64[1], eta[1, :n].astype(np.float64)) and dmax[1] == 0
        for k in (0, 2):
            best = max((abs(np.float32(C.EA_STEP[k] * deta[k, i])) for i in range(n)
                        if M[C.EA_FIT_MASK[k], i]), default=0)
            assert dmax[k] == np.float32(best)
            if n > 1:                                       # the largest step is off the mask
                assert dmax[k] < np.abs(C.EA_STEP[k] * deta[k, :n]).max()


def _aa_kernel_f32(P, q, delta, raw, used, gam):
    """the kernel's element arithmetic in numpy float32, no contraction"""
    k = C.AA_SLOTS[q]
    f = delta[k]
    df = f - raw[k]
    db = used[k] * C.AA_TPREV[q]
    return f - np.float32(gam) * (db + df)


@pytest.mark.parametrize("P,p", C.AA_SHAPES)
def test_aa_cases_take_every_branch_with_margin(P, p):
    delta, raw, used, gtot, rm = C.aa_case(P, p)
    o = C.aa_oracle(P, p, delta, raw, used, gtot)
    names = set(range(C.AA_NSLOT)) - set(C.AA_SLOTS)
    assert names == {1, 4, 6} and all(np.isnan(delta[k]).all() for k in names)
    acc, ghi, glo, same, up, off = o
    assert [x["good"] for x in o] == [True, False, False, False, False, False]
    for x in o:
        assert min(abs(x["gamma"] + 2), abs(x["gamma"] - 0.5)) >= 0.1
        assert abs(x["gd"]) >= 1e-3 * x["gd_abs"]
        assert x["den"] >= 1e-6 * x["ff"] or x["den"] == 0.0
    assert -1.9 <= acc["gamma"] <= 0.4 and acc["gd"] < 0
    assert ghi["gamma"] > 0.6 and ghi["gd"] < 0             # only the gamma clause rejects it
    assert glo["gamma"] < -2.1 and glo["gd"] < 0
    assert same["den"] == 0.0 and same["gd"] < 0
    assert np.array_equal(raw[C.AA_SLOTS[3]], delta[C.AA_SLOTS[3]])
    assert up["gd"] > 0 and up["gamma"] == acc["gamma"]
    assert off["gd"] < 0 and -1.9 <= off["gamma"] <= 0.4    # would be accepted if selected
    # the bound covers a float32 evaluation of the same expressions with the float64 gamma
    got = _aa_kernel_f32(P, 0, delta, raw, used, acc["gamma"]).astype(np.float64)
    assert (np.abs(got - acc["dnew"]) <= acc["bound"]).all()
    # the definition against the torch-style expressions of the engine, in float64
    k = C.AA_SLOTS[0]
    f, r, u = (a[k].astype(np.float64) for a in (delta, raw, used))
    df = f - r
    gam = (df * f).sum() / max((df * df).sum(), 1e-30)
    assert np.allclose(acc["dnew"], f - gam * (u * 1.0 + df), rtol=0, atol=1e-14)
    assert acc["rm"] == (np.abs(delta[k][:p]).max(), abs(delta[k][p])) and off["rm"] == (0.0, 0.0)


def _outcomes(o):
    f = o["flags"]
    hit = (f & 1) != 0
    return {
        "hit1": int((hit & (o["tix"] == 1)).sum()), "hit2": int((hit & (o["tix"] == 2)).sum()),
        "hit3": int((hit & (o["tix"] == 3)).sum()), "hit4": int((hit & (o["tix"] == 4)).sum()),
        "nohit": int((f == (256 | 512)).sum()),
        "flat": int(o["by_flat"].sum()),
        "tol": int(((f & (16 | 4 | 2)) == (16 | 4 | 2)).sum()),
        "stag": int(((f & (32 | 2 | 16)) == (32 | 2)).sum()),
        "ooi": int(((f & 8) != 0).sum()),
        "cont": int((f == (1 | 512)).sum()),
    }


@pytest.mark.parametrize("legacy", [0, 1])
@pytest.mark.parametrize("nts", [5, 12])
@pytest.mark.parametrize("na", [1024, 1025, 2050])
def test_decide_cases_reach_every_outcome(na, nts, legacy):
    act, L, sc, aa_rm, prev_rel, fresh, n_iter, max_iter, kind = C.decide_case(na, nts)
    assert len(set(act)) == na and act.max() < C.SD_NSLOT and (np.diff(act) < 0).any()
    ts = C.decide_ts(nts)
    assert ts.size == nts and np.array_equal(np.frexp(ts[1:])[0], np.full(nts - 1, 0.5))
    seen = {}
    for rm in (None, aa_rm):
        o = C.decide_oracle(act, L, sc, nts, ts, C.SD_SIGMA, C.SD_TOL, C.SD_SFLOOR, legacy, rm,
                            prev_rel, fresh, n_iter, max_iter)
        out = _outcomes(o)
        assert all(v > 0 for v in out.values()), out
        assert o["cnt"] == out["cont"] + out["nohit"] == len(o["nxt"])
        assert o["cnt"] > 0 and (o["rpos"] >= 0).sum() == o["cnt"]
        if na > 1024:                                       # rows past the first chunk of 1024
            assert (o["rpos"][1024:] >= 0).any() and (o["flags"][:1024] & 512).any()
        seen[rm is None] = o
    # the secant's raw steps change verdicts (and so the rows), through the slot act[q]
    assert not np.array_equal(seen[True]["flags"], seen[False]["flags"])
    assert seen[True]["cnt"] != seen[False]["cnt"]


def test_decide_oracle_by_hand():
    """three fits worked by hand: a full step that goes on, a half step within tol, no hit"""
    nts = 5
    ts = C.decide_ts(nts)
    act = np.array([4, 2, 9], dtype=np.int32)
    L = np.array([[10.0, 9.0, 0, 0, 0], [10.0, 11.0, 9.9, 0, 0], [10.0, 11, 11, 11, 11]])
    sc = np.zeros((3, 11))
    sc[:, 0] = -1.0                                          # g.d
    sc[:, 4] = (0.5, 1e-7, 0.5)                              # max|d|
    sc[:, 5:10] = 2.0                                        # max|w + t d|
    sc[:, 10] = (0.125, 0.0, 0.0)                            # |d_intercept|
    o = C.decide_oracle(act, L, sc, nts, ts, 2.0 ** -11, 3e-6, 0.1, 0, None,
                        np.ones(3), np.ones(3, np.uint8), np.zeros(3, np.int32),
                        np.full(3, 100, np.int32))
    assert o["step64"].tolist() == [1.0, 0.5, 0.0] and o["tix"].tolist() == [1, 2, 0]
    assert o["prop"].tolist() == [0.25, 5e-8, 0.0] and o["relv"].tolist() == [0.25, 2.5e-8, 0.0]
    assert o["flags"].tolist() == [1 | 512, 1 | 16 | 4 | 2, 256 | 512]
    assert o["rpos"].tolist() == [0, -1, 1] and o["nxt"].tolist() == [4, 9] and o["cnt"] == 2
    leg = C.decide_oracle(act, L, sc, nts, ts, 2.0 ** -11, 3e-6, 0.1, 1, None,
                          np.ones(3), np.ones(3, np.uint8), np.zeros(3, np.int32),
                          np.full(3, 1, np.int32))
    assert leg["prop"].tolist() == [0.5 / 3.0, 1e-7 / 3.0, 0.0]
    assert leg["flags"].tolist() == [1 | 8, 1 | 16 | 4 | 2, 256 | 512]
