"""The entry points of csrc/predict.hip through the C ABI against the np.longdouble oracle of
tests/predict_cases.py, on random symmetric positive definite C and random beta in float64.

Shapes: n = 1000 and 4099 (past every multiple of 32, 64 and the 1024-row group tile), P = 64
(one word per row), 256 and 512, row density 0.06 and 0.5, the edge rows of
predict_cases.kernel_design (all zeros, all ones, only the last real column, only the first),
B = 1 and 3 fits, groups of 1, 21 and 64 columns and one of 65 (NaN).

Every output is held to its own rounding bound (predict_cases' docstring) as a ratio <= 1, which
each test prints; rows without a bit in a group are exact zeros; a repeated call, a fit alone
or in a batch and a row list give the same bits; the intercept adds exactly its own terms.  The
planes carry set bits in the padding columns and the ones column, the arrays NaN at the padding
coordinates (and at the intercept's for a fit without one): none of them may reach a result."""
from functools import lru_cache

import numpy as np
import pytest

import infer_cases as C
import predict_cases as PC
import test_gpu_infer_kernels as IK

pytestmark = pytest.mark.gpu
SENT = -7.25
bits, dev, ptr = IK.bits, IK.dev, IK.ptr

# name: (n, p, P, density, icpt flag per fit)
CASES = {
    "n1000_P64_d50_B3": (1000, 63, 64, 0.5, (1, 0, 1)),
    "n4099_P256_d06_B1": (4099, 255, 256, 0.06, (1,)),
    "n1000_P512_d50_B1": (1000, 500, 512, 0.5, (1,)),
    "n4099_P512_d06_B3": (4099, 510, 512, 0.06, (1, 0, 1)),
}


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def group_ids(p):
    """Groups of 1, 21, 64 and 65 columns and the rest (p >= 152), else 1, 21 and the rest;
    interleaved, so that a group's columns are not consecutive."""
    sizes = [1, 21, 64, 65] if p >= 152 else [1, 21]
    ids = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)]
                         + [np.full(p - sum(sizes), len(sizes))])
    return np.random.default_rng(p).permutation(ids)


@lru_cache(maxsize=None)
def case(name):
    n, p, P, density, icpt = CASES[name]
    rng = np.random.default_rng([3101, n, P])
    B = len(icpt)
    X = PC.kernel_design(rng, n, p, density)
    ldim = (n + 63) // 64 * 64
    planes = np.ones((n, P))                 # the ones column and set bits in every padding column
    planes[:, :p] = X
    rb = PC.pack_rbits(planes, ldim, P)
    rb[:, n:] = 0xFFFFFFFF                   # rows >= n: never evaluated
    rb = rb.view(np.int32)
    beta = np.full((B, P), np.nan)
    cov = np.full((B, P, P), np.nan)
    for f in range(B):
        k = p + 1 if icpt[f] else p
        if f == 1:                           # fit 1 = fit 0 without its intercept
            beta[1, :p], cov[1, :p, :p] = beta[0, :p], cov[0, :p, :p]
            continue
        beta[f, :k] = rng.normal(0, 1, k)
        cov[f, :k, :k] = PC.spd(rng, k, 0.5 + f)
    state = np.zeros((B, P), np.uint8)
    state[:, p + 1:] = C.EXCL
    for f in range(B):
        if not icpt[f]:
            state[f, p] = C.EXCL
    Xt = np.hstack([X, np.ones((n, 1))])
    ref = []
    for f in range(B):
        cols = np.arange(p + 1 if icpt[f] else p)
        ref.append(PC.traces_rows(Xt, np.nan_to_num(beta[f, :p + 1]),
                                  np.nan_to_num(cov[f, :p + 1, :p + 1]), cols))
    for a in (X, Xt, rb, beta, cov, state):
        a.setflags(write=False)
    return dict(n=n, p=p, P=P, ld=ldim, icpt=np.array(icpt, np.int32), X=X, Xt=Xt, rb=rb,
                beta=beta, cov=cov, state=state, ref=ref)


def run_rows(torch, c, fits=None, rows=None, state=None):
    from sglm_hip import _lib
    fits = list(range(len(c["icpt"]))) if fits is None else list(fits)
    B = len(fits)
    nr = c["n"] if rows is None else len(rows)
    st = c["state"] if state is None else state
    d = [dev(torch, a) for a in (c["rb"], None if rows is None else np.asarray(rows, np.int32),
                                 c["beta"][fits], c["cov"][fits], st[fits], c["icpt"][fits])]
    out = torch.full((2, B + 1, nr), SENT, dtype=torch.float64, device="cuda")
    _lib.call("sglm_predict_rows", ptr(d[0]), c["ld"], c["P"], c["p"], c["n"], ptr(d[1]), nr,
              ptr(d[2]), ptr(d[3]), ptr(d[4]), ptr(d[5]), B, ptr(out[0]), ptr(out[1]), 0)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, B] == SENT)
    return o[0, :B], o[1, :B]


def run_groups(torch, c, ids, fits=None, rows=None, state=None):
    from sglm_hip import _lib
    fits = list(range(len(c["icpt"]))) if fits is None else list(fits)
    B = len(fits)
    u, goff, gcols = C.csr(ids)
    ng = len(u)
    nr = c["n"] if rows is None else len(rows)
    st = c["state"] if state is None else state
    d = [dev(torch, a) for a in (c["rb"], None if rows is None else np.asarray(rows, np.int32),
                                 c["beta"][fits], c["cov"][fits], st[fits], goff, gcols)]
    out = torch.full((2, B + 1, ng, nr), SENT, dtype=torch.float64, device="cuda")
    _lib.call("sglm_predict_groups", ptr(d[0]), c["ld"], c["P"], c["p"], c["n"], ptr(d[1]), nr,
              ptr(d[2]), ptr(d[3]), ptr(d[4]), B, ptr(d[5]), ptr(d[6]), ng, ptr(out[0]),
              ptr(out[1]), 0)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, B] == SENT)
    return o[0, :B], o[1, :B]


@pytest.mark.parametrize("name", list(CASES))
def test_predict_rows(engine, torch_mod, name):
    c = case(name)
    n, p, B = c["n"], c["p"], len(c["icpt"])
    eta, var = run_rows(torch_mod, c)
    eta2, var2 = run_rows(torch_mod, c)
    assert np.array_equal(bits(eta), bits(eta2)) and np.array_equal(bits(var), bits(var2))
    assert np.all(np.isfinite(eta)) and np.all(np.isfinite(var))
    we = wv = 0.0
    for f in range(B):
        r_eta, r_v, eb, vb = c["ref"][f]
        we = max(we, PC.ratio(PC.ld(eta[f]) - r_eta, eb))
        wv = max(wv, PC.ratio(PC.ld(var[f]) - r_v, vb))
        if not c["icpt"][f]:
            assert eta[f, 0] == 0.0 and var[f, 0] == 0.0        # the all-zero row, exactly
        # alone: the same bits as in the batch
        e1, v1 = run_rows(torch_mod, c, fits=[f])
        assert np.array_equal(bits(e1[0]), bits(eta[f])) and np.array_equal(bits(v1[0]), bits(var[f]))
    print(f"WORST predict_rows {name}: eta {we:.3e} var {wv:.3e} (ratio to the rounding bound)")
    assert we <= 1.0 and wv <= 1.0
    # a row list, unsorted and with a repeat, in another launch geometry: the full call's rows
    rows = [5, 5, 3, n - 1]
    er, vr = run_rows(torch_mod, c, rows=rows)
    assert np.array_equal(bits(er), bits(eta[:, rows])) and np.array_equal(bits(vr), bits(var[:, rows]))
    if B == 3:
        # fit 1 is fit 0 without the intercept: they differ by the intercept's own terms
        Xt, b0, c0 = c["Xt"], c["beta"][0], c["cov"][0]
        S = Xt[:, :p]
        d_eta = PC.ld(eta[0]) - PC.ld(eta[1]) - PC.LD(b0[p])
        d_var = PC.ld(var[0]) - PC.ld(var[1]) - (PC.LD(c0[p, p]) + 2 * (PC.ld(S) @ PC.ld(c0[:p, p])))
        ri = max(PC.ratio(d_eta, c["ref"][0][2] + c["ref"][1][2]),
                 PC.ratio(d_var, c["ref"][0][3] + c["ref"][1][3]))
        print(f"WORST predict_rows {name}: intercept terms {ri:.3e}")
        assert ri <= 1.0
        assert eta[0, 0] == b0[p] and var[0, 0] == c0[p, p]     # the all-zero row: exactly them


def test_predict_rows_nan_and_validation(engine, torch_mod):
    from sglm_hip import _lib
    c = case("n1000_P64_d50_B3")
    n, p = c["n"], c["p"]
    st = c["state"].copy()
    st[0, 7] = C.ZERO                                   # a coordinate infer reports as NaN
    eta, var = run_rows(torch_mod, c, state=st)
    e0, v0 = run_rows(torch_mod, c)
    has = c["X"][:, 7] != 0
    assert has.any() and (~has).any()
    assert np.all(np.isnan(var[0, has])) and np.array_equal(bits(var[0, ~has]), bits(v0[0, ~has]))
    assert np.array_equal(bits(var[1:]), bits(v0[1:])) and np.array_equal(bits(eta), bits(e0))
    for rows in ([0, n], [-1, 2]):                      # refused on the host, before the launch
        with pytest.raises(_lib.HipEngineError, match="outside"):
            run_rows(torch_mod, c, rows=rows)
    with pytest.raises(_lib.HipEngineError, match="bad args"):
        _lib.call("sglm_predict_rows", None, c["ld"], c["P"], p, n, None, n, None, None, None,
                  None, 1, None, None, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_predict_groups(engine, torch_mod, name):
    c = case(name)
    n, p, B = c["n"], c["p"], len(c["icpt"])
    ids = group_ids(p)
    u, goff, gcols = C.csr(ids)
    sizes = np.diff(goff)
    ge, gv = run_groups(torch_mod, c, ids)
    ge2, gv2 = run_groups(torch_mod, c, ids)
    assert np.array_equal(bits(ge), bits(ge2)) and np.array_equal(bits(gv), bits(gv2))
    we = wv = 0.0
    total = np.zeros((B, n), PC.LD)
    for f in range(B):
        for g in range(len(u)):
            cols = gcols[goff[g]:goff[g + 1]]
            if sizes[g] > 64:
                assert np.all(np.isnan(ge[f, g])) and np.all(np.isnan(gv[f, g]))
                continue
            r_eta, r_v, eb, vb = PC.traces_rows(c["X"], c["beta"][f, :p], c["cov"][f, :p, :p], cols)
            we = max(we, PC.ratio(PC.ld(ge[f, g]) - r_eta, eb))
            wv = max(wv, PC.ratio(PC.ld(gv[f, g]) - r_v, vb))
            empty = ~c["X"][:, cols].any(axis=1)
            assert empty.any() or sizes[g] > 21
            assert np.all(bits(ge[f, g, empty]) == 0) and np.all(bits(gv[f, g, empty]) == 0)
            total[f] += PC.ld(ge[f, g])
        one_e, one_v = run_groups(torch_mod, c, ids, fits=[f])
        assert np.array_equal(bits(one_e[0]), bits(ge[f])) and np.array_equal(bits(one_v[0]), bits(gv[f]))
    print(f"WORST predict_groups {name}: eta {we:.3e} var {wv:.3e} (ratio to the rounding bound)")
    assert we <= 1.0 and wv <= 1.0
    assert np.any(sizes == 1) and np.any(sizes == 21) and (p < 152 or {64, 65} <= set(sizes))
    rows = [5, 5, 3, n - 1]
    er, vr = run_groups(torch_mod, c, ids, rows=rows)
    assert np.array_equal(bits(er), bits(ge[:, :, rows])) and np.array_equal(bits(vr), bits(gv[:, :, rows]))
    if p < 152:
        # the groups cover every column: their predictors add up to the trace without intercept
        eta, _ = run_rows(torch_mod, c)
        f = 1
        assert PC.ratio(total[f] - PC.ld(eta[f]), 2 * c["ref"][f][2] + 3 * PC.U53 * np.abs(eta[f])) <= 1.0
    # a coordinate that is not kept: NaN where the row has its bit, in its group alone
    st = c["state"].copy()
    col = int(gcols[goff[1]])
    st[0, col] = C.ZERO
    _, gn = run_groups(torch_mod, c, ids, state=st)
    has = c["X"][:, col] != 0
    assert np.all(np.isnan(gn[0, 1, has])) and np.array_equal(bits(gn[0, 1, ~has]), bits(gv[0, 1, ~has]))
    keep = np.ones(len(u), bool)
    keep[1] = False
    assert np.array_equal(bits(gn[0, keep]), bits(gv[0, keep]), ) and np.array_equal(bits(gn[1:]), bits(gv[1:]))
