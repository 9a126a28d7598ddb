"""The full-step link inside the trial-loss pass (sglm_loss_trials_link, engine.STEP_LINK):
the kernel against sglm_loss_trials_max followed by sglm_link_update_rp at step 1, bitwise, and
small Poisson grids solved with the switch on (1: the link inside the trial-loss pass, 2: the
link alone behind the read-back) and off, where every fit takes full steps and where the first
Newton step overshoots and the fits are put back from the undo copy."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192                      # rows per block partial (csrc/api.hip, kRowChunk)
N = 40002                         # not a multiple of 4; five row chunks
SLOTS = np.array([3, 11, 0, 7, 8], dtype=np.int32)
TV1 = np.array([0.0, 1.0, 0.5, 0.25, 0.125], dtype=np.float32)
FAMILIES = [(1, 1.0), (1, 2.0), (0, 0.0)]
BP = 32


def pad256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


@pytest.fixture(scope="module")
def inp(torch_mod):
    """One batch of 12 fit rows on the device: two responses from a lag design's Poisson counts
    and four masks -- 0.8 density whose zero rows include whole aligned 4-row blocks (one of them
    across a chunk end), every row, no row, and multiplicities 0 / 1 / 2 -- each used by a fit
    of SLOTS."""
    from sglm_hip import synth
    s = synth.make(N=N, m=12, L=4, rho=0.08, seed=71)
    n = int(s.N)
    assert n == N and n % 4 and (n + CHUNK - 1) // CHUNK == 5
    ld, B = pad256(n), 12
    rng = np.random.default_rng(73)
    Y = np.zeros((2, ld), np.float32)
    Y[0, :n] = s.y
    Y[1, :n] = np.roll(s.y, 7)
    M = np.zeros((4, ld), np.uint8)
    m0 = (rng.random(n) < 0.8).astype(np.uint8)
    for i0 in (0, 400, 2 * CHUNK - 8, 3 * CHUNK, n - n % 4 - 24):
        m0[i0:i0 + 16] = 0                     # aligned blocks of four rows, all zero
    M[0, :n] = m0
    M[1, :n] = 1
    M[3, :n] = rng.integers(0, 3, n)
    fr = rng.integers(0, 2, B).astype(np.int32)
    fm = rng.integers(0, 4, B).astype(np.int32)
    fm[SLOTS] = [0, 1, 2, 3, 0]
    eta = np.zeros((B, ld), np.float32)
    eta[:, :n] = rng.normal(-1.0, 0.5, (B, n))
    deta = np.zeros((B, ld), np.float32)
    deta[:, :n] = rng.normal(0, 0.1, (B, n))
    h = dict(n=n, ld=ld, B=B, Y=Y, M=M, fr=fr, fm=fm, eta=eta, deta=deta)
    return {k: (torch_mod.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v)
            for k, v in h.items()}


def bits(t):
    """Integer view of a tensor (bitwise comparisons that also hold for NaN fill values)."""
    import torch
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("fam,power", FAMILIES)
def test_kernel_matches_trials_then_link(engine, torch_mod, inp, fam, power):
    """out, dmax, eta and the three packed R planes (their zero rows included) are bitwise what
    sglm_loss_trials_max followed by sglm_link_update_rp (step 1, positions 0..) leave on copies
    of the same inputs; undo is the eta that went in; unlisted slots and unlisted packed rows
    are untouched.  Poisson takes the halving branch, the others the general one (T = 5)."""
    torch = torch_mod
    from sglm_hip import _lib
    dv = inp
    n, ld, B = dv["n"], dv["ld"], dv["B"]
    ns = len(SLOTS)
    sl = torch.from_numpy(SLOTS).cuda()
    tv = torch.from_numpy(TV1).cuda()
    nan = float("nan")

    def bufs():
        return dict(e=dv["eta"].clone(),
                    out=torch.full((ns * 5,), nan, dtype=torch.float64, device="cuda"),
                    dm=torch.full((ns,), nan, dtype=torch.float32, device="cuda"),
                    Rp=torch.full((3 * BP * ld,), nan, dtype=torch.bfloat16, device="cuda"),
                    wk=torch.empty(_lib.query("sglm_rowsum_work_bytes", ns, 8, n),
                                   dtype=torch.uint8, device="cuda"))
    common = (dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr())
    a = bufs()
    _lib.call("sglm_loss_trials_max", fam, power, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, tv.data_ptr(), 5, a["out"].data_ptr(),
              a["dm"].data_ptr(), a["wk"].data_ptr(), 0)
    one = torch.ones(ns, dtype=torch.float32, device="cuda")
    rpos = torch.arange(ns, dtype=torch.int32, device="cuda")
    _lib.call("sglm_link_update_rp", fam, power, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              *common, None, None, a["Rp"].data_ptr(), BP, rpos.data_ptr(), one.data_ptr(),
              dv["deta"].data_ptr(), 0)
    b = bufs()
    undo = torch.full((ns, ld), nan, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_link", fam, power, n, ld, ns, sl.data_ptr(), b["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, tv.data_ptr(), 5, b["out"].data_ptr(),
              b["dm"].data_ptr(), undo.data_ptr(), b["Rp"].data_ptr(), BP, b["wk"].data_ptr(), 0)
    torch.cuda.synchronize()
    # the link alone (out = dmax = NULL: the sums taken by sglm_loss_trials_max before it)
    c = bufs()
    undo2 = torch.full((ns, ld), nan, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_link", fam, power, n, ld, ns, sl.data_ptr(), c["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, None, 0, None, None, undo2.data_ptr(),
              c["Rp"].data_ptr(), BP, None, 0)
    torch.cuda.synchronize()
    assert torch.equal(bits(c["e"]), bits(a["e"])) and torch.equal(bits(c["Rp"]), bits(a["Rp"]))
    assert torch.equal(bits(undo2), bits(undo)) and bool(torch.isnan(c["out"]).all())
    assert torch.equal(bits(b["out"]), bits(a["out"]))
    assert torch.equal(bits(b["dm"]), bits(a["dm"]))
    assert torch.isfinite(b["out"]).all() and float(b["dm"].max()) > 0
    assert torch.equal(bits(b["e"]), bits(a["e"]))
    assert torch.equal(bits(b["Rp"]), bits(a["Rp"]))
    assert torch.equal(bits(undo[:, :n]), bits(dv["eta"][sl.long(), :n]))
    # the predictor moved on every row of a listed fit, the masked-out ones too (slot 0's mask
    # is empty), and nowhere else
    listed = np.zeros(B, dtype=bool)
    listed[SLOTS] = True
    for k in range(B):
        same = torch.equal(bits(b["e"][k]), bits(dv["eta"][k]))
        assert same != listed[k], k
    assert torch.equal(b["e"][0, :n], dv["eta"][0, :n] + dv["deta"][0, :n])
    planes = b["Rp"].view(3, BP, ld)
    assert bool((planes[:, :ns, n:] == 0).all())             # the padding rows
    assert bool((planes[:, 2, :] == 0).all())                # the empty mask (SLOTS[2])
    assert bool(torch.isnan(planes[:, ns:, :]).all())        # packed rows beyond the list
    assert float(planes[0, 0, :n].float().abs().max()) > 0
    m0 = dv["M"][0, :n] == 0
    assert bool((planes[:, 0, :n][:, m0] == 0).all())        # masked-out rows of SLOTS[0]


def test_bad_arguments_are_refused():
    """Null pointers and a bad plane stride return SGLM_EINVAL before anything is launched."""
    from sglm_hip import _lib
    ok = [1, 1.0, 1000, 1024, 5, None] + [8] * 7 + [5, 8, 8, 8, 8, 32, 8, 0]
    for pos, val in ((6, None), (7, None), (14, None), (16, None), (17, None), (19, None),
                     (18, 4), (18, 48), (13, 7), (2, 2000), (3, 1000)):
        args = list(ok)
        args[pos] = val
        with pytest.raises(_lib.HipEngineError, match="sglm_loss_trials_link"):
            _lib.call("sglm_loss_trials_link", *args)


def small_grid(num_folds=3, lams=(1e-3, 1e-2, 1e-1)):
    """A 20000 x 80 Poisson lag design, 3 splits x 3 penalties and their refits (12 fits)."""
    import pandas as pd
    from sglm_hip import engine as E, folds, synth
    from sglm_hip.estimators import Objective
    s = synth.make(N=20000, m=10, L=4, family="poisson", rho=0.03, seed=5)
    d = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    codes = folds.trial_keys_codes(pd.DataFrame({"nTrial": s.trial}), ["nTrial"]).values
    np.random.seed(3)
    cv_idx = folds.cv_idx_from_bucket_ids(codes, num_folds=num_folds)
    objs = [Objective("irls", E.FAM_TWEEDIE_LOG, 1.0, a, "n", True, 100) for a in lams]
    return s, d, cv_idx, objs, lams


MODES = [1, 2]           # the link inside the trial-loss pass / alone, behind the read-back


def run_on_off(monkeypatch, mode, d, y, cv_idx, objs, **kw):
    from sglm_hip import engine as E, grid
    monkeypatch.setattr(E, "STEP_LINK", mode)
    st_on = E.IrlsStats()
    on = grid.run(d, y, cv_idx, objs, [0] * len(objs), stats=st_on, **kw)
    monkeypatch.setattr(E, "STEP_LINK", 0)
    st_off = E.IrlsStats()
    off = grid.run(d, y, cv_idx, objs, [0] * len(objs), stats=st_off, **kw)
    assert st_off.step_link == 0 and st_off.step_restored == 0
    assert st_on.fit_iters == st_off.fit_iters and st_on.newton_iters == st_off.newton_iters
    assert st_on.step_link + st_on.step_restored == st_on.fit_iters
    return on, off, st_on


def assert_bitwise(on, off):
    keys = ("cv_coefs", "cv_intercepts", "refit_coef", "refit_intercept", "cv_scores_train",
            "cv_scores_test", "cv_R2_score", "cv_mse_score")
    for a, b in zip(on, off):
        for key in keys:
            x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), key
        assert a["n_iter"] == b["n_iter"] and a["converged"] == b["converged"]
        assert a["converged"]


@pytest.mark.parametrize("mode", MODES)
def test_grid_full_steps_bitwise(engine, monkeypatch, mode):
    """From the usual start every accepted step is the full one: the pass links them all, and
    coefficients, intercepts, iteration counts and scores are bitwise those of the two-pass
    flow."""
    s, d, cv_idx, objs, _ = small_grid()
    on, off, st = run_on_off(monkeypatch, mode, d, s.y, cv_idx, objs)
    print(f"\n[steplink] full-step grid: fused {st.step_link}, restored {st.step_restored}, "
          f"fit-iterations {st.fit_iters}")
    assert st.step_link > 0
    assert_bitwise(on, off)


@pytest.mark.parametrize("mode", MODES)
def test_grid_freed_group_bitwise(engine, monkeypatch, mode):
    """4 splits x 9 penalties over five decades and their refits (45 fits, two 32-fit groups of
    packed R rows): the fits stop at different iterations, so the continuing ones drop to one
    group while rows of the second are still in use -- those fits are re-linked into rows that
    stopped fits freed, and the gradient keeps the group count (hence the bits) of the two-pass
    flow."""
    s, d, cv_idx, objs, _ = small_grid(4, tuple(np.logspace(1, -4, 9)))
    on, off, st = run_on_off(monkeypatch, mode, d, s.y, cv_idx, objs)
    print(f"\n[steplink] 45-fit grid: fused {st.step_link}, restored {st.step_restored}, "
          f"n_iter {[a['n_iter'] for a in on]}")
    iters = [it for a in on for it in a["n_iter"]]
    # the heavily penalised fits head the list and stop first; once at most 32 fits go on, some
    # of them still sit in rows 32.. (fit order = list order = packed row order)
    early = max(iters[:13])
    assert len(iters) == 45 and early < min(iters[32:])
    assert sum(it > early for it in iters) <= 32
    assert_bitwise(on, off)


def oracle_first_step(X, y, alpha, b0):
    """Step length the oracle's damped Newton (glm_ref.fit_tweedie_newton: Armijo halving with
    sigma = 2^-11) accepts for its first step from w = 0, intercept b0."""
    import scipy.linalg
    from oracle import glm_ref
    Xa = glm_ref._augment(X, True)
    n, pa = Xa.shape
    pen = np.full(pa, float(alpha))
    pen[-1] = 0.0
    coef = np.zeros(pa)
    coef[-1] = b0
    eta = Xa @ coef

    def objective(c, e):
        return glm_ref.half_loss(1.0, True, y, e)[0].mean() + 0.5 * np.dot(pen * c, c)
    _, g_i, h_i = glm_ref.half_loss(1.0, True, y, eta)
    grad = Xa.T @ g_i / n + pen * coef
    H = glm_ref.weighted_gram(Xa, h_i) / n
    H[np.diag_indices_from(H)] += pen
    step = -scipy.linalg.cho_solve(scipy.linalg.cho_factor(H), grad)
    f0, gs, d_eta = objective(coef, eta), float(grad @ step), Xa @ step
    t = 1.0
    for _ in range(40):
        if objective(coef + t * step, eta + t * d_eta) - f0 <= 2.0 ** -11 * t * gs:
            return t
        t *= 0.5
    return 0.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offset,where", [(3.0, "first"), (4.0, "second")])
def test_grid_restore_path_bitwise(engine, monkeypatch, mode, offset, where):
    """Started `offset` below log(mean y) the intercept's first Newton step is e^offset - 1 and
    overshoots: the oracle's damped Newton accepts 1/8 from 3 below (the first round of trial
    steps here) and 1/16 from 4 below (the second round, which reads the predictor that was put
    back).  Every fit of the first iteration is restored from the undo copy, and the results are
    bitwise those of the two-pass flow."""
    s, d, cv_idx, objs, lams = small_grid()
    b0 = math.log(float(np.mean(s.y))) - offset
    t = oracle_first_step(s.dense_X(), s.y, lams[1], b0)
    print(f"\n[steplink] {offset} below log(mean y): the oracle's first step length is {t}")
    assert t == (0.125 if where == "first" else 0.0625)
    on, off, st = run_on_off(monkeypatch, mode, d, s.y, cv_idx, objs, coef0=np.zeros(d.p),
                             intercept0=b0)
    print(f"[steplink] restore grid: fused {st.step_link}, restored {st.step_restored}, "
          f"fit-iterations {st.fit_iters}")
    assert st.step_restored >= 1 and st.step_link > 0
    assert_bitwise(on, off)
