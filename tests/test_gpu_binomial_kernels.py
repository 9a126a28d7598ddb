"""The row passes of an IRLS step at the Binomial family (SGLM_FAM_BINOMIAL_LOGIT = 2): link and
weights, the trial losses summed as differences (and their float64 guard on rows with a large
step), the general float64 branch, the fused trials + link kernel and the score sums, against
float64 numpy on the same f32 inputs.

Inputs as tests/test_gpu_rowpass.py builds them -- 40002 ordinary rows (not a multiple of 4, five
row chunks), a 0.8-density mask with all-zero aligned 4-row blocks, a full mask, an empty one --
with 0/1 responses and 32 appended extreme rows (eta in {+-0, +-20, +-90, +-200}, |deta| up to
300) that only the last mask selects: the accuracy bounds are evaluated on the ordinary rows, the
extreme rows must come out finite or +inf, never NaN."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAM = 2
EPS64 = float(np.finfo(np.float64).eps)
CHUNK = 8192
N_ORD = 40002
ETA_X = np.array([0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 200.0, -200.0], dtype=np.float32)
DETA_X = np.array([-300.0, -60.0, 3.5, 300.0], dtype=np.float32)
N = N_ORD + ETA_X.size * DETA_X.size
SLOTS = np.array([3, 11, 0, 7, 8], dtype=np.int32)
TV1 = np.array([0.0, 1.0, 0.5, 0.25, 0.125], dtype=np.float32)
BP = 32
MASK_X = 3                              # the mask of the extreme rows
# the general branch's error on the Poisson inputs of tests/test_gpu_rowpass.py before the row
# passes were trimmed (GENERAL_BRANCH_PARENT_ERR there): the logit loss has two transcendentals
# per term instead of one, and a margin of 2
GENERAL_BOUND = 4 * 2.3532406933311805e-16


def pad256(n):
    return (n + 255) // 256 * 256


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def make_inputs(B=12, seed=172):
    from sglm_hip import synth
    s = synth.make(N=N_ORD, m=12, L=4, family="binomial", rho=0.08, seed=71, beta_scale=0.5,
                   intercept=-0.5)
    n, no = N, N_ORD
    assert n % 4 and (n + CHUNK - 1) // CHUNK == 5
    ld = pad256(n)
    rng = np.random.default_rng(seed)
    Y = np.zeros((2, ld), np.float32)
    Y[0, :no] = s.y
    Y[1, :no] = np.roll(s.y, 7)
    Y[:, no:n] = np.arange(n - no) % 2
    Y[1, no:n] = 1 - Y[1, no:n]
    M = np.zeros((5, ld), np.uint8)
    m0 = (rng.random(no) < 0.8).astype(np.uint8)
    for i0 in (0, 400, 2 * CHUNK - 8, 3 * CHUNK, no - no % 4 - 24):
        m0[i0:i0 + 16] = 0                     # aligned blocks of four rows, all zero
    M[0, :no] = m0
    M[1, :no] = 1
    M[MASK_X, no:n] = 1                        # mask 2 stays empty
    M[4, :no] = rng.integers(0, 3, no)         # multiplicities 0 / 1 / 2
    fr = rng.integers(0, 2, B).astype(np.int32)
    fm = rng.choice([0, 1, 4], B).astype(np.int32)
    fm[SLOTS] = [0, 1, 2, MASK_X, 4]
    eta = np.zeros((B, ld), np.float32)
    deta = np.zeros((B, ld), np.float32)
    # predictor and step scales per fit: the usual small steps, steps on both sides of the
    # float64 guard (|deta| = 3), and predictors far enough out that sigma rounds to 0 / 1
    # (|eta| stays below 44, where the f32 exponential's argument x log2(e) < 64 still carries
    # the 2e-6 relative bound of the weights)
    esd = np.array([0.5, 1.5, 4.0, 6.0])[np.arange(B) % 4]
    dsd = np.array([0.1, 1.0, 2.5])[np.arange(B) % 3]
    eta[:, :no] = rng.normal(-1.0, 1.0, (B, no)) * esd[:, None]
    deta[:, :no] = rng.normal(0.0, 1.0, (B, no)) * dsd[:, None]
    eta[:, no:n] = np.repeat(ETA_X, DETA_X.size)[None, :]
    deta[:, no:n] = np.tile(DETA_X, ETA_X.size)[None, :]
    step = rng.random(B).astype(np.float32)
    sets = rng.choice([-1, 0, 1, 4], (B, 2)).astype(np.int32)
    sets[0] = [0, 1]
    sets[1] = [-1, -1]
    sets[2] = [MASK_X, 4]
    return dict(n=n, ld=ld, B=B, Y=Y, M=M, fr=fr, fm=fm, eta=eta, deta=deta, step=step, sets=sets)


@pytest.fixture(scope="module")
def inp(torch_mod):
    h = make_inputs()
    dv = {k: (torch_mod.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v)
          for k, v in h.items()}
    return h, dv


def bits(t):
    import torch
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def fit_rows(h, k, eta=None, deta=None):
    """float64 (m, y, eta, deta) of fit k over the ordinary rows."""
    no = N_ORD
    e = h["eta"] if eta is None else eta
    d = h["deta"] if deta is None else deta
    return (h["M"][h["fm"][k], :no].astype(np.float64), h["Y"][h["fr"][k], :no].astype(np.float64),
            e[k, :no].astype(np.float64), d[k, :no].astype(np.float64))


def loss_trials(torch, _lib, dv, slots, eta, deta, tv, with_max=True):
    n, ld = dv["n"], dv["ld"]
    T = int(tv.numel())
    rows = dv["B"] if slots is None else int(slots.numel())
    wk = torch.empty(_lib.query("sglm_rowsum_work_bytes", rows, 8, n), dtype=torch.uint8,
                     device="cuda")
    out = torch.full((rows * T,), float("nan"), dtype=torch.float64, device="cuda")
    sp = None if slots is None else slots.data_ptr()
    common = (dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr())
    if with_max:
        dm = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.call("sglm_loss_trials_max", FAM, 0.0, n, ld, rows, sp, eta.data_ptr(),
                  deta.data_ptr(), *common, tv.data_ptr(), T, out.data_ptr(), dm.data_ptr(),
                  wk.data_ptr(), 0)
        return out.view(rows, T).cpu().numpy(), dm.cpu().numpy()
    _lib.call("sglm_loss_trials", FAM, 0.0, n, ld, rows, sp, eta.data_ptr(), deta.data_ptr(),
              *common, tv.data_ptr(), T, out.data_ptr(), wk.data_ptr(), 0)
    return out.view(rows, T).cpu().numpy(), None


def test_link_accuracy_weights_and_null_w(engine, torch_mod, inp):
    """Every row, the extreme ones included: |g - g64| <= 2e-6, |h - h64| <= 2e-6 h64 + 1e-37,
    nothing NaN or inf, h >= 0; sglm_link_weights is bitwise the W of sglm_link_update; W = NULL
    leaves eta, R and Rp bitwise as the call with W does."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
    common = (dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr())

    def link(with_w, slots, ns, step, deta):
        e = dv["eta"].clone()
        W = torch.full_like(e, float("nan")) if with_w else None
        R = torch.full_like(e, float("nan"))
        Rp = torch.zeros(3 * BP * ld, dtype=torch.bfloat16, device="cuda")
        _lib.call("sglm_link_update", FAM, 0.0, n, ld, ns, slots, e.data_ptr(), *common,
                  None if W is None else W.data_ptr(), R.data_ptr(), Rp.data_ptr(), step, deta, 0)
        return e, W, R, Rp
    # all fits at the stored predictor
    e, W, R, _ = link(True, None, B, None, None)
    assert torch.equal(bits(e), bits(dv["eta"]))
    Wh, Rh = W.cpu().numpy().astype(np.float64), R.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(Wh)) and np.all(np.isfinite(Rh)) and np.all(Wh >= 0)
    assert np.all(Wh[:, n:] == 0) and np.all(Rh[:, n:] == 0)
    worst_g = worst_h = 0.0
    for k in range(B):
        m = h["M"][h["fm"][k], :n].astype(np.float64)
        y = h["Y"][h["fr"][k], :n].astype(np.float64)
        z = h["eta"][k, :n].astype(np.float64)
        mu = sigmoid(z)
        ez = np.exp(-np.abs(z))
        g64, h64 = m * (mu - y), m * ez / (1.0 + ez) ** 2
        sc = np.maximum(m, 1.0)                      # a multiplicity scales both sides
        worst_g = max(worst_g, np.max(np.abs(Rh[k, :n] - g64) / sc))
        worst_h = max(worst_h, np.max(np.abs(Wh[k, :n] - h64) / (2e-6 * h64 + 1e-37 * sc)))
    print(f"link: max |g - g64| {worst_g:.3e} (bound 2e-6); |h - h64| / bound {worst_h:.3f}")
    assert worst_g <= 2e-6 and worst_h <= 1.0
    xk = int(SLOTS[3])                               # the fit on the extreme rows
    assert np.any(Wh[xk, N_ORD:n] == 0) and np.any(Wh[xk, N_ORD:n] == 0.25)
    # weights on demand, and the link without W (fused predictor update included)
    sl = torch.from_numpy(SLOTS).cuda()
    ns = len(SLOTS)
    st = dv["step"][:ns].contiguous()
    e1, W1, R1, Rp1 = link(True, sl.data_ptr(), ns, st.data_ptr(), dv["deta"].data_ptr())
    e0, _, R0, Rp0 = link(False, sl.data_ptr(), ns, st.data_ptr(), dv["deta"].data_ptr())
    assert torch.equal(bits(e0), bits(e1)) and not torch.equal(bits(e1), bits(dv["eta"]))
    assert torch.equal(bits(R0[sl.long()]), bits(R1[sl.long()]))
    assert torch.equal(bits(Rp0), bits(Rp1))
    assert not torch.isnan(R1[sl.long()]).any() and not torch.isnan(W1[sl.long()]).any()
    W2 = torch.full_like(e0, float("nan"))
    _lib.call("sglm_link_weights", FAM, 0.0, n, ld, ns, sl.data_ptr(), e0.data_ptr(), *common,
              W2.data_ptr(), 0)
    listed = np.zeros(B, dtype=bool)
    listed[SLOTS] = True
    for k in range(B):
        if listed[k]:
            assert torch.equal(bits(W2[k]), bits(W1[k])), k
            assert bool((W2[k] >= 0).all()) and bool((W2[k, n:] == 0).all()), k
        else:
            assert bool(torch.isnan(W2[k]).all()) and bool(torch.isnan(W1[k]).all()), k
    assert float(W2[int(SLOTS[0]), :n].max()) > 0


def test_trial_losses_as_differences(engine, torch_mod, inp):
    """The difference branch on the ordinary rows (steps on both sides of the float64 guard):
    D_j = out[j] - out[0] within 4e-6 S_j + 4 eps64 |L0| of float64 numpy on the same f32 inputs,
    S_j = sum m (|log1p(sigma x_j)| + |y t_j d|) -- the Poisson branch's bound and derivation
    (2-ulp expf / expm1f / log1pf, three squarings that each double the relative error); out[0]
    within 1e-6 sum m (softplus(eta) + |y eta|); dmax exact; the slot-list call bitwise the rows
    of the all-slot call.  The fit on the extreme rows: finite or +inf, never NaN."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, B = h["n"], h["B"]
    tv = torch.from_numpy(TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, None, dv["eta"], dv["deta"], tv)
    assert not np.any(np.isnan(out))
    worst = worst0 = 0.0
    guarded = 0
    for k in range(B):
        mk = h["M"][h["fm"][k], :n] > 0
        assert dm[k] == (np.max(np.abs(h["deta"][k, :n][mk])) if mk.any() else 0.0), k
        if h["fm"][k] == MASK_X:
            assert np.all(np.isfinite(out[k]) | (out[k] == np.inf)), k
            continue
        m, y, e, d = fit_rows(h, k)
        guarded += int(np.sum((m > 0) & (np.abs(d) > 3)))
        sg = sigmoid(e)
        L0 = math.fsum(m * (softplus(e) - y * e))
        b0 = 1e-6 * math.fsum(m * (softplus(e) + np.abs(y * e)))
        if b0:
            worst0 = max(worst0, abs(out[k, 0] - L0) / b0)
        else:
            assert out[k, 0] == 0
        for j in range(1, 5):
            t = float(TV1[j])
            ref = math.fsum(m * (softplus(e + t * d) - softplus(e) - y * t * d))
            S = math.fsum(m * (np.abs(np.log1p(sg * np.expm1(t * d))) + np.abs(y * t * d)))
            bound = 4e-6 * S + 4 * EPS64 * abs(L0)
            err = abs((out[k, j] - out[k, 0]) - ref)
            if bound:
                worst = max(worst, err / bound)
            else:
                assert err == 0
    print(f"logit trial differences: worst error / bound {worst:.3f}; L(0): {worst0:.3f}; "
          f"{guarded} rows on the float64 guard")
    assert guarded > 1000                       # both sides of |deta| = 3 are exercised
    assert worst <= 1.0 and worst0 <= 1.0
    sl = torch.from_numpy(SLOTS).cuda()
    out2, dm2 = loss_trials(torch, _lib, dv, sl, dv["eta"], dv["deta"], tv)
    assert np.array_equal(out2.view(np.int64), out[SLOTS].view(np.int64))
    assert np.array_equal(dm2, dm[SLOTS])


def test_trial_losses_zero_step_bitwise(engine, torch_mod, inp):
    """With deta == 0 the five outputs of a fit are bitwise equal (extreme rows included)."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    tv = torch.from_numpy(TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, None, dv["eta"], torch.zeros_like(dv["deta"]), tv)
    assert np.all(np.isfinite(out))
    assert np.all((out[:, 0] != 0) == (h["fm"] != 2))
    for j in range(1, 5):
        assert np.array_equal(out[:, j].view(np.int64), out[:, 0].view(np.int64)), j
    assert np.all(dm == 0)


def test_trial_losses_general_branch(engine, torch_mod, inp):
    """T = 7 (engine.TV2: the general float64 branch) on the ordinary rows against float64 numpy,
    relative to sum m (softplus(z) + |y z|): at most 4 x the existing general branch's measured
    error (2.353e-16)."""
    torch = torch_mod
    from sglm_hip import _lib, engine as E
    h, dv = inp
    tvh = E.TV2.astype(np.float32)
    assert tvh.size == 7
    out, _ = loss_trials(torch, _lib, dv, None, dv["eta"], dv["deta"], torch.from_numpy(tvh).cuda(),
                         with_max=False)
    assert not np.any(np.isnan(out))
    worst = 0.0
    for k in range(h["B"]):
        if h["fm"][k] in (2, MASK_X):
            continue
        m, y, e, d = fit_rows(h, k)
        for j, t in enumerate(tvh.astype(np.float64)):
            z = e + t * d
            ref = math.fsum(m * (softplus(z) - y * z))
            scale = math.fsum(m * (softplus(z) + np.abs(y * z)))
            worst = max(worst, abs(out[k, j] - ref) / scale)
    print(f"logit general branch: error {worst:.3e} (bound {GENERAL_BOUND:.3e})")
    assert worst <= GENERAL_BOUND


def test_fused_kernel_matches_trials_then_link(engine, torch_mod, inp):
    """sglm_loss_trials_link at family 2: sums, dmax, undo, eta and the packed R planes bitwise
    those of sglm_loss_trials_max followed by sglm_link_update_rp at step 1 (the empty mask, the
    multiplicity mask and the extreme rows among the listed fits), and the link-alone call too."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
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
    _lib.call("sglm_loss_trials_max", FAM, 0.0, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, tv.data_ptr(), 5, a["out"].data_ptr(),
              a["dm"].data_ptr(), a["wk"].data_ptr(), 0)
    one = torch.ones(ns, dtype=torch.float32, device="cuda")
    rpos = torch.arange(ns, dtype=torch.int32, device="cuda")
    _lib.call("sglm_link_update_rp", FAM, 0.0, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              *common, None, None, a["Rp"].data_ptr(), BP, rpos.data_ptr(), one.data_ptr(),
              dv["deta"].data_ptr(), 0)
    b = bufs()
    undo = torch.full((ns, ld), nan, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_link", FAM, 0.0, n, ld, ns, sl.data_ptr(), b["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, tv.data_ptr(), 5, b["out"].data_ptr(),
              b["dm"].data_ptr(), undo.data_ptr(), b["Rp"].data_ptr(), BP, b["wk"].data_ptr(), 0)
    c = bufs()
    undo2 = torch.full((ns, ld), nan, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_link", FAM, 0.0, n, ld, ns, sl.data_ptr(), c["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, None, 0, None, None, undo2.data_ptr(),
              c["Rp"].data_ptr(), BP, None, 0)
    torch.cuda.synchronize()
    assert torch.equal(bits(c["e"]), bits(a["e"])) and torch.equal(bits(c["Rp"]), bits(a["Rp"]))
    assert torch.equal(bits(undo2), bits(undo)) and bool(torch.isnan(c["out"]).all())
    assert torch.equal(bits(b["out"]), bits(a["out"]))
    assert torch.equal(bits(b["dm"]), bits(a["dm"]))
    assert not torch.isnan(b["out"]).any() and float(b["dm"].max()) == 300.0
    assert torch.equal(bits(b["e"]), bits(a["e"]))
    assert torch.equal(bits(b["Rp"]), bits(a["Rp"]))
    assert torch.equal(bits(undo[:, :n]), bits(dv["eta"][sl.long(), :n]))
    listed = np.zeros(B, dtype=bool)
    listed[SLOTS] = True
    for k in range(B):
        same = torch.equal(bits(b["e"][k]), bits(dv["eta"][k]))
        assert same != listed[k], k
    planes = b["Rp"].view(3, BP, ld)
    assert bool((planes[:, :ns, n:] == 0).all())             # the padding rows
    assert bool((planes[:, 2, :] == 0).all())                # the empty mask (SLOTS[2])
    assert bool(torch.isnan(planes[:, ns:, :]).all())        # packed rows beyond the list
    assert not torch.isnan(planes[:, :ns, :].float()).any()
    assert float(planes[0, 0, :n].float().abs().max()) > 0
    # R of the extreme rows: sigma(eta + deta) - y, finite at every one of them
    r = planes[:, 3, N_ORD:n].float().sum(dim=0).cpu().numpy().astype(np.float64)
    z = (h["eta"][SLOTS[3], N_ORD:n] + h["deta"][SLOTS[3], N_ORD:n]).astype(np.float64)
    y = h["Y"][h["fr"][SLOTS[3]], N_ORD:n].astype(np.float64)
    assert np.max(np.abs(r - (sigmoid(z) - y))) <= 2e-6


def test_score_sums(engine, torch_mod, inp):
    """sglm_score_sums at family 2 against float64 numpy (every row, the extreme ones included):
    sum m (y - sigma(eta))^2 and sum m loss within 16 eps64 sum m |term|."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
    wk = torch.zeros(_lib.query("sglm_rowsum_work_bytes", B, 4, n) // 8, dtype=torch.float64,
                     device="cuda")
    out = torch.full((B, 4), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("sglm_score_sums", FAM, 0.0, n, ld, B, dv["eta"].data_ptr(), dv["Y"].data_ptr(),
              dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["sets"].data_ptr(), out.data_ptr(),
              wk.data_ptr(), 0)
    got = out.cpu().numpy().reshape(B, 2, 2)
    assert np.all(np.isfinite(got))
    worst = 0.0
    for k in range(B):
        y = h["Y"][h["fr"][k], :n].astype(np.float64)
        z = h["eta"][k, :n].astype(np.float64)
        r2 = (y - sigmoid(z)) ** 2
        l = softplus(z) - y * z
        for s in range(2):
            ms = h["sets"][k, s]
            if ms < 0:
                assert got[k, s, 0] == 0 and got[k, s, 1] == 0
                continue
            m = h["M"][ms, :n].astype(np.float64)
            for q, term in enumerate((m * r2, m * l)):
                bound = 16 * EPS64 * math.fsum(np.abs(term))
                err = abs(got[k, s, q] - math.fsum(term))
                if bound:
                    worst = max(worst, err / bound)
                else:
                    assert err == 0
    print(f"logit score sums: worst error / bound {worst:.3f}")
    assert worst <= 1.0 and np.any(got != 0)
