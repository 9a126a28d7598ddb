"""The row passes of an IRLS step at the negative-binomial family (SGLM_FAM_NB2_LOG = 3, the
dispersion kappa in the `power` argument): link and weights, the trial losses summed as
differences (and their float64 guard on rows with a large step), the general float64 branch, the
fused trials + link kernel, the score sums and the saturated-constant sums, against float64 numpy
on the same f32 inputs.

Inputs as tests/test_gpu_binomial_kernels.py builds them -- 40002 ordinary rows (not a multiple
of 4, five row chunks), a 0.8-density mask with all-zero aligned 4-row blocks, a full mask, an
empty one, a multiplicity mask -- with count responses and 32 appended extreme rows (eta in
{+-0, +-20, +-90, +-200}, |deta| up to 300) that only the last mask selects.  kappa in {0.25, 8}
(exact in float32), and 2^-10 for the link."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAM = 3
KAPPAS = (0.25, 8.0)
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
# GENERAL_BOUND of tests/test_gpu_binomial_kernels.py, copied: the general branch's error on the
# Poisson inputs of tests/test_gpu_rowpass.py before the row passes were trimmed
# (GENERAL_BRANCH_PARENT_ERR there), times 2 for the second transcendental per term (the NB2 loss
# is a softplus too: exp and log1p; ln kappa is one value for the whole call) and a margin of 2
GENERAL_BOUND = 4 * 2.3532406933311805e-16


def pad256(n):
    return (n + 255) // 256 * 256


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def nb2_loss(kappa, y, eta):
    return (y + 1.0 / kappa) * softplus(eta + math.log(kappa)) - y * eta


def nb2_gh(kappa, y, eta):
    """float64 (d loss / d eta, d2 loss / d eta2, the bound scale mu (1 + kappa y) / (1 + kappa mu)
    + y), overflow-free."""
    z = eta + math.log(kappa)
    e = np.exp(-np.abs(z))
    q = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    f = y + 1.0 / kappa
    return f * q - y, f * e / (1.0 + e) ** 2, f * q + y


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def make_inputs(B=12, seed=172):
    from sglm_hip import synth
    s = synth.make(N=N_ORD, m=12, L=4, family="nb2", rho=0.08, seed=71, beta_scale=0.5,
                   intercept=0.5, kappa=0.5)
    n, no = N, N_ORD
    assert n % 4 and (n + CHUNK - 1) // CHUNK == 5
    ld = pad256(n)
    rng = np.random.default_rng(seed)
    Y = np.zeros((2, ld), np.float32)
    Y[0, :no] = s.y
    Y[1, :no] = np.roll(s.y, 7)
    Y[:, no:n] = np.arange(n - no) % 5
    Y[1, no:n] = 4 - Y[1, no:n]
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
    # float64 guard (|deta| = 3), and predictors far enough out that sigma(eta + ln kappa)
    # rounds to 0 / 1
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


def loss_trials(torch, _lib, dv, kappa, slots, eta, deta, tv, with_max=True):
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
        _lib.call("sglm_loss_trials_max", FAM, kappa, n, ld, rows, sp, eta.data_ptr(),
                  deta.data_ptr(), *common, tv.data_ptr(), T, out.data_ptr(), dm.data_ptr(),
                  wk.data_ptr(), 0)
        return out.view(rows, T).cpu().numpy(), dm.cpu().numpy()
    _lib.call("sglm_loss_trials", FAM, kappa, n, ld, rows, sp, eta.data_ptr(), deta.data_ptr(),
              *common, tv.data_ptr(), T, out.data_ptr(), wk.data_ptr(), 0)
    return out.view(rows, T).cpu().numpy(), None


def link_call(torch, _lib, dv, kappa, with_w, slots, ns, step, deta):
    n, ld = dv["n"], dv["ld"]
    common = (dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr())
    e = dv["eta"].clone()
    W = torch.full_like(e, float("nan")) if with_w else None
    R = torch.full_like(e, float("nan"))
    Rp = torch.zeros(3 * BP * ld, dtype=torch.bfloat16, device="cuda")
    _lib.call("sglm_link_update", FAM, kappa, n, ld, ns, slots, e.data_ptr(), *common,
              None if W is None else W.data_ptr(), R.data_ptr(), Rp.data_ptr(), step, deta, 0)
    return e, W, R, Rp


@pytest.mark.parametrize("kappa", KAPPAS + (2.0 ** -10,))
def test_link_accuracy_weights_and_null_w(engine, torch_mod, inp, kappa):
    """Every row, the extreme ones included: |g - g64| <= 2e-6 (mu (1 + kappa y) / (1 + kappa mu)
    + y) + 1e-37, |h - h64| <= 2e-6 h64 + 1e-37, nothing NaN or inf, h >= 0; sglm_link_weights is
    bitwise the W of sglm_link_update; W = NULL leaves eta, R and Rp bitwise as the call with W
    does.  The 1e-37 on g is the one the weights' bound carries, for the same reason: at eta =
    -90 and -200 with y = 0 the float64 gradient is mu = 8e-40 and 1e-87, below float32's smallest
    normal number (1.2e-38), so no float32 output can be relative to it."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
    common = (dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr())
    # all fits at the stored predictor
    e, W, R, _ = link_call(torch, _lib, dv, kappa, True, None, B, None, None)
    assert torch.equal(bits(e), bits(dv["eta"]))
    Wh, Rh = W.cpu().numpy().astype(np.float64), R.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(Wh)) and np.all(np.isfinite(Rh)) and np.all(Wh >= 0)
    assert np.all(Wh[:, n:] == 0) and np.all(Rh[:, n:] == 0)
    worst_g = worst_h = 0.0
    for k in range(B):
        m = h["M"][h["fm"][k], :n].astype(np.float64)
        y = h["Y"][h["fr"][k], :n].astype(np.float64)
        g64, h64, gs = nb2_gh(kappa, y, h["eta"][k, :n].astype(np.float64))
        sc = np.maximum(m, 1.0)                      # a multiplicity scales both sides
        worst_g = max(worst_g, np.max(np.abs(Rh[k, :n] - m * g64) / sc / (2e-6 * gs + 1e-37)))
        worst_h = max(worst_h, np.max(np.abs(Wh[k, :n] - m * h64) / (2e-6 * m * h64 + 1e-37 * sc)))
    print(f"nb2 link kappa={kappa:g}: |g - g64| / bound {worst_g:.3f}; "
          f"|h - h64| / bound {worst_h:.3f}")
    assert worst_g <= 1.0 and worst_h <= 1.0
    xk = int(SLOTS[3])                               # the fit on the extreme rows
    assert np.any(Wh[xk, N_ORD:n] == 0) and np.any(Wh[xk, N_ORD:n] > 0)
    # weights on demand, and the link without W (fused predictor update included)
    sl = torch.from_numpy(SLOTS).cuda()
    ns = len(SLOTS)
    st = dv["step"][:ns].contiguous()
    e1, W1, R1, Rp1 = link_call(torch, _lib, dv, kappa, True, sl.data_ptr(), ns, st.data_ptr(),
                                dv["deta"].data_ptr())
    e0, _, R0, Rp0 = link_call(torch, _lib, dv, kappa, False, sl.data_ptr(), ns, st.data_ptr(),
                               dv["deta"].data_ptr())
    assert torch.equal(bits(e0), bits(e1)) and not torch.equal(bits(e1), bits(dv["eta"]))
    assert torch.equal(bits(R0[sl.long()]), bits(R1[sl.long()]))
    assert torch.equal(bits(Rp0), bits(Rp1))
    assert not torch.isnan(R1[sl.long()]).any() and not torch.isnan(W1[sl.long()]).any()
    assert not torch.isinf(R1[sl.long()]).any() and not torch.isinf(W1[sl.long()]).any()
    W2 = torch.full_like(e0, float("nan"))
    _lib.call("sglm_link_weights", FAM, kappa, n, ld, ns, sl.data_ptr(), e0.data_ptr(), *common,
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


@pytest.mark.parametrize("kappa", KAPPAS)
def test_trial_losses_as_differences(engine, torch_mod, inp, kappa):
    """The difference branch on the ordinary rows (steps on both sides of the float64 guard):
    D_j = out[j] - out[0] within 4e-6 S_j + 4 eps64 |L0| of float64 numpy on the same f32 inputs,
    S_j = sum m ((y + 1/kappa) |log1p(q x_j)| + |y t_j d|), q = sigma(eta + ln kappa) -- the
    Binomial test's bound and derivation (2-ulp expf / expm1f / log1pf, three squarings that each
    double the relative error).  The constant is that test's: the row factor y + 1/kappa
    multiplies the log1p term and its error alike and is itself one f32 rounding (half an ulp, 3e-8
    relative), and q = kappa expf(eta) / (1 + e) carries one product more than sigma does (one
    ulp): together 1e-7 against the 4e-6 that the 16-ulp x_1 = expm1 after three squarings
    already needs.  out[0] within 1e-6 sum m ((y + 1/kappa) softplus(z) + |y eta|); dmax exact;
    the slot-list call bitwise the rows of the all-slot call.  The fit on the extreme rows:
    finite or +inf, never NaN."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, B = h["n"], h["B"]
    lk = math.log(kappa)
    tv = torch.from_numpy(TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, kappa, None, dv["eta"], dv["deta"], tv)
    assert not np.any(np.isnan(out))
    worst = worst0 = 0.0
    guarded = plain = 0
    for k in range(B):
        mk = h["M"][h["fm"][k], :n] > 0
        assert dm[k] == (np.max(np.abs(h["deta"][k, :n][mk])) if mk.any() else 0.0), k
        if h["fm"][k] == MASK_X:
            assert np.all(np.isfinite(out[k]) | (out[k] == np.inf)), k
            continue
        m, y, e, d = fit_rows(h, k)
        guarded += int(np.sum((m > 0) & (np.abs(d) > 3)))
        plain += int(np.sum((m > 0) & (np.abs(d) <= 3)))
        f = y + 1.0 / kappa
        q = sigmoid(e + lk)
        L0 = math.fsum(m * nb2_loss(kappa, y, e))
        b0 = 1e-6 * math.fsum(m * (f * softplus(e + lk) + np.abs(y * e)))
        if b0:
            worst0 = max(worst0, abs(out[k, 0] - L0) / b0)
        else:
            assert out[k, 0] == 0
        for j in range(1, 5):
            t = float(TV1[j])
            ref = math.fsum(m * (f * (softplus(e + t * d + lk) - softplus(e + lk)) - y * t * d))
            S = math.fsum(m * (f * np.abs(np.log1p(q * np.expm1(t * d))) + np.abs(y * t * d)))
            bound = 4e-6 * S + 4 * EPS64 * abs(L0)
            err = abs((out[k, j] - out[k, 0]) - ref)
            if bound:
                worst = max(worst, err / bound)
            else:
                assert err == 0
    print(f"nb2 trial differences kappa={kappa:g}: worst error / bound {worst:.3f}; "
          f"L(0): {worst0:.3f}; {guarded} rows on the float64 guard, {plain} below it")
    assert guarded > 1000 and plain > 1000      # both sides of |deta| = 3 are exercised
    assert worst <= 1.0 and worst0 <= 1.0
    sl = torch.from_numpy(SLOTS).cuda()
    out2, dm2 = loss_trials(torch, _lib, dv, kappa, sl, dv["eta"], dv["deta"], tv)
    assert np.array_equal(out2.view(np.int64), out[SLOTS].view(np.int64))
    assert np.array_equal(dm2, dm[SLOTS])


@pytest.mark.parametrize("kappa", KAPPAS)
def test_trial_losses_zero_step_bitwise(engine, torch_mod, inp, kappa):
    """With deta == 0 the five outputs of a fit are bitwise equal (extreme rows included)."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    tv = torch.from_numpy(TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, kappa, None, dv["eta"],
                          torch.zeros_like(dv["deta"]), tv)
    assert np.all(np.isfinite(out))
    assert np.all((out[:, 0] != 0) == (h["fm"] != 2))
    for j in range(1, 5):
        assert np.array_equal(out[:, j].view(np.int64), out[:, 0].view(np.int64)), j
    assert np.all(dm == 0)


@pytest.mark.parametrize("kappa", KAPPAS)
def test_trial_losses_general_branch(engine, torch_mod, inp, kappa):
    """T = 7 (engine.TV2: the general float64 branch) on the ordinary rows against float64 numpy,
    relative to sum m ((y + 1/kappa) softplus(z + ln kappa) + |y z|): within GENERAL_BOUND."""
    torch = torch_mod
    from sglm_hip import _lib, engine as E
    h, dv = inp
    lk = math.log(kappa)
    tvh = E.TV2.astype(np.float32)
    assert tvh.size == 7
    out, _ = loss_trials(torch, _lib, dv, kappa, None, dv["eta"], dv["deta"],
                         torch.from_numpy(tvh).cuda(), with_max=False)
    assert not np.any(np.isnan(out))
    worst = 0.0
    for k in range(h["B"]):
        if h["fm"][k] in (2, MASK_X):
            continue
        m, y, e, d = fit_rows(h, k)
        for j, t in enumerate(tvh.astype(np.float64)):
            z = e + t * d
            ref = math.fsum(m * nb2_loss(kappa, y, z))
            scale = math.fsum(m * ((y + 1.0 / kappa) * softplus(z + lk) + np.abs(y * z)))
            worst = max(worst, abs(out[k, j] - ref) / scale)
    print(f"nb2 general branch kappa={kappa:g}: error {worst:.3e} (bound {GENERAL_BOUND:.3e})")
    assert worst <= GENERAL_BOUND


@pytest.mark.parametrize("kappa", KAPPAS)
def test_fused_kernel_matches_trials_then_link(engine, torch_mod, inp, kappa):
    """sglm_loss_trials_link at family 3: sums, dmax, undo, eta and the packed R planes bitwise
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
    _lib.call("sglm_loss_trials_max", FAM, kappa, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, tv.data_ptr(), 5, a["out"].data_ptr(),
              a["dm"].data_ptr(), a["wk"].data_ptr(), 0)
    one = torch.ones(ns, dtype=torch.float32, device="cuda")
    rpos = torch.arange(ns, dtype=torch.int32, device="cuda")
    _lib.call("sglm_link_update_rp", FAM, kappa, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              *common, None, None, a["Rp"].data_ptr(), BP, rpos.data_ptr(), one.data_ptr(),
              dv["deta"].data_ptr(), 0)
    b = bufs()
    undo = torch.full((ns, ld), nan, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_link", FAM, kappa, n, ld, ns, sl.data_ptr(), b["e"].data_ptr(),
              dv["deta"].data_ptr(), *common, tv.data_ptr(), 5, b["out"].data_ptr(),
              b["dm"].data_ptr(), undo.data_ptr(), b["Rp"].data_ptr(), BP, b["wk"].data_ptr(), 0)
    c = bufs()
    undo2 = torch.full((ns, ld), nan, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_link", FAM, kappa, n, ld, ns, sl.data_ptr(), c["e"].data_ptr(),
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
    assert not torch.isinf(planes[:, :ns, :].float()).any()
    assert float(planes[0, 0, :n].float().abs().max()) > 0
    # R of the extreme rows: the gradient at eta + deta, finite at every one, within the link's
    # bound (eta + deta is formed in f32, as the kernel forms it)
    r = planes[:, 3, N_ORD:n].float().sum(dim=0).cpu().numpy().astype(np.float64)
    z = (h["eta"][SLOTS[3], N_ORD:n] + h["deta"][SLOTS[3], N_ORD:n]).astype(np.float64)
    y = h["Y"][h["fr"][SLOTS[3]], N_ORD:n].astype(np.float64)
    g64, _, gs = nb2_gh(kappa, y, z)
    assert np.all(np.abs(r - g64) <= 2e-6 * gs + 1e-37)


@pytest.mark.parametrize("kappa", KAPPAS)
def test_score_sums(engine, torch_mod, inp, kappa):
    """sglm_score_sums at family 3 against float64 numpy on the ordinary rows' masks and the
    extreme rows' (|eta| <= 200: exp(eta) is finite in float64): sum m (y - exp(eta))^2 and
    sum m loss within 1e-12 sum m |term|."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
    wk = torch.zeros(_lib.query("sglm_rowsum_work_bytes", B, 4, n) // 8, dtype=torch.float64,
                     device="cuda")
    out = torch.full((B, 4), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("sglm_score_sums", FAM, kappa, n, ld, B, dv["eta"].data_ptr(), dv["Y"].data_ptr(),
              dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["sets"].data_ptr(), out.data_ptr(),
              wk.data_ptr(), 0)
    got = out.cpu().numpy().reshape(B, 2, 2)
    assert np.all(np.isfinite(got))
    lk = math.log(kappa)
    worst = 0.0
    for k in range(B):
        y = h["Y"][h["fr"][k], :n].astype(np.float64)
        z = h["eta"][k, :n].astype(np.float64)
        r2 = (y - np.exp(z)) ** 2
        l = nb2_loss(kappa, y, z)
        labs = (y + 1.0 / kappa) * softplus(z + lk) + np.abs(y * z)
        for s in range(2):
            ms = h["sets"][k, s]
            if ms < 0:
                assert got[k, s, 0] == 0 and got[k, s, 1] == 0
                continue
            m = h["M"][ms, :n].astype(np.float64)
            for q, (term, ab) in enumerate(((m * r2, m * r2), (m * l, m * labs))):
                bound = 1e-12 * math.fsum(ab)
                err = abs(got[k, s, q] - math.fsum(term))
                if bound:
                    worst = max(worst, err / bound)
                else:
                    assert err == 0
    print(f"nb2 score sums kappa={kappa:g}: worst error / bound {worst:.3f}")
    assert worst <= 1.0 and np.any(got != 0)


@pytest.mark.parametrize("kappa", KAPPAS + (2.0 ** -16,))
def test_constant_sums(engine, torch_mod, inp, kappa):
    """sglm_nb2_const_sums: sum m c_kappa(y) of every (mask, response), float64 responses, within
    1e-12 sum m (|y ln y| + (y + 1/kappa) ln(1 + kappa y)) of math.fsum; 0 on the empty mask; the
    same call twice is bitwise equal (fixed-order sums)."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld = h["n"], h["ld"]
    F_, R = h["M"].shape[0], h["Y"].shape[0]
    Y64 = h["Y"][:, :n].astype(np.float64) * 1.25        # non-integer responses too
    Yd = torch.from_numpy(np.ascontiguousarray(Y64)).cuda()
    assert _lib.query("sglm_nb2_const_sums_work_bytes", F_, R, n) == F_ * R * 5 * 8
    wk = torch.empty(_lib.query("sglm_nb2_const_sums_work_bytes", F_, R, n), dtype=torch.uint8,
                     device="cuda")
    outs = []
    for _ in range(2):
        out = torch.full((R, F_), float("nan"), dtype=torch.float64, device="cuda")
        _lib.call("sglm_nb2_const_sums", dv["M"].data_ptr(), ld, F_, Yd.data_ptr(), R, n, kappa,
                  out.data_ptr(), wk.data_ptr(), 0)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    got = outs[0]
    worst = 0.0
    for r in range(R):
        y = Y64[r]
        ys = np.where(y > 0, y, 1.0)
        a, b = ys * np.log(ys) * (y > 0), (ys + 1.0 / kappa) * np.log1p(kappa * ys) * (y > 0)
        for f in range(F_):
            m = h["M"][f, :n].astype(np.float64)
            bound = 1e-12 * math.fsum(m * (np.abs(a) + b))
            err = abs(got[r, f] - math.fsum(m * (a - b)))
            if bound:
                worst = max(worst, err / bound)
            else:
                assert got[r, f] == 0
    print(f"nb2 constant sums kappa={kappa:g}: worst error / bound {worst:.3f}")
    assert worst <= 1.0 and np.all(got[:, 2] == 0) and np.all(got[:, 1] != 0)
