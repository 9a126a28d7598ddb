"""The row passes of an IRLS step at the squared loss and the log-link Tweedie losses (power 1,
2, 1.5 and 1.2; family kind 0 of csrc/api.hip) against the float64 references and the derived
limits of tests/tweedie_rows_cases.py: link and weights row by row (extreme predictors up to
|eta| = 80 included), the packed bf16 planes of R, the general float64 branch of the trial
losses, the Poisson difference branch at steps of order 1, the score sums and the fused
trials + link kernel at the general powers.  Every output buffer is NaN before the call."""
import numpy as np
import pytest

import tweedie_rows_cases as C

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAN = float("nan")
IDS = [f"f{f}-p{p:g}" for f, p in C.FORMS]


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


@pytest.fixture(scope="module")
def dev(torch_mod):
    """(host arrays, device tensors) of the case, one copy per response set."""
    cache = {}

    def get(fam, power):
        g = C.is_gamma(fam, power)
        if g not in cache:
            h = C.make_inputs(g)
            cache[g] = (h, {k: (torch_mod.from_numpy(v.copy()).cuda()
                                if isinstance(v, np.ndarray) else v) for k, v in h.items()})
        return cache[g]
    return get


def bits(t):
    import torch
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def common(dv):
    return (dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr())


def ptr(t):
    return None if t is None else t.data_ptr()


def link_update(torch, _lib, dv, fam, power, slots=None, step=None, deta=None, with_w=True):
    """sglm_link_update on a copy of eta: (eta, W, R, planes [3][BP][ld])."""
    ns = dv["B"] if slots is None else int(slots.numel())
    e = dv["eta"].clone()
    W = torch.full_like(e, NAN) if with_w else None
    R = torch.full_like(e, NAN)
    Rp = torch.full((3 * C.BP * dv["ld"],), NAN, dtype=torch.bfloat16, device="cuda")
    _lib.call("sglm_link_update", fam, power, dv["n"], dv["ld"], ns, ptr(slots), e.data_ptr(),
              *common(dv), ptr(W), R.data_ptr(), Rp.data_ptr(), ptr(step), ptr(deta), 0)
    return e, W, R, Rp.view(3, C.BP, dv["ld"])


def check_link_rows(fam, power, h, k, eta_k, Rk, Wk):
    """R and W of fit k (float64 host rows) against the references at the float32 eta_k; returns
    the worst error / limit of g and of h."""
    n = h["n"]
    m, y, _, _ = C.fit_rows(h, k)
    e = eta_k[:n].astype(np.float64)
    assert np.all(Rk[n:] == 0) and np.all(Wk[n:] == 0), k
    assert np.all(Rk[:n][m == 0] == 0) and np.all(Wk[:n][m == 0] == 0), k
    on = m > 0
    if not on.any():
        return 0.0, 0.0
    if fam == 0:
        m32, y32, e32 = m.astype(np.float32), y.astype(np.float32), eta_k[:n]
        assert np.array_equal(Rk[:n].astype(np.float32), m32 * (e32 - y32)), k
        assert np.array_equal(Wk[:n], m), k
        return 0.0, 0.0
    ref = C.reference(fam, power, y, e)
    lg, lh = C.link_limits(fam, power, y, e)
    rg = np.abs(Rk[:n] - m * ref["g"])[on] / (m * lg)[on]
    rh = np.abs(Wk[:n] - m * ref["h"])[on] / (m * lh)[on]
    return float(rg.max()), float(rh.max())


@pytest.mark.parametrize("fam,power", C.FORMS, ids=IDS)
def test_link_accuracy(engine, torch_mod, dev, fam, power):
    """sglm_link_update over all fits: eta bitwise unchanged, R and W within the limits on every
    row (squared loss: bitwise m (eta - y) and m), nothing NaN or inf, W >= 0, exact zeros on the
    rows n..ld-1 and where the mask is 0.  Then the slot list with the fused predictor update:
    the new eta is float32(eta + step deta) to one rounding (fused or not), R and W within the
    limits at the eta the kernel stored, unlisted slots untouched; sglm_link_weights on that eta
    bitwise the W of the link."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = dev(fam, power)
    n, ld, B = h["n"], h["ld"], h["B"]
    e, W, R, _ = link_update(torch, _lib, dv, fam, power)
    assert torch.equal(bits(e), bits(dv["eta"]))
    Wh, Rh = W.cpu().numpy().astype(np.float64), R.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(Wh)) and np.all(np.isfinite(Rh)) and np.all(Wh >= 0)
    worst_g = worst_h = 0.0
    for k in range(B):
        rg, rh = check_link_rows(fam, power, h, k, h["eta"][k], Rh[k], Wh[k])
        worst_g, worst_h = max(worst_g, rg), max(worst_h, rh)
    xk = int(C.SLOTS[3])                               # the fit on the extreme rows
    assert np.all(Wh[xk, C.N_ORD:n] > 0)
    assert np.any(Rh[xk, C.N_ORD:n] != 0) and np.any(Rh[int(C.SLOTS[4]), :n] != 0)
    # the slot list with the fused predictor update
    sl = torch.from_numpy(C.SLOTS).cuda()
    ns = len(C.SLOTS)
    st = dv["step"][:ns].contiguous()
    e1, W1, R1, _ = link_update(torch, _lib, dv, fam, power, sl, st, dv["deta"])
    e1h = e1.cpu().numpy()
    W1h, R1h = W1.cpu().numpy().astype(np.float64), R1.cpu().numpy().astype(np.float64)
    listed = np.zeros(B, dtype=bool)
    listed[C.SLOTS] = True
    worst_g2 = worst_h2 = 0.0
    for q, k in enumerate(C.SLOTS):
        t32 = h["step"][q]
        fused = (h["eta"][k, :n].astype(np.float64)
                 + float(t32) * h["deta"][k, :n].astype(np.float64)).astype(np.float32)
        plain = h["eta"][k, :n] + t32 * h["deta"][k, :n]
        assert np.all((e1h[k, :n] == fused) | (e1h[k, :n] == plain)), k
        assert np.array_equal(e1h[k, n:], h["eta"][k, n:]), k
        assert np.all(np.isfinite(W1h[k])) and np.all(np.isfinite(R1h[k])) and np.all(W1h[k] >= 0)
        rg, rh = check_link_rows(fam, power, h, k, e1h[k], R1h[k], W1h[k])
        worst_g2, worst_h2 = max(worst_g2, rg), max(worst_h2, rh)
    assert not np.array_equal(e1h[C.SLOTS[0], :n], h["eta"][C.SLOTS[0], :n])
    for k in np.flatnonzero(~listed):
        assert torch.equal(bits(e1[k]), bits(dv["eta"][k])), k
        assert bool(torch.isnan(W1[k]).all()) and bool(torch.isnan(R1[k]).all()), k
    print(f"\n[tweedie rows] link ({fam}, {power}): worst error / limit g {worst_g:.3f} "
          f"h {worst_h:.3f}; after the fused update g {worst_g2:.3f} h {worst_h2:.3f}")
    assert max(worst_g, worst_h, worst_g2, worst_h2) <= 1.0
    # weights on demand
    W2 = torch.full_like(e1, NAN)
    _lib.call("sglm_link_weights", fam, power, n, ld, ns, sl.data_ptr(), e1.data_ptr(),
              *common(dv), W2.data_ptr(), 0)
    for k in range(B):
        if listed[k]:
            assert torch.equal(bits(W2[k]), bits(W1[k])), k
        else:
            assert bool(torch.isnan(W2[k]).all()), k
    assert float(W2[int(C.SLOTS[0]), :n].max()) > 0
    W3 = torch.full_like(e1, NAN)
    _lib.call("sglm_link_weights", fam, power, n, ld, B, None, e1.data_ptr(), *common(dv),
              W3.data_ptr(), 0)
    assert torch.equal(bits(W3[sl.long()]), bits(W1[sl.long()])) and not torch.isnan(W3).any()


@pytest.mark.parametrize("fam,power", C.FORMS, ids=IDS)
def test_packed_r_planes(engine, torch_mod, dev, fam, power):
    """split3's contract on the R of every fit: (hi + mid) + lo == R in float32 wherever
    |R| >= 2^-100 (compared as numbers: the planes of R = -0 sum to +0), within 2^-16 |R| below;
    rows n..ld-1 and masked-out rows are 0 in all three planes.  sglm_link_update_rp with
    rpos = [2, -1, 0, 1, 3] writes each listed fit's planes at its rpos row, bitwise the rows of
    the plain call, and no other row."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = dev(fam, power)
    n, ld, B = h["n"], h["ld"], h["B"]
    _, _, R, planes = link_update(torch, _lib, dv, fam, power, with_w=False)
    assert not torch.isnan(planes[:, :B].float()).any()
    assert bool(torch.isnan(planes[:, B:]).all())
    pf = planes[:, :B].float()
    total = (pf[0] + pf[1]) + pf[2]
    big = R.abs() >= 2.0 ** -100
    assert bool((total[big] == R[big]).all())
    assert bool(((total - R).abs()[~big] <= 2.0 ** -16 * R.abs()[~big]).all())
    assert bool((planes[:, :B, n:] == 0).all())
    for k in range(B):
        off = dv["M"][int(h["fm"][k])] == 0
        assert bool((planes[:, k][:, off] == 0).all()), k
    assert int(big.sum()) > 0
    if (fam, power) == (1, 1.0):                     # e^-80 < 2^-100: the lower range is met
        assert int((~big & (R != 0)).sum()) > 0
    sl = torch.from_numpy(C.SLOTS).cuda()
    rpos = torch.from_numpy(C.RPOS).cuda()
    e = dv["eta"].clone()
    Rp = torch.full((3 * C.BP * ld,), NAN, dtype=torch.bfloat16, device="cuda")
    _lib.call("sglm_link_update_rp", fam, power, n, ld, len(C.SLOTS), sl.data_ptr(), e.data_ptr(),
              *common(dv), None, None, Rp.data_ptr(), C.BP, rpos.data_ptr(), None, None, 0)
    assert torch.equal(bits(e), bits(dv["eta"]))
    got = Rp.view(3, C.BP, ld)
    written = np.zeros(C.BP, dtype=bool)
    for q, k in enumerate(C.SLOTS):
        if C.RPOS[q] >= 0:
            written[C.RPOS[q]] = True
            assert torch.equal(bits(got[:, int(C.RPOS[q])]), bits(planes[:, int(k)])), q
    for r in np.flatnonzero(~written):
        assert bool(torch.isnan(got[:, int(r)]).all()), r


def loss_trials(torch, _lib, dv, fam, power, slots, eta, deta, tv):
    """(out [rows][T] float64, dmax [rows] float32) of one sglm_loss_trials_max call."""
    n, ld = dv["n"], dv["ld"]
    T = int(tv.numel())
    rows = dv["B"] if slots is None else int(slots.numel())
    wk = torch.empty(_lib.query("sglm_rowsum_work_bytes", rows, 8, n), dtype=torch.uint8,
                     device="cuda")
    out = torch.full((rows * T,), NAN, dtype=torch.float64, device="cuda")
    dm = torch.full((rows,), NAN, dtype=torch.float32, device="cuda")
    _lib.call("sglm_loss_trials_max", fam, power, n, ld, rows, ptr(slots), eta.data_ptr(),
              deta.data_ptr(), *common(dv), tv.data_ptr(), T, out.data_ptr(), dm.data_ptr(),
              wk.data_ptr(), 0)
    return out.view(rows, T).cpu().numpy(), dm.cpu().numpy()


def check_dmax(h, dm):
    n = h["n"]
    for k in range(h["B"]):
        mk = h["M"][h["fm"][k], :n] > 0
        assert dm[k] == (np.max(np.abs(h["deta"][k, :n][mk])) if mk.any() else 0.0), k


GENERAL = [(f, p, "TV2") for f, p in C.FORMS] + [(0, 0.0, "TV1"), (1, 1.5, "TV1")]


@pytest.mark.parametrize("fam,power,steps", GENERAL,
                         ids=[f"f{f}-p{p:g}-{s}" for f, p, s in GENERAL])
def test_trial_losses_general_branch(engine, torch_mod, dev, fam, power, steps):
    """The general float64 branch (engine.TV2, T = 7; the first-round steps too where they take
    it) on the ordinary rows: |out[k][j] - ref| <= 64 eps64 S with S the sum of m times the
    absolute values of the parts of each term.  About 50 roundings of the running sum (32 serial
    adds per thread, an 8-level butterfly, 4 waves, 5 chunks) and about 12 eps for the term (a
    float64 exp of at most 2 ulp, argument and product roundings).  The reference takes the
    predictor eta + t deta and the terms in long double and sums them with fsum.  The fit on the
    extreme rows stays finite; dmax is numpy's float32 max of |deta| over the mask's rows; the
    slot-list call is bitwise the rows of the all-slot call."""
    torch = torch_mod
    from sglm_hip import _lib, engine as E
    h, dv = dev(fam, power)
    tvh = (E.TV2 if steps == "TV2" else C.TV1).astype(np.float32)
    assert tvh.size == (7 if steps == "TV2" else 5)
    tv = torch.from_numpy(tvh).cuda()
    out, dm = loss_trials(torch, _lib, dv, fam, power, None, dv["eta"], dv["deta"], tv)
    assert np.all(np.isfinite(out))
    check_dmax(h, dm)
    worst = 0.0
    for k in range(h["B"]):
        if h["fm"][k] == C.MASK_X:
            continue
        m, y, e, d = C.fit_rows(h, k, rows=C.N_ORD)
        for j, t in enumerate(tvh):
            r = C.reference(fam, power, y.astype(LD), e.astype(LD) + LD(t) * d.astype(LD), LD)
            ref = C.fsum(m * r["l"].astype(np.float64))
            bound = 64 * C.EPS64 * C.fsum(m * r["parts"].astype(np.float64))
            err = abs(out[k, j] - ref)
            if bound:
                worst = max(worst, err / bound)
            else:
                assert err == 0 and h["fm"][k] == C.MASK_EMPTY
    print(f"\n[tweedie rows] general branch ({fam}, {power}) {steps}: worst error / limit "
          f"{worst:.3f}")
    assert worst <= 1.0
    sl = torch.from_numpy(C.SLOTS).cuda()
    out2, dm2 = loss_trials(torch, _lib, dv, fam, power, sl, dv["eta"], dv["deta"], tv)
    assert np.array_equal(out2.view(np.int64), out[C.SLOTS].view(np.int64))
    assert np.array_equal(dm2, dm[C.SLOTS])


def test_poisson_differences_at_real_steps(engine, torch_mod, dev):
    """test_trial_losses_as_differences of tests/test_gpu_rowpass.py on this file's inputs (deta
    sd up to 2.5, eta sd up to 6, the multiplicity mask, the extreme rows), with that test's
    bound and argument: D_j = out[j] - out[0] within 4e-6 S_j + 4 eps64 |L0| of float64 numpy,
    S_j = sum m (mu |x_j| + |y t_j d|) (2-ulp expf / expm1f and three squarings that each at most
    double the relative error); out[0] within 1e-6 sum m (mu + |y eta|); dmax exact; the
    slot-list call bitwise the rows of the all-slot call.  With deta = 0 the five outputs of a
    fit are bitwise equal."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = dev(1, 1.0)
    tv = torch.from_numpy(C.TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, 1, 1.0, None, dv["eta"], dv["deta"], tv)
    assert np.all(np.isfinite(out))
    check_dmax(h, dm)
    worst = worst0 = 0.0
    for k in range(h["B"]):
        m, y, e, d = C.fit_rows(h, k)
        mu = np.exp(e)
        L0 = C.fsum(m * (mu - y * e))
        b0 = 1e-6 * C.fsum(m * (mu + np.abs(y * e)))
        if not b0:
            assert np.all(out[k] == 0) and h["fm"][k] == C.MASK_EMPTY
            continue
        worst0 = max(worst0, abs(out[k, 0] - L0) / b0)
        for j in range(1, 5):
            t = float(C.TV1[j])
            x = np.expm1(t * d)
            ref = C.fsum(m * (mu * x - y * t * d))
            S = C.fsum(m * (mu * np.abs(x) + np.abs(y * t * d)))
            worst = max(worst, abs((out[k, j] - out[k, 0]) - ref) / (4e-6 * S + 4 * C.EPS64 * abs(L0)))
    print(f"\n[tweedie rows] Poisson differences: worst error / limit {worst:.3f}; "
          f"L(0): {worst0:.3f}")
    assert worst <= 1.0 and worst0 <= 1.0
    sl = torch.from_numpy(C.SLOTS).cuda()
    out2, dm2 = loss_trials(torch, _lib, dv, 1, 1.0, sl, dv["eta"], dv["deta"], tv)
    assert np.array_equal(out2.view(np.int64), out[C.SLOTS].view(np.int64))
    assert np.array_equal(dm2, dm[C.SLOTS])
    outz, dmz = loss_trials(torch, _lib, dv, 1, 1.0, None, dv["eta"], torch.zeros_like(dv["deta"]),
                            tv)
    assert np.all(np.isfinite(outz))
    assert np.all((outz[:, 0] != 0) == (h["fm"] != C.MASK_EMPTY))
    assert np.array_equal(outz[:, 0].view(np.int64), out[:, 0].view(np.int64))
    for j in range(1, 5):
        assert np.array_equal(outz[:, j].view(np.int64), outz[:, 0].view(np.int64)), j
    assert np.all(dmz == 0)


@pytest.mark.parametrize("fam,power", C.FORMS, ids=IDS)
def test_score_sums(engine, torch_mod, dev, fam, power):
    """sglm_score_sums against float64 numpy on every row, the extreme set included:
    out[k][s][0] = sum m (y - mu)^2 and out[k][s][1] = sum m loss, each within
    64 eps64 sum m |parts| (relative to the parts: (y - mu)^2 reaches 3e69 at eta = 80); an
    unused set gives exactly 0."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = dev(fam, power)
    n, ld, B = h["n"], h["ld"], h["B"]
    wk = torch.full((_lib.query("sglm_rowsum_work_bytes", B, 4, n) // 8,), NAN,
                    dtype=torch.float64, device="cuda")
    out = torch.full((B, 4), NAN, dtype=torch.float64, device="cuda")
    _lib.call("sglm_score_sums", fam, power, n, ld, B, dv["eta"].data_ptr(), dv["Y"].data_ptr(),
              dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["sets"].data_ptr(), out.data_ptr(),
              wk.data_ptr(), 0)
    got = out.cpu().numpy().reshape(B, 2, 2)
    assert np.all(np.isfinite(got))
    worst = [0.0, 0.0]
    for k in range(B):
        _, y, e, _ = C.fit_rows(h, k)
        r = C.reference(fam, power, y, e)
        r2 = (y - r["mu"]) ** 2
        for s in range(2):
            ms = h["sets"][k, s]
            if ms < 0 or ms == C.MASK_EMPTY:
                assert got[k, s, 0] == 0 and got[k, s, 1] == 0
                continue
            m = h["M"][ms, :n].astype(np.float64)
            for q, (term, parts) in enumerate(((m * r2, m * r2), (m * r["l"], m * r["parts"]))):
                bound = 64 * C.EPS64 * C.fsum(parts)
                assert bound > 0
                worst[q] = max(worst[q], abs(got[k, s, q] - C.fsum(term)) / bound)
    print(f"\n[tweedie rows] score sums ({fam}, {power}): worst error / limit "
          f"{worst[0]:.3f} (squared residuals), {worst[1]:.3f} (loss)")
    assert max(worst) <= 1.0 and np.any(got[2, 0] != 0)


@pytest.mark.parametrize("fam,power", [(1, 1.5), (1, 1.2)], ids=["p1.5", "p1.2"])
def test_fused_trials_link_general_power(engine, torch_mod, dev, fam, power):
    """sglm_loss_trials_link at a general power: sums, dmax, undo, the new eta and the packed R
    planes bitwise those of sglm_loss_trials_max followed by sglm_link_update_rp at step 1 (the
    empty mask, the multiplicity mask and the extreme rows among the listed fits), and the
    link-alone call (out = dmax = NULL) gives the same eta, undo and planes."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = dev(fam, power)
    n, ld, B = h["n"], h["ld"], h["B"]
    ns = len(C.SLOTS)
    sl = torch.from_numpy(C.SLOTS).cuda()
    tv = torch.from_numpy(C.TV1).cuda()

    def bufs():
        return dict(e=dv["eta"].clone(),
                    out=torch.full((ns * 5,), NAN, dtype=torch.float64, device="cuda"),
                    dm=torch.full((ns,), NAN, dtype=torch.float32, device="cuda"),
                    Rp=torch.full((3 * C.BP * ld,), NAN, dtype=torch.bfloat16, device="cuda"),
                    undo=torch.full((ns, ld), NAN, dtype=torch.float32, device="cuda"),
                    wk=torch.empty(_lib.query("sglm_rowsum_work_bytes", ns, 8, n),
                                   dtype=torch.uint8, device="cuda"))
    a = bufs()
    _lib.call("sglm_loss_trials_max", fam, power, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              dv["deta"].data_ptr(), *common(dv), tv.data_ptr(), 5, a["out"].data_ptr(),
              a["dm"].data_ptr(), a["wk"].data_ptr(), 0)
    one = torch.ones(ns, dtype=torch.float32, device="cuda")
    rpos = torch.arange(ns, dtype=torch.int32, device="cuda")
    _lib.call("sglm_link_update_rp", fam, power, n, ld, ns, sl.data_ptr(), a["e"].data_ptr(),
              *common(dv), None, None, a["Rp"].data_ptr(), C.BP, rpos.data_ptr(), one.data_ptr(),
              dv["deta"].data_ptr(), 0)
    b = bufs()
    _lib.call("sglm_loss_trials_link", fam, power, n, ld, ns, sl.data_ptr(), b["e"].data_ptr(),
              dv["deta"].data_ptr(), *common(dv), tv.data_ptr(), 5, b["out"].data_ptr(),
              b["dm"].data_ptr(), b["undo"].data_ptr(), b["Rp"].data_ptr(), C.BP,
              b["wk"].data_ptr(), 0)
    c = bufs()
    _lib.call("sglm_loss_trials_link", fam, power, n, ld, ns, sl.data_ptr(), c["e"].data_ptr(),
              dv["deta"].data_ptr(), *common(dv), None, 0, None, None, c["undo"].data_ptr(),
              c["Rp"].data_ptr(), C.BP, None, 0)
    torch.cuda.synchronize()
    for x in (b, c):
        assert torch.equal(bits(x["e"]), bits(a["e"]))
        assert torch.equal(bits(x["Rp"]), bits(a["Rp"]))
        assert torch.equal(bits(x["undo"][:, :n]), bits(dv["eta"][sl.long(), :n]))
    assert bool(torch.isnan(c["out"]).all()) and bool(torch.isnan(c["dm"]).all())
    assert torch.equal(bits(b["out"]), bits(a["out"]))
    assert torch.equal(bits(b["dm"]), bits(a["dm"]))
    assert bool(torch.isfinite(b["out"]).all()) and float(b["dm"].min()) == 0.0
    assert float(b["dm"][3]) == 3.5 and float(b["dm"].max()) > 3.5
    listed = np.zeros(B, dtype=bool)
    listed[C.SLOTS] = True
    for k in range(B):
        assert torch.equal(bits(b["e"][k]), bits(dv["eta"][k])) != listed[k], k
    planes = b["Rp"].view(3, C.BP, ld)
    assert bool((planes[:, :ns, n:] == 0).all())             # the padding rows
    assert bool((planes[:, 2, :] == 0).all())                # the empty mask (SLOTS[2])
    assert bool(torch.isnan(planes[:, ns:, :]).all())        # packed rows beyond the list
    assert not torch.isnan(planes[:, :ns, :].float()).any()
    # R of the extreme rows at eta + deta, within the link's limits
    xk = int(C.SLOTS[3])
    ex = slice(C.N_ORD, n)
    r = ((planes[0, 3, ex].float() + planes[1, 3, ex].float()) + planes[2, 3, ex].float())
    z = b["e"][xk, ex].cpu().numpy().astype(np.float64)
    y = h["Y"][h["fr"][xk], ex].astype(np.float64)
    lg, _ = C.link_limits(fam, power, y, z)
    g64 = C.reference(fam, power, y, z)["g"]
    assert np.all(np.abs(g64) >= 2.0 ** -100)
    assert np.all(np.abs(r.cpu().numpy().astype(np.float64) - g64) <= lg)
