"""The elementwise row passes of an IRLS step and the small reductions behind them:
the link without stored weights and the weights on demand, the Poisson trial losses summed as
differences, the wave-per-row chunk sums, the grouped pair distances and the score sums."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
CHUNK = 8192                      # rows per block partial (csrc/api.hip, kRowChunk)
N = 40002                         # not a multiple of 4; five row chunks
SLOTS = np.array([3, 11, 0, 7, 8], dtype=np.int32)
TV1 = np.array([0.0, 1.0, 0.5, 0.25, 0.125], dtype=np.float32)
PAIRS = [(0, 1), (1, 2), (2, 3), (5, 4), (6, 4), (7, 4), (9, 8), (1, 0)]
SCORE_FAMILIES = [(1, 1.0), (1, 2.0), (0, 0.0)]
SCORE_N2 = CHUNK + 1021           # two chunks: every summation order of two terms agrees
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowpass_score.npz")


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def pad256(n):
    return (n + 255) // 256 * 256


def make_inputs(n=N, B=12, seed=72):
    """Host arrays of one batch: two responses from a lag design's Poisson counts, a 0.8-density
    mask whose zero rows include whole aligned 4-row blocks, a full mask and an empty one."""
    from sglm_hip import synth
    s = synth.make(N=n, m=12, L=4, rho=0.08, seed=71)
    n = int(s.N)
    ld = pad256(n)
    rng = np.random.default_rng(seed)
    Y = np.zeros((2, ld), np.float32)
    Y[0, :n] = s.y
    Y[1, :n] = np.roll(s.y, 7)
    M = np.zeros((3, ld), np.uint8)
    m0 = (rng.random(n) < 0.8).astype(np.uint8)
    for i0 in (0, 400, 2 * CHUNK - 8, 3 * CHUNK, n - n % 4 - 24):
        m0[i0:i0 + 16] = 0                     # aligned blocks of four rows, all zero
    M[0, :n] = m0
    M[1, :n] = 1
    fr = rng.integers(0, 2, B).astype(np.int32)
    fm = rng.integers(0, 2, B).astype(np.int32)
    fm[:4] = [0, 0, 1, 1]
    eta = np.zeros((B, ld), np.float32)
    eta[:, :n] = rng.normal(-1.0, 0.5, (B, n))
    deta = np.zeros((B, ld), np.float32)
    deta[:, :n] = rng.normal(0, 0.1, (B, n))
    step = rng.random(B).astype(np.float32)
    sets = rng.integers(-1, 2, (B, 2)).astype(np.int32)
    sets[0] = [0, 1]
    sets[1] = [-1, -1]
    return dict(n=n, ld=ld, B=B, Y=Y, M=M, fr=fr, fm=fm, eta=eta, deta=deta, step=step, sets=sets)


def to_dev(torch, h):
    return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v)
            for k, v in h.items()}


@pytest.fixture(scope="module")
def inp(torch_mod):
    h = make_inputs()
    return h, to_dev(torch_mod, h)


def loss_trials(torch, _lib, dv, n, ld, B, slots, eta, deta, tv, with_max=True):
    """(out [rows][T] float64, dmax [rows] float32 or None) of one trial-loss call."""
    T = int(tv.numel())
    rows = B if slots is None else int(slots.numel())
    wk = torch.empty(_lib.query("sglm_rowsum_work_bytes", rows, 8, n), dtype=torch.uint8,
                     device="cuda")
    out = torch.full((rows * T,), float("nan"), dtype=torch.float64, device="cuda")
    sp = None if slots is None else slots.data_ptr()
    if with_max:
        dm = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.call("sglm_loss_trials_max", 1, 1.0, n, ld, rows, sp, eta.data_ptr(),
                  deta.data_ptr(), dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(),
                  dv["fm"].data_ptr(), tv.data_ptr(), T, out.data_ptr(), dm.data_ptr(),
                  wk.data_ptr(), 0)
        return out.view(rows, T).cpu().numpy(), dm.cpu().numpy()
    _lib.call("sglm_loss_trials", 1, 1.0, n, ld, rows, sp, eta.data_ptr(), deta.data_ptr(),
              dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr(),
              tv.data_ptr(), T, out.data_ptr(), wk.data_ptr(), 0)
    return out.view(rows, T).cpu().numpy(), None


def fit_rows(h, k):
    """float64 (m, y, eta, deta) of fit k over the rows i < n."""
    n = h["n"]
    return (h["M"][h["fm"][k], :n].astype(np.float64), h["Y"][h["fr"][k], :n].astype(np.float64),
            h["eta"][k, :n].astype(np.float64), h["deta"][k, :n].astype(np.float64))


def general_branch_error(torch, _lib, h, dv):
    """Largest |out - float64 reference| / sum m (exp(eta + t d) + |y (eta + t d)|) of the
    seven second-round trial steps (the kernel's general float64 branch)."""
    from sglm_hip import engine
    tv = engine.TV2.astype(np.float32)
    out, _ = loss_trials(torch, _lib, dv, h["n"], h["ld"], h["B"], None, dv["eta"], dv["deta"],
                         torch.from_numpy(tv).cuda(), with_max=False)
    worst = 0.0
    for k in range(h["B"]):
        m, y, e, d = fit_rows(h, k)
        for j, t in enumerate(tv.astype(np.float64)):
            z = e + t * d
            ref = math.fsum(m * (np.exp(z) - y * z))
            scale = math.fsum(m * (np.exp(z) + np.abs(y * z)))
            worst = max(worst, abs(out[k, j] - ref) / scale)
    return worst


def score_call(torch, _lib, dv, fam, power, n, ld, B):
    """(block partials [B][4][chunks], out [B][4]) of one sglm_score_sums call."""
    nc = (n + CHUNK - 1) // CHUNK
    wk = torch.zeros(_lib.query("sglm_rowsum_work_bytes", B, 4, n) // 8, dtype=torch.float64,
                     device="cuda")
    out = torch.full((B, 4), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("sglm_score_sums", fam, float(power), n, ld, B, dv["eta"].data_ptr(),
              dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["sets"].data_ptr(),
              out.data_ptr(), wk.data_ptr(), 0)
    return wk[: B * 4 * nc].view(B, 4, nc).cpu().numpy(), out.cpu().numpy()


def score_golden_arrays(torch, _lib):
    """What tests/golden/rowpass_score.npz holds (recorded once with the library as it was before
    the exponential of the Poisson score was shared and the chunk sums went to one wave per row)."""
    h = make_inputs()
    dv = to_dev(torch, h)
    arrs = {}
    for fam, power in SCORE_FAMILIES:
        tag = f"f{fam}_p{power:g}"
        arrs[tag + "_part"], arrs[tag + "_out"] = score_call(torch, _lib, dv, fam, power, h["n"],
                                                             h["ld"], h["B"])
        _, arrs[tag + "_out2"] = score_call(torch, _lib, dv, fam, power, SCORE_N2, h["ld"],
                                            h["B"])
    return arrs


@pytest.mark.parametrize("fam,power", [(1, 1.0), (1, 2.0), (1, 1.5), (0, 0.0)])
def test_link_without_w_and_weights_on_demand(engine, torch_mod, inp, fam, power):
    """W = NULL leaves eta and R / Rp bitwise what the call with W gives (fused predictor update
    included); sglm_link_weights on the resulting eta is bitwise the W that call wrote, rows
    n..ld are 0 and unlisted slots are not touched."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
    sl = torch.from_numpy(SLOTS).cuda()
    ns = len(SLOTS)
    st = dv["step"][:ns].contiguous()

    def link(with_w):
        e = dv["eta"].clone()
        W = torch.full_like(e, float("nan")) if with_w else None
        R = torch.full_like(e, float("nan"))
        Rp = torch.zeros(3 * 32 * ld, dtype=torch.bfloat16, device="cuda")
        _lib.call("sglm_link_update", fam, power, n, ld, ns, sl.data_ptr(), e.data_ptr(),
                  dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(),
                  dv["fm"].data_ptr(), None if W is None else W.data_ptr(), R.data_ptr(),
                  Rp.data_ptr(), st.data_ptr(), dv["deta"].data_ptr(), 0)
        return e, W, R, Rp
    e1, W1, R1, Rp1 = link(True)
    e0, _, R0, Rp0 = link(False)
    assert torch.equal(e0, e1)
    assert not torch.equal(e1, dv["eta"])                   # the predictor update took place
    assert torch.equal(R0[sl.long()], R1[sl.long()]) and torch.equal(Rp0, Rp1)
    W2 = torch.full_like(e0, float("nan"))
    _lib.call("sglm_link_weights", fam, power, n, ld, ns, sl.data_ptr(), e0.data_ptr(),
              dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr(),
              W2.data_ptr(), 0)
    listed = np.zeros(B, dtype=bool)
    listed[SLOTS] = True
    for k in range(B):
        if listed[k]:
            assert torch.equal(W2[k], W1[k]), k
            assert torch.all(W2[k, n:] == 0) and not torch.isnan(W2[k]).any(), k
        else:
            assert torch.isnan(W2[k]).all() and torch.isnan(W1[k]).all(), k
    assert float(W2[int(SLOTS[0]), :n].abs().max()) > 0
    # sglm_link_update_rp without W: packed rows at the given positions, as with W
    rpos = torch.from_numpy(np.array([2, -1, 0, 1, 3], dtype=np.int32)).cuda()

    def link_rp(with_w):
        e = dv["eta"].clone()
        W = torch.full_like(e, float("nan")) if with_w else None
        Rp = torch.zeros(3 * 32 * ld, dtype=torch.bfloat16, device="cuda")
        _lib.call("sglm_link_update_rp", fam, power, n, ld, ns, sl.data_ptr(), e.data_ptr(),
                  dv["Y"].data_ptr(), dv["M"].data_ptr(), dv["fr"].data_ptr(),
                  dv["fm"].data_ptr(), None if W is None else W.data_ptr(), None, Rp.data_ptr(),
                  32, rpos.data_ptr(), st.data_ptr(), dv["deta"].data_ptr(), 0)
        return e, W, Rp
    e3, W3, Rp3 = link_rp(True)
    e4, _, Rp4 = link_rp(False)
    assert torch.equal(e3, e4) and torch.equal(Rp3, Rp4) and torch.equal(e3, e1)
    assert torch.equal(W3[sl.long()], W1[sl.long()])
    # all slots (slots = NULL)
    W5 = torch.full_like(e0, float("nan"))
    _lib.call("sglm_link_weights", fam, power, n, ld, B, None, e0.data_ptr(), dv["Y"].data_ptr(),
              dv["M"].data_ptr(), dv["fr"].data_ptr(), dv["fm"].data_ptr(), W5.data_ptr(), 0)
    assert torch.equal(W5[sl.long()], W1[sl.long()]) and not torch.isnan(W5).any()


def test_trial_losses_as_differences(engine, torch_mod, inp):
    """Poisson halving branch: D_j = out[j] - out[0] against float64 numpy on the same f32
    inputs within 4e-6 S_j + 4 eps64 |L0|, S_j = sum m (mu |x_j| + |y t_j d|) (2-ulp expf /
    expm1f and three squarings that each double the relative error, about 1.3e-6, times the
    usual 3); out[0] within 1e-6 sum m (mu + |y eta|); dmax exact; the slot-list call bitwise
    the rows of the all-slot call."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld, B = h["n"], h["ld"], h["B"]
    tv = torch.from_numpy(TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, n, ld, B, None, dv["eta"], dv["deta"], tv)
    worst = worst0 = 0.0
    for k in range(B):
        m, y, e, d = fit_rows(h, k)
        mu = np.exp(e)
        L0 = math.fsum(m * (mu - y * e))
        b0 = 1e-6 * math.fsum(m * (mu + np.abs(y * e)))
        worst0 = max(worst0, abs(out[k, 0] - L0) / b0)
        for j in range(1, 5):
            t = float(TV1[j])
            x = np.expm1(t * d)
            ref = math.fsum(m * (mu * x - y * t * d))
            S = math.fsum(m * (mu * np.abs(x) + np.abs(y * t * d)))
            worst = max(worst, abs((out[k, j] - out[k, 0]) - ref) / (4e-6 * S + 4 * EPS64 * abs(L0)))
        assert dm[k] == np.max(np.abs(h["deta"][k, :n][h["M"][h["fm"][k], :n] > 0])), k
    print(f"trial differences: worst error / bound {worst:.3f}; L(0): {worst0:.3f}")
    assert worst <= 1.0 and worst0 <= 1.0
    sl = torch.from_numpy(SLOTS).cuda()
    out2, dm2 = loss_trials(torch, _lib, dv, n, ld, B, sl, dv["eta"], dv["deta"], tv)
    assert np.array_equal(out2, out[SLOTS]) and np.array_equal(dm2, dm[SLOTS])


def test_trial_losses_zero_step_bitwise(engine, torch_mod, inp):
    """With deta == 0 the five outputs of a fit are bitwise equal."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    tv = torch.from_numpy(TV1).cuda()
    out, dm = loss_trials(torch, _lib, dv, h["n"], h["ld"], h["B"], None, dv["eta"],
                          torch.zeros_like(dv["deta"]), tv)
    assert np.all(np.isfinite(out)) and np.all(out[:, 0] != 0)
    for j in range(1, 5):
        assert np.array_equal(out[:, j].view(np.int64), out[:, 0].view(np.int64)), j
    assert np.all(dm == 0)


# the largest error of the library before this file's changes on these inputs (one MI355X run,
# relative to sum m (exp(eta + t d) + |y (eta + t d)|) as general_branch_error measures it)
GENERAL_BRANCH_PARENT_ERR = 2.3532406933311805e-16


def test_trial_losses_general_branch(engine, torch_mod, inp):
    """T = 7 (the general float64 branch) equals float64 numpy at twice the error the library
    had before the row-pass changes on the same inputs: 2.353e-16 of sum m (exp(eta + t d) +
    |y (eta + t d)|), measured once on an MI355X (GENERAL_BRANCH_PARENT_ERR); with the chunk sums
    one wave per row the same run gave 1.484e-16."""
    from sglm_hip import _lib
    h, dv = inp
    err = general_branch_error(torch_mod, _lib, h, dv)
    print(f"general branch: error {err:.3e} (parent {GENERAL_BRANCH_PARENT_ERR})")
    assert err <= 2 * GENERAL_BRANCH_PARENT_ERR


@pytest.mark.parametrize("n", [3 * CHUNK + 5, 65 * CHUNK + 3])
def test_chunk_sums_fixed_order(engine, torch_mod, n):
    """The chunk sums behind sglm_loss_trials at fewer and at more than 64 chunks: each equals
    math.fsum of the per-row float64 terms within n eps64 sum |term|, and is bitwise itself over
    two calls."""
    torch = torch_mod
    from sglm_hip import _lib
    rng = np.random.default_rng(n)
    ld, B = pad256(n), 2
    h = dict(n=n, ld=ld, B=B, Y=np.zeros((1, ld), np.float32), M=np.zeros((1, ld), np.uint8),
             fr=np.zeros(B, np.int32), fm=np.zeros(B, np.int32),
             eta=np.zeros((B, ld), np.float32), deta=np.zeros((B, ld), np.float32))
    h["Y"][0, :n] = rng.poisson(0.4, n)
    h["M"][0, :n] = rng.random(n) < 0.8
    h["eta"][:, :n] = rng.normal(-1.0, 0.5, (B, n))
    h["deta"][:, :n] = rng.normal(0, 0.1, (B, n))
    dv = to_dev(torch, h)
    tvh = np.array([0.0, 0.75], dtype=np.float32)           # T = 2: float64 row terms
    tv = torch.from_numpy(tvh).cuda()
    out, _ = loss_trials(torch, _lib, dv, n, ld, B, None, dv["eta"], dv["deta"], tv, False)
    again, _ = loss_trials(torch, _lib, dv, n, ld, B, None, dv["eta"], dv["deta"], tv, False)
    assert np.array_equal(out.view(np.int64), again.view(np.int64))
    for k in range(B):
        m, y, e, d = fit_rows(h, k)
        for j, t in enumerate(tvh.astype(np.float64)):
            z = e + t * d
            term = m * (np.exp(z) - y * z)
            ref, scale = math.fsum(term), math.fsum(np.abs(term))
            print(f"n={n} fit {k} trial {j}: error {abs(out[k, j] - ref):.3e}, "
                  f"bound {n * EPS64 * scale:.3e}")
            assert abs(out[k, j] - ref) <= n * EPS64 * scale, (k, j)


@pytest.mark.parametrize("npairs", [8, 7, 5, 1])
def test_pair_distances_grouped(engine, torch_mod, inp, npairs):
    """Pairs that share a fit with their neighbour, under mixed masks, at lengths that are and
    are not multiples of the group: each distance is bitwise numpy's float32 max |a - b| over
    the rows of fit a's mask; an all-zero mask gives 0."""
    torch = torch_mod
    from sglm_hip import _lib
    h, dv = inp
    n, ld = h["n"], h["ld"]
    fm = np.array([0, 0, 1, 1, 0, 1, 0, 0, 2, 2, 0, 0], dtype=np.int32)   # mask 2 is all zero
    pairs = np.array(PAIRS[:npairs], dtype=np.int32)
    out = torch.full((npairs,), float("nan"), dtype=torch.float32, device="cuda")
    pairs_d, fm_d = torch.from_numpy(pairs).cuda(), torch.from_numpy(fm).cuda()
    _lib.call("sglm_eta_pair_absmax", n, ld, npairs, pairs_d.data_ptr(), dv["M"].data_ptr(),
              fm_d.data_ptr(), dv["eta"].data_ptr(), out.data_ptr(), 0)
    got = out.cpu().numpy()
    for q, (a, b) in enumerate(pairs):
        rows = h["M"][fm[a], :n] > 0
        diff = np.abs(h["eta"][a, :n] - h["eta"][b, :n])[rows]
        ref = np.float32(diff.max()) if diff.size else np.float32(0)
        assert got[q].view(np.int32) == ref.view(np.int32), (q, a, b, got[q], ref)
        if fm[a] == 2:
            assert got[q] == 0


@pytest.mark.parametrize("fam,power", SCORE_FAMILIES)
def test_score_sums_match_recorded_values(engine, torch_mod, inp, fam, power):
    """sglm_score_sums against the values the library gave before the Poisson exponential was
    shared between mu and the loss (tests/golden/rowpass_score.npz): the block partials bitwise
    at every chunk, the sums bitwise where a fit has two chunks (one order of summation), and
    at five chunks within chunks * eps64 * sum |partial| of the recorded sequential sum."""
    from sglm_hip import _lib
    h, dv = inp
    g = np.load(GOLDEN)
    tag = f"f{fam}_p{power:g}"
    part, out = score_call(torch_mod, _lib, dv, fam, power, h["n"], h["ld"], h["B"])
    assert np.array_equal(part.view(np.int64), g[tag + "_part"].view(np.int64))
    _, out2 = score_call(torch_mod, _lib, dv, fam, power, SCORE_N2, h["ld"], h["B"])
    assert np.array_equal(out2.view(np.int64), g[tag + "_out2"].view(np.int64))
    bound = part.shape[2] * EPS64 * np.abs(part).sum(axis=2)
    assert np.all(np.abs(out - g[tag + "_out"]) <= bound)
    assert np.any(out != 0)
