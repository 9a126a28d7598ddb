"""The mixed-block kernels of csrc/mixed.hip against np.longdouble sums of the same terms, called
directly through the C ABI at the shapes where their tiling, chunking, tails and encodings take
another path (k = 2 at n = 12000, all the rest of the suite has, takes one path through each),
then through ``Design`` at k = 5 and k = 80 and two fits at k = 5.

Inputs, references and the derived bounds are in tests/mixed_cases.py; its CPU checks are in
tests/test_mixed_cases_cpu.py.  Every float64 reduction: |got - ref| <= (m + 8) 2^-53 sum|term|
per output (m rows); the predictor: 2^-24 |ref| + (k + 9) 2^-53 sum|term| per element; the f32
products of sglm_mixed_wc and the f32 roundings of sglm_mixed_to_h bitwise.  Each test prints its
worst error / bound ("Mixed-block kernels against float64").
"""
import numpy as np
import pytest

import mixed_cases as mc
from oracle import glm_ref

pytestmark = pytest.mark.gpu
TOL_POIS, TOL_GAUSS = 1e-4, 1e-5
SENT = mc.SENT


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def bits(a):
    """The bit patterns of a float array (bitwise comparisons, NaN-safe)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def dev(torch, a):
    """Device copy of a numpy array (bf16 bit patterns travel as int16)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def work_with_guard(torch, nbytes):
    """float64 tensor of the queried work size followed by a 4 KiB guard, all sentinel."""
    assert nbytes % 8 == 0
    return torch.full(((nbytes + mc.GUARD) // 8,), SENT, dtype=torch.float64, device="cuda")


def guard_intact(work, nbytes):
    g = work[nbytes // 8:].cpu().numpy()
    return g.size == mc.GUARD // 8 and np.array_equal(bits(g), bits(np.full_like(g, SENT)))


# ------------------------------------------------------------------------------ sglm_mixed_gram
@pytest.mark.parametrize("n,k,wmode", mc.GRAM_CASES)
def test_mixed_gram(engine, torch_mod, n, k, wmode):
    """Pair tiles 1 / 8 + 7 / 5 x 8 + 5, one chunk and three (the last of 5 rows), f32 weights and
    uint8 multiplicities selected by wsel: both orders bitwise equal and inside the bound, nothing
    else of S written, the partial sums inside the queried work size."""
    torch = torch_mod
    from sglm_hip import _lib
    c = mc.gram_case(n, k, wmode)
    ns, P, npairs = mc.GRAM_NS, mc.P, c["npairs"]
    C, W = dev(torch, c["C"]), dev(torch, c["W"])
    wsel = dev(torch, np.array(mc.GRAM_WSEL, np.int32))
    cpos, pg = dev(torch, c["cpos"]), dev(torch, c["pg"])
    S = torch.full((ns, k, P), SENT, dtype=torch.float64, device="cuda")
    wb = _lib.query("sglm_mixed_work_bytes", ns, k, n)
    work = work_with_guard(torch, wb)
    _lib.call("sglm_mixed_gram", wmode, W.data_ptr(), c["ldw"], wsel.data_ptr(), ns, C.data_ptr(),
              c["ldc"], k, n, cpos.data_ptr(), P, pg.data_ptr(), S.data_ptr(), work.data_ptr(), 0)
    torch.cuda.synchronize()
    Sh = S.cpu().numpy()
    a, b = c["pg"][:npairs], c["pg"][npairs:]
    up, lo = Sh[:, a, c["cpos"][b]], Sh[:, b, c["cpos"][a]]              # [ns][npairs]
    assert np.array_equal(bits(up), bits(lo))
    r = mc.ratio(up, c["ref"], c["bound"])
    print(f"RATIO gram n={n} k={k} wmode={wmode}: {r:.3e}")
    assert r <= 1.0
    other = np.setdiff1d(np.arange(P), c["cpos"])
    assert np.array_equal(bits(Sh[:, :, other]), bits(np.full((ns, k, other.size), SENT)))
    assert guard_intact(work, wb)


# ------------------------------------------------------------------------------ sglm_mixed_xtr
def _xtr_call(torch, c, ldr=None):
    from sglm_hip import _lib
    n, k, nq, P = c["n"], c["k"], c["nq"], mc.P
    C, R = dev(torch, c["C"]), dev(torch, c["R"])
    rsel, gsl = dev(torch, c["rsel"]), dev(torch, c["gslots"])
    cpos, px = dev(torch, c["cpos"]), dev(torch, c["px"])
    g = torch.full((mc.XTR_GROWS, P), SENT, dtype=torch.float64, device="cuda")
    wb = _lib.query("sglm_mixed_work_bytes", nq, k, n)       # the size Design.mix_xtr requests
    work = work_with_guard(torch, wb)
    _lib.call("sglm_mixed_xtr", c["mode"], R.data_ptr(), c["ldr"] if ldr is None else ldr,
              mc.XTR_BP if c["mode"] == 2 else 0, rsel.data_ptr(), gsl.data_ptr(), nq,
              C.data_ptr(), c["ldc"], k, n, cpos.data_ptr(), P, px.data_ptr(), g.data_ptr(),
              work.data_ptr(), 0)
    torch.cuda.synchronize()
    return g.cpu().numpy(), work, wb


@pytest.mark.parametrize("mode,n,k,nq,indep", mc.XTR_CASES)
def test_mixed_xtr(engine, torch_mod, mode, n, k, nq, indep):
    """f32 rows, the three packed bf16 pieces (Bp = 16 > nq; successive roundings of an f32 R and,
    once, three independent planes) and one bf16 plane; column tiles 1 / 4 + 1, fit groups 1 /
    8 + 3, one chunk of 3 rows and two chunks (32768 + 1027 rows: a full sweep, then 3 rows),
    rows of R chosen by rsel, rows of g by gslots.  Finite junk in rows n .. ldr of R must not
    reach g; nothing else of g is written."""
    c = mc.xtr_case(mode, n, k, nq, indep)
    gh, work, wb = _xtr_call(torch_mod, c)
    got = gh[np.ix_(c["gslots"], c["cpos"])]
    r = mc.ratio(got, c["ref"], c["bound"])
    print(f"RATIO xtr mode={mode} n={n} k={k} nq={nq} indep={int(indep)}: {r:.3e}")
    assert r <= 1.0
    keep = np.ones(gh.shape, bool)
    keep[np.ix_(c["gslots"], c["cpos"])] = False
    assert np.array_equal(bits(gh[keep]), bits(np.full(int(keep.sum()), SENT)))
    assert guard_intact(work, wb)


def test_mixed_xtr_rejects_unaligned_stride(engine, torch_mod):
    from sglm_hip import _lib
    c = mc.xtr_case(0, 3, 1, 1, False)
    with pytest.raises(_lib.HipEngineError):
        _xtr_call(torch_mod, c, ldr=c["ldr"] - 1)            # 7 >= n, not a multiple of 4


# ------------------------------------------------------------------------------ sglm_mixed_eta
@pytest.mark.parametrize("name", [c[0] for c in mc.ETA_CASES])
def test_mixed_eta(engine, torch_mod, name):
    """The grouped kernel with its LDS table to the edge (k = 64), fit groups 8 + 3, the 4-row
    tail (n = 16389) and a capped grid (1024 fits: 16 blocks for 17 row tiles); the one-row
    fallback by k = 65 and by a row stride of 16391.  eta starts random (the add is checked);
    rows n .. ld of every slot and all unlisted slots stay bitwise as they were."""
    torch = torch_mod
    from sglm_hip import _lib
    c = mc.eta_case(name)
    C, beta, eta = dev(torch, c["C"]), dev(torch, c["beta"]), dev(torch, c["eta0"])
    cpos, slots = dev(torch, c["cpos"]), dev(torch, c["slots"])
    _lib.call("sglm_mixed_eta", C.data_ptr(), c["ldc"], c["k"], c["n"], cpos.data_ptr(),
              beta.data_ptr(), mc.P, slots.data_ptr(), c["nb"], eta.data_ptr(), c["ld"], 0)
    torch.cuda.synchronize()
    got = eta.cpu().numpy()
    r = mc.eta_ratio(c, got)
    print(f"RATIO eta {name}: {r:.3e}")
    assert r <= 1.0
    assert np.array_equal(bits(got[:, c["n"]:]), bits(c["eta0"][:, c["n"]:]))
    other = np.setdiff1d(np.arange(c["rows"]), c["slots"])
    assert np.array_equal(bits(got[other]), bits(c["eta0"][other]))
    assert not np.array_equal(got[c["slots"], :c["n"]], c["eta0"][c["slots"], :c["n"]])


def test_mixed_eta_rejects_k_1025(engine, torch_mod):
    torch = torch_mod
    from sglm_hip import _lib
    k = 1025
    C = torch.zeros((k, 4), dtype=torch.float64, device="cuda")
    cpos = torch.arange(k, dtype=torch.int32, device="cuda")
    beta = torch.zeros((1, 2048), dtype=torch.float32, device="cuda")
    eta = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.HipEngineError):
        _lib.call("sglm_mixed_eta", C.data_ptr(), 4, k, 1, cpos.data_ptr(), beta.data_ptr(), 2048,
                  None, 1, eta.data_ptr(), 4, 0)


# ------------------------------------------------------------------------------ wc, to_h
def test_mixed_wc_bitwise(engine, torch_mod):
    """R[s * k + c] = f32(W[slots[s]]) * f32(C[c]) bitwise for r < n, exactly +0.0 on rows
    n .. ld although W and C hold junk there."""
    torch = torch_mod
    from sglm_hip import _lib
    rng = np.random.default_rng(15)
    ns, k, n, ld, ldw, ldc = 3, 5, 1000, 1280, 1536, 1288
    slots = np.array([4, 0, 2], np.int32)
    W = mc.signed_mags(rng, (5, ldw)).astype(np.float32)
    C = mc.signed_mags(rng, (k, ldc))
    R = torch.full((ns * k, ld), SENT, dtype=torch.float32, device="cuda")
    Wd, Cd, sd = dev(torch, W), dev(torch, C), dev(torch, slots)
    _lib.call("sglm_mixed_wc", Wd.data_ptr(), ldw, sd.data_ptr(), ns, Cd.data_ptr(), ldc, k, n, ld,
              R.data_ptr(), 0)
    torch.cuda.synchronize()
    got = R.cpu().numpy().reshape(ns, k, ld)
    ref = np.zeros((ns, k, ld), np.float32)
    ref[:, :, :n] = W[slots][:, None, :n] * C[:, :n].astype(np.float32)[None]
    assert np.array_equal(bits(got), bits(ref))


def test_mixed_to_h_bitwise(engine, torch_mod):
    """Rows and columns cpos of H[slots[s]] = f32(S[s]) in both orders (P = 512: two blocks of
    columns), every other entry and slot of H untouched."""
    torch = torch_mod
    from sglm_hip import _lib
    rng = np.random.default_rng(16)
    P, k, ns = 512, 5, 2
    slots = np.array([3, 1], np.int32)
    cpos = np.array([300, 3, 511, 4, 130], np.int32)
    S = mc.signed_mags(rng, (ns, k, P))
    iu = np.triu_indices(k, 1)
    S[:, iu[1], cpos[iu[0]]] = S[:, iu[0], cpos[iu[1]]]       # symmetric inside the block
    H = torch.full((5, P, P), SENT, dtype=torch.float32, device="cuda")
    Sd, cd, sd = dev(torch, S), dev(torch, cpos), dev(torch, slots)
    _lib.call("sglm_mixed_to_h", Sd.data_ptr(), ns, k, P, cd.data_ptr(), sd.data_ptr(),
              H.data_ptr(), 0)
    torch.cuda.synchronize()
    ref = np.full((5, P, P), SENT, np.float32)
    for s, slot in enumerate(slots):
        for c in range(k):
            ref[slot, :, cpos[c]] = S[s, c].astype(np.float32)
            ref[slot, cpos[c], :] = S[s, c].astype(np.float32)
    assert np.array_equal(bits(H.cpu().numpy()), bits(ref))


# ------------------------------------------------------------------------------ through Design
@pytest.mark.parametrize("k", [5, 80])
def test_design_products(engine, torch_mod, k):
    """from_host on 9003 rows of 12 0/1 columns and k continuous ones at scattered positions;
    X beta (11 of 16 slots; k = 80 through the fallback predictor kernel), X^T R of 11 rows, the
    weighted and the exact Gram rows and their copy into a sentinel H, against float64 numpy at
    the bars of test_gpu_mixed.test_mixed_split_and_products."""
    torch = torch_mod
    c = mc.design_case(k)
    X, N, p, cp = c["X"], c["n"], c["p"], c["cpos"]
    d = engine.Design.from_host(X)
    assert d.k == k and np.array_equal(np.asarray(d.cpos), cp) and d.xbits is not None
    assert np.array_equal(d.cont[:, :N].cpu().numpy(), X[:, cp].T)
    assert not d.cont[:, N:].any()
    Xa = np.hstack([X, np.ones((N, 1))])
    rng = np.random.default_rng(17)
    # eta
    beta = np.zeros((16, d.P), np.float32)
    beta[:, :p + 1] = rng.normal(0, 1, (16, p + 1))
    slots = rng.permutation(16)[:11].astype(np.int32)
    out = torch.full((16, d.ld), SENT, dtype=torch.float32, device="cuda")
    d.eta(dev(torch, beta), out=out, slots=dev(torch, slots))
    eta = out.cpu().numpy()
    ref = beta[slots][:, :p + 1].astype(np.float64) @ Xa.T
    assert np.max(np.abs(eta[slots, :N] - ref)) < 1e-6 * np.max(np.abs(ref))
    other = np.setdiff1d(np.arange(16), slots)
    assert np.array_equal(bits(eta[other]), bits(np.full((other.size, d.ld), SENT, np.float32)))
    # X^T R
    B = 11
    R = np.zeros((B, d.ld), np.float32)
    R[:, :N] = rng.normal(0, 1, (B, N))
    G = torch.empty((B, d.P), dtype=torch.float64, device="cuda")
    d.xtr(dev(torch, R), B, G)
    Gh = G.cpu().numpy()
    ref = R[:, :N].astype(np.float64) @ Xa
    assert np.max(np.abs(Gh[:, :p + 1] - ref)) < 1e-6 * np.max(np.abs(ref))
    assert np.max(np.abs(Gh[:, cp] - ref[:, cp])) < 1e-12 * np.max(np.abs(ref[:, cp]))
    # Gram rows of the continuous columns: exact (mask multiplicities), weighted (f32 weights)
    M = np.zeros((2, d.ld), np.uint8)
    M[0, :N] = 1
    M[1, :N] = rng.integers(0, 3, N)
    S = d.mix_gram_rows(M=dev(torch, M), mrows=[0, 1]).cpu().numpy()
    for s in range(2):
        ref = (Xa * M[s, :N, None]).T @ X[:, cp]
        assert np.max(np.abs(S[s][:, :p + 1] - ref.T)) < 1e-11 * np.max(np.abs(ref))
    W = np.zeros((3, d.ld), np.float32)
    W[:, :N] = rng.random((3, N))
    Sd = d.mix_gram_rows(W=dev(torch, W), wslots=[2, 0])
    S = Sd.cpu().numpy()
    for s, slot in enumerate((2, 0)):
        ref = (Xa * W[slot, :N, None].astype(np.float64)).T @ X[:, cp]
        assert np.max(np.abs(S[s][:, :p + 1] - ref.T)) < 1e-6 * np.max(np.abs(ref))
    # into the f32 Hessians of slots 2 and 0 of three
    H = torch.full((3, d.P, d.P), SENT, dtype=torch.float32, device="cuda")
    d.mix_to_h(Sd, [2, 0], H)
    href = np.full((3, d.P, d.P), SENT, np.float32)
    for s, slot in enumerate((2, 0)):
        for j, col in enumerate(cp):
            href[slot, :, col] = S[s, j].astype(np.float32)
            href[slot, col, :] = S[s, j].astype(np.float32)
    assert np.array_equal(bits(H.cpu().numpy()), bits(href))


def test_design_fits_k5(engine):
    """OLS and a ridge-penalised Poisson fit of the k = 5 design through the drop-in GLM against
    the float64 oracle (1e-5 / 1e-4, as tests/test_gpu_mixed.py)."""
    import sglm
    c = mc.design_case(5)
    X = c["X"]
    glm = sglm.GLM("Normal", alpha=0.0)
    glm.fit(X, c["y"])
    w, b = glm_ref.fit_ols(X, c["y"])
    assert rel(glm.model.coef_, w) < TOL_GAUSS
    assert abs(glm.model.intercept_ - b) < TOL_GAUSS * max(1.0, abs(b))
    glm = sglm.GLM("Poisson", alpha=1e-3)
    glm.fit(X, c["ypois"])
    w, b = glm_ref.fit_tweedie_newton(X, c["ypois"], 1e-3, 1.0)
    assert rel(glm.model.coef_, w) < TOL_POIS
    assert abs(glm.model.intercept_ - b) < TOL_POIS * max(1.0, abs(b))
