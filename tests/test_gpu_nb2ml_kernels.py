"""The two row passes of csrc/nb2ml.hip on the MI355X: sglm_count_hist against np.bincount
(exactly) and sglm_nb2_kappa_sums against the longdouble oracle of tests/nb2ml_cases.py on the same
f32 inputs.

n = 8192 + 37 rows: one 8192-row chunk boundary is crossed and the last quad of rows is partial.
The histogram keeps bins below 1024 in LDS and sends higher counts straight to global atomics; one
response stays below 7, the other has counts up to about 1500, on both sides of that split."""
import numpy as np
import pytest

import nb2ml_cases as mc

pytestmark = pytest.mark.gpu

N = 8192 + 37
LDS_BINS = 1024                        # kLdsBins of csrc/nb2ml.hip
KAPPAS = np.array([2.0 ** -20, 2.0 ** -16, 0.25, 8.0, 2.0 ** 10])
SLOTS = np.array([2, 0, 5], dtype=np.int32)
BAR = 1e-12                            # the fixed-order float64 sums of test_gpu_tweedie_enet.py


def pad256(n):
    return (n + 255) // 256 * 256


def masks():
    rng = np.random.default_rng(11)
    M = rng.integers(0, 4, (3, N)).astype(np.uint8)         # multiplicities 0..3
    M[0, 4096:4096 + 64] = 0                                # whole quads left out
    M[:, -5:] = 0                                           # rows no mask holds (see the flags)
    return M


def counts():
    rng = np.random.default_rng(12)
    y0 = rng.integers(0, 7, N).astype(np.float64)
    y1 = rng.poisson(3.0, N).astype(np.float64)
    big = rng.choice(N - 5, 40, replace=False)
    y1[big] = rng.integers(900, 1500, 40)
    y1[big[0]], y1[big[1]] = 1023.0, 1024.0                 # both sides of the LDS / global split
    return np.stack([y0, y1])


def hist_call(torch, lib, M, Y, nbins):
    Md = torch.from_numpy(M).cuda()
    Yd = torch.from_numpy(Y).cuda()
    F, R = M.shape[0], Y.shape[0]
    hist = torch.full((R, F, nbins), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((R, F), -1, dtype=torch.int32, device="cuda")
    lib.call("sglm_count_hist", Md.data_ptr(), M.shape[1], F, Yd.data_ptr(), R, Y.shape[1],
             nbins, hist.data_ptr(), flags.data_ptr(), None)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), flags.cpu().numpy()


def test_count_hist_equals_bincount(engine):
    import torch
    from sglm_hip import _lib
    M, Y = masks(), counts()
    nbins = int(Y.max()) + 1
    assert Y[1].max() >= LDS_BINS > Y[0].max()
    hist, flags = hist_call(torch, _lib, M, Y, nbins)
    for r in range(2):
        for f in range(3):
            ref = np.bincount(Y[r].astype(np.int64), weights=M[f].astype(np.float64),
                              minlength=nbins).astype(np.int64)
            assert np.array_equal(hist[r, f], ref), (r, f)
    assert not flags.any()
    again, flags2 = hist_call(torch, _lib, M, Y, nbins)
    assert again.tobytes() == hist.tobytes() and flags2.tobytes() == flags.tobytes()


def test_count_hist_flags(engine):
    """A non-integer, a negative and a >= nbins value on a row some mask holds set that
    (response, mask)'s flag and are not counted; on the rows every mask leaves out they do not."""
    import torch
    from sglm_hip import _lib
    M, Y0 = masks(), counts()
    nbins = int(Y0.max()) + 1
    M[:, 100:103] = 0
    for bad in (2.5, -1.0, float(nbins), np.nan):
        Y = Y0.copy()
        Y[:, -5:] = bad                                     # left out by every mask
        Y[0, 100] = bad                                     # left out too
        _, flags = hist_call(torch, _lib, M, Y, nbins)
        assert not flags.any(), bad
        M1 = M.copy()
        M1[1, 100] = 2                                      # held by mask 1 alone
        hist, flags = hist_call(torch, _lib, M1, Y, nbins)
        assert flags.tolist() == [[0, 1, 0], [0, 0, 0]], bad
        ok = np.ones(N, bool)
        ok[100] = False
        ref = np.bincount(Y[0][ok & (M1[1] > 0)].astype(np.int64),
                          weights=M1[1][ok & (M1[1] > 0)].astype(np.float64), minlength=nbins)
        assert np.array_equal(hist[0, 1], ref.astype(np.int64))


def sums_inputs():
    rng = np.random.default_rng(13)
    ld = pad256(N)
    eta = np.full((6, ld), np.nan, dtype=np.float32)        # slots 1, 3, 4 stay NaN: unread
    for s in SLOTS:
        eta[s, :N] = rng.uniform(-30.0, 30.0, N).astype(np.float32)
        eta[s, 10:14] = np.array([80.0, -80.0, 200.0, -200.0], dtype=np.float32)
        eta[s, 8200:8204] = np.array([-200.0, 200.0, -80.0, 80.0], dtype=np.float32)
    Yc = counts()
    Y = np.zeros((2, ld), dtype=np.float32)
    Y[:, :N] = Yc
    Y[:, N:] = np.nan                                       # the padding is not read
    M = np.zeros((3, ld), dtype=np.uint8)
    M[:, :N] = masks()
    M[:, 10:14] = 1
    M[:, 8200:8204] = 2
    fit_resp = np.array([0, 1, 1], dtype=np.int32)
    fit_mask = np.array([1, 0, 2], dtype=np.int32)
    kap = np.tile(KAPPAS, (3, 1))
    return ld, eta, Y, M, fit_resp, fit_mask, kap


def sums_call(torch, lib, ld, eta, Y, M, fit_resp, fit_mask, kap):
    dev = [torch.from_numpy(a).cuda() for a in (SLOTS, eta, Y, M, fit_resp, fit_mask, kap)]
    nfit, K = kap.shape
    out = torch.full((nfit, K, 3), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(lib.query("sglm_nb2_kappa_sums_work_bytes", nfit, K, N),
                       dtype=torch.uint8, device="cuda")
    lib.call("sglm_nb2_kappa_sums", N, ld, nfit, dev[0].data_ptr(), dev[1].data_ptr(),
             dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(),
             dev[6].data_ptr(), K, out.data_ptr(), work.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_kappa_sums_against_longdouble(engine):
    """|got - ref| <= 1e-12 sum m |term| per output, the terms those of the cancellation-free
    form: y eta and (y + 1/k) log1p(k mu) for [0]; mu^2 g and y mu / (1 + k mu) for [1].  The
    third sum only steers the search: it is checked against a central difference of [1]."""
    import torch
    from sglm_hip import _lib
    args = sums_inputs()
    ld, eta, Y, M, fit_resp, fit_mask, kap = args
    out = sums_call(torch, _lib, *args)
    assert np.all(np.isfinite(out))
    worst = np.zeros((KAPPAS.size, 2))
    for f in range(3):
        e = eta[SLOTS[f], :N]
        y = Y[fit_resp[f], :N]
        m = M[fit_mask[f], :N]
        keep = m > 0
        for k, kappa in enumerate(KAPPAS):
            ref, mag = mc.eta_sums(kappa, y[keep], e[keep], m[keep])
            for q in range(2):
                ratio = abs(float(np.longdouble(out[f, k, q]) - ref[q])) / float(mag[q])
                worst[k, q] = max(worst[k, q], ratio)
            h = 1e-5 * kappa
            fd = (mc.eta_sums(kappa + h, y[keep], e[keep], m[keep])[0][1]
                  - mc.eta_sums(kappa - h, y[keep], e[keep], m[keep])[0][1]) / (2 * h)
            assert abs(out[f, k, 2] - float(fd)) <= 1e-6 * abs(float(fd)) + 1e-9 * float(
                mag[1]) / kappa, (f, kappa)
    for k, kappa in enumerate(KAPPAS):
        print(f"kappa = {kappa:.6g}: worst |got - ref| / sum m |term| = {worst[k, 0]:.3g} "
              f"(likelihood sum), {worst[k, 1]:.3g} (score sum); bar {BAR:g}")
    assert np.all(worst <= BAR)
    again = sums_call(torch, _lib, *args)
    assert again.tobytes() == out.tobytes()


def test_kappa_sums_k1_and_null_slots(engine):
    """K = 1 (the search's later passes: another instantiation of the kernel, so the compiler's
    contractions may differ in the last bit) meets the same bar as the K = 5 call; slots = NULL
    (launch row f reads slot f) gives the K = 5 call's bits."""
    import torch
    from sglm_hip import _lib
    ld, eta, Y, M, fit_resp, fit_mask, kap = sums_inputs()
    full = sums_call(torch, _lib, ld, eta, Y, M, fit_resp, fit_mask, kap)
    one = sums_call(torch, _lib, ld, eta, Y, M, fit_resp, fit_mask,
                    np.ascontiguousarray(kap[:, 2:3]))
    assert np.all(np.isfinite(one))
    for f in range(3):
        keep = M[fit_mask[f], :N] > 0
        ref, mag = mc.eta_sums(KAPPAS[2], Y[fit_resp[f], :N][keep], eta[SLOTS[f], :N][keep],
                               M[fit_mask[f], :N][keep])
        for q in range(2):
            assert abs(float(np.longdouble(one[f, 0, q]) - ref[q])) <= BAR * float(mag[q])
        assert abs(one[f, 0, 2] - full[f, 2, 2]) <= 1e-12 * abs(full[f, 2, 2])
    dense = np.ascontiguousarray(eta[SLOTS])
    dev = [torch.from_numpy(a).cuda() for a in (dense, Y, M, fit_resp, fit_mask, kap)]
    out = torch.empty((3, KAPPAS.size, 3), dtype=torch.float64, device="cuda")
    work = torch.empty(_lib.query("sglm_nb2_kappa_sums_work_bytes", 3, KAPPAS.size, N),
                       dtype=torch.uint8, device="cuda")
    _lib.call("sglm_nb2_kappa_sums", N, ld, 3, None, dev[0].data_ptr(), dev[1].data_ptr(),
              dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(),
              KAPPAS.size, out.data_ptr(), work.data_ptr(), None)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == full.tobytes()


def test_bad_arguments_are_refused(engine):
    import torch
    from sglm_hip import _lib
    ld, eta, Y, M, fit_resp, fit_mask, kap = sums_inputs()
    big = np.tile(KAPPAS[:1], (3, 9))
    with pytest.raises(_lib.HipEngineError, match="sglm_nb2_kappa_sums"):
        sums_call(torch, _lib, ld, eta, Y, M, fit_resp, fit_mask, big)
    with pytest.raises(_lib.HipEngineError, match="sglm_count_hist"):
        hist_call(torch, _lib, masks(), counts(), 0)
