"""tests/tweedie_rows_cases.py held to account without a GPU: the references against centred
differences in long double, against each other in the limits p -> 1 and p -> 2 and against
oracle/glm_ref.py; the float32 emulation of the kernel's expression against the derived limits
(the proof that correct arithmetic passes them, and by how much); the properties of the inputs
that the GPU tests rely on."""
import numpy as np
import pytest

import tweedie_rows_cases as C

LD = np.longdouble


def sample_rows(fam, power, count=300):
    """(y, eta) float64 of a few hundred rows of the case: a stride through every fit's ordinary
    rows and all the extreme ones."""
    h = C.inputs(fam, power)
    ys, es = [], []
    for k in range(h["B"]):
        _, y, e, _ = C.fit_rows(h, k)
        idx = np.arange(k, C.N_ORD, C.N_ORD // (count // h["B"]))
        ys += [y[idx], y[C.N_ORD:]]
        es += [e[idx], e[C.N_ORD:]]
    return np.concatenate(ys), np.concatenate(es)


def part_magnitudes(fam, power, y, eta, order):
    """Sum of the magnitudes of the parts of the loss's ``order``-th derivative (long double)."""
    r = C.reference(fam, power, y, eta, dtype=LD)
    if fam == 0:
        return np.abs(LD(eta)) + np.abs(LD(y)) + 1
    p = LD(C.p64(power))
    if p == 1:
        return r["A"] + np.abs(LD(y))
    if p == 2:
        return 1 + r["Bq"]
    return (2 - p) ** (order - 1) * r["A"] + np.abs(1 - p) ** (order - 1) * r["Bq"]


@pytest.mark.parametrize("fam,power", C.FORMS)
def test_reference_derivatives(fam, power):
    """g and h are the centred differences of l and of g in long double: step 2^-20, 1e-9 of the
    magnitudes of the parts (a wrong (2-p) or (1-p) factor in the oracle is an error of order
    1)."""
    y, eta = sample_rows(fam, power)
    assert eta.size >= 300 + 12 * C.N_X - 12 and np.max(np.abs(eta)) == 80.0
    hs = LD(2.0) ** -20
    y, eta = y.astype(LD), eta.astype(LD)
    up, dn = C.reference(fam, power, y, eta + hs, LD), C.reference(fam, power, y, eta - hs, LD)
    mid = C.reference(fam, power, y, eta, LD)
    dg = (up["l"] - dn["l"]) / (2 * hs)
    dh = (up["g"] - dn["g"]) / (2 * hs)
    rg = np.max(np.abs(dg - mid["g"]) / part_magnitudes(fam, power, y, eta, 1))
    rh = np.max(np.abs(dh - mid["h"]) / part_magnitudes(fam, power, y, eta, 2))
    print(f"form ({fam}, {power}): centred differences off by {float(rg):.2e} (g), "
          f"{float(rh):.2e} (h) of the parts")
    assert rg <= 1e-9 and rh <= 1e-9
    # the float64 reference is the long double one to float64 rounding of its parts
    r64 = C.reference(fam, power, y.astype(np.float64), eta.astype(np.float64))
    for key, order in (("g", 1), ("h", 2)):
        err = np.abs(r64[key].astype(LD) - mid[key]) / part_magnitudes(fam, power, y, eta, order)
        assert np.max(err) <= 256 * C.EPS64, key


@pytest.mark.parametrize("p_near,power", [(1.0 + 1e-6, 1.0), (1.0 - 1e-6, 1.0),
                                          (2.0 - 1e-6, 2.0), (2.0 + 1e-6, 2.0)])
def test_general_power_tends_to_poisson_and_gamma(p_near, power):
    """g and h of the general form at p = 1 +- 1e-6 and 2 +- 1e-6 are the Poisson and Gamma
    forms within 1e-5 of the magnitudes of the parts (ordinary rows with |eta| <= 8: the
    difference grows like 1e-6 |eta|)."""
    y, eta = sample_rows(1, power)
    keep = np.abs(eta) <= 8
    y, eta = y[keep].astype(LD), eta[keep].astype(LD)
    assert y.size >= 100
    lim = C.reference(1, power, y, eta, LD)
    p = LD(p_near)
    a, q = np.exp((2 - p) * eta), y * np.exp((1 - p) * eta)
    g, hh = a - q, (2 - p) * a - (1 - p) * q
    scale = np.exp(eta) + y * np.exp(-eta) + y + 1
    assert np.max(np.abs(g - lim["g"]) / scale) <= 1e-5
    assert np.max(np.abs(hh - lim["h"]) / scale) <= 1e-5


@pytest.mark.parametrize("fam,power", C.FORMS)
def test_reference_matches_oracle_half_loss(fam, power):
    """oracle/glm_ref.half_loss exposes the loss (without its y-only constant) and both
    derivatives: the references here are those, at the float32-rounded power, so the constant
    by which the two losses may differ is 0."""
    from oracle import glm_ref
    y, eta = sample_rows(fam, power)
    l, g, hh = glm_ref.half_loss(C.p64(power) if fam else 0, bool(fam), y, eta)
    r = C.reference(fam, power, y, eta)
    for got, key in ((l, "l"), (g, "g"), (hh, "h")):
        assert np.max(np.abs(got - r[key]) / (r["parts"] + r["A"] + r["Bq"] + 1)) <= 64 * C.EPS64


@pytest.mark.parametrize("fam,power", C.FORMS)
def test_emulation_stays_inside_the_limits(fam, power):
    """The float32 restatement of half_loss (exp2 of the float32-rounded x log2 e, each
    exponential pushed one ulp either way) on every row of the case stays at or below 0.75 of
    the limits: correct arithmetic passes them.  The squared loss is exact."""
    h = C.inputs(fam, power)
    worst_g = worst_h = 0.0
    for k in range(h["B"]):
        _, y, e, _ = C.fit_rows(h, k)
        y32, e32 = y.astype(np.float32), e.astype(np.float32)
        ref = C.reference(fam, power, y, e)
        if fam == 0:
            g, w = C.emulate_link(fam, power, y32, e32)
            assert np.array_equal(g, (e32 - y32)) and np.all(w == 1)
            assert np.max(np.abs(g - ref["g"]) / np.maximum(np.abs(ref["g"]), 1e-300)) <= C.U
            continue
        lg, lh = C.link_limits(fam, power, y, e)
        general = C.p64(power) not in (1.0, 2.0)
        for na in (-1, 0, 1):
            for nb in ((-1, 0, 1) if general else (0,)):
                with np.errstate(over="raise", invalid="raise"):
                    g, w = C.emulate_link(fam, power, y32, e32, na, nb)
                worst_g = max(worst_g, np.max(np.abs(g - ref["g"]) / lg))
                bad = lh == 0
                assert np.all(w[bad] == 0)
                worst_h = max(worst_h, np.max(np.abs(w - ref["h"])[~bad] / lh[~bad]))
    print(f"form ({fam}, {power}): emulation / limit {worst_g:.3f} (g), {worst_h:.3f} (h)")
    assert worst_g <= 0.75 and worst_h <= 0.75


def test_case_properties():
    """What the GPU tests rely on: n % 4 != 0 and five chunks; the 0.8-density mask has a
    whole-zero aligned quad in the first and in the last chunk; the multiplicity mask holds a 2;
    ordinary rows with |eta| > 20; every float32 reference value on the extreme rows finite; the
    listed slots use the five masks; Gamma's responses positive."""
    for gamma in (False, True):
        h = C.make_inputs(gamma)
        n, ld = h["n"], h["ld"]
        assert n == C.N == 40026 and n % 4 and (n + C.CHUNK - 1) // C.CHUNK == 5
        assert ld == C.pad256(n) and ld % 256 == 0 and ld > n
        quads = h["M"][0, :n - n % 4].reshape(-1, 4).max(axis=1) == 0
        first, last = C.CHUNK // 4, 4 * C.CHUNK // 4
        assert quads[:first].any() and quads[last:].any()
        assert h["M"][0, :C.N_ORD].mean() > 0.75
        assert h["M"][C.MASK_MULT].max() == 2 and np.all(h["M"][C.MASK_EMPTY] == 0)
        assert np.all(h["M"][C.MASK_X, :C.N_ORD] == 0) and np.all(h["M"][C.MASK_X, C.N_ORD:n])
        assert np.all(h["M"][:, n:] == 0) and np.all(h["Y"][:, n:] == 0)
        assert list(h["fm"][C.SLOTS]) == [0, 1, C.MASK_EMPTY, C.MASK_X, C.MASK_MULT]
        assert np.sum(np.abs(h["eta"][:, :C.N_ORD]) > 20) >= 1
        assert np.max(np.abs(h["eta"][:, :C.N_ORD])) < 44
        assert np.max(np.abs(h["deta"][:, :C.N_ORD])) > 8
        assert np.all(h["Y"][:, :n] >= (0.25 if gamma else 0.0))
        assert list(h["sets"][2]) == [C.MASK_X, C.MASK_MULT] and list(h["sets"][1]) == [-1, -1]
        ex = slice(C.N_ORD, n)
        assert sorted(set(np.abs(h["eta"][0, ex]).tolist())) == [0.0, 20.0, 44.0, 80.0]
        assert np.signbit(h["eta"][0, ex]).sum() == 12
        for fam, power in C.FORMS:
            if C.is_gamma(fam, power) != gamma:
                continue
            for k in range(h["B"]):
                _, y, e, d = C.fit_rows(h, k)
                for z in (e[ex], (e + d)[ex]) if k == C.SLOTS[3] else (e[ex],):
                    r = C.reference(fam, power, y[ex], z)
                    with np.errstate(over="raise"):
                        for key in ("g", "h", "l"):
                            assert np.all(np.isfinite((2 * r[key]).astype(np.float32))), key
