"""Inputs, float64 references and derived error limits of the IRLS row passes at the squared loss
and the log-link Tweedie losses (power 1: Poisson, power 2: Gamma, a general power), CPU only
(numpy).  Shared by tests/test_tweedie_rows_cpu.py, which holds this module to account, and
tests/test_gpu_tweedie_rows.py, which holds the kernels of csrc/api.hip to it.

Inputs, as tests/test_gpu_binomial_kernels.py builds them: N_ORD = 40002 ordinary rows (not a
multiple of 4, five 8192-row chunks) and 24 appended extreme rows (eta in {+-0, +-20, +-44,
+-80}, each with y in {0, 1, 5}; {0.25, 1, 5} for Gamma, which needs y > 0) that only mask
MASK_X selects; 12 fits, two responses (a lag design's Poisson counts and their roll by 7;
max(y, 0.25) for Gamma) and five masks: 0.8 density with all-zero aligned 4-row blocks, full,
empty, the extreme rows, multiplicities 0 / 1 / 2.  eta's sd per fit cycles over {0.5, 1.5, 4, 6}
around minus that, deta's over {0.1, 1, 2.5}.

References, per row, on the float32 inputs widened to float64, p = float(float32(power)):
    squared    g = eta - y          h = 1                           l = (eta - y)^2 / 2
    power 1    g = mu - y           h = mu                          l = mu - y eta
    power 2    g = 1 - y e^-eta     h = y e^-eta                    l = eta + y e^-eta
    general    g = a - y b          h = (2-p) a - (1-p) y b         l = a/(2-p) - y b/(1-p)
               a = e^((2-p) eta), b = e^((1-p) eta)

Limits of the float32 link (link_limits), derived, not measured.  u = 2^-24, and one fast
exponential e^x = v_exp_f32(x log2 e) carries the relative error delta(x) = (2 |x| + 4) u: the
float32 rounding of x log2 e and of the rounded constant (|x| u each in the result), a 1-ulp
v_exp_f32 and one slack ulp.  With A = a and Bq = y b (power 1: A = mu, no Bq; power 2: no A,
b = e^-eta, unit factors), eA = delta((2-p) eta) A and eB = (delta((1-p) eta) + u) Bq:
    |g - g64| <= 2 [eA + eB + u |g64|]
    |h - h64| <= 2 [(2-p)(eA + u A) + |1-p|(eB + u Bq) + u |h64|]
    Poisson: 2 [delta(eta) mu + u |g64|], 2 delta(eta) mu
    Gamma:   2 [(delta(eta) + u) Bq + u |g64|], 2 (delta(eta) + u) Bq
times the row's multiplicity; the factor 2 is the margin over the model.  emulate_link restates
the kernel's float32 expression on the CPU (exp2 of the float32-rounded x log2 e, pushed one ulp
either way): the CPU test holds it below 0.75 of every limit on these rows."""
import math
from functools import lru_cache

import numpy as np

FORMS = [(0, 0.0), (1, 1.0), (1, 2.0), (1, 1.5), (1, 1.2)]
CHUNK = 8192                      # rows per block partial (csrc/api.hip, kRowChunk)
N_ORD = 40002
ETA_X = np.array([0.0, -0.0, 20.0, -20.0, 44.0, -44.0, 80.0, -80.0], dtype=np.float32)
Y_X = np.array([0.0, 1.0, 5.0], dtype=np.float32)
Y_X_GAMMA = np.array([0.25, 1.0, 5.0], dtype=np.float32)
DETA_X = np.array([-3.5, 0.0, 3.5], dtype=np.float32)
N_X = ETA_X.size * Y_X.size
N = N_ORD + N_X
B = 12
SLOTS = np.array([3, 11, 0, 7, 8], dtype=np.int32)
RPOS = np.array([2, -1, 0, 1, 3], dtype=np.int32)
TV1 = np.array([0.0, 1.0, 0.5, 0.25, 0.125], dtype=np.float32)
BP = 32
MASK_EMPTY, MASK_X, MASK_MULT = 2, 3, 4
ZERO_QUADS = (0, 400, 2 * CHUNK - 8, 3 * CHUNK, N_ORD - N_ORD % 4 - 24)
U = 2.0 ** -24
EPS64 = float(np.finfo(np.float64).eps)
LOG2E_F32 = np.float32(1.4426950408889634)


def pad256(n):
    return (n + 255) // 256 * 256


def is_gamma(fam, power):
    return fam == 1 and power == 2.0


def p64(power):
    """The power as the C ABI carries it: rounded to float32 once."""
    return float(np.float32(power))


@lru_cache(maxsize=None)
def make_inputs(gamma=False, seed=172):
    """Host arrays of the batch (read-only); ``gamma``: the responses raised to >= 0.25."""
    from sglm_hip import synth
    s = synth.make(N=N_ORD, m=12, L=4, rho=0.08, seed=71)
    n, no = N, N_ORD
    ld = pad256(n)
    rng = np.random.default_rng(seed)
    Y = np.zeros((2, ld), np.float32)
    Y[0, :no] = s.y
    Y[1, :no] = np.roll(s.y, 7)
    yx = Y_X_GAMMA if gamma else Y_X
    Y[0, no:n] = np.tile(yx, ETA_X.size)
    Y[1, no:n] = np.tile(np.roll(yx, 1), ETA_X.size)
    if gamma:
        Y[:, :n] = np.maximum(Y[:, :n], np.float32(0.25))
    M = np.zeros((5, ld), np.uint8)
    m0 = (rng.random(no) < 0.8).astype(np.uint8)
    for i0 in ZERO_QUADS:
        m0[i0:i0 + 16] = 0                     # aligned blocks of four rows, all zero
    M[0, :no] = m0
    M[1, :no] = 1
    M[MASK_X, no:n] = 1                        # MASK_EMPTY stays empty
    M[MASK_MULT, :no] = rng.integers(0, 3, no)
    fr = rng.integers(0, 2, B).astype(np.int32)
    fm = rng.choice([0, 1, MASK_MULT], B).astype(np.int32)
    fm[SLOTS] = [0, 1, MASK_EMPTY, MASK_X, MASK_MULT]
    eta = np.zeros((B, ld), np.float32)
    deta = np.zeros((B, ld), np.float32)
    esd = np.array([0.5, 1.5, 4.0, 6.0])[np.arange(B) % 4]
    dsd = np.array([0.1, 1.0, 2.5])[np.arange(B) % 3]
    eta[:, :no] = rng.normal(-1.0, 1.0, (B, no)) * esd[:, None]
    deta[:, :no] = rng.normal(0.0, 1.0, (B, no)) * dsd[:, None]
    eta[:, no:n] = np.repeat(ETA_X, Y_X.size)[None, :]
    ix = np.arange(N_X)
    deta[:, no:n] = DETA_X[(ix + ix // Y_X.size) % DETA_X.size][None, :]
    step = (0.25 + 0.75 * rng.random(B)).astype(np.float32)
    sets = rng.choice([-1, 0, 1, MASK_MULT], (B, 2)).astype(np.int32)
    sets[0] = [0, 1]
    sets[1] = [-1, -1]
    sets[2] = [MASK_X, MASK_MULT]
    h = dict(n=n, ld=ld, B=B, Y=Y, M=M, fr=fr, fm=fm, eta=eta, deta=deta, step=step, sets=sets)
    for v in h.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return h


def inputs(fam, power):
    return make_inputs(is_gamma(fam, power))


def fit_rows(h, k, eta=None, rows=None):
    """float64 (m, y, eta, deta) of fit k over the rows i < ``rows`` (default: every row)."""
    r = h["n"] if rows is None else rows
    e = h["eta"] if eta is None else eta
    return (h["M"][h["fm"][k], :r].astype(np.float64), h["Y"][h["fr"][k], :r].astype(np.float64),
            e[k, :r].astype(np.float64), h["deta"][k, :r].astype(np.float64))


# ------------------------------------------------------------------------------ references
def reference(fam, power, y, eta, dtype=np.float64):
    """dict(g, h, l, mu, A, Bq, parts) per row in ``dtype`` (float64 or longdouble).  A and Bq
    are the two exponential parts the limits are written in; ``parts`` is the sum of the absolute
    values of the loss's parts."""
    y = np.asarray(y, dtype=dtype)
    eta = np.asarray(eta, dtype=dtype)
    zero = np.zeros_like(eta)
    if fam == 0:
        r = eta - y
        return dict(g=r, h=np.ones_like(eta), l=0.5 * r * r, mu=eta, A=zero, Bq=zero,
                    parts=0.5 * r * r)
    p = dtype(p64(power))
    mu = np.exp(eta)
    if p == 1:
        return dict(g=mu - y, h=mu, l=mu - y * eta, mu=mu, A=mu, Bq=zero,
                    parts=mu + np.abs(y * eta))
    if p == 2:
        q = y * np.exp(-eta)
        return dict(g=1 - q, h=q, l=eta + q, mu=mu, A=zero, Bq=q, parts=np.abs(eta) + q)
    a = np.exp((2 - p) * eta)
    q = y * np.exp((1 - p) * eta)
    return dict(g=a - q, h=(2 - p) * a - (1 - p) * q, l=a / (2 - p) - q / (1 - p), mu=mu, A=a,
                Bq=q, parts=a / (2 - p) + q / abs(1 - p))


def delta(x):
    """Relative error of one fast float32 exponential at the argument x."""
    return (2.0 * np.abs(x) + 4.0) * U


def link_limits(fam, power, y, eta):
    """(limit of |g - g64|, limit of |h - h64|) per row at multiplicity 1; None for the squared
    loss, whose outputs are exact float32 expressions."""
    if fam == 0:
        return None
    ref = reference(fam, power, y, eta)
    A, Bq, g, h = ref["A"], ref["Bq"], np.abs(ref["g"]), np.abs(ref["h"])
    p = p64(power)
    if p == 1:
        return 2 * (delta(eta) * A + U * g), 2 * delta(eta) * A
    if p == 2:
        return 2 * ((delta(eta) + U) * Bq + U * g), 2 * (delta(eta) + U) * Bq
    eA = delta((2 - p) * eta) * A
    eB = (delta((1 - p) * eta) + U) * Bq
    return (2 * (eA + eB + U * g),
            2 * ((2 - p) * (eA + U * A) + abs(1 - p) * (eB + U * Bq) + U * h))


def fast_exp32(x, nudge):
    """float32 exp2 of the float32-rounded x log2 e, moved ``nudge`` (-1, 0, 1) ulp."""
    x = np.asarray(x, dtype=np.float32)
    t = (x * LOG2E_F32).astype(np.float32)
    r = np.exp2(t.astype(np.float64)).astype(np.float32)
    if nudge:
        r = np.nextafter(r, np.float32(np.inf if nudge > 0 else -np.inf))
    return r


def emulate_link(fam, power, y, eta, nudge=0, nudge_b=0):
    """(g, h) float32 as half_loss of csrc/common.h forms them, one float32 rounding per
    operation, on float32 y and eta; ``nudge`` moves the first exponential by that many ulp,
    ``nudge_b`` the general power's second one."""
    y = np.asarray(y, dtype=np.float32)
    eta = np.asarray(eta, dtype=np.float32)
    p = np.float32(power)
    one, two = np.float32(1), np.float32(2)
    if fam == 0:
        return eta - y, np.ones_like(eta)
    if p == 1:
        mu = fast_exp32(eta, nudge)
        return mu - y, mu
    if p == 2:
        q = y * fast_exp32(-eta, nudge)
        return one - q, q
    a = fast_exp32((two - p) * eta, nudge)
    b = fast_exp32((one - p) * eta, nudge_b)
    return a - y * b, (two - p) * a - (one - p) * y * b


def fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel())
