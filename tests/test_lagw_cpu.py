"""Host-side figures of the event-structured Gram (engine._lagw_exec_flop): the MFMA work the
launch issues covers the structured products (the H entries' own terms) and does not shrink with the fit
count; no GPU needed."""
import numpy as np


class _Lag:
    def __init__(self, m, K, cnt):
        self.m, self.K, self.cnt = m, K, np.asarray(cnt)


def test_exec_flop_covers_the_algorithmic_products():
    from sglm_hip import engine as E
    rng = np.random.default_rng(0)
    for m, K in ((50, 40), (13, 10), (7, 41), (40, 12)):
        lg = _Lag(m, K, rng.integers(100, 30000, m))
        prev = 0.0
        for nact in (1, 2, 5, 14):
            ex = E._lagw_exec_flop(lg, nact)
            alg = E._lagw_alg_flop1(m, K, lg.cnt) * nact
            assert ex >= alg, (m, K, nact, ex, alg)   # the kernel's own decomposition, padded
            # every H entry of the upper triangle once: (mK(mK+1)/2 + mK) entries, each summing
            # the occurrences of one of its two events (equal counts: exactly that many terms)
            flat = E._lagw_alg_flop1(m, K, np.full(m, 7))
            pl = m * K
            assert flat == 2.0 * 7 * (pl * (pl + 1) // 2 + pl)
            assert ex >= prev                                    # 32-column tiles: flat inside one
            prev = ex
        assert E._lagw_exec_flop(lg, 5) == lg.exec_flop[5]    # memoised per launch size


def _work_bytes1(n_raw, K, P):
    """sglm_lag_gram_w_work_bytes(n_raw, K, 1, P) (csrc/lagw.hip: 8 weight copies of lagw_wlen
    2-byte elements, 128 f32 partial sums, rounded to 256, and one P x P f32 image)."""
    wlen = ((n_raw + 2 * K + 16) + 512 + 7) // 8 * 8
    return (8 * wlen * 2 + 128 * 4 + 255) // 256 * 256 + P * P * 4


def test_chunk_stays_within_the_32_bit_offsets():
    """engine._lagw_chunk: the fits of one sglm_lag_gram_w launch are bounded by the scratch
    budget and by the launch's 32-bit weight offsets (the call refuses wlen >= 2^27): at 2 M raw
    rows an unbounded budget no longer asks for a launch the kernel refuses, and within the
    default budget the choice is the budget's alone."""
    from sglm_hip import engine as E
    n_raw, K, nact, P = 2_000_000, 40, 200, 2048
    per1 = _work_bytes1(n_raw, K, P)
    chunk = E._lagw_chunk(n_raw, K, nact, per1, float(1 << 40))
    assert 1 <= chunk <= nact
    assert (n_raw + 2 * K + 16) * chunk + 519 < 1 << 27
    assert (n_raw + 2 * K + 16) * (chunk + 1) + 519 >= 1 << 27       # and no smaller than needed
    # one fit per launch is the floor, whatever the budget
    assert E._lagw_chunk(n_raw, K, nact, per1, 1.0) == 1
    assert E._lagw_chunk((1 << 27), K, nact, _work_bytes1(1 << 27, K, P), float(1 << 40)) == 1
    budget = float(2 << 30)                                           # LAGW_WORK_BUDGET's default
    for n_raw, K, nact, P in ((2_000_000, 40, 200, 2048), (1_000_039, 40, 120, 2048),
                              (6000, 12, 7, 256), (3000, 96, 29, 256), (50_000_000, 40, 9, 2048),
                              (100_000_000, 1, 5, 256), (20000, 40, 1, 2048)):
        per1 = _work_bytes1(n_raw, K, P)
        assert E._lagw_chunk(n_raw, K, nact, per1, budget) == \
            max(1, min(nact, int(budget // max(1, per1)))), (n_raw, K, nact)
