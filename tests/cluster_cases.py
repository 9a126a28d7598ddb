"""Cases and the numpy oracle of the cluster-robust covariance tests.  No engine
code.  The families, the lagged design, the draws, the score residuals and the longdouble inverse
are those of tests/infer_cases.py; the oracle is

    C = kappa A^-1 (sum_c g_c g_c^T) A^-1,  g_c = sum_{i in c} m_i s_i x~_i,
    kappa = G/(G-1) (n-1)/(n-k)   (1 without the correction)

on the dense X~ with the g_c, the meat and everything after them in np.longdouble, and the
per-group statistics as infer_cases.oracle computes them (NaN where a group keeps more than G - 1
coordinates: the meat's rank).  It takes coefficients as input, like infer_cases.oracle.

The cases: trials of 20-60 rows over infer_cases.gpu_design() (n = 4000: 97 trials), and a
per-trial N(0, 0.4^2) effect added to the predictor before the draw, so that the rows of a trial
are correlated and the clustered errors differ from HC0's (tests/test_cluster_cpu.py holds the
intercept's ratio to >= 1.3 in every family)."""
from functools import lru_cache

import numpy as np

import infer_cases as C

LD = C.LD
TRIAL_SD = 0.4
TRIAL_LEN = (20, 60)


def trial_ids(rng, n, lo=TRIAL_LEN[0], hi=TRIAL_LEN[1]):
    """Contiguous trial ids 0, 0, .., 1, 1, .. with trial lengths uniform on lo..hi."""
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(lo, hi + 1)))
    return np.repeat(np.arange(len(lens)), lens)[:n]


@lru_cache(maxsize=None)
def gpu_clusters():
    return trial_ids(np.random.default_rng(2901), C.GPU_N)


GPU_G = int(gpu_clusters().max()) + 1


@lru_cache(maxsize=None)
def gpu_case(name, resp=0):
    """(frame, y, column group ids, generating beta, trial ids) of a clustered GPU case."""
    fam, power, alpha, b0, phi = C.GPU_FAMILIES[name]
    X, gids = C.gpu_design()
    beta = C.true_beta(C.GPU_M, C.GPU_L, b0)
    cid = gpu_clusters()
    rng = np.random.default_rng([2902, sorted(C.GPU_FAMILIES).index(name), resp])
    u = rng.normal(0.0, TRIAL_SD, int(cid.max()) + 1)
    y = C.draw(rng, fam, power, C.xt(X) @ beta + u[cid], phi)
    return X, y, gids, beta, cid


def kappa(G, n, k):
    return LD(G) / LD(G - 1) * (LD(n) - 1) / (LD(n) - LD(k))


def cluster_sums(Xt, ms, clusters):
    """(G x P longdouble matrix of the g_c, G): rows of one label summed, labels in np.unique
    order."""
    u, inv = np.unique(np.asarray(clusters), return_inverse=True)
    g = np.zeros((len(u), Xt.shape[1]), LD)
    np.add.at(g, np.asarray(inv).reshape(-1), C.ld(Xt) * C.ld(ms)[:, None])
    return g, len(u)


def oracle(Xt, y, fam, power, lam, beta, clusters, correction=True, fit_intercept=True,
           groups=None, m=None):
    """Clustered inference at ``beta`` (length p + 1, intercept last) on the dense X~: a dict with
    se (NaN where not kept), cov, kappa, G, n, state and, with ``groups``, ids / stat / dof."""
    n, P = Xt.shape
    m = np.ones(n) if m is None else np.asarray(m, dtype=np.float64)
    base = C.oracle(Xt, y, fam, power, lam, beta, fit_intercept=fit_intercept, cov_type="bayes",
                    scale=1.0, m=m)
    Ainv, state = base["Ainv"], base["state"]
    s = C.score_resid(fam, power, y, Xt @ beta)
    g, G = cluster_sums(Xt, m * s, clusters)
    M = g.T @ g
    k = int(np.sum(state == C.KEPT))
    kap = kappa(G, m.sum(), k) if correction else LD(1)
    Cc = kap * (Ainv @ M @ Ainv)
    var = np.diag(Cc).astype(np.float64)
    var[state != C.KEPT] = np.nan
    out = dict(se=np.sqrt(var), cov=Cc.astype(np.float64), kappa=float(kap), G=G,
               n=float(m.sum()), state=state, M=M.astype(np.float64), df=base["df"])
    if groups is not None:
        ids, goff, gcols = C.csr(groups)
        stat, dof = [], []
        for gi in range(len(ids)):
            c = gcols[goff[gi]:goff[gi + 1]]
            c = c[state[c] == C.KEPT]
            dof.append(c.size)
            if c.size == 0:
                stat.append(0.0)
            elif c.size > G - 1:
                stat.append(np.nan)
            else:
                Tg, _ = C.ld_chol_inv(Cc[np.ix_(c, c)])
                z = Tg.T @ C.ld(beta[c])
                stat.append(float(z @ z))
        out.update(ids=ids, stat=np.array(stat), dof=np.array(dof))
    return out


def runs_of(clusters):
    """(G, roff, run cluster index, coff, cruns) by plain loops: the maximal runs of equal label
    in row order and the runs of each cluster (np.unique order) in ascending run order."""
    labels = list(np.asarray(clusters))
    u = sorted(set(labels))
    idx = [u.index(v) for v in labels]
    roff, rc = [0], []
    for i, c in enumerate(idx):
        if i == 0 or c != idx[i - 1]:
            if i:
                roff.append(i)
            rc.append(c)
    roff.append(len(idx))
    per = [[r for r, c in enumerate(rc) if c == g] for g in range(len(u))]
    coff = np.concatenate([[0], np.cumsum([len(v) for v in per])])
    return len(u), np.array(roff), np.array(rc), coff, np.concatenate(per)
