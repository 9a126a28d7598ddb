"""Regenerate tests/golden/binomial.npz (CPU, needs scikit-learn):

    python tests/golden/make_golden_binomial.py

sklearn ``LogisticRegression(solver="newton-cholesky", tol=1e-12)`` on the cases of
tests/binomial_cases.py.  It minimises sum_i loss_i + |w|^2 / (2 C), so C = 1 / (alpha N) gives
the minimiser of mean_i loss_i + alpha/2 |w|^2; penalty=None at alpha = 0.  Only coefficients,
intercepts and scores are stored (D^2 and -mean((y - mu)^2) of the sklearn fit on its own rows);
the designs are rebuilt from their seeds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sabatinilab-glm_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    from sklearn.linear_model import LogisticRegression
    import binomial_cases as bc
    out = {}

    def record(tag, X, y, alpha):
        kw = dict(penalty=None) if alpha == 0 else dict(C=1.0 / (alpha * X.shape[0]))
        m = LogisticRegression(solver="newton-cholesky", tol=1e-12, max_iter=1000, **kw).fit(X, y)
        w, b = m.coef_.reshape(-1), float(m.intercept_[0])
        eta = X @ w + b
        out[tag + "_coef"] = w
        out[tag + "_intercept"] = np.float64(b)
        out[tag + "_d2"] = np.float64(bc.d2(y, eta))
        out[tag + "_neg_mse"] = np.float64(bc.neg_mse(y, eta))

    _, X, y = bc.case_a()
    for j, a in enumerate(bc.ALPHAS_A):
        record(f"A{j}", X, y, a)
    out["A_alphas"] = np.array(bc.ALPHAS_A)
    _, X, y = bc.case_s()
    record("S", X, y, bc.ALPHA_S)
    np.savez(os.path.join(HERE, "binomial.npz"), **out)
    print("wrote binomial.npz:", sorted(out))


if __name__ == "__main__":
    main()
