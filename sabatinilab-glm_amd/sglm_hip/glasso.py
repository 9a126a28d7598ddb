"""Group lasso on shared per-mask Grams (MI355X): one penalty term per column group.

  objective  1/(2n)|y - Xw - b|^2 + alpha rho sum_g sqrt(k_g) |w_g|_2 + alpha (1 - rho)/2 |w|^2
  (sklearn's ElasticNet scaling; g over the groups, k_g columns each), multiplied by n it is
  1/2 w^T Q w - q^T w + sum_g lam_g |w_g| + l2/2 |w|^2 on centred data,
  lam_g = alpha rho n sqrt(k_g), l2 = alpha (1 - rho) n -- the form csrc/cd.hip documents with
  the L1 term replaced by group norms.  An event's kernel (its block of lag columns) is one
  group: the whole kernel is in the model or exactly zero.

Everything but the descent itself is ``enet``'s: the exact Grams, the centred float64 Q, q, the
intercept recovery and the scores (``enet.solve_arrays(..., groups=csr)``).  The descent is
``sglm_group_cd_shared`` (csrc/gcd.hip: block-wise majorised descent, majoriser from
``sglm_group_bound``).
"""
from __future__ import annotations

import numpy as np


def group_csr(groups, p: int):
    """(goff [ng + 1], gcols [p]) int32 of a length-``p`` group-id array: equal ids form one
    group, groups ordered by id, columns ascending inside a group."""
    ids = np.asarray(groups).reshape(-1)
    if ids.shape[0] != p:
        raise ValueError(f"groups has {ids.shape[0]} entries, X has {p} columns")
    if ids.size and not np.issubdtype(ids.dtype, np.integer):
        raise TypeError("groups: integer group ids")
    _, inv, counts = np.unique(ids, return_inverse=True, return_counts=True)
    gcols = np.argsort(inv.reshape(-1), kind="stable").astype(np.int32)
    goff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return goff, gcols


def block_descent(grams, p: int, qidx: np.ndarray, alpha: np.ndarray, q, lam_scale, l2, csr,
                  max_sweeps: int, tol: float, w, sw):
    """The descent call of ``enet.solve_arrays`` for a group CSR: fills ``w`` [B][p] and ``sw``
    [B] (device).  Fits go to the kernel sorted by (Q, alpha) -- a workgroup solves consecutive
    fits and those of one Q share its row stream; equal penalties converge alike -- and come
    back in the caller's order."""
    import torch
    from . import _lib
    from . import engine as E
    goff, gcols = csr
    dev = q.device
    ng = int(goff.size) - 1
    goff_d = torch.from_numpy(np.ascontiguousarray(goff, dtype=np.int32)).to(dev)
    gcols_d = torch.from_numpy(np.ascontiguousarray(gcols, dtype=np.int32)).to(dev)
    nq = int(grams.Qt.shape[0])
    gamma = torch.empty((nq, ng), dtype=torch.float64, device=dev)
    _lib.call("sglm_group_bound", E._p(grams.Qt), p, nq, E._p(goff_d), E._p(gcols_d), ng,
              E._p(gamma), E._stream())
    B = int(qidx.size)
    order = np.lexsort((np.arange(B), alpha, qidx))
    od = torch.from_numpy(order.astype(np.int64)).to(dev)
    qs, ls, l2s = q[od].contiguous(), lam_scale[od].contiguous(), l2[od].contiguous()
    qidx_d = torch.from_numpy(np.ascontiguousarray(qidx[order], dtype=np.int32)).to(dev)
    ws = torch.empty_like(qs)
    sws = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("sglm_group_cd_shared", E._p(grams.Qt), p, E._p(qidx_d), B, E._p(qs),
              E._p(goff_d), E._p(gcols_d), ng, E._p(gamma), E._p(ls), E._p(l2s),
              int(max_sweeps), float(tol), E._p(ws), E._p(sws), E._stream())
    w[od] = ws
    sw[od] = sws
