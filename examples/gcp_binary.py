"""Generalized CPD of a binary tensor: positives plus sampled zeros.

A knowledge-base-like tensor stores only its positive triples. GCP fits the
STORED entries, so the negatives have to be stored too: `sample_zeros` adds
a sample of explicit zeros, and the Bernoulli-logit loss then fits
P(x = 1) = sigmoid(model).

Runs on CPU in seconds; put the tensor on "cuda" for the gfx950 HIP path.
    python examples/gcp_binary.py
"""
import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import torch

import splatt_amd as sp


def main():
    # 1. planted logits, and the positives they produce
    g = torch.Generator().manual_seed(7)
    dims, rank = [40, 30, 20], 3
    truth = [torch.randn(d, rank, generator=g, dtype=torch.float64)
             for d in dims]
    logits = torch.einsum("if,jf,kf->ijk", *truth) - 1.0
    x = torch.rand(logits.shape, generator=g, dtype=torch.float64) \
        < torch.sigmoid(logits)
    inds = x.nonzero().T.contiguous()
    pos = sp.SpTensor(inds, torch.ones(inds.shape[1], dtype=torch.float64),
                      dims)
    print("positives:", pos.nnz, "of", x.numel(), "cells")

    # 2. store as many sampled zeros as there are positives
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    t = sp.sample_zeros(pos.to(dev), pos.nnz, seed=1)
    print("observed entries:", t.nnz)

    # 3. fit
    k = sp.cpd_gcp(t, rank, "bernoulli-logit",
                   sp.GcpOptions(max_iters=60, seed=3))
    print(f"final loss {k.loss_trace[-1]:.4f} after {k.niters} iterations "
          f"({k.nfev} evaluations)")

    # 4. the model separates stored positives from stored zeros
    p = torch.sigmoid(sp.kruskal_predict(k.factors, t.inds, k.lam)).cpu()
    v = t.vals.cpu()
    print(f"mean P(x=1): stored positives {float(p[v == 1].mean()):.3f}, "
          f"stored zeros {float(p[v == 0].mean()):.3f}")


if __name__ == "__main__":
    main()
