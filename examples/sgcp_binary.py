"""Stochastic GCP of a binary tensor: every cell counts, nothing is frozen.

A knowledge-base-like tensor stores only its positive triples, and a cell
that is not stored IS a zero. `cpd_gcp` fits stored entries only and needs
one frozen sample of negatives (examples/gcp_binary.py). `cpd_sgcp` fits
the loss over ALL cells instead: every Adam step draws a fresh sample of
stored entries and of cells and forms an unbiased estimate of the
full-tensor gradient.

Runs on CPU in seconds; put the tensor on "cuda" for the gfx950 HIP path.
    python examples/sgcp_binary.py
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
    x = (torch.rand(logits.shape, generator=g, dtype=torch.float64)
         < torch.sigmoid(logits)).double()
    inds = x.nonzero().T.contiguous()
    pos = sp.SpTensor(inds, torch.ones(inds.shape[1], dtype=torch.float64),
                      dims)
    print("positives:", pos.nnz, "of", x.numel(), "cells")

    # 2. fit: only the positives are stored
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    opts = sp.SgcpOptions(lr=1e-2, p=2000, q=2000, p_loss=5000, q_loss=5000,
                          iters_per_epoch=200, max_epochs=5, seed=3,
                          verbose=True)
    k = sp.cpd_sgcp(pos.to(dev), rank, "bernoulli-logit", opts)
    print(f"{k.nepochs} epochs, {k.nsteps} steps, {k.nfails} undone")

    # 3. the exact loss over all cells, and the separation of ones and zeros
    m = torch.einsum("if,jf,kf,f->ijk", *[f.cpu() for f in k.factors],
                     k.lam.cpu())
    exact = float((torch.logaddexp(torch.zeros_like(m), m) - x * m).sum())
    print(f"exact loss over all cells {exact:.1f} (estimate "
          f"{min(k.loss_trace):.1f})")
    p = torch.sigmoid(m)
    print(f"mean P(x=1): ones {float(p[x == 1].mean()):.3f}, "
          f"zeros {float(p[x == 0].mean()):.3f}")


if __name__ == "__main__":
    main()
