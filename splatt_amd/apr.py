"""Poisson CPD by alternating Poisson regression (CP-APR, Chi & Kolda 2012;
`cp_apr` in Tensor Toolbox), multiplicative-update variant.

For count data the model is x ~ Poisson(m), m = sum_f lam_f prod_t A_t[., f]
with nonnegative factors whose columns sum to 1, and the fit minimises the
negative log-likelihood sum(m) - sum_x x log m_x. For output mode m, with
B = A_m diag(lam), Omega_i the nonzeros of row i and pi_x the Hadamard
product of the other modes' factor rows at nonzero x, the subproblem
separates over rows and is solved by the multiplicative iteration

    for l = 1 .. max_inner:
        mdl_x   = max(sum_f B[i,f] pi_x[f], eps_div)          x in Omega_i
        Phi[i]  = sum_{x in Omega_i} (val_x / mdl_x) pi_x
        v       = max_f |min(B[i,f], 1 - Phi[i,f])|           KKT violation
        stop if inner_tol > 0 and v < inner_tol               (B[i] untouched)
        B[i]   *= Phi[i]

The textbook algorithm stops a mode when the largest violation over its
rows is below the tolerance. Here every row stops on its own violation:
the rows are independent subproblems, so this is exact, it meets the same
mode-wide criterion with less work, and it is the choice AO-ADMM (admm.py)
made per block.

Device path: csrc/hip/apr.hip — one wave per stream segment, the inner
iterations of a single-segment row inside one launch, no atomics.
`impl="torch"` is the vectorised torch implementation: the CPU path, and
the benchmark baseline on device.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from splatt_amd._ext import native
from splatt_amd.completion import (_plan, _resolve, _stream, _train_coo,
                                   kruskal_predict)
from splatt_amd.cpd import seeded_init
from splatt_amd.csf import Csf, CsfSet, csf_alloc
from splatt_amd.sptensor import SpTensor

MAX_RANK = 64
# A workspace slot is only F doubles, so every multi-segment row of a mode
# fits at once: the planner is asked for one batch and never grows segments.
_UNBOUNDED = 1 << 62


def apr_plan(src: CsfSet | Csf, mode: int) -> dict:
    """The segment plan `apr_update(impl="hip")` uses for this mode (for
    inspection and tests)."""
    return _plan(_resolve(src, mode), _UNBOUNDED)


def _check_counts(c: Csf) -> None:
    """Poisson data is nonnegative. Checked once per stream and remembered,
    so repeated updates do not synchronise with the device."""
    ok = getattr(c, "_apr_nonneg", None)
    if ok is None:
        ok = bool((c.vals >= 0).all())
        object.__setattr__(c, "_apr_nonneg", ok)
    if not ok:
        raise ValueError("apr needs tensor values >= 0 (Poisson counts); "
                         "the tensor has negative or NaN entries")


def _update_hip(c: Csf, mats: List[torch.Tensor], B: torch.Tensor,
                inner_tol: float, max_inner: int, eps_div: float) -> Tuple:
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    nrows, rank = int(B.shape[0]), int(B.shape[1])
    st = _stream(c)
    plan = _plan(c, _UNBOUNDED)
    nmseg = int(plan["seg_start"].numel()) - plan["nsingle"]
    need = max(1, nmseg * rank)
    ws = getattr(c, "_apr_ws", None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float64, device=c.device)
        object.__setattr__(c, "_apr_ws", ws)
    dev = c.device
    # rows with no nonzero keep these zeros, and B = 0
    Phi = torch.zeros(nrows, rank, dtype=torch.float64, device=dev)
    iters = torch.zeros(nrows, dtype=torch.int32, device=dev)
    viol0 = torch.zeros(nrows, dtype=torch.float64, device=dev)
    done = torch.zeros(nrows, dtype=torch.int32, device=dev)
    B.masked_fill_((st["cnt"] == 0).unsqueeze(1), 0.0)
    ms = [mats[c.dim_perm[l]].contiguous() for l in range(1, c.nmodes)]
    native().hip_apr_update(
        st["idx"], ms, st["vals"], plan["seg_start"], plan["seg_len"],
        plan["seg_row"], plan["seg_slot"], plan["nsingle"], plan["mrow"],
        plan["mslot"], float(eps_div), float(inner_tol), int(max_inner), ws,
        done, B, Phi, iters, viol0,
        torch.cuda.current_stream().cuda_stream)
    return Phi, iters, viol0


def _update_torch(c: Csf, mats: List[torch.Tensor], B: torch.Tensor,
                  inner_tol: float, max_inner: int, eps_div: float) -> Tuple:
    """Every inner iteration is one chunked pass over the key stream
    (gather, row-wise dot, index_add_ of the weighted pi rows) for all rows;
    rows that have stopped are masked out of the updates."""
    nrows, rank = int(B.shape[0]), int(B.shape[1])
    st = _stream(c)
    dev, dt = c.device, torch.float64
    key = st["key"].long()
    idx = [ix.long() for ix in st["idx"]]
    vals = st["vals"]
    ms = [mats[c.dim_perm[l]] for l in range(1, c.nmodes)]
    nnz = int(vals.numel())
    chunk = max(1, (64 << 20) // (rank * 8))
    active = st["cnt"] > 0
    B.masked_fill_((~active).unsqueeze(1), 0.0)
    Phi = torch.zeros(nrows, rank, dtype=dt, device=dev)
    iters = torch.zeros(nrows, dtype=torch.int32, device=dev)
    viol0 = torch.zeros(nrows, dtype=dt, device=dev)
    for l in range(1, max_inner + 1):
        phi = torch.zeros(nrows, rank, dtype=dt, device=dev)
        for q0 in range(0, nnz, chunk):
            q1 = min(nnz, q0 + chunk)
            pi = None
            for ix, A in zip(idx, ms):
                g = A.index_select(0, ix[q0:q1])
                pi = g if pi is None else pi * g
            k = key[q0:q1]
            mdl = (B.index_select(0, k) * pi).sum(1).clamp_min(eps_div)
            phi.index_add_(0, k, (vals[q0:q1] / mdl).unsqueeze(1) * pi)
        v = torch.minimum(B, 1.0 - phi).abs().amax(1)
        Phi = torch.where(active.unsqueeze(1), phi, Phi)
        iters = torch.where(active, torch.full_like(iters, l), iters)
        if l == 1:
            viol0 = torch.where(active, v, viol0)
        if inner_tol > 0:
            active = active & ~(v < inner_tol)
            if dev.type == "cpu" and not bool(active.any()):
                break
        B.copy_(torch.where(active.unsqueeze(1), B * phi, B))
    return Phi, iters, viol0


def apr_update(src: CsfSet | Csf, mats: Sequence[torch.Tensor], mode: int,
               B: torch.Tensor, *, inner_tol: float, max_inner: int,
               eps_div: float = 1e-10, impl: str = "auto") -> Tuple:
    """The CP-APR row update of `mode`: B ([dims[mode], rank], the factor
    with the weights absorbed) is updated IN PLACE by up to `max_inner`
    multiplicative iterations per row; returns (Phi, iters, viol0): the Phi
    of each row's last executed iteration, the iterations each row ran
    (int32) and each row's KKT violation at its first iteration. A row
    stops once its violation is below `inner_tol`; `inner_tol <= 0` runs
    exactly `max_inner` iterations. Rows without nonzeros get B = Phi = 0,
    iters = viol0 = 0. `mats` is indexed by tensor mode (the entry for `mode`
    itself is not read).

    `src` must hold `mode` at depth 0 of a key-sorted stream — any
    csf_alloc(t, "all") build — with values >= 0. `impl`: "hip" (the gfx950
    kernels; default on device tensors), "torch" (vectorised torch: the CPU
    path, and a baseline that also runs on device tensors when asked —
    never chosen automatically there)."""
    c = _resolve(src, mode)
    mats = list(mats)
    if len(mats) != c.nmodes:
        raise ValueError(f"need {c.nmodes} factor matrices, got {len(mats)}")
    if c.nmodes < 3 or c.nmodes > 8:
        raise ValueError(f"apr supports 3..8 modes, got {c.nmodes}")
    if not isinstance(B, torch.Tensor) or B.dim() != 2:
        raise ValueError("B must be a 2-D tensor [rows, rank]")
    rank = int(B.shape[1])
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"apr supports rank 1..{MAX_RANK}, got {rank}")
    if (int(B.shape[0]) != c.dims[mode] or not B.is_contiguous()
            or B.dtype != torch.float64 or B.device != c.device):
        raise ValueError("B must be a contiguous float64 "
                         f"({c.dims[mode]}, {rank}) tensor on {c.device}")
    for m, A in enumerate(mats):
        if tuple(A.shape) != (c.dims[m], rank):
            raise ValueError(f"factor {m} has shape {tuple(A.shape)}, "
                             f"expected ({c.dims[m]}, {rank})")
        if A.dtype != torch.float64 or A.device != c.device:
            raise ValueError(
                f"factor {m}: dtype/device {A.dtype}/{A.device} does not "
                f"match tensor {c.vals.dtype}/{c.device}")
    if int(max_inner) < 1:
        raise ValueError(f"max_inner must be >= 1, got {max_inner}")
    if not eps_div > 0:
        raise ValueError(f"eps_div must be > 0, got {eps_div}")
    if impl == "auto":
        impl = "hip" if c.device.type == "cuda" else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto)")
    if impl == "hip" and c.device.type != "cuda":
        raise ValueError("impl='hip' needs a device tensor")
    _check_counts(c)
    fn = _update_hip if impl == "hip" else _update_torch
    return fn(c, mats, B, float(inner_tol), int(max_inner), float(eps_div))


# ------------------------------------------------------------------ driver

@dataclass
class AprOptions:
    max_iters: int = 100
    max_inner: int = 10
    tolerance: float = 1e-4   # KKT tolerance, outer and inner; <= 0: fixed
    #                           schedule of max_iters x max_inner
    eps_div: float = 1e-10    # floor of a model value before it divides
    kappa: float = 1e-2       # inadmissible-zero fix: offset ...
    kappa_tol: float = 1e-10  # ... applied to entries below this
    seed: int = 0x5EED5EED
    verbose: bool = False


@dataclass
class PoissonKruskal:
    factors: List[torch.Tensor]
    lam: torch.Tensor
    loglik_trace: List[float] = field(default_factory=list)  # negative
    kkt_trace: List[float] = field(default_factory=list)
    inner_trace: List[int] = field(default_factory=list)
    niters: int = 0
    converged: bool = False


def poisson_loglik(factors: Sequence[torch.Tensor], lam: torch.Tensor,
                   inds: torch.Tensor, vals: torch.Tensor,
                   eps_div: float = 1e-10) -> float:
    """Negative Poisson log-likelihood (without the log x! term) of a model
    whose factor columns sum to 1: sum(lam) is then the model's total mass.
    sum(lam) - sum_x val_x log(max(model_x, eps_div))."""
    model = kruskal_predict(factors, inds, lam=lam)
    return float(lam.sum() - (vals * model.clamp_min(eps_div).log()).sum())


def cpd_apr(t: SpTensor | CsfSet, rank: int,
            opts: Optional[AprOptions] = None) -> PoissonKruskal:
    """Poisson CPD of a nonnegative (count) tensor by CP-APR.

    Each outer iteration updates the modes in order with `apr_update` and
    records the negative log-likelihood, the largest first-iteration KKT
    violation over all rows and modes, and the inner iterations spent. It
    has converged when that violation is below `tolerance`. The returned
    factors are nonnegative with columns summing to 1 (or all zero), the
    weights in `lam`."""
    opts = opts or AprOptions()
    if isinstance(t, SpTensor):
        if t.dtype != torch.float64:
            raise ValueError("apr supports float64 tensors only, got "
                             f"{t.dtype} (load the tensor as f64)")
        cs = csf_alloc(t, "all")
    else:
        cs = t
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"apr supports rank 1..{MAX_RANK}, got {rank}")
    nm, dims = cs.nmodes, cs.dims
    for m in range(nm):
        _check_counts(_resolve(cs, m))
    dev = cs.csfs[0].device
    tinds, tvals = _train_coo(cs)
    factors = []
    for m in range(nm):
        A = seeded_init(dims[m], rank, m, opts.seed).to(dev).abs()
        factors.append(A / A.sum(0))
    lam = torch.full((rank,), float(tvals.sum()) / rank, dtype=torch.float64,
                     device=dev)
    res = PoissonKruskal(factors=factors, lam=lam)
    phi_prev: List[Optional[torch.Tensor]] = [None] * nm
    tol = float(opts.tolerance)
    for it in range(opts.max_iters):
        kkt, inner = 0.0, 0
        for m in range(nm):
            A = factors[m]
            if it > 0:
                # inadmissible zeros: an entry stuck at 0 whose gradient
                # says it should grow would stay 0 under a multiplicative
                # update
                A = A + opts.kappa * ((A < opts.kappa_tol)
                                      & (phi_prev[m] > 1.0)).to(A.dtype)
            B = (A * lam).contiguous()
            phi_prev[m], iters, viol0 = apr_update(
                cs, factors, m, B, inner_tol=tol, max_inner=opts.max_inner,
                eps_div=opts.eps_div)
            lam = B.sum(0)
            factors[m] = B / torch.where(lam > 0, lam, torch.ones_like(lam))
            kkt = max(kkt, float(viol0.max()))
            inner += int(iters.sum())
        ll = poisson_loglik(factors, lam, tinds, tvals, opts.eps_div)
        res.loglik_trace.append(ll)
        res.kkt_trace.append(kkt)
        res.inner_trace.append(inner)
        res.niters = it + 1
        if opts.verbose:
            print(f"  its = {it + 1} loglik = {ll:.8e} kkt = {kkt:.3e} "
                  f"inner = {inner}")
        if kkt < tol:
            res.converged = True
            break
    res.lam = lam
    return res
