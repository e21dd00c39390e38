"""Constrained CPD by AO-ADMM (Huang, Sidiropoulos, Liavas 2016; blocked as
in Smith et al. 2017).

The outer loop is CPD-ALS's (cpd.py): per mode one MTTKRP `K` and the
Hadamard product `G` of the other modes' Grams. Instead of the closed-form
solve H = K G^-1, a constrained mode runs ADMM on

    min_H 0.5 * tr(H G H^T) - tr(K H^T) + r(H)

with a scaled dual `U` that persists across outer iterations:

    rho  = trace(G) / F
    Ginv = (G + rho*I)^-1
    repeat:  Ht = (K + rho*(H + U)) @ Ginv
             H  = prox_{r/rho}(Ht - U)
             U  = U + H - Ht

The constraints here are elementwise, so rows are independent and the rows
are cut into blocks of BLOCK_ROWS that iterate and stop on their own:

    pr = ||H - Ht||^2  pn = ||H||^2  dr = ||H - Hold||^2  dn = ||U||^2
    stop when pr <= inner_tol*pn and dr <= inner_tol*max(dn, pn)

(product form, so a zero norm never divides; `max(dn, pn)` so that a block
on which the constraint is inactive, where U stays ~0, stops once H has
stopped moving relative to its own size). A block whose solution is exactly
zero never meets a relative test and runs to `max_inner`.

Device path: csrc/hip/admm.hip, one workgroup per block, the whole inner
loop in registers. `impl="torch"` is the vectorised torch implementation —
the CPU path, and the benchmark baseline on device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import torch

from splatt_amd._ext import native
from splatt_amd.cpd import Kruskal, seeded_init
from splatt_amd.csf import CsfSet, csf_alloc
from splatt_amd.mttkrp import mttkrp
from splatt_amd.ops.dense import gram, solve_rows, spd_inverse
from splatt_amd.sptensor import SpTensor

# Rows per independently-stopping block. A constant, not an option: the
# stopping rule is evaluated per block, so results depend on it.
BLOCK_ROWS = 64
MAX_RANK = 64

KINDS = ("nonneg", "l1", "nonneg_l1", "box")


# -------------------------------------------------------------- constraints

@dataclass(frozen=True)
class Constraint:
    """An elementwise constraint / regulariser on one factor.

      nonneg      H >= 0                         prox max(x, 0)
      l1          weight*|H|_1                   prox sign(x)*max(|x|-w/rho, 0)
      nonneg_l1   H >= 0 and weight*|H|_1        prox max(x - w/rho, 0)
      box         lo <= H <= hi                  prox min(max(x, lo), hi)
    """
    kind: str
    weight: float = 0.0
    lo: float = 0.0
    hi: float = 1.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"unknown constraint kind {self.kind!r} "
                             f"({', '.join(KINDS)})")
        for name in ("weight", "lo", "hi"):
            v = getattr(self, name)
            if not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"constraint {name} must be a finite "
                                 f"number, got {v!r}")
        if self.kind in ("l1", "nonneg_l1") and not self.weight > 0:
            raise ValueError(f"{self.kind} needs weight > 0, got "
                             f"{self.weight}")
        if self.kind == "box" and not self.lo < self.hi:
            raise ValueError(f"box needs lo < hi, got [{self.lo}, {self.hi}]")

    @property
    def code(self) -> int:
        return KINDS.index(self.kind)

    def prox(self, x: torch.Tensor, rho) -> torch.Tensor:
        if self.kind == "nonneg":
            return x.clamp(min=0.0)
        if self.kind == "l1":
            return torch.sign(x) * (x.abs() - self.weight / rho).clamp(min=0.0)
        if self.kind == "nonneg_l1":
            return (x - self.weight / rho).clamp(min=0.0)
        return x.clamp(min=self.lo, max=self.hi)


def nonneg() -> Constraint:
    return Constraint("nonneg")


def l1(w: float) -> Constraint:
    return Constraint("l1", weight=w)


def nonneg_l1(w: float) -> Constraint:
    return Constraint("nonneg_l1", weight=w)


def box(lo: float, hi: float) -> Constraint:
    return Constraint("box", lo=lo, hi=hi)


# ------------------------------------------------------------ block update

def _update_torch(K, Ginv, rho, H, U, con, inner_tol, max_inner):
    """All blocks at once on [nblocks, BLOCK_ROWS, F] views; a converged
    block is frozen by the `active` mask. No host sync on device tensors."""
    n, F = H.shape
    nb = (n + BLOCK_ROWS - 1) // BLOCK_ROWS
    dev = H.device
    iters = torch.zeros(nb, dtype=torch.int32, device=dev)
    if n == 0:
        return iters
    pad = nb * BLOCK_ROWS - n

    def blocks(X):
        if pad:
            X = torch.cat([X, X.new_zeros(pad, F)], 0)
        return X.reshape(nb, BLOCK_ROWS, F)

    Kb, Hb, Ub = blocks(K), blocks(H).clone(), blocks(U).clone()
    # rows past n stay zero whatever prox(0) is
    valid = (torch.arange(nb * BLOCK_ROWS, device=dev) < n).reshape(
        nb, BLOCK_ROWS, 1)
    active = torch.ones(nb, dtype=torch.bool, device=dev)
    for _ in range(max_inner):
        Ht = ((Kb + rho * (Hb + Ub)).reshape(-1, F) @ Ginv).reshape(
            nb, BLOCK_ROWS, F)
        Hn = con.prox(Ht - Ub, rho)
        if pad:
            Hn = torch.where(valid, Hn, torch.zeros_like(Hn))
        Un = Ub + Hn - Ht
        act = active.reshape(nb, 1, 1)
        iters += active.to(torch.int32)
        if inner_tol > 0:
            pr = (Hn - Ht).square().sum(dim=(1, 2))
            pn = Hn.square().sum(dim=(1, 2))
            dr = (Hn - Hb).square().sum(dim=(1, 2))
            dn = Un.square().sum(dim=(1, 2))
            stop = (pr <= inner_tol * pn) & (
                dr <= inner_tol * torch.maximum(dn, pn))
        Hb = torch.where(act, Hn, Hb)
        Ub = torch.where(act, Un, Ub)
        if inner_tol > 0:
            active = active & ~stop
            # free on the CPU; on device it would be a host sync
            if dev.type == "cpu" and not bool(active.any()):
                break
    H.copy_(Hb.reshape(-1, F)[:n])
    U.copy_(Ub.reshape(-1, F)[:n])
    return iters


_VARIANTS = {"hip": 0, "hip_valu": 1, "hip_mfma": 2}


def admm_update(K: torch.Tensor, Ginv: torch.Tensor, rho, H: torch.Tensor,
                U: torch.Tensor, constraint: Constraint,
                inner_tol: float = 1e-2, max_inner: int = 50,
                impl: str = "auto") -> torch.Tensor:
    """Blocked ADMM inner loop for one factor. Updates `H` and `U` in place
    and returns the int32 inner-iteration count of every block of
    BLOCK_ROWS rows. `Ginv` is used as given (the caller inverts
    G + rho*I); `rho` is a Python float or a one-element tensor.

    `impl`: "hip" (the gfx950 kernel; default on device tensors), "torch"
    (vectorised torch: the CPU path, and a baseline that also runs on device
    tensors when asked — never chosen automatically there). "hip_valu" and
    "hip_mfma" force one of the kernel's two GEMV forms (benchmarking;
    "hip_mfma" exists at ranks 16, 32 and 64)."""
    if not isinstance(constraint, Constraint):
        raise TypeError(f"constraint must be a Constraint, got "
                        f"{type(constraint).__name__}")
    for name, X in (("K", K), ("Ginv", Ginv), ("H", H), ("U", U)):
        if not isinstance(X, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if X.dtype != torch.float64:
            raise ValueError(f"{name} has dtype {X.dtype}: admm_update "
                             "supports float64 only")
        if X.device != H.device:
            raise ValueError(f"{name} is on {X.device}, H on {H.device}")
        if X.dim() != 2:
            raise ValueError(f"{name} must be 2-D, got shape "
                             f"{tuple(X.shape)}")
        if not X.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    n, F = int(H.shape[0]), int(H.shape[1])
    if not 1 <= F <= MAX_RANK:
        raise ValueError(f"admm_update supports rank 1..{MAX_RANK}, got {F}")
    if tuple(K.shape) != (n, F) or tuple(U.shape) != (n, F):
        raise ValueError(f"K {tuple(K.shape)}, H {tuple(H.shape)} and U "
                         f"{tuple(U.shape)} must have the same shape")
    if tuple(Ginv.shape) != (F, F):
        raise ValueError(f"Ginv has shape {tuple(Ginv.shape)}, expected "
                         f"({F}, {F})")
    if int(max_inner) != max_inner or max_inner < 0:
        raise ValueError(f"max_inner must be an integer >= 0, got "
                         f"{max_inner}")
    dev = H.device
    if isinstance(rho, torch.Tensor):
        if rho.numel() != 1:
            raise ValueError("rho must have one element")
        rho_t = rho.to(device=dev, dtype=torch.float64).reshape(1)
    else:
        if not float(rho) > 0:
            raise ValueError(f"rho must be > 0, got {rho}")
        rho_t = torch.full((1,), float(rho), dtype=torch.float64, device=dev)
    if impl == "auto":
        impl = "hip" if dev.type == "cuda" else "torch"
    if impl not in _VARIANTS and impl != "torch":
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto, "
                         "hip_valu, hip_mfma)")
    if impl == "torch":
        return _update_torch(K, Ginv, rho_t.reshape(()), H, U, constraint,
                             float(inner_tol), int(max_inner))
    if dev.type != "cuda":
        raise ValueError(f"impl={impl!r} needs device tensors")
    if impl == "hip_mfma" and F not in (16, 32, 64):
        raise ValueError("impl='hip_mfma' exists for ranks 16, 32 and 64")
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    iters = torch.zeros((n + BLOCK_ROWS - 1) // BLOCK_ROWS,
                        dtype=torch.int32, device=dev)
    native().gpu_admm_update(
        K, Ginv, rho_t, H, U, iters, constraint.code,
        float(constraint.weight), float(constraint.lo), float(constraint.hi),
        float(inner_tol), int(max_inner), _VARIANTS[impl],
        torch.cuda.current_stream().cuda_stream)
    return iters


def admm_solve(K: torch.Tensor, G: torch.Tensor, H: torch.Tensor,
               U: torch.Tensor, constraint: Constraint,
               inner_tol: float = 1e-2, max_inner: int = 50,
               impl: str = "auto") -> torch.Tensor:
    """rho = trace(G)/F and Ginv = (G + rho*I)^-1 on the device (no host
    sync), then `admm_update`."""
    F = int(G.shape[0])
    rho = G.diagonal().sum() / F
    Ginv = spd_inverse(G + rho * torch.eye(F, dtype=G.dtype, device=G.device))
    return admm_update(K, Ginv.contiguous(), rho, H, U, constraint,
                       inner_tol, max_inner, impl)


# ------------------------------------------------------------------ driver

@dataclass
class AoAdmmOptions:
    tolerance: float = 1e-5
    max_iters: int = 50
    seed: int = 0x5EED5EED
    csf_alloc: str = "two"
    nthreads: int = 0
    verbose: bool = False
    regularize: float = 0.0
    inner_tol: float = 1e-2
    max_inner: int = 50


@dataclass
class ConstrainedKruskal(Kruskal):
    duals: List[torch.Tensor] = field(default_factory=list)
    # per outer iteration, per mode: inner iterations summed over the blocks
    inner_iters: List[List[int]] = field(default_factory=list)


ConstraintSpec = Union[Constraint, Sequence[Optional[Constraint]],
                       Dict[int, Constraint], None]


def _per_mode(constraints: ConstraintSpec, nm: int) -> List[Optional[Constraint]]:
    if constraints is None or isinstance(constraints, Constraint):
        return [constraints] * nm
    if isinstance(constraints, dict):
        out: List[Optional[Constraint]] = [None] * nm
        for m, c in constraints.items():
            if not isinstance(m, int) or not 0 <= m < nm:
                raise ValueError(f"constraint mode {m!r} out of range for "
                                 f"{nm} modes")
            out[m] = c
    else:
        out = list(constraints)
        if len(out) != nm:
            raise ValueError(f"need one constraint (or None) per mode: got "
                             f"{len(out)} for {nm} modes")
    for c in out:
        if c is not None and not isinstance(c, Constraint):
            raise TypeError(f"constraints must be Constraint or None, got "
                            f"{type(c).__name__}")
    return out


def cpd_aoadmm(src: CsfSet | SpTensor, rank: int,
               constraints: ConstraintSpec,
               opts: Optional[AoAdmmOptions] = None) -> ConstrainedKruskal:
    """Constrained CPD. `constraints`: one Constraint for every mode, a list
    of length nmodes (None: that mode gets the plain least-squares solve),
    or a {mode: Constraint} dict.

    Initialisation, MTTKRP, Gram upkeep, the fit formula and the stop on
    |fit - old_fit| < tolerance are cpd_als's. The factors are neither
    normalised during the run nor afterwards: they satisfy their
    constraints exactly as returned, and `lam` is all ones."""
    opts = opts or AoAdmmOptions()
    cs = src if isinstance(src, CsfSet) else csf_alloc(src, opts.csf_alloc)
    nm = cs.nmodes
    dims = cs.dims
    dev = cs.csfs[0].device
    dtype = cs.csfs[0].vals.dtype
    if dtype != torch.float64:
        raise ValueError(f"cpd_aoadmm supports float64 tensors only, got "
                         f"{dtype} (load the tensor as f64)")
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"cpd_aoadmm supports rank 1..{MAX_RANK}, got {rank}")
    cons = _per_mode(constraints, nm)

    factors = [seeded_init(dims[m], rank, m, opts.seed, dtype=dtype).to(dev)
               for m in range(nm)]
    duals = [torch.zeros_like(f) for f in factors]
    grams = [gram(f) for f in factors]
    from splatt_amd.mttkrp import factor_store_dtype
    qdt = factor_store_dtype() if dev.type == "cuda" else None
    qfactors = [f.to(qdt) for f in factors] if qdt else None
    norm_x = float(cs.csfs[0].vals.double().square().sum())
    buf = torch.empty(max(dims), rank, dtype=dtype, device=dev)
    ones = torch.ones(rank, rank, dtype=dtype, device=dev)
    eye = torch.eye(rank, dtype=dtype, device=dev)

    fit = old_fit = 0.0
    trace: List[float] = []
    counts: List[List[Optional[torch.Tensor]]] = []
    niters = 0
    import time as _time
    for it in range(opts.max_iters):
        _t0 = _time.perf_counter()
        row: List[Optional[torch.Tensor]] = []
        for m in range(nm):
            mb = buf[: dims[m]]
            mttkrp(cs, qfactors or factors, m, out=mb, nthreads=opts.nthreads)
            G = ones.clone()
            for o in range(nm):
                if o != m:
                    G *= grams[o]
            if opts.regularize:
                G += opts.regularize * eye
            if cons[m] is None:
                factors[m] = solve_rows(mb, spd_inverse(G))
                row.append(None)
            else:
                row.append(admm_solve(mb, G, factors[m], duals[m], cons[m],
                                      opts.inner_tol, opts.max_inner).sum())
            if qfactors is not None:
                qfactors[m] = factors[m].to(qdt)
            grams[m] = gram(factors[m])
        counts.append(row)

        # fit from the last mode's MTTKRP, which does not depend on that
        # mode's factor: <X,K> = sum(buf * A_last), lambda = 1
        mlast = nm - 1
        inner = float((buf[: dims[mlast]] * factors[mlast]).sum())
        Gall = ones.clone()
        for o in range(nm):
            Gall *= grams[o]
        knorm = float(Gall.sum())
        residual = math.sqrt(max(0.0, norm_x + knorm - 2 * inner))
        fit = 1.0 - residual / math.sqrt(norm_x)
        trace.append(fit)
        niters = it + 1
        if opts.verbose:
            print(f"  its = {it + 1} ({_time.perf_counter() - _t0:.3f}s) "
                  f"fit = {fit:.5f} delta = {fit - old_fit:+.4e}")
        if it > 0 and abs(fit - old_fit) < opts.tolerance:
            break
        old_fit = fit

    # the count tensors are read only now: the loop's one host sync per
    # iteration is the fit scalar
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    flat = torch.stack([zero if c is None else c.to(torch.int64)
                        for r in counts for c in r]) if counts else zero
    inner_iters = flat.reshape(-1, nm).cpu().tolist() if counts else []
    return ConstrainedKruskal(
        factors=factors, lam=torch.ones(rank, dtype=dtype, device=dev),
        fit=fit, niters=niters, fit_trace=trace, duals=duals,
        inner_iters=inner_iters)
