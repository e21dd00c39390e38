"""Poisson CPD by alternating Poisson regression (CP-APR, Chi & Kolda 2012;
`cp_apr` in Tensor Toolbox): the multiplicative-update row solver (the
default) and the damped-Newton row solver PDNR (further down).

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
iterations of a single-segment row inside one launch, no atomics; for PDNR
csrc/hip/apr_pdnr.hip — one workgroup per row, the row's whole inner loop
inside one launch.
`impl="torch"` is the vectorised torch implementation: the CPU path, and
the benchmark baseline on device.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
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


def _check_update(src, mats, mode: int, B, max_inner, eps_div,
                  impl: str) -> Tuple[Csf, str]:
    """The argument checks the row updates share; returns the stream
    and the resolved `impl`."""
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
    return c, impl


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
    c, impl = _check_update(src, mats, mode, B, max_inner, eps_div, impl)
    fn = _update_hip if impl == "hip" else _update_torch
    return fn(c, list(mats), B, float(inner_tol), int(max_inner),
              float(eps_div))


# ------------------------------------------------- damped-Newton row solver
#
# PDNR (Hansen, Plantenga & Kolda 2015; the Newton-type row solver of
# Tensor Toolbox's cp_apr). With m_x(b) = max(b . pi_x, eps_div),
#
#   f(b)   = sum_c b_c - sum_x v_x log m_x(b)
#   Phi(b) = sum_x (v_x / m_x) pi_x            g = 1 - Phi
#   H(b)   = sum_x (v_x / m_x^2) pi_x pi_x^T
#
#   mu = mu0
#   for l = 1 .. max_inner:
#       pass A at b: m, f, Phi, g, H
#       viol = max_c |min(b_c, g_c)|; iters = l; Phi[i] = Phi
#       stop if inner_tol > 0 and viol < inner_tol            (b untouched)
#       eps_act = min(1e-8, || b - max(b - g, 0) ||_2)
#       fixed  = (b == 0) & (g > 0)                d_c = 0
#       active = (0 < b <= eps_act) & (g > 0)      d_c = -g_c
#       free   = the rest         (H_ff + mu I) d_f = -g_f   by Cholesky
#       pred   = g_f . d_f + 1/2 d_f^T H_ff d_f
#       alpha = 1; up to 11 evaluations, alpha halved after a rejection:
#           b' = max(b + alpha d, 0); accept if f(b') <= f + 1e-4 g.(b' - b)
#       accepted:     rho = (f(b') - f) / pred; b = b'
#                     pred == 0: mu *= 10, else rho < 0.25: mu *= 3.5,
#                     else rho > 0.75: mu *= 2/7
#       not accepted: b stays, mu *= 10, nfail += 1
#       a Cholesky pivot <= 0 or NaN counts as not accepted
#       nback += evaluations spent
#
# The constants are Tensor Toolbox's except the x10 on a failed line search
# (x3.5 there). A zero entry whose gradient is negative is a free variable,
# so the driver needs no inadmissible-zero fix with this solver.

LS_MAX = 11


def _pdnr_rows(c: Csf) -> torch.Tensor:
    """The rows that have nonzeros, longest first (int32), cached on the Csf
    as the plans are: the order in which the kernel's workgroups are issued."""
    r = getattr(c, "_apr_pdnr_rows", None)
    if r is None:
        cnt = _stream(c)["cnt"]
        order = torch.argsort(cnt, descending=True, stable=True)
        r = order[:int((cnt > 0).sum())].to(torch.int32).contiguous()
        object.__setattr__(c, "_apr_pdnr_rows", r)
    return r


def _pdnr_hip(c: Csf, mats: List[torch.Tensor], B: torch.Tensor,
              inner_tol: float, max_inner: int, eps_div: float,
              mu0: float) -> Tuple:
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    nrows, rank = int(B.shape[0]), int(B.shape[1])
    st = _stream(c)
    dev = c.device
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    # rows with no nonzero keep these zeros, and B = 0
    Phi = torch.zeros(nrows, rank, **f64)
    iters = torch.zeros(nrows, **i32)
    viol0 = torch.zeros(nrows, **f64)
    stats = {"f0": torch.zeros(nrows, **f64), "f": torch.zeros(nrows, **f64),
             "mu": torch.zeros(nrows, **f64),
             "nback": torch.zeros(nrows, **i32),
             "nfail": torch.zeros(nrows, **i32)}
    B.masked_fill_((st["cnt"] == 0).unsqueeze(1), 0.0)
    ms = [mats[c.dim_perm[l]].contiguous() for l in range(1, c.nmodes)]
    native().hip_apr_pdnr(
        st["idx"], ms, st["vals"], st["rowptr"], _pdnr_rows(c),
        float(eps_div), float(inner_tol), int(max_inner), float(mu0), B, Phi,
        iters, viol0, stats["f0"], stats["f"], stats["mu"], stats["nback"],
        stats["nfail"], torch.cuda.current_stream().cuda_stream)
    return Phi, iters, viol0, stats


def _pdnr_torch(c: Csf, mats: List[torch.Tensor], B: torch.Tensor,
                inner_tol: float, max_inner: int, eps_div: float,
                mu0: float) -> Tuple:
    """All rows at once: chunked passes over the key stream build f, Phi and
    the batch of row Hessians, batched torch.linalg factors and solves them,
    and masks carry the rows that have stopped, failed or been accepted. On
    CPU tensors the passes visit only the nonzeros of rows still at work."""
    nrows, rank = int(B.shape[0]), int(B.shape[1])
    st = _stream(c)
    dev, dt = c.device, torch.float64
    cpu = dev.type == "cpu"
    key = st["key"].long()
    idx = [ix.long() for ix in st["idx"]]
    vals = st["vals"]
    ms = [mats[c.dim_perm[l]] for l in range(1, c.nmodes)]

    def run_pass(Bc, full, rows_on):
        """-sum v log m per row (and Phi, H when `full`) at the point Bc."""
        sel = None
        if cpu:
            sel = rows_on[key].nonzero(as_tuple=True)[0]
        n = int(vals.numel()) if sel is None else int(sel.numel())
        fd = torch.zeros(nrows, dtype=dt, device=dev)
        phi = torch.zeros(nrows, rank, dtype=dt, device=dev) if full else None
        H = (torch.zeros(nrows, rank, rank, dtype=dt, device=dev)
             if full else None)
        chunk = max(1, (64 << 20) // ((rank * rank if full else rank) * 8))
        for q0 in range(0, n, chunk):
            q1 = min(n, q0 + chunk)
            q = slice(q0, q1) if sel is None else sel[q0:q1]
            pi = None
            for ix, A in zip(idx, ms):
                gth = A.index_select(0, ix[q])
                pi = gth if pi is None else pi * gth
            k, v = key[q], vals[q]
            mdl = (Bc.index_select(0, k) * pi).sum(1).clamp_min(eps_div)
            fd.index_add_(0, k, -(v * mdl.log()))
            if full:
                phi.index_add_(0, k, (v / mdl).unsqueeze(1) * pi)
                x = (v.sqrt() / mdl).unsqueeze(1) * pi
                H.index_add_(0, k, x.unsqueeze(2) * x.unsqueeze(1))
        return fd, phi, H

    has = st["cnt"] > 0
    B.masked_fill_((~has).unsqueeze(1), 0.0)
    live = has.clone()
    Phi = torch.zeros(nrows, rank, dtype=dt, device=dev)
    iters = torch.zeros(nrows, dtype=torch.int32, device=dev)
    viol0 = torch.zeros(nrows, dtype=dt, device=dev)
    f0 = torch.zeros(nrows, dtype=dt, device=dev)
    fv = torch.zeros(nrows, dtype=dt, device=dev)
    mu = torch.where(has, torch.full_like(fv, mu0), torch.zeros_like(fv))
    nback = torch.zeros(nrows, dtype=torch.int32, device=dev)
    nfail = torch.zeros(nrows, dtype=torch.int32, device=dev)
    eye = torch.eye(rank, dtype=dt, device=dev)
    for l in range(1, max_inner + 1):
        fd, phi, H = run_pass(B, True, live)
        fcur = B.sum(1) + fd
        g = 1.0 - phi
        viol = torch.minimum(B, g).abs().amax(1)
        Phi = torch.where(live.unsqueeze(1), phi, Phi)
        iters = torch.where(live, torch.full_like(iters, l), iters)
        fv = torch.where(live, fcur, fv)
        if l == 1:
            viol0 = torch.where(live, viol, viol0)
            f0 = torch.where(live, fcur, f0)
        if inner_tol > 0:
            live = live & ~(viol < inner_tol)
            if cpu and not bool(live.any()):
                break
        eps_act = (B - (B - g).clamp_min(0.0)).norm(dim=1).clamp_max(1e-8)
        fix = (B == 0) & (g > 0)
        act = (B > 0) & (B <= eps_act.unsqueeze(1)) & (g > 0)
        fre = ~(fix | act)
        ff = fre.unsqueeze(2) & fre.unsqueeze(1)
        Hff = torch.where(ff, H, torch.zeros_like(H))
        # rows and columns that are not free become identity rows
        M = Hff + torch.diag_embed(torch.where(fre, mu.unsqueeze(1),
                                               torch.ones_like(B)))
        M = torch.where(live.view(-1, 1, 1), M, eye)
        L, info = torch.linalg.cholesky_ex(M)
        bad = (info != 0) | ~torch.isfinite(L).all(2).all(1)
        L = torch.where(bad.view(-1, 1, 1), eye, L)
        rhs = torch.where(fre, -g, torch.zeros_like(g))
        df = torch.cholesky_solve(rhs.unsqueeze(2), L).squeeze(2)
        df = torch.where(fre, df, torch.zeros_like(df))
        pred = (g * df).sum(1) + 0.5 * (
            df * torch.bmm(Hff, df.unsqueeze(2)).squeeze(2)).sum(1)
        d = torch.where(fre, df, torch.where(act, -g, torch.zeros_like(g)))
        pending = live & ~bad
        accepted = torch.zeros_like(live)
        fnew, Bn = fcur.clone(), B.clone()
        alpha = 1.0
        for _ in range(LS_MAX):
            if cpu and not bool(pending.any()):
                break
            bn = (B + alpha * d).clamp_min(0.0)
            fn = bn.sum(1) + run_pass(bn, False, pending)[0]
            ok = pending & (fn <= fcur + 1e-4 * (g * (bn - B)).sum(1))
            nback = nback + pending.to(torch.int32)
            Bn = torch.where(ok.unsqueeze(1), bn, Bn)
            fnew = torch.where(ok, fn, fnew)
            accepted = accepted | ok
            pending = pending & ~ok
            alpha *= 0.5
        rho = (fnew - fcur) / pred
        one = torch.ones_like(mu)
        fac = torch.where(pred == 0, 10.0 * one, torch.where(
            rho < 0.25, 3.5 * one, torch.where(rho > 0.75, (2.0 / 7.0) * one,
                                               one)))
        mu = torch.where(accepted, mu * fac,
                         torch.where(live, mu * 10.0, mu))
        nfail = nfail + (live & ~accepted).to(torch.int32)
        fv = torch.where(accepted, fnew, fv)
        B.copy_(torch.where(accepted.unsqueeze(1), Bn, B))
    return Phi, iters, viol0, {"f0": f0, "f": fv, "mu": mu, "nback": nback,
                               "nfail": nfail}


def apr_update_pdnr(src: CsfSet | Csf, mats: Sequence[torch.Tensor],
                    mode: int, B: torch.Tensor, *, inner_tol: float,
                    max_inner: int, eps_div: float = 1e-10,
                    mu0: float = 1e-5, impl: str = "auto") -> Tuple:
    """The CP-APR row update of `mode` by the damped-Newton row solver
    (PDNR, the box above): B is updated IN PLACE by up to `max_inner` Newton
    iterations per row; returns (Phi, iters, viol0, stats) as `apr_update`
    does, with `stats` a dict of per-row tensors: `f0` and `f` (the row
    objective at entry and at exit), `mu` (the damping at exit), `nback`
    (line-search evaluations, int32) and `nfail` (rejected steps, int32).
    Rows without nonzeros get B = Phi = 0 and zeros everywhere else.

    `src`, `mats` and `impl` are as in `apr_update`; `mu0 > 0` is every
    row's initial damping."""
    c, impl = _check_update(src, mats, mode, B, max_inner, eps_div, impl)
    if not mu0 > 0:
        raise ValueError(f"mu0 must be > 0, got {mu0}")
    fn = _pdnr_hip if impl == "hip" else _pdnr_torch
    return fn(c, list(mats), B, float(inner_tol), int(max_inner),
              float(eps_div), float(mu0))


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
    method: str = "mu"        # row solver: "mu" (multiplicative updates) or
    #                           "pdnr" (damped Newton; kappa is not used)
    mu0: float = 1e-5         # pdnr: every row's initial damping


@dataclass
class PoissonKruskal:
    factors: List[torch.Tensor]
    lam: torch.Tensor
    loglik_trace: List[float] = field(default_factory=list)  # negative
    kkt_trace: List[float] = field(default_factory=list)
    inner_trace: List[int] = field(default_factory=list)
    nback_trace: List[int] = field(default_factory=list)  # pdnr: line-search
    #                           evaluations per outer iteration; empty for mu
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
            opts: Optional[AprOptions] = None, **overrides) -> PoissonKruskal:
    """Poisson CPD of a nonnegative (count) tensor by CP-APR. Keyword
    arguments override the fields of `opts` (or of the defaults).

    Each outer iteration updates the modes in order with `apr_update`
    (`method="mu"`) or `apr_update_pdnr` (`method="pdnr"`, which also
    records its line-search evaluations in `nback_trace`) and records the
    negative log-likelihood, the largest first-iteration KKT violation
    over all rows and modes, and the inner iterations spent. It
    has converged when that violation is below `tolerance`. The returned
    factors are nonnegative with columns summing to 1 (or all zero), the
    weights in `lam`."""
    opts = opts or AprOptions()
    if overrides:
        opts = replace(opts, **overrides)
    if opts.method not in ("mu", "pdnr"):
        raise ValueError(f"unknown method {opts.method!r} (mu, pdnr)")
    pdnr = opts.method == "pdnr"
    if pdnr and not opts.mu0 > 0:
        raise ValueError(f"mu0 must be > 0, got {opts.mu0}")
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
        kkt, inner, nback = 0.0, 0, 0
        for m in range(nm):
            A = factors[m]
            if it > 0 and not pdnr:
                # inadmissible zeros: an entry stuck at 0 whose gradient
                # says it should grow would stay 0 under a multiplicative
                # update
                A = A + opts.kappa * ((A < opts.kappa_tol)
                                      & (phi_prev[m] > 1.0)).to(A.dtype)
            B = (A * lam).contiguous()
            if pdnr:
                phi_prev[m], iters, viol0, stats = apr_update_pdnr(
                    cs, factors, m, B, inner_tol=tol,
                    max_inner=opts.max_inner, eps_div=opts.eps_div,
                    mu0=opts.mu0)
                nback += int(stats["nback"].sum())
            else:
                phi_prev[m], iters, viol0 = apr_update(
                    cs, factors, m, B, inner_tol=tol,
                    max_inner=opts.max_inner, eps_div=opts.eps_div)
            lam = B.sum(0)
            factors[m] = B / torch.where(lam > 0, lam, torch.ones_like(lam))
            kkt = max(kkt, float(viol0.max()))
            inner += int(iters.sum())
        ll = poisson_loglik(factors, lam, tinds, tvals, opts.eps_div)
        res.loglik_trace.append(ll)
        res.kkt_trace.append(kkt)
        res.inner_trace.append(inner)
        if pdnr:
            res.nback_trace.append(nback)
        res.niters = it + 1
        if opts.verbose:
            print(f"  its = {it + 1} loglik = {ll:.8e} kkt = {kkt:.3e} "
                  f"inner = {inner}" + (f" evals = {nback}" if pdnr else ""))
        if kkt < tol:
            res.converged = True
            break
    res.lam = lam
    return res
