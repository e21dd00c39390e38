"""Tensor completion: ALS over the OBSERVED entries only.

CPD-ALS (cpd.py) treats a sparse tensor's absent entries as zeros. For
ratings / tag tensors an absent entry means "unknown", and the model to fit
is  min sum_{x in Omega} (val_x - model_x)^2 + reg * sum_m ||A_m||_F^2.
Its ALS update is row-wise: for output mode m and row i, with Omega_i the
observed entries whose mode-m index is i and h_x the Hadamard product of the
other modes' factor rows at x,

    A_m[i,:] = (sum_{Omega_i} h_x h_x^T + reg*I)^-1  sum_{Omega_i} val_x h_x

Device path: csrc/hip/complete_als.hip (MFMA normal equations + in-LDS
Cholesky per row; no atomics). `impl="torch"` is the vectorised torch
implementation — the CPU path, and the benchmark baseline on device.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from splatt_amd._ext import native
from splatt_amd.cpd import seeded_init
from splatt_amd.csf import Csf, CsfSet, csf_alloc
from splatt_amd.sptensor import SpTensor

# Nonzeros per segment of the HIP kernel (one wave per segment). The
# epilogue of a segment costs about as much as a few hundred nonzeros of
# accumulation (a Cholesky, or an F^2-sized workspace store), so segments
# should be several hundred nonzeros at least; 1024 keeps a multi-segment
# row's workspace traffic under 2% of its gathered bytes while still cutting
# a 77M-nnz stream into ~85k independent waves.
SEG = 1024
MAX_RANK = 64

_ALL_HINT = ("build the tensor with csf_alloc='all' (every mode at depth 0 "
             "of a key-sorted stream)")


# ----------------------------------------------------------------- streams

def _resolve(src: CsfSet | Csf, mode: int) -> Csf:
    if isinstance(src, CsfSet):
        if not 0 <= mode < src.nmodes:
            raise IndexError(f"mode {mode} out of range for {src.nmodes} modes")
        c, depth = src.csfs[src.mode_csf[mode]], src.mode_depth[mode]
    else:
        if not 0 <= mode < src.nmodes:
            raise IndexError(f"mode {mode} out of range for {src.nmodes} modes")
        c, depth = src, src.level_of_mode(mode)
    if depth != 0:
        raise ValueError(
            f"completion needs mode {mode} at the root of its CSF, got depth "
            f"{depth}; {_ALL_HINT}")
    if getattr(c, "_stage", None) is not None:
        raise ValueError(
            "completion does not support bucketed / LDS-staged streams; "
            + _ALL_HINT)
    if c.vals.dtype != torch.float64:
        raise ValueError(
            f"completion supports float64 tensors only, got {c.vals.dtype} "
            "(load the tensor as f64)")
    return c


def _stream(c: Csf) -> dict:
    """Root-sorted stream of a Csf for the completion kernels, cached on the
    Csf: contiguous int32 index columns of the non-root levels, per-row
    counts and the row pointer."""
    st = getattr(c, "_cmpl_stream", None)
    if st is not None:
        return st
    key = c.ancestor_expand(0)
    if key.numel() > 1 and not bool((key[1:] >= key[:-1]).all()):
        raise ValueError("completion needs a key-sorted stream; " + _ALL_HINT)
    nrows = c.dims[c.dim_perm[0]]
    cnt = torch.bincount(key.long(), minlength=nrows)
    rowptr = torch.zeros(nrows + 1, dtype=torch.int64, device=c.device)
    torch.cumsum(cnt, 0, out=rowptr[1:])
    st = {
        "idx": [c.ancestor_expand(l).to(torch.int32).contiguous()
                for l in range(1, c.nmodes)],
        "key": key,
        "vals": c.vals.contiguous(),
        "cnt": cnt,
        "rowptr": rowptr,
        "nrows": nrows,
    }
    object.__setattr__(c, "_cmpl_stream", st)
    return st


def workspace_budget_bytes() -> int:
    """Byte budget of the multi-segment-row workspace (SPLATT_COMPLETE_MB,
    default 1024; fractions allowed)."""
    return int(float(os.environ.get("SPLATT_COMPLETE_MB", "1024")) * (1 << 20))


def slot_bytes(rank: int) -> int:
    """Workspace bytes one segment of a multi-segment row occupies."""
    return int(native().complete_slot_elems(rank)) * 8


def _cap_slots(rank: int) -> int:
    return max(1, workspace_budget_bytes() // slot_bytes(rank))


def _plan(c: Csf, cap: int) -> dict:
    """Segment descriptors for the HIP kernels, cached per slot capacity.

    Every row with observed entries is cut into segments of SEG nonzeros
    (the last one shorter); no segment crosses a row. Rows of one segment
    come first in the descriptor arrays (slot -1: solved in place), then the
    segments of multi-segment rows in stream order, numbered by workspace
    slot. A row with more than `cap` segments gets proportionally longer
    segments so that any single row fits the workspace. `batches` cuts the
    multi-segment rows into runs whose slots fit `cap`."""
    cache = getattr(c, "_cmpl_plan", None)
    if cache is None:
        cache = {}
        object.__setattr__(c, "_cmpl_plan", cache)
    if cap in cache:
        return cache[cap]
    st = _stream(c)
    dev = c.device
    cnt, rowptr, nrows = st["cnt"], st["rowptr"], st["nrows"]
    slen = torch.full_like(cnt, SEG)
    nseg = (cnt + (SEG - 1)) // SEG
    big = nseg > cap
    if bool(big.any()):
        grown = ((cnt + (cap - 1)) // cap + 3) // 4 * 4
        slen = torch.where(big, grown, slen)
        nseg = (cnt + slen - 1) // slen
    rows = torch.repeat_interleave(torch.arange(nrows, device=dev), nseg)
    first = torch.cumsum(nseg, 0) - nseg
    j = torch.arange(rows.numel(), device=dev) - first[rows]
    start = rowptr[rows] + j * slen[rows]
    length = torch.minimum(slen[rows], cnt[rows] - j * slen[rows])
    multi = nseg[rows] > 1
    order = torch.argsort(multi.to(torch.int8), stable=True)
    nsingle = int((~multi).sum())
    nmseg = int(rows.numel()) - nsingle
    slot = torch.full((rows.numel(),), -1, dtype=torch.int32, device=dev)
    slot[nsingle:] = torch.arange(nmseg, dtype=torch.int32, device=dev)
    mrow = (nseg > 1).nonzero(as_tuple=True)[0]
    mslot = torch.zeros(mrow.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nseg[mrow], 0, out=mslot[1:])
    # batches of whole rows whose slots fit the workspace: (m0, m1, s0, s1)
    ms = mslot.cpu().tolist()
    batches = []
    m0 = 0
    while m0 < len(ms) - 1:
        m1 = m0 + 1
        while m1 < len(ms) - 1 and ms[m1 + 1] - ms[m0] <= cap:
            m1 += 1
        batches.append((m0, m1, ms[m0], ms[m1]))
        m0 = m1
    plan = {
        "seg_start": start[order].contiguous(),
        "seg_len": length[order].to(torch.int32).contiguous(),
        "seg_row": rows[order].to(torch.int32).contiguous(),
        "seg_slot": slot,
        "nsingle": nsingle,
        "mrow": mrow.to(torch.int32).contiguous(),
        "mslot": mslot,
        "batches": batches,
        "max_slots": max([b[3] - b[2] for b in batches], default=0),
    }
    cache[cap] = plan
    return plan


def completion_plan(src: CsfSet | Csf, mode: int, rank: int) -> dict:
    """The segment plan `complete_update(impl="hip")` uses for this mode and
    rank under the current SPLATT_COMPLETE_MB (for inspection and tests)."""
    return _plan(_resolve(src, mode), _cap_slots(rank))


# ------------------------------------------------------------ row update

def _update_hip(c: Csf, mats: List[torch.Tensor], reg: float,
                out: torch.Tensor) -> None:
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    rank = int(out.shape[1])
    st = _stream(c)
    plan = _plan(c, _cap_slots(rank))
    need = max(1, plan["max_slots"] * int(native().complete_slot_elems(rank)))
    ws = getattr(c, "_cmpl_ws", None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float64, device=c.device)
        object.__setattr__(c, "_cmpl_ws", ws)
    ms = [mats[c.dim_perm[l]].contiguous() for l in range(1, c.nmodes)]
    stream = torch.cuda.current_stream().cuda_stream
    # rows with no observed entry solve reg*I*a = 0: exact zeros
    out.zero_()

    def launch(seg0, nseg, m0, nm, slot0, nslots):
        native().gpu_complete_update(
            st["idx"], ms, st["vals"], plan["seg_start"], plan["seg_len"],
            plan["seg_row"], plan["seg_slot"], seg0, nseg, plan["mrow"],
            plan["mslot"], m0, nm, slot0, nslots, float(reg), ws, out, stream)

    nsingle = plan["nsingle"]
    launch(0, nsingle, 0, 0, 0, 0)
    for m0, m1, s0, s1 in plan["batches"]:
        launch(nsingle + s0, s1 - s0, m0, m1 - m0, s0, s1 - s0)


def _update_torch(c: Csf, mats: List[torch.Tensor], reg: float,
                  out: torch.Tensor) -> None:
    """Chunked index_add_ of h (x) h into per-row normal matrices, then a
    batched Cholesky solve. Rows are processed in blocks so the F x F
    matrices never exceed ~256 MB."""
    rank = int(out.shape[1])
    st = _stream(c)
    dev, dt = c.device, torch.float64
    nrows = st["nrows"]
    rowptr = st["rowptr"].cpu()
    key = st["key"]
    idx = st["idx"]
    vals = st["vals"]
    ms = [mats[c.dim_perm[l]] for l in range(1, c.nmodes)]
    ff = rank * rank
    rblock = max(1, (256 << 20) // (ff * 8))
    nchunk = max(1, (256 << 20) // (ff * 8))
    eye = torch.eye(rank, dtype=dt, device=dev)
    for r0 in range(0, nrows, rblock):
        r1 = min(nrows, r0 + rblock)
        N = torch.zeros(r1 - r0, ff, dtype=dt, device=dev)
        b = torch.zeros(r1 - r0, rank, dtype=dt, device=dev)
        p0, p1 = int(rowptr[r0]), int(rowptr[r1])
        for q0 in range(p0, p1, nchunk):
            q1 = min(p1, q0 + nchunk)
            h = None
            for ix, A in zip(idx, ms):
                g = A.index_select(0, ix[q0:q1].long())
                h = g if h is None else h * g
            k = key[q0:q1].long() - r0
            N.index_add_(0, k, (h.unsqueeze(2) * h.unsqueeze(1)).view(-1, ff))
            b.index_add_(0, k, h * vals[q0:q1].unsqueeze(1))
        N = N.view(-1, rank, rank) + reg * eye
        L = torch.linalg.cholesky(N)
        out[r0:r1] = torch.cholesky_solve(b.unsqueeze(2), L).squeeze(2)
    # a row with no observed entry is the solution of reg*I*a = 0
    out[st["cnt"] == 0] = 0.0


def complete_update(src: CsfSet | Csf, mats: Sequence[torch.Tensor],
                    mode: int, reg: float,
                    out: Optional[torch.Tensor] = None,
                    impl: str = "auto") -> torch.Tensor:
    """One row-wise completion update of `mode`'s factor; `mats` indexed by
    tensor mode (the entry for `mode` itself is not read).

    `src` must hold `mode` at depth 0 of a key-sorted stream — any
    csf_alloc(t, "all") build. `impl`: "hip" (the gfx950 kernels; default on
    device tensors), "torch" (vectorised torch: the CPU path, and a
    baseline that also runs on device tensors when asked — never chosen
    automatically there)."""
    if not reg > 0:
        raise ValueError(f"reg must be > 0 (got {reg}): the row systems are "
                         "only guaranteed SPD with a ridge term")
    c = _resolve(src, mode)
    mats = list(mats)
    if len(mats) != c.nmodes:
        raise ValueError(f"need {c.nmodes} factor matrices, got {len(mats)}")
    rank = int(mats[0].shape[1])
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"completion supports rank 1..{MAX_RANK}, got {rank}")
    if c.nmodes < 3 or c.nmodes > 8:
        raise ValueError(f"completion supports 3..8 modes, got {c.nmodes}")
    for m, A in enumerate(mats):
        if tuple(A.shape) != (c.dims[m], rank):
            raise ValueError(f"factor {m} has shape {tuple(A.shape)}, "
                             f"expected ({c.dims[m]}, {rank})")
        if A.dtype != torch.float64 or A.device != c.device:
            raise ValueError(
                f"factor {m}: dtype/device {A.dtype}/{A.device} does not "
                f"match tensor {c.vals.dtype}/{c.device}")
    if impl == "auto":
        impl = "hip" if c.device.type == "cuda" else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto)")
    if impl == "hip" and c.device.type != "cuda":
        raise ValueError("impl='hip' needs a device tensor")
    if out is None:
        out = torch.empty(c.dims[mode], rank, dtype=torch.float64,
                          device=c.device)
    elif (tuple(out.shape) != (c.dims[mode], rank) or not out.is_contiguous()
          or out.dtype != torch.float64 or out.device != c.device):
        raise ValueError("out must be a contiguous float64 "
                         f"({c.dims[mode]}, {rank}) tensor on {c.device}")
    if impl == "hip":
        _update_hip(c, mats, reg, out)
    else:
        _update_torch(c, mats, reg, out)
    return out


# ------------------------------------------------------------ evaluation

def kruskal_predict(factors: Sequence[torch.Tensor], inds: torch.Tensor,
                    lam: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Model values sum_f lam_f prod_t A_t[inds[t][p], f] at the COO
    coordinates `inds` ([nmodes, n] int64). HIP on device, torch on CPU."""
    factors = list(factors)
    dev = factors[0].device
    if not isinstance(inds, torch.Tensor):
        inds = torch.stack([torch.as_tensor(i) for i in inds], 0)
    if inds.dim() != 2 or inds.shape[0] != len(factors):
        raise ValueError(f"inds must be [{len(factors)}, n], got "
                         f"{tuple(inds.shape)}")
    inds = inds.to(device=dev, dtype=torch.int64).contiguous()
    n = int(inds.shape[1])
    rank = int(factors[0].shape[1])
    if dev.type == "cuda":
        if any(A.dtype != torch.float64 for A in factors):
            raise ValueError("kruskal_predict on device supports float64 "
                             "factors only")
        if len(factors) > 8:
            raise ValueError("kruskal_predict supports up to 8 modes")
        out = torch.empty(n, dtype=torch.float64, device=dev)
        lm = None if lam is None else lam.to(dev, torch.float64).contiguous()
        native().gpu_kruskal_predict(
            inds, [A.contiguous() for A in factors], lm, out,
            torch.cuda.current_stream().cuda_stream)
        return out
    w = torch.ones(n, rank, dtype=torch.float64) if lam is None \
        else lam.double().unsqueeze(0).expand(n, -1).clone()
    for m, A in enumerate(factors):
        w *= A.double().index_select(0, inds[m])
    return w.sum(dim=1)


def rmse(factors: Sequence[torch.Tensor], t: SpTensor) -> float:
    """Root-mean-square error of the model on the entries of `t`."""
    if t.nnz == 0:
        return 0.0
    dev = factors[0].device
    pred = kruskal_predict(factors, t.inds.to(dev))
    return float((t.vals.to(dev).double() - pred).square().mean().sqrt())


# ------------------------------------------------------------------ driver

@dataclass
class CompleteOptions:
    max_iters: int = 50
    regularize: float = 1e-2
    tolerance: float = 1e-4   # <= 0: always run max_iters
    seed: int = 0x5EED5EED
    verbose: bool = False


@dataclass
class Completion:
    factors: List[torch.Tensor]
    objective_trace: List[float] = field(default_factory=list)
    rmse_train_trace: List[float] = field(default_factory=list)
    rmse_val_trace: List[float] = field(default_factory=list)
    niters: int = 0
    best_iter: int = 0        # index into the traces


def _train_coo(cs: CsfSet) -> tuple:
    """COO view (inds [nmodes, nnz] int64, vals) of an ALLMODE set's first
    stream — the training entries for the objective / RMSE."""
    c = cs.csfs[0]
    cols = [None] * c.nmodes
    for l in range(c.nmodes):
        cols[c.dim_perm[l]] = c.ancestor_expand(l).long()
    return torch.stack(cols, 0).contiguous(), c.vals


def complete_als(train: SpTensor | CsfSet, rank: int,
                 opts: Optional[CompleteOptions] = None,
                 validate: Optional[SpTensor] = None) -> Completion:
    """Regularised tensor completion by ALS over the observed entries.

    Each iteration updates the modes in order and records the regularised
    objective sum_train (x - model)^2 + reg * sum_m ||A_m||_F^2, the train
    RMSE and (with `validate`) the validation RMSE. It stops when the
    relative improvement — of the validation RMSE if given, else of the
    objective — falls below `tolerance`. With validation data the returned
    factors are those of the best-validation iteration."""
    opts = opts or CompleteOptions()
    if isinstance(train, SpTensor):
        if train.dtype != torch.float64:
            raise ValueError("completion supports float64 tensors only, got "
                             f"{train.dtype} (load the tensor as f64)")
        cs = csf_alloc(train, "all")
    else:
        cs = train
    nm, dims = cs.nmodes, cs.dims
    for m in range(nm):
        _resolve(cs, m)
    dev = cs.csfs[0].device
    reg = float(opts.regularize)
    tinds, tvals = _train_coo(cs)
    nnz = max(1, int(tvals.numel()))
    factors = [seeded_init(dims[m], rank, m, opts.seed).to(dev)
               for m in range(nm)]
    res = Completion(factors=factors)
    best, best_factors = math.inf, None
    prev = None
    for it in range(opts.max_iters):
        for m in range(nm):
            factors[m] = complete_update(cs, factors, m, reg)
        sse = float((tvals - kruskal_predict(factors, tinds)).square().sum())
        obj = sse + reg * sum(float(A.square().sum()) for A in factors)
        res.objective_trace.append(obj)
        res.rmse_train_trace.append(math.sqrt(sse / nnz))
        metric = obj
        if validate is not None:
            metric = rmse(factors, validate)
            res.rmse_val_trace.append(metric)
            if metric < best:
                best, res.best_iter = metric, it
                best_factors = [A.clone() for A in factors]
        else:
            res.best_iter = it
        res.niters = it + 1
        if opts.verbose:
            line = (f"  its = {it + 1} obj = {obj:.6e} "
                    f"rmse-train = {res.rmse_train_trace[-1]:.5f}")
            if validate is not None:
                line += f" rmse-val = {metric:.5f}"
            print(line)
        if prev is not None and opts.tolerance > 0:
            improve = (prev - metric) / max(abs(prev), 1e-300)
            if improve < opts.tolerance:
                break
        prev = metric
    res.factors = best_factors if best_factors is not None else factors
    return res
