"""Sparse Tucker decomposition: TTMc and HOOI.

The Tucker model is a small dense core G (R_1 x .. x R_N) times one
orthonormal factor U_m (I_m x R_m) per mode. HOOI (higher-order orthogonal
iteration) updates one mode at a time: with every other factor fixed,

    Y_n[i, :] = sum_{x in Omega_i} val_x * KRON_{t != n} U_t[i_t(x), :]

(the TTMc, "tensor times matrix chain", of width P_n = prod_{t != n} R_t)
and U_n becomes the leading R_n left singular vectors of Y_n.

Device path: csrc/hip/ttmc.hip (MFMA, no atomics, bitwise reproducible).
`impl="torch"` is chunked gather + Kronecker + index_add_: the CPU path, and
the benchmark baseline on device.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from splatt_amd._ext import native
from splatt_amd.completion import SEG, _plan, _stream
from splatt_amd.cpd import seeded_init
from splatt_amd.csf import Csf, CsfSet, csf_alloc
from splatt_amd.sptensor import SpTensor

MAX_RANK = 32     # per mode
MAX_COLS = 4096   # widest P_n of the HIP kernel (ttmc.hip)

_ALL_HINT = ("build the tensor with csf_alloc='all' (every mode at depth 0 "
             "of a key-sorted stream)")


def _resolve(src: CsfSet | Csf, mode: int) -> Csf:
    if not isinstance(src, (CsfSet, Csf)):
        raise TypeError(f"ttmc needs a CsfSet or Csf, got {type(src).__name__}")
    if not 0 <= mode < src.nmodes:
        raise IndexError(f"mode {mode} out of range for {src.nmodes} modes")
    if isinstance(src, CsfSet):
        c, depth = src.csfs[src.mode_csf[mode]], src.mode_depth[mode]
    else:
        c, depth = src, src.level_of_mode(mode)
    if depth != 0:
        raise ValueError(
            f"ttmc needs mode {mode} at the root of its CSF, got depth "
            f"{depth}; {_ALL_HINT}")
    if getattr(c, "_stage", None) is not None:
        raise ValueError(
            "ttmc does not support bucketed / LDS-staged streams; "
            + _ALL_HINT)
    if c.vals.dtype != torch.float64:
        raise ValueError(
            f"ttmc supports float64 tensors only, got {c.vals.dtype} "
            "(load the tensor as f64)")
    return c


# --------------------------------------------------------------- workspace

def workspace_budget_bytes() -> int:
    """Byte budget of the multi-segment-row workspace (SPLATT_TTMC_MB,
    default 1024; fractions allowed)."""
    return int(float(os.environ.get("SPLATT_TTMC_MB", "1024")) * (1 << 20))


def slot_bytes(cols: int) -> int:
    """Workspace bytes one segment of a multi-segment row occupies: one
    output row."""
    return int(cols) * 8


def _cap_slots(cols: int) -> int:
    return max(1, workspace_budget_bytes() // slot_bytes(cols))


def ttmc_plan(src: CsfSet | Csf, mode: int, cols: int) -> dict:
    """The segment plan `ttmc(impl="hip")` uses for this mode and output
    width under the current SPLATT_TTMC_MB (for inspection and tests)."""
    return _plan(_resolve(src, mode), _cap_slots(cols))


# -------------------------------------------------------------------- TTMc

def _ttmc_hip(c: Csf, ms: List[torch.Tensor], out: torch.Tensor) -> None:
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    cols = int(out.shape[1])
    st = _stream(c)
    plan = _plan(c, _cap_slots(cols))
    need = max(1, plan["max_slots"] * cols)
    ws = getattr(c, "_ttmc_ws", None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float64, device=c.device)
        object.__setattr__(c, "_ttmc_ws", ws)
    stream = torch.cuda.current_stream().cuda_stream
    # rows with no nonzero are exact zeros
    out.zero_()

    def launch(seg0, nseg, m0, nm, slot0, nslots):
        native().gpu_ttmc(
            st["idx"], ms, st["vals"], plan["seg_start"], plan["seg_len"],
            plan["seg_row"], plan["seg_slot"], seg0, nseg, plan["mrow"],
            plan["mslot"], m0, nm, slot0, nslots, ws, out, stream)

    nsingle = plan["nsingle"]
    launch(0, nsingle, 0, 0, 0, 0)
    for m0, m1, s0, s1 in plan["batches"]:
        launch(nsingle + s0, s1 - s0, m0, m1 - m0, s0, s1 - s0)


def _ttmc_torch(c: Csf, ms: List[torch.Tensor], out: torch.Tensor) -> None:
    """Chunks of the stream: gather the level rows, build the val-scaled
    Kronecker row of every nonzero, index_add_ into the output rows. A
    chunk's nnz x P intermediate stays under ~256 MB."""
    cols = int(out.shape[1])
    st = _stream(c)
    key, idx, vals = st["key"], st["idx"], st["vals"]
    nnz = int(vals.numel())
    nchunk = max(1, (256 << 20) // (cols * 8))
    out.zero_()
    for q0 in range(0, nnz, nchunk):
        q1 = min(nnz, q0 + nchunk)
        h = vals[q0:q1].unsqueeze(1) * ms[0].index_select(0, idx[0][q0:q1].long())
        for ix, A in zip(idx[1:], ms[1:]):
            g = A.index_select(0, ix[q0:q1].long())
            h = (h.unsqueeze(2) * g.unsqueeze(1)).reshape(q1 - q0, -1)
        out.index_add_(0, key[q0:q1].long(), h)


def _pick_impl(impl: str, c: Csf, cols: int) -> str:
    if impl == "auto":
        if c.device.type != "cuda":
            return "torch"
        return "hip" if cols <= MAX_COLS else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto)")
    if impl == "hip":
        if c.device.type != "cuda":
            raise ValueError("impl='hip' needs a device tensor")
        if cols > MAX_COLS:
            raise ValueError(
                f"impl='hip' supports at most {MAX_COLS} output columns, got "
                f"{cols}; use impl='torch' (impl='auto' does)")
    return impl


def _ttmc_levels(c: Csf, mats: Sequence[torch.Tensor], impl: str,
                 out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TTMc of the root mode of `c` as a contiguous [rows, P] matrix whose
    columns are in CSF level order (level 1 slowest)."""
    ms = [mats[c.dim_perm[l]].contiguous() for l in range(1, c.nmodes)]
    cols = math.prod(int(A.shape[1]) for A in ms)
    impl = _pick_impl(impl, c, cols)
    nrows = c.dims[c.dim_perm[0]]
    if out2 is None:
        out2 = torch.empty(nrows, cols, dtype=torch.float64, device=c.device)
    if impl == "hip":
        _ttmc_hip(c, ms, out2)
    else:
        _ttmc_torch(c, ms, out2)
    return out2


def _check_mats(c: Csf, mats: Sequence[torch.Tensor], mode: int) -> list:
    mats = list(mats)
    if len(mats) != c.nmodes:
        raise ValueError(f"need {c.nmodes} factor matrices, got {len(mats)}")
    if c.nmodes < 3 or c.nmodes > 8:
        raise ValueError(f"ttmc supports 3..8 modes, got {c.nmodes}")
    for m, A in enumerate(mats):
        if m == mode:
            continue
        if A.dim() != 2 or A.shape[0] != c.dims[m]:
            raise ValueError(f"factor {m} has shape {tuple(A.shape)}, "
                             f"expected ({c.dims[m]}, R_{m})")
        if not 1 <= A.shape[1] <= MAX_RANK:
            raise ValueError(f"ttmc supports rank 1..{MAX_RANK} per mode, "
                             f"factor {m} has rank {A.shape[1]}")
        if A.dtype != torch.float64 or A.device != c.device:
            raise ValueError(
                f"factor {m}: dtype/device {A.dtype}/{A.device} does not "
                f"match tensor {c.vals.dtype}/{c.device}")
    return mats


def ttmc(src: CsfSet | Csf, mats: Sequence[torch.Tensor], mode: int,
         out: Optional[torch.Tensor] = None,
         impl: str = "auto") -> torch.Tensor:
    """Y[i, r_t1, .., r_tk] = sum over the nonzeros x of row i of `mode` of
    val_x * prod_t mats[t][i_t(x), r_t], t over the other modes in ascending
    tensor-mode order; `mats` indexed by tensor mode (the entry for `mode`
    itself is not read).

    `src` must hold `mode` at depth 0 of a key-sorted stream — any
    csf_alloc(t, "all") build. `impl`: "hip" (the gfx950 kernel; default on
    device tensors while the row width P = prod R_t is at most MAX_COLS),
    "torch" (the CPU path, and a baseline that also runs on device tensors).
    The kernel computes in CSF level order; the result may be a permuted
    view of that buffer."""
    c = _resolve(src, mode)
    mats = _check_mats(c, mats, mode)
    levels = [c.dim_perm[l] for l in range(1, c.nmodes)]
    others = sorted(levels)
    nrows = c.dims[mode]
    shape = (nrows, *[int(mats[m].shape[1]) for m in others])
    lshape = (nrows, *[int(mats[m].shape[1]) for m in levels])
    perm = [0] + [1 + levels.index(m) for m in others]
    direct = levels == others
    if out is not None and (
            tuple(out.shape) != shape or not out.is_contiguous()
            or out.dtype != torch.float64 or out.device != c.device):
        raise ValueError(f"out must be a contiguous float64 {shape} tensor "
                         f"on {c.device}")
    if out is not None and direct:
        _ttmc_levels(c, mats, impl, out.view(nrows, -1))
        return out
    y = _ttmc_levels(c, mats, impl).view(lshape).permute(perm)
    if out is None:
        return y
    out.copy_(y)
    return out


# -------------------------------------------------------------------- HOOI

@dataclass
class TuckerOptions:
    max_iters: int = 50
    tol: float = 1e-5         # <= 0: always run max_iters
    seed: int = 0x5EED5EED
    verbosity: int = 0


@dataclass
class Tucker:
    core: torch.Tensor                 # [R_0, .., R_{N-1}], tensor-mode order
    factors: List[torch.Tensor]        # [dims[m], R_m], orthonormal columns
    fit: float = 0.0
    fit_trace: List[float] = field(default_factory=list)
    iters: int = 0

    def to(self, device) -> "Tucker":
        return Tucker(self.core.to(device),
                      [U.to(device) for U in self.factors], self.fit,
                      list(self.fit_trace), self.iters)

    def predict(self, inds) -> torch.Tensor:
        """Model values at the COO coordinates `inds` ([nmodes, n] int64).
        Plain torch, chunked so that the widest intermediate stays under
        ~256 MB."""
        nm = len(self.factors)
        dev = self.core.device
        if not isinstance(inds, torch.Tensor):
            inds = torch.stack([torch.as_tensor(i) for i in inds], 0)
        if inds.dim() != 2 or inds.shape[0] != nm:
            raise ValueError(f"inds must be [{nm}, n], got "
                             f"{tuple(inds.shape)}")
        inds = inds.to(device=dev, dtype=torch.int64)
        n = int(inds.shape[1])
        r0 = int(self.core.shape[0])
        rest = self.core.numel() // r0
        g0 = self.core.reshape(r0, rest)
        out = torch.empty(n, dtype=self.core.dtype, device=dev)
        chunk = max(1, (256 << 20) // (max(rest, r0) * 8))
        for q0 in range(0, n, chunk):
            q1 = min(n, q0 + chunk)
            x = self.factors[0].index_select(0, inds[0, q0:q1]) @ g0
            for m in range(1, nm):
                u = self.factors[m].index_select(0, inds[m, q0:q1])
                x = (x.view(q1 - q0, u.shape[1], -1) * u.unsqueeze(2)).sum(1)
            out[q0:q1] = x.view(-1)
        return out


def _leading_left(Y: torch.Tensor, r: int) -> torch.Tensor:
    """The leading r left singular vectors of Y [I, P], each column signed
    so that its largest-magnitude entry is positive. I >= P goes through a
    QR and the SVD of the P x P triangle, else a direct thin SVD."""
    if Y.shape[0] >= Y.shape[1]:
        Q, R = torch.linalg.qr(Y)
        W = torch.linalg.svd(R, full_matrices=False)[0]
        U = Q @ W[:, :r]
    else:
        U = torch.linalg.svd(Y, full_matrices=False)[0][:, :r]
    big = U.abs().argmax(dim=0)
    sgn = torch.sign(U[big, torch.arange(r, device=U.device)])
    sgn = torch.where(sgn == 0, torch.ones_like(sgn), sgn)
    return (U * sgn).contiguous()


def _norm2(c: Csf) -> float:
    """||X||^2 of the tensor a stream stands for. Repeated coordinates add
    up in the TTMc, so they add up here as well: they are neighbours in the
    sorted stream and are merged before squaring."""
    st = _stream(c)
    vals = st["vals"]
    if vals.numel() < 2:
        return float(vals.square().sum())
    same = st["key"][1:] == st["key"][:-1]
    for ix in st["idx"]:
        same &= ix[1:] == ix[:-1]
    if not bool(same.any()):
        return float(vals.square().sum())
    group = torch.zeros(vals.numel(), dtype=torch.int64, device=vals.device)
    torch.cumsum((~same).long(), 0, out=group[1:])
    merged = torch.zeros(int(group[-1]) + 1, dtype=vals.dtype,
                         device=vals.device)
    merged.index_add_(0, group, vals)
    return float(merged.square().sum())


def tucker_hooi(t: SpTensor | CsfSet, ranks: Sequence[int],
                opts: Optional[TuckerOptions] = None) -> Tucker:
    """Tucker decomposition of a sparse tensor by HOOI.

    Factors start as the Q of a QR of `seeded_init`. Every iteration
    updates the modes in order (TTMc, then the leading R_n left singular
    vectors); after the last mode the core is G = U_N^T Y_N and
    fit = 1 - sqrt(max(||X||^2 - ||G||^2, 0)) / ||X||. Stops when the fit
    changes by less than `tol`."""
    opts = opts or TuckerOptions()
    if t.nmodes < 3 or t.nmodes > 8:
        raise ValueError(f"tucker supports 3..8 modes, got {t.nmodes}")
    if isinstance(t, SpTensor):
        if t.dtype != torch.float64:
            raise ValueError("tucker supports float64 tensors only, got "
                             f"{t.dtype} (load the tensor as f64)")
        cs = csf_alloc(t, "all")
    else:
        cs = t
    nm, dims = cs.nmodes, list(cs.dims)
    ranks = [int(r) for r in ranks]
    if len(ranks) != nm:
        raise ValueError(f"need {nm} ranks, got {len(ranks)}")
    for n in range(nm):
        pn = math.prod(ranks[:n] + ranks[n + 1:])
        if not 1 <= ranks[n] <= min(dims[n], pn, MAX_RANK):
            raise ValueError(
                f"rank of mode {n} must be in 1..min(dims[{n}]={dims[n]}, "
                f"P_{n}={pn}, {MAX_RANK}), got {ranks[n]}")
    csfs = [_resolve(cs, n) for n in range(nm)]
    dev = csfs[0].device
    xnorm2 = _norm2(csfs[0])
    xnorm = math.sqrt(xnorm2)
    factors = [
        torch.linalg.qr(seeded_init(dims[m], ranks[m], m, opts.seed))[0]
        .contiguous().to(dev) for m in range(nm)]
    res = Tucker(core=torch.zeros(ranks, dtype=torch.float64, device=dev),
                 factors=factors)
    prev = None
    for it in range(opts.max_iters):
        for n in range(nm):
            Y = _ttmc_levels(csfs[n], factors, "auto")
            factors[n] = _leading_left(Y, ranks[n])
        # core from the last mode's Y (level order), to tensor-mode order
        c = csfs[nm - 1]
        axes = list(c.dim_perm)
        G = (factors[nm - 1].T @ Y).view([ranks[m] for m in axes])
        res.core = G.permute([axes.index(m) for m in range(nm)]).contiguous()
        gnorm2 = float(res.core.square().sum())
        fit = 1.0 - math.sqrt(max(xnorm2 - gnorm2, 0.0)) / xnorm \
            if xnorm > 0 else 1.0
        res.fit_trace.append(fit)
        res.fit, res.iters = fit, it + 1
        if opts.verbosity > 0:
            print(f"  its = {it + 1} fit = {fit:.6f}")
        if prev is not None and opts.tol > 0 and abs(fit - prev) < opts.tol:
            break
        prev = fit
    return res
