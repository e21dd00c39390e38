"""Stochastic generalized CPD (Kolda & Hong, "Stochastic gradients for
large-scale tensor decomposition", 2020; `gcp_opt` with Adam in Tensor
Toolbox): a CP model fitted under an elementwise loss over ALL cells of a
sparse tensor by Adam on sampled gradients.

Here the tensor is the whole array: A CELL THAT IS NOT STORED HAS THE VALUE
0, and the objective is

    F(A_0, .., A_{N-1}) = sum over ALL cells of l(x_cell, mdl_cell),
    mdl_cell = sum_f prod_t A_t[i_t(cell), f].

This is unlike `cpd_gcp` (splatt_amd/gcp.py), whose objective is the sum
over the STORED entries only and for which cells that are not stored are
unknown. `cpd_gcp` fits completion-style data; `cpd_sgcp` fits binary and
count tensors, where an unstored cell is a zero that carries information
and no loss but gaussian (`cpd_als`) and poisson (`cpd_apr`) has a closed
form for the zeros.

The gradient estimate is Kolda & Hong's SEMI-STRATIFIED one, which needs no
membership test. With nnz stored entries, total = prod(dims) cells, p stored
entries drawn uniformly with replacement and q cells drawn uniformly with
replacement from all cells (stored or not), dl = dl/dm:

    y_j  = (nnz/p)   * (dl(x_j, m_j) - dl(0, m_j))     j <  p  (stored draws)
    y_j  = (total/q) *  dl(0, m_j)                      j >= p  (cell draws)
    G_t[i] += y_j * prod_{u != t} A_u[i_u(j), :]    every mode t, i = i_t(j)
    Fhat   = (nnz/p) * sum_{j<p} (l(x_j, m_j) - l(0, m_j))
             + (total/q) * sum_{j>=p} l(0, m_j)

Both are unbiased for the full-tensor gradient and loss. The losses, eps
and `param` are exactly those of splatt_amd/gcp.py (`LOSSES`,
`loss_terms`); the model is never clamped.

Device path: csrc/hip/sgcp.hip — a sample-parallel pass that forms all N
gradients from one evaluation of the model value and adds them with f64
atomics, and a fused Adam step. Because the order of the atomic adds varies,
the gradients of `impl="hip"` are NOT bitwise reproducible from run to run
(the loss estimate and everything else in a step are); this is the standing
of the default MTTKRP. `impl="torch"` is the vectorised torch
implementation: the CPU path, and the benchmark baseline on device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from splatt_amd._ext import native
from splatt_amd.cpd import seeded_init
from splatt_amd.gcp import (_DOMAIN_TEXT, LOSSES, MAX_RANK, _check_loss,
                            loss_terms)
from splatt_amd.sptensor import SpTensor

_CHUNK_BYTES = 64 << 20


# ---------------------------------------------------------------- sampling

@dataclass
class GcpSample:
    """p draws of stored entries followed by q draws of cells."""
    inds: torch.Tensor      # [N, p + q] int32, contiguous
    vals: torch.Tensor      # [p + q] float64, zeros for the cell draws
    p: int
    q: int
    wnz: float              # nnz / p
    wz: float               # total / q
    dims: Tuple[int, ...] = ()
    # what has been verified about inds / vals: "range", value domains
    _checked: set = field(default_factory=set, repr=False)


def _total_cells(dims: Sequence[int]) -> int:
    total = 1
    for d in dims:
        total *= int(d)
    return total


def gcp_sample(t: SpTensor, p: int, q: int,
               generator: torch.Generator) -> GcpSample:
    """Draw p stored entries and q cells of `t`, each uniformly with
    replacement, on the tensor's device; deterministic in `generator` (which
    must live on that device). A cell draw has the value 0 whether or not
    the cell is stored: that is what the semi-stratified estimator expects.
    Nothing here synchronises with the host."""
    p, q = int(p), int(q)
    if p < 1 or q < 1:
        raise ValueError(f"gcp_sample: p and q must be >= 1, got {p}, {q}")
    if t.vals.dtype != torch.float64:
        raise ValueError("gcp_sample supports float64 tensors only, got "
                         f"{t.vals.dtype}")
    if t.nnz < 1:
        raise ValueError("gcp_sample: the tensor has no stored entries")
    if any(int(d) >= 1 << 31 for d in t.dims):
        raise ValueError("gcp_sample: every dim must be below 2^31, got "
                         f"{list(t.dims)}")
    total = _total_cells(t.dims)
    if total >= 1 << 62:
        raise ValueError("gcp_sample: the tensor has too many cells to "
                         "index in 64 bits")
    dev = t.device
    si = torch.randint(0, t.nnz, (p,), generator=generator, device=dev)
    rem = torch.randint(0, total, (q,), generator=generator, device=dev)
    cols = []
    for d in reversed(t.dims):
        cols.append(rem % int(d))
        rem = rem // int(d)
    zi = torch.stack(list(reversed(cols)), 0)
    inds = torch.cat([t.inds.index_select(1, si), zi], 1).to(torch.int32)
    vals = torch.cat([t.vals.index_select(0, si),
                      torch.zeros(q, dtype=torch.float64, device=dev)])
    s = GcpSample(inds.contiguous(), vals, p, q, t.nnz / p, total / q,
                  tuple(int(d) for d in t.dims))
    s._checked.add("range")     # by construction
    return s


def _check_sample(s: GcpSample, dims: Sequence[int], loss: str) -> None:
    """Index range and value domain of a sample. Each is verified once per
    sample and remembered; samples from `gcp_sample` are in range by
    construction, and the driver vouches for the domain after checking the
    tensor, so a step does not synchronise with the host."""
    if "range" not in s._checked or s.dims != tuple(dims):
        lim = torch.tensor(list(dims), dtype=torch.int32,
                           device=s.inds.device).unsqueeze(1)
        if not bool(((s.inds >= 0) & (s.inds < lim)).all()):
            raise ValueError("gcp_sgrad: the sample has indices outside the "
                             "factors")
        s.dims = tuple(int(d) for d in dims)
        s._checked.add("range")
    dom = LOSSES[loss][2]
    if dom == "any" or dom in s._checked:
        return
    v = s.vals
    if dom == "nonneg":
        ok = bool((v >= 0).all())
    elif dom == "positive":
        # cell draws carry 0 by definition; the stored draws are the data
        ok = bool((v[:s.p] > 0).all())
    else:
        ok = bool(((v == 0) | (v == 1)).all())
    if not ok:
        raise ValueError(f"gcp loss {loss!r} needs tensor {_DOMAIN_TEXT[dom]}"
                         "; the sample has values outside that domain")
    s._checked.add(dom)


# ---------------------------------------------------------------- gradient

def _sgrad_torch(s: GcpSample, mats: List[torch.Tensor], loss: str,
                 param: float, want_loss: bool,
                 out: List[torch.Tensor]) -> Optional[torch.Tensor]:
    nm = len(mats)
    rank = int(mats[0].shape[1])
    n = s.p + s.q
    chunk = max(1, _CHUNK_BYTES // (rank * 8 * nm))
    fhat = (torch.zeros((), dtype=torch.float64, device=s.vals.device)
            if want_loss else None)
    for j0 in range(0, n, chunk):
        j1 = min(n, j0 + chunk)
        idx = [s.inds[t, j0:j1].long() for t in range(nm)]
        a = [mats[t].index_select(0, idx[t]) for t in range(nm)]
        # suf[t] = prod_{u > t} a[u], pre = prod_{u < t} a[u]: no division
        suf = [None] * nm
        suf[nm - 1] = torch.ones_like(a[0])
        for t in range(nm - 2, -1, -1):
            suf[t] = suf[t + 1] * a[t + 1]
        mdl = (a[0] * suf[0]).sum(1)
        x = s.vals[j0:j1]
        stored = torch.arange(j0, j1, device=x.device) < s.p
        d0, l0 = loss_terms(loss, torch.zeros_like(x), mdl, param, want_loss)
        dx, lx = loss_terms(loss, x, mdl, param, want_loss)
        y = torch.where(stored, s.wnz * (dx - d0), s.wz * d0)
        if want_loss:
            fhat += torch.where(stored, s.wnz * (lx - l0), s.wz * l0).sum()
        pre = torch.ones_like(a[0])
        for t in range(nm):
            out[t].index_add_(0, idx[t], y.unsqueeze(1) * (pre * suf[t]))
            pre = pre * a[t]
    return fhat


def _sgrad_hip(s: GcpSample, mats: List[torch.Tensor], loss: str,
               param: float, want_loss: bool,
               out: List[torch.Tensor]) -> Optional[torch.Tensor]:
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    parts = None
    if want_loss:
        # an upper bound of the launcher's count (one double per wave)
        parts = torch.empty(8192, dtype=torch.float64, device=s.vals.device)
    used = native().hip_sgcp_grad(
        s.inds, s.vals, s.p, mats, out, LOSSES[loss][0], float(param),
        float(s.wnz), float(s.wz), parts,
        torch.cuda.current_stream().cuda_stream)
    return parts[:used].sum() if want_loss else None


def gcp_sgrad(sample: GcpSample, mats: Sequence[torch.Tensor], loss: str, *,
              param: Optional[float] = None, want_loss: bool = False,
              impl: str = "auto",
              out: Optional[Sequence[torch.Tensor]] = None) -> Tuple:
    """The semi-stratified estimate of the full-tensor GCP gradient (module
    docstring) from one sample: returns (fhat, [G_0 .. G_{N-1}]) with G_t
    [dims[t], rank] float64 and fhat the loss estimate as a 0-d tensor on
    the sample's device (None without `want_loss`). Rows no sample touches
    get zeros. Unstored cells count as zeros: this estimates the gradient of
    the loss over ALL cells, not `gcp_grad`'s sum over stored entries.

    `out`: optional list of contiguous float64 [dims[t], rank] tensors (for
    example views of one flat buffer); they are zeroed and filled, and
    returned. `impl`: "hip" (csrc/hip/sgcp.hip; default on device tensors)
    or "torch" (vectorised index_select / index_add_: the CPU path, and a
    baseline that also runs on device tensors when asked — never chosen
    automatically there). The hip gradients are accumulated with atomics
    and are not bitwise reproducible from run to run; fhat is."""
    mats = list(mats)
    nm = len(mats)
    if not isinstance(sample, GcpSample):
        raise ValueError("gcp_sgrad needs a GcpSample (gcp_sample)")
    if nm < 3 or nm > 8:
        raise ValueError(f"gcp supports 3..8 modes, got {nm}")
    if not isinstance(mats[0], torch.Tensor) or mats[0].dim() != 2:
        raise ValueError("factors must be 2-D tensors [rows, rank]")
    rank = int(mats[0].shape[1])
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"gcp supports rank 1..{MAX_RANK}, got {rank}")
    n = int(sample.p) + int(sample.q)
    inds, vals = sample.inds, sample.vals
    if sample.p < 1 or sample.q < 1:
        raise ValueError("the sample needs p >= 1 and q >= 1")
    if (inds.dtype != torch.int32 or tuple(inds.shape) != (nm, n)
            or not inds.is_contiguous()):
        raise ValueError(f"sample.inds must be contiguous int32 [{nm}, {n}], "
                         f"got {inds.dtype} {tuple(inds.shape)}")
    if vals.dtype != torch.float64 or tuple(vals.shape) != (n,):
        raise ValueError(f"sample.vals must be float64 [{n}], got "
                         f"{vals.dtype} {tuple(vals.shape)}")
    dev = vals.device
    if inds.device != dev:
        raise ValueError("sample.inds and sample.vals are on different "
                         "devices")
    for m, A in enumerate(mats):
        if (not isinstance(A, torch.Tensor) or A.dim() != 2
                or int(A.shape[1]) != rank):
            raise ValueError(f"factor {m} must be [rows, {rank}]")
        if A.dtype != torch.float64 or A.device != dev:
            raise ValueError(
                f"factor {m}: dtype/device {A.dtype}/{A.device} does not "
                f"match sample {vals.dtype}/{dev}")
    prm = _check_loss(loss, param)
    if impl == "auto":
        impl = "hip" if dev.type == "cuda" else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto)")
    if impl == "hip" and dev.type != "cuda":
        raise ValueError("impl='hip' needs a device tensor")
    dims = [int(A.shape[0]) for A in mats]
    _check_sample(sample, dims, loss)
    if out is None:
        out = [torch.zeros_like(A, memory_format=torch.contiguous_format)
               for A in mats]
    else:
        out = list(out)
        if len(out) != nm:
            raise ValueError(f"out needs {nm} tensors, got {len(out)}")
        for m, G in enumerate(out):
            if (tuple(G.shape) != (dims[m], rank) or G.dtype != torch.float64
                    or G.device != dev or not G.is_contiguous()):
                raise ValueError(f"out[{m}] must be a contiguous float64 "
                                 f"({dims[m]}, {rank}) tensor on {dev}")
            G.zero_()
    if impl == "hip":
        mats = [A.contiguous() for A in mats]
    fn = _sgrad_hip if impl == "hip" else _sgrad_torch
    return fn(sample, mats, loss, prm, bool(want_loss), out), out


# -------------------------------------------------------------------- Adam

def adam_step(x: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
              v: torch.Tensor, *, step: int, lr: float, beta1: float = 0.9,
              beta2: float = 0.999, eps: float = 1e-8,
              lower: Optional[float] = None, impl: str = "auto") -> None:
    """One Adam step, in place on flat float64 buffers of one length:

        m = beta1*m + (1-beta1)*g
        v = beta2*v + ((1-beta2)*g)*g
        x = x - (lr*(m*c1)) / (sqrt(v*c2) + eps)
        x = max(x, lower)                      (only when lower is not None)
        g = 0                                  (ready for the next sample)

    with the bias corrections c1 = 1/(1-beta1^step), c2 = 1/(1-beta2^step)
    computed once here, on the host, in double: both implementations use the
    same numbers, and every operation rounds once in both. `impl`: "hip"
    (one fused pass, csrc/hip/sgcp.hip; default on device tensors) or
    "torch"."""
    step = int(step)
    if step < 1:
        raise ValueError(f"adam_step: step counts from 1, got {step}")
    bufs = {"x": x, "g": g, "m": m, "v": v}
    for name, b in bufs.items():
        if (not isinstance(b, torch.Tensor) or b.dim() != 1
                or b.dtype != torch.float64 or not b.is_contiguous()
                or b.shape != x.shape or b.device != x.device):
            raise ValueError(f"adam_step: {name} must be a flat contiguous "
                             "float64 buffer of the length and device of x")
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError("adam_step: beta1 and beta2 must lie in [0, 1)")
    c1 = 1.0 / (1.0 - float(beta1) ** step)
    c2 = 1.0 / (1.0 - float(beta2) ** step)
    if impl == "auto":
        impl = "hip" if x.device.type == "cuda" else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto)")
    if impl == "hip":
        if x.device.type != "cuda":
            raise ValueError("impl='hip' needs a device tensor")
        if native().hip_arch() != 950:
            raise RuntimeError("HIP kernels not built for gfx950")
        native().hip_adam_step(
            x, g, m, v, float(lr), float(beta1), float(beta2), float(eps),
            c1, c2, None if lower is None else float(lower),
            torch.cuda.current_stream().cuda_stream)
        return
    # no `alpha=` / addcmul forms: they may contract a product into the sum
    m.mul_(beta1).add_(g * (1.0 - beta1))
    v.mul_(beta2).add_((g * (1.0 - beta2)) * g)
    x.sub_((m * c1).mul_(lr).div_((v * c2).sqrt_().add_(eps)))
    if lower is not None:
        x.clamp_(min=lower)
    g.zero_()


# ------------------------------------------------------------------ driver

@dataclass
class SgcpOptions:
    """The defaults are those of Kolda & Hong's paper (and of `gcp_opt`'s
    Adam); they have not been tuned here."""
    p: Optional[int] = None         # gradient sample: stored draws
    q: Optional[int] = None         # gradient sample: cell draws
    #                                 None: max(1000, ceil(3 nnz / iters_per_epoch))
    p_loss: Optional[int] = None    # the fixed loss-estimate sample
    q_loss: Optional[int] = None    # None: max(10000, ceil(nnz / 100))
    lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    decay: float = 0.1              # lr multiplier after a failed epoch
    max_fails: int = 1              # the run ends after max_fails + 1 failures
    iters_per_epoch: int = 1000
    max_epochs: int = 1000
    seed: int = 0x5EED5EED
    param: Optional[float] = None   # huber's delta
    verbose: bool = False
    impl: str = "auto"              # of gcp_sgrad and adam_step


@dataclass
class SgcpKruskal:
    factors: List[torch.Tensor]
    lam: torch.Tensor
    loss_trace: List[float] = field(default_factory=list)  # [0] = initial
    lr_trace: List[float] = field(default_factory=list)    # lr of each epoch
    nepochs: int = 0
    nsteps: int = 0     # Adam steps in the returned state (undone ones not)
    nfails: int = 0


def _check_tensor_values(t: SpTensor, loss: str) -> None:
    dom = LOSSES[loss][2]
    if dom == "any":
        return
    v = t.vals
    if dom == "nonneg":
        ok = bool((v >= 0).all())
    elif dom == "positive":
        ok = bool((v > 0).all())
    else:
        ok = bool(((v == 0) | (v == 1)).all())
    if not ok:
        raise ValueError(f"gcp loss {loss!r} needs tensor {_DOMAIN_TEXT[dom]}"
                         "; the tensor has entries outside that domain")


def cpd_sgcp(t: SpTensor, rank: int, loss: str = "bernoulli-logit",
             opts: Optional[SgcpOptions] = None) -> SgcpKruskal:
    """Stochastic generalized CPD of `t` under `loss`, every cell counted:
    a cell that is not stored is a zero (module docstring; `cpd_gcp` fits
    the stored entries only).

    Takes an SpTensor; no CSF is built, the solver never walks a stream.
    Factors, gradient and both Adam moments are views of flat float64
    buffers on the tensor's device. The initial factors are `seeded_init`,
    scaled by 0.3 for losses with free factors and made nonnegative for
    bounded ones, as in `cpd_gcp`. One fixed loss sample (p_loss, q_loss) is
    drawn up front; its estimate Fhat is recorded in `loss_trace` before the
    first epoch and after every epoch. An epoch is `iters_per_epoch` steps,
    each a fresh `gcp_sample`, a `gcp_sgrad` and an `adam_step`; nothing
    inside an epoch synchronises with the host. An epoch whose Fhat is not
    below the best so far is undone — factors, moments and step counter go
    back to the epoch's start — lr is multiplied by `decay` and the failure
    counted (its Fhat stays in `loss_trace`). The run ends after
    `max_fails + 1` failures or `max_epochs`. The returned factors have unit
    column 2-norms (or zero columns), the weights in `lam`.

    Samples and the loss estimates are deterministic in `seed` (per device
    type); on the device the gradients, and so the iterates, are not bitwise
    reproducible (atomics)."""
    opts = opts or SgcpOptions()
    if not isinstance(t, SpTensor):
        raise ValueError("cpd_sgcp takes an SpTensor")
    if t.dtype != torch.float64:
        raise ValueError("sgcp supports float64 tensors only, got "
                         f"{t.dtype} (load the tensor as f64)")
    nm, dims = t.nmodes, [int(d) for d in t.dims]
    if nm < 3 or nm > 8:
        raise ValueError(f"gcp supports 3..8 modes, got {nm}")
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"gcp supports rank 1..{MAX_RANK}, got {rank}")
    _check_loss(loss, opts.param)
    if opts.iters_per_epoch < 1 or opts.max_epochs < 0 or opts.max_fails < 0:
        raise ValueError("sgcp: iters_per_epoch >= 1, max_epochs >= 0 and "
                         "max_fails >= 0 are required")
    _check_tensor_values(t, loss)
    dom = LOSSES[loss][2]
    nnz = t.nnz
    dflt = max(1000, math.ceil(3 * nnz / opts.iters_per_epoch))
    p = dflt if opts.p is None else int(opts.p)
    q = dflt if opts.q is None else int(opts.q)
    dflt = max(10000, math.ceil(nnz / 100))
    p_loss = dflt if opts.p_loss is None else int(opts.p_loss)
    q_loss = dflt if opts.q_loss is None else int(opts.q_loss)
    dev = t.device
    lower = LOSSES[loss][1]
    sizes = [d * rank for d in dims]
    npar = sum(sizes)
    x = torch.empty(npar, dtype=torch.float64, device=dev)
    g = torch.zeros(npar, dtype=torch.float64, device=dev)
    m = torch.zeros(npar, dtype=torch.float64, device=dev)
    v = torch.zeros(npar, dtype=torch.float64, device=dev)

    def split(buf):
        views, o = [], 0
        for k in range(nm):
            views.append(buf[o:o + sizes[k]].view(dims[k], rank))
            o += sizes[k]
        return views

    X, Gv = split(x), split(g)
    for k in range(nm):
        A = seeded_init(dims[k], rank, k, opts.seed).to(dev)
        X[k].copy_(A * 0.3 if lower is None else A.abs())

    gen = torch.Generator(device=dev)
    gen.manual_seed(int(opts.seed))

    def draw(pp, qq):
        s = gcp_sample(t, pp, qq, gen)
        s._checked.add(dom)     # the tensor's values were checked above
        return s

    fixed = draw(p_loss, q_loss)

    def estimate() -> float:
        f, _ = gcp_sgrad(fixed, X, loss, param=opts.param, want_loss=True,
                         impl=opts.impl, out=Gv)
        g.zero_()
        return float(f)

    lr = float(opts.lr)
    best = estimate()
    if not math.isfinite(best):
        raise ValueError(f"sgcp: the loss at the initial factors is {best}")
    trace, lrs = [best], []
    step = nfails = nepochs = 0
    if opts.verbose:
        print(f"  epoch = 0 loss = {best:.8e}")
    while nepochs < opts.max_epochs and nfails <= opts.max_fails:
        saved = (x.clone(), m.clone(), v.clone(), step)
        for _ in range(opts.iters_per_epoch):
            s = draw(p, q)
            gcp_sgrad(s, X, loss, param=opts.param, impl=opts.impl, out=Gv)
            step += 1
            adam_step(x, g, m, v, step=step, lr=lr, beta1=opts.beta1,
                      beta2=opts.beta2, eps=opts.eps, lower=lower,
                      impl=opts.impl)
        f = estimate()
        nepochs += 1
        trace.append(f)
        lrs.append(lr)
        failed = not f < best       # a NaN fails
        if opts.verbose:
            print(f"  epoch = {nepochs} loss = {f:.8e} lr = {lr:.3e}"
                  + (" (undone)" if failed else ""))
        if failed:
            x.copy_(saved[0])
            m.copy_(saved[1])
            v.copy_(saved[2])
            step = saved[3]
            lr *= opts.decay
            nfails += 1
        else:
            best = f
    lam = torch.ones(rank, dtype=torch.float64, device=dev)
    factors = []
    for A in X:
        nrm = A.norm(dim=0)
        lam = lam * nrm
        factors.append(A / torch.where(nrm > 0, nrm, torch.ones_like(nrm)))
    return SgcpKruskal(factors=factors, lam=lam, loss_trace=trace,
                       lr_trace=lrs, nepochs=nepochs, nsteps=step,
                       nfails=nfails)
