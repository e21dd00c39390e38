"""Generalized CPD (GCP; Hong, Kolda & Duersch 2020; `gcp_opt` in Tensor
Toolbox): a CP model fitted under an elementwise loss l(x, m) by a
gradient method.

The STORED entries of the tensor are the OBSERVED entries: the objective is

    f(A_0, .., A_{N-1}) = sum_{x stored} l(val_x, mdl_x),
    mdl_x = sum_f prod_t A_t[i_t(x), f]

and nothing else — the convention of `complete_als`. A stored value of 0 is
an observation of zero; cells that are not stored are unknown. For binary
data, store the positives plus a sample of zeros (`sample_zeros`). For
the loss over ALL cells, unstored cells counted as zeros, use `cpd_sgcp`
(splatt_amd/sgcp.py). For output mode m, with Omega_i the stored entries of
row i and pi_x the Hadamard product of the other modes' factor rows at x,

    G_m[i]  = sum_{x in Omega_i} dl/dm(val_x, mdl_x) pi_x
    frow[i] = sum_{x in Omega_i} l(val_x, mdl_x)

Losses (eps = 1e-10; `param` is huber's delta):

    name             l(x, m)                               factors  values
    gaussian         (m - x)^2                             free     any
    huber            (x-m)^2 if |x-m| <= delta             free     any
                     else 2 delta |x-m| - delta^2
    poisson          m - x log(m + eps)                    >= 0     >= 0
    poisson-log      exp(m) - x m                          free     >= 0
    bernoulli-odds   log(m + 1) - x log(m + eps)           >= 0     0 or 1
    bernoulli-logit  log(1 + exp(m)) - x m                 free     0 or 1
    gamma            x/(m + eps) + log(m + eps)            >= 0     > 0
    rayleigh         2 log(m + eps)                        >= 0     >= 0
                     + (pi/4) (x/(m + eps))^2

The model is never clamped: a model value outside a loss's domain gives what
the formulas give.

Device path: csrc/hip/gcp.hip — one wave per stream segment, one pass, no
atomics. `impl="torch"` is the chunked vectorised torch implementation: the
CPU path, and the benchmark baseline on device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from splatt_amd._ext import native
from splatt_amd.completion import _plan, _resolve, _stream
from splatt_amd.cpd import seeded_init
from splatt_amd.csf import Csf, CsfSet, csf_alloc
from splatt_amd.sptensor import SpTensor

MAX_RANK = 64
EPS = 1e-10     # csrc/hip/gcp.hip: GCP_EPS
# A workspace slot is only F (+ 1) doubles, so every multi-segment row of a
# mode fits at once: the planner is asked for one batch and never grows
# segments.
_UNBOUNDED = 1 << 62

# name -> (kernel id, lower bound on the factors or None, value domain)
LOSSES = {
    "gaussian": (0, None, "any"),
    "huber": (1, None, "any"),
    "poisson": (2, 0.0, "nonneg"),
    "poisson-log": (3, None, "nonneg"),
    "bernoulli-odds": (4, 0.0, "binary"),
    "bernoulli-logit": (5, None, "binary"),
    "gamma": (6, 0.0, "positive"),
    "rayleigh": (7, 0.0, "nonneg"),
}
_DOMAIN_TEXT = {"nonneg": "values >= 0", "binary": "values 0 or 1",
                "positive": "values > 0"}


def loss_terms(loss: str, x: torch.Tensor, m: torch.Tensor,
               param: Optional[float] = None,
               want_loss: bool = True) -> Tuple:
    """(dl/dm, l) of the table above, elementwise in torch (l is None
    without `want_loss`). The formulas of csrc/hip/gcp.hip, term by term."""
    w = want_loss
    if loss == "gaussian":
        d = m - x
        return 2.0 * d, (d * d if w else None)
    if loss == "huber":
        r = x - m
        ar = r.abs()
        inside = ar <= param
        y = torch.where(inside, -2.0 * r, -2.0 * param * torch.sign(r))
        return y, (torch.where(inside, r * r,
                               2.0 * param * ar - param * param)
                   if w else None)
    if loss == "poisson":
        t = m + EPS
        return 1.0 - x / t, (m - x * torch.log(t) if w else None)
    if loss == "poisson-log":
        ex = torch.exp(m)
        return ex - x, (ex - x * m if w else None)
    if loss == "bernoulli-odds":
        t = m + EPS
        return (1.0 / (m + 1.0) - x / t,
                torch.log(m + 1.0) - x * torch.log(t) if w else None)
    if loss == "bernoulli-logit":
        ex = torch.exp(-m.abs())
        # sigmoid without overflow: 1/(1+e^-m) for m >= 0, e^m/(1+e^m) below
        y = torch.where(m >= 0, torch.ones_like(ex), ex) / (1.0 + ex) - x
        return y, (m.clamp_min(0.0) + torch.log1p(ex) - x * m if w else None)
    if loss == "gamma":
        t = m + EPS
        return -x / (t * t) + 1.0 / t, (x / t + torch.log(t) if w else None)
    if loss == "rayleigh":
        t = m + EPS
        y = 2.0 / t - (math.pi / 2.0) * (x * x) / (t * t * t)
        q = x / t
        return y, (2.0 * torch.log(t) + (math.pi / 4.0) * (q * q)
                   if w else None)
    raise ValueError(f"unknown loss {loss!r} ({', '.join(LOSSES)})")


def _check_loss(loss: str, param: Optional[float]) -> float:
    if loss not in LOSSES:
        raise ValueError(f"unknown loss {loss!r} ({', '.join(LOSSES)})")
    if loss == "huber":
        if param is None or not float(param) > 0:
            raise ValueError("huber needs param = delta > 0, got "
                             f"{param!r}")
        return float(param)
    return 0.0 if param is None else float(param)


def _check_values(c: Csf, loss: str) -> None:
    """The value domain of the loss. Checked once per (stream, domain) and
    remembered, so repeated calls do not synchronise with the device."""
    dom = LOSSES[loss][2]
    if dom == "any":
        return
    cache = getattr(c, "_gcp_domain", None)
    if cache is None:
        cache = {}
        object.__setattr__(c, "_gcp_domain", cache)
    ok = cache.get(dom)
    if ok is None:
        v = c.vals
        if dom == "nonneg":
            ok = bool((v >= 0).all())
        elif dom == "positive":
            ok = bool((v > 0).all())
        else:
            ok = bool(((v == 0) | (v == 1)).all())
        cache[dom] = ok
    if not ok:
        raise ValueError(f"gcp loss {loss!r} needs tensor {_DOMAIN_TEXT[dom]}"
                         "; the tensor has entries outside that domain")


def gcp_plan(src: CsfSet | Csf, mode: int) -> dict:
    """The segment plan `gcp_grad(impl="hip")` uses for this mode (for
    inspection and tests)."""
    return _plan(_resolve(src, mode), _UNBOUNDED)


def _grad_hip(c: Csf, mats: List[torch.Tensor], mode: int, loss: str,
              param: float, want_loss: bool) -> Tuple:
    if native().hip_arch() != 950:
        raise RuntimeError("HIP kernels not built for gfx950")
    A = mats[mode].contiguous()
    nrows, rank = int(A.shape[0]), int(A.shape[1])
    st = _stream(c)
    plan = _plan(c, _UNBOUNDED)
    nmseg = int(plan["seg_start"].numel()) - plan["nsingle"]
    need = max(1, nmseg * (rank + 1))
    ws = getattr(c, "_gcp_ws", None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float64, device=c.device)
        object.__setattr__(c, "_gcp_ws", ws)
    dev = c.device
    # rows without entries keep these zeros
    G = torch.zeros(nrows, rank, dtype=torch.float64, device=dev)
    frow = (torch.zeros(nrows, dtype=torch.float64, device=dev)
            if want_loss else None)
    ms = [mats[c.dim_perm[l]].contiguous() for l in range(1, c.nmodes)]
    native().hip_gcp_grad(
        st["idx"], ms, st["vals"], plan["seg_start"], plan["seg_len"],
        plan["seg_row"], plan["seg_slot"], plan["nsingle"], plan["mrow"],
        plan["mslot"], LOSSES[loss][0], float(param), A, ws, G, frow,
        torch.cuda.current_stream().cuda_stream)
    return G, frow


def _grad_torch(c: Csf, mats: List[torch.Tensor], mode: int, loss: str,
                param: float, want_loss: bool) -> Tuple:
    """One chunked pass over the key stream: gather, row-wise dot,
    index_add_ of the weighted pi rows."""
    A = mats[mode]
    nrows, rank = int(A.shape[0]), int(A.shape[1])
    st = _stream(c)
    dev, dt = c.device, torch.float64
    key = st["key"].long()
    idx = [ix.long() for ix in st["idx"]]
    vals = st["vals"]
    ms = [mats[c.dim_perm[l]] for l in range(1, c.nmodes)]
    nnz = int(vals.numel())
    chunk = max(1, (64 << 20) // (rank * 8))
    G = torch.zeros(nrows, rank, dtype=dt, device=dev)
    frow = torch.zeros(nrows, dtype=dt, device=dev) if want_loss else None
    for q0 in range(0, nnz, chunk):
        q1 = min(nnz, q0 + chunk)
        pi = None
        for ix, M in zip(idx, ms):
            g = M.index_select(0, ix[q0:q1])
            pi = g if pi is None else pi * g
        k = key[q0:q1]
        mdl = (A.index_select(0, k) * pi).sum(1)
        y, l = loss_terms(loss, vals[q0:q1], mdl, param, want_loss)
        G.index_add_(0, k, y.unsqueeze(1) * pi)
        if want_loss:
            frow.index_add_(0, k, l)
    return G, frow


def gcp_grad(src: CsfSet | Csf, mats: Sequence[torch.Tensor], mode: int,
             loss: str, *, param: Optional[float] = None,
             want_loss: bool = False, impl: str = "auto") -> Tuple:
    """The GCP gradient with respect to the factor of `mode`: returns
    (G, frow) with G [dims[mode], rank] float64 and frow [dims[mode]] the
    loss summed over each row's stored entries (None without `want_loss`).
    Rows without stored entries get zeros. `mats` is indexed by tensor mode.

    `src` must hold `mode` at depth 0 of a key-sorted stream — any
    csf_alloc(t, "all") build — with values in the loss's domain. `impl`:
    "hip" (the gfx950 kernels; default on device tensors), "torch"
    (vectorised torch: the CPU path, and a baseline that also runs on device
    tensors when asked — never chosen automatically there)."""
    c = _resolve(src, mode)
    mats = list(mats)
    if len(mats) != c.nmodes:
        raise ValueError(f"need {c.nmodes} factor matrices, got {len(mats)}")
    if c.nmodes < 3 or c.nmodes > 8:
        raise ValueError(f"gcp supports 3..8 modes, got {c.nmodes}")
    if not isinstance(mats[mode], torch.Tensor) or mats[mode].dim() != 2:
        raise ValueError("factors must be 2-D tensors [rows, rank]")
    rank = int(mats[mode].shape[1])
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"gcp supports rank 1..{MAX_RANK}, got {rank}")
    for m, A in enumerate(mats):
        if tuple(A.shape) != (c.dims[m], rank):
            raise ValueError(f"factor {m} has shape {tuple(A.shape)}, "
                             f"expected ({c.dims[m]}, {rank})")
        if A.dtype != torch.float64 or A.device != c.device:
            raise ValueError(
                f"factor {m}: dtype/device {A.dtype}/{A.device} does not "
                f"match tensor {c.vals.dtype}/{c.device}")
    prm = _check_loss(loss, param)
    if impl == "auto":
        impl = "hip" if c.device.type == "cuda" else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r} (hip, torch, auto)")
    if impl == "hip" and c.device.type != "cuda":
        raise ValueError("impl='hip' needs a device tensor")
    _check_values(c, loss)
    fn = _grad_hip if impl == "hip" else _grad_torch
    return fn(c, mats, mode, loss, prm, bool(want_loss))


def gcp_fg(cs: CsfSet, mats: Sequence[torch.Tensor], loss: str, *,
           param: Optional[float] = None, impl: str = "auto") -> Tuple:
    """Loss value and all gradients: (f, [G_0 .. G_{N-1}]), one `gcp_grad`
    per mode. The loss value is computed in mode 0's pass only; f is a 0-d
    tensor on the tensor's device."""
    mats = list(mats)
    f, grads = None, []
    for m in range(len(mats)):
        G, frow = gcp_grad(cs, mats, m, loss, param=param, want_loss=(m == 0),
                           impl=impl)
        if m == 0:
            f = frow.sum()
        grads.append(G)
    return f, grads


# ------------------------------------------------------------------ driver

@dataclass
class GcpOptions:
    max_iters: int = 200
    tolerance: float = 1e-6   # relative loss decrease; <= 0: run max_iters
    #                           (or until the line search fails)
    history: int = 5          # L-BFGS pairs kept
    seed: int = 0x5EED5EED
    verbose: bool = False
    param: Optional[float] = None   # huber's delta


@dataclass
class GcpKruskal:
    factors: List[torch.Tensor]
    lam: torch.Tensor
    loss_trace: List[float] = field(default_factory=list)
    pg_trace: List[float] = field(default_factory=list)   # |projected grad|
    nfev: int = 0
    niters: int = 0
    converged: bool = False


_ARMIJO = 1e-4
_MAX_HALVINGS = 40
_CURVATURE = 1e-10


def _two_loop(q: torch.Tensor, S: list, Y: list) -> torch.Tensor:
    """H q of the L-BFGS inverse Hessian built from the pairs (S, Y)."""
    q = q.clone()
    alphas = []
    for s, y in zip(reversed(S), reversed(Y)):
        a = s.dot(q) / y.dot(s)
        alphas.append(a)
        q -= a * y
    if S:
        q *= S[-1].dot(Y[-1]) / Y[-1].dot(Y[-1])
    for (s, y), a in zip(zip(S, Y), reversed(alphas)):
        b = y.dot(q) / y.dot(s)
        q += (a - b) * s
    return q


def gcp_minimize(fg, x: torch.Tensor, lower: Optional[float],
                 opts: GcpOptions) -> Tuple:
    """Bound-constrained limited-memory quasi-Newton minimisation of
    fg(x) -> (f, g) over x >= lower (None: unconstrained), x updated in
    place. The free set is the entries not (at the bound with a positive
    gradient); the two-loop recursion runs on the projected gradient and
    the direction is masked to the free set; a non-descent direction falls
    back to steepest descent and resets the history; the line search is
    projected backtracking under the Armijo condition. Returns
    (loss_trace, pg_trace, nfev, niters, converged)."""
    f, g = fg(x)
    nfev = 1
    if not math.isfinite(f):
        raise ValueError(f"gcp: the loss at the initial factors is {f}")
    S: list = []
    Y: list = []
    trace, pgs = [], []
    converged = False
    niters = 0
    tol = float(opts.tolerance)
    for it in range(opts.max_iters):
        if lower is None:
            pg = g
            free = None
        else:
            free = ~((x <= lower) & (g > 0))
            pg = g * free
        pgn = float(pg.norm())
        if pgn == 0.0:
            converged = True
            break
        d = -_two_loop(pg, S, Y)
        if free is not None:
            d = d * free
        if not float(g.dot(d)) < 0.0:
            d = -pg
            S, Y = [], []
        a = 1.0 if S else min(1.0, 1.0 / pgn)
        ok = False
        for _ in range(_MAX_HALVINGS + 1):
            xn = x + a * d
            if lower is not None:
                xn.clamp_(min=lower)
            fn, gn = fg(xn)
            nfev += 1
            if (math.isfinite(fn)
                    and fn <= f + _ARMIJO * float(g.dot(xn - x))):
                ok = True
                break
            a *= 0.5
        if not ok:
            break           # line-search failure: x is kept
        s, y = xn - x, gn - g
        if float(s.dot(y)) > _CURVATURE * float(s.norm()) * float(y.norm()):
            S.append(s)
            Y.append(y)
            if len(S) > opts.history:
                S.pop(0)
                Y.pop(0)
        rel = (f - fn) / max(abs(f), 1e-300)
        x.copy_(xn)
        f, g = fn, gn
        niters = it + 1
        trace.append(f)
        pgs.append(pgn)
        if opts.verbose:
            print(f"  its = {niters} loss = {f:.8e} pg = {pgn:.3e} "
                  f"step = {a:.3e} nfev = {nfev}")
        if tol > 0 and rel <= tol:
            converged = True
            break
    return trace, pgs, nfev, niters, converged


def cpd_gcp(t: SpTensor | CsfSet, rank: int, loss: str = "gaussian",
            opts: Optional[GcpOptions] = None) -> GcpKruskal:
    """Generalized CPD of the stored entries of `t` under `loss`.

    All factors are views of one flat float64 buffer on the tensor's device;
    every iteration of the optimiser (`gcp_minimize`) evaluates loss and
    gradient with `gcp_fg`. The initial factors are `seeded_init`, scaled by
    0.3 for losses with free factors and made nonnegative for bounded ones.
    `loss_trace` and `pg_trace` hold the loss after, and the projected-
    gradient norm before, each iteration. It has converged when the relative
    loss decrease of an iteration is <= `tolerance` (> 0); it also stops
    when the line search fails or after `max_iters`. The returned factors
    have unit column 2-norms (or zero columns), the weights in `lam`."""
    opts = opts or GcpOptions()
    if isinstance(t, SpTensor):
        if t.dtype != torch.float64:
            raise ValueError("gcp supports float64 tensors only, got "
                             f"{t.dtype} (load the tensor as f64)")
        cs = csf_alloc(t, "all")
    else:
        cs = t
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"gcp supports rank 1..{MAX_RANK}, got {rank}")
    _check_loss(loss, opts.param)
    nm, dims = cs.nmodes, cs.dims
    for m in range(nm):
        _check_values(_resolve(cs, m), loss)
    dev = cs.csfs[0].device
    lower = LOSSES[loss][1]
    sizes = [d * rank for d in dims]
    x = torch.empty(sum(sizes), dtype=torch.float64, device=dev)
    off = 0
    for m in range(nm):
        A = seeded_init(dims[m], rank, m, opts.seed).to(dev)
        A = A * 0.3 if lower is None else A.abs()
        x[off:off + sizes[m]] = A.reshape(-1)
        off += sizes[m]

    def split(v):
        out, o = [], 0
        for m in range(nm):
            out.append(v[o:o + sizes[m]].view(dims[m], rank))
            o += sizes[m]
        return out

    def fg(v):
        f, grads = gcp_fg(cs, split(v), loss, param=opts.param)
        return float(f), torch.cat([G.reshape(-1) for G in grads])

    trace, pgs, nfev, niters, converged = gcp_minimize(fg, x, lower, opts)
    lam = torch.ones(rank, dtype=torch.float64, device=dev)
    factors = []
    for A in split(x):
        nrm = A.norm(dim=0)
        lam = lam * nrm
        factors.append(A / torch.where(nrm > 0, nrm, torch.ones_like(nrm)))
    return GcpKruskal(factors=factors, lam=lam, loss_trace=trace,
                      pg_trace=pgs, nfev=nfev, niters=niters,
                      converged=converged)


# ------------------------------------------------------------ zero sampling

_ENUMERATE_MAX = 1 << 24


def sample_zeros(t: SpTensor, n: int, seed: int) -> SpTensor:
    """`t` plus `n` stored zeros at coordinates not stored in `t`, drawn
    uniformly without replacement; deterministic in `seed` (per device
    type), computed on the tensor's device. The zeros come after the
    entries of `t`. Raises if `t` has fewer than `n` empty cells."""
    n = int(n)
    if n < 0:
        raise ValueError(f"sample_zeros: n must be >= 0, got {n}")
    total = 1
    for d in t.dims:
        total *= int(d)
    if total >= 1 << 62:
        raise ValueError("sample_zeros: the tensor has too many cells to "
                         "index in 64 bits")
    dev = t.device
    lin = torch.zeros(t.nnz, dtype=torch.int64, device=dev)
    for m, d in enumerate(t.dims):
        lin = lin * int(d) + t.inds[m]
    stored = torch.unique(lin)
    empty = total - int(stored.numel())
    if n > empty:
        raise ValueError(f"sample_zeros: asked for {n} zeros, the tensor has "
                         f"only {empty} empty cells")
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    if total <= _ENUMERATE_MAX:
        # small: a random permutation of the empty cells
        free = torch.ones(total, dtype=torch.bool, device=dev)
        free[stored] = False
        cells = free.nonzero(as_tuple=True)[0]
        pick = cells[torch.randperm(int(cells.numel()), generator=gen,
                                    device=dev)[:n]]
    else:
        # large and sparse: rejection sampling, first n distinct draws
        pick = torch.zeros(0, dtype=torch.int64, device=dev)
        while int(pick.numel()) < n:
            k = 2 * (n - int(pick.numel())) + 1024
            cand = torch.randint(0, total, (k,), generator=gen, device=dev)
            cand = cand[~torch.isin(cand, stored)]
            both = torch.cat([pick, cand])
            # keep first occurrences, in draw order
            u, inv = torch.unique(both, return_inverse=True)
            first = torch.full((int(u.numel()),), int(both.numel()),
                               dtype=torch.int64, device=dev)
            first.scatter_reduce_(0, inv, torch.arange(
                int(both.numel()), device=dev), "amin")
            pick = both[torch.sort(first).values][:n]
    cols = []
    rem = pick
    for d in reversed(t.dims):
        cols.append(rem % int(d))
        rem = rem // int(d)
    zi = torch.stack(list(reversed(cols)), 0)
    inds = torch.cat([t.inds, zi], 1).contiguous()
    vals = torch.cat([t.vals, torch.zeros(n, dtype=t.vals.dtype, device=dev)])
    return SpTensor(inds, vals, list(t.dims))
