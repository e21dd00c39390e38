"""Stochastic GCP: the sampler, the semi-stratified estimator against the
dense full-tensor loss and its autograd gradient, the torch path against a
per-sample Python loop, Adam against a scalar loop, the driver on planted
data, the CLI, the example and the binding checks.

The inputs, oracles and bounds here are shared with tests/test_sgcp_gpu.py.

Bounds. A gradient element G_t[i, f] is a sum of contributions
c_j = y_j * pi_t,j[f]; comparisons are relative to S = sum_j |c_j| of that
element (elements with S = 0 must be exactly 0), the loss estimate relative
to the sum of its absolute terms:

    |got - ref| <= TOL * S.

Two CPU f64 evaluations that add the samples in opposite orders (the torch
path on the sample and on the sample with stored draws and cell draws each
reversed) differ by at most 1.6e-15 * S over the cases of GRID_CASES and
ALL_LOSS_CASES (`PYTHONPATH=. python tests/test_sgcp.py` re-measures it);
TOL is that figure with three orders of margin, the project's usual
derivation, which also covers the few ulp by which an exp or log may differ
between implementations. The per-sample loop oracle differs from the torch
path by at most 4.2e-16 * S.

ENUM_TOL bounds the estimator-by-enumeration test, relative to
max(1, max|dense|): the dense side evaluated twice (einsum over the full
array and its autograd; the model built cell by cell from gathered rows and
the analytic derivative) differs by at most 5.7e-16 over all eight losses
and 3, 4 and 5 modes; ENUM_TOL is that with about three orders of margin.
The estimator itself was within 1.1e-15 of the dense side.
"""
import functools
import math
import os
import runpy

import pytest
import torch

import splatt_amd as sp
from splatt_amd._ext import native

from test_gcp import BOUNDED, LOSSES, o_dloss, o_loss, param_of

TOL = 1.6e-12
ENUM_TOL = 5.7e-13
F64, I32 = torch.float64, torch.int32

DIMS = {3: [7, 5, 9], 4: [5, 4, 6, 3], 5: [4, 3, 5, 2, 3],
        8: [3, 2, 2, 3, 2, 2, 2, 3]}
VALUE_KIND = {"gaussian": "any", "huber": "any", "poisson": "count",
              "poisson-log": "count", "bernoulli-odds": "binary",
              "bernoulli-logit": "binary", "gamma": "positive",
              "rayleigh": "count"}


def draw_values(kind, n, g):
    if kind == "any":
        return torch.randn(n, generator=g, dtype=F64)
    if kind == "count":
        return torch.randint(1, 4, (n,), generator=g).double()
    if kind == "binary":
        return torch.ones(n, dtype=F64)
    return torch.rand(n, generator=g, dtype=F64) + 0.5


def make_mats(dims, rank, bounded, seed=321):
    """Positive factors for the bounded losses (model values > 0), signed
    and scaled for the free ones (model values of a few units at most)."""
    out = []
    for m, d in enumerate(dims):
        A = sp.seeded_init(d, rank, m, seed)
        out.append(A.abs() + 0.05 if bounded
                   else (A - A.mean()) * (1.5 / math.sqrt(rank)))
    return out


def make_sample(dims, p, q, kind, seed, wnz=None, wz=None):
    """A hand-made sample with duplicates (the dims are small): random
    coordinates, values of `kind` on the stored draws."""
    g = torch.Generator().manual_seed(seed)
    n = p + q
    inds = torch.stack([torch.randint(0, d, (n,), generator=g) for d in dims])
    vals = torch.cat([draw_values(kind, p, g), torch.zeros(q, dtype=F64)])
    total = math.prod(dims)
    return sp.GcpSample(inds.to(I32).contiguous(), vals, p, q,
                        37.0 / p if wnz is None else wnz,
                        total / q if wz is None else wz)


def reversed_sample(s):
    """The same sample with the stored draws and the cell draws each in
    reversed order: the sums are added the other way round."""
    perm = torch.cat([torch.arange(s.p - 1, -1, -1),
                      torch.arange(s.p + s.q - 1, s.p - 1, -1)])
    perm = perm.to(s.inds.device)
    return sp.GcpSample(s.inds[:, perm].contiguous(), s.vals[perm], s.p, s.q,
                        s.wnz, s.wz)


def to_device(s, device):
    return sp.GcpSample(s.inds.to(device), s.vals.to(device), s.p, s.q,
                        s.wnz, s.wz)


def loop_oracle(s, mats, loss, param=None):
    """Sample by sample, with the formulas of the loss table written out
    (tests/test_gcp.py: o_loss, o_dloss). Returns (fhat, grads, S, fabs):
    S[t] the sum of absolute contributions per element of G_t, fabs the sum
    of the absolute terms of fhat."""
    nm = len(mats)
    grads = [torch.zeros_like(A) for A in mats]
    S = [torch.zeros_like(A) for A in mats]
    fhat = fabs = 0.0
    zero = torch.zeros((), dtype=F64)
    for j in range(s.p + s.q):
        rows = [mats[t][int(s.inds[t, j])] for t in range(nm)]
        prod = torch.ones_like(rows[0])
        for r in rows:
            prod = prod * r
        mdl = prod.sum()
        x = s.vals[j]
        if j < s.p:
            y = s.wnz * (o_dloss(loss, x, mdl, param)
                         - o_dloss(loss, zero, mdl, param))
            l = s.wnz * (o_loss(loss, x, mdl, param)
                         - o_loss(loss, zero, mdl, param))
        else:
            y = s.wz * o_dloss(loss, zero, mdl, param)
            l = s.wz * o_loss(loss, zero, mdl, param)
        fhat += float(l)
        fabs += abs(float(l))
        for t in range(nm):
            pi = torch.ones_like(rows[0])
            for u in range(nm):
                if u != t:
                    pi = pi * rows[u]
            i = int(s.inds[t, j])
            grads[t][i] += y * pi
            S[t][i] += (y * pi).abs()
    return fhat, grads, S, fabs


def abs_sums(s, mats, loss, param=None):
    """S and fabs of `loop_oracle`, vectorised (for the larger samples)."""
    nm = len(mats)
    idx = [s.inds[t].long() for t in range(nm)]
    a = [mats[t][idx[t]] for t in range(nm)]
    prod = a[0]
    for r in a[1:]:
        prod = prod * r
    mdl = prod.sum(1)
    zero = torch.zeros_like(mdl)
    stored = torch.arange(s.p + s.q) < s.p
    d0, l0 = o_dloss(loss, zero, mdl, param), o_loss(loss, zero, mdl, param)
    y = torch.where(stored, s.wnz * (o_dloss(loss, s.vals, mdl, param) - d0),
                    s.wz * d0)
    l = torch.where(stored, s.wnz * (o_loss(loss, s.vals, mdl, param) - l0),
                    s.wz * l0)
    S = []
    for t in range(nm):
        pi = torch.ones_like(a[0])
        for u in range(nm):
            if u != t:
                pi = pi * a[u]
        S.append(torch.zeros_like(mats[t]).index_add_(
            0, idx[t], (y.unsqueeze(1) * pi).abs()))
    return S, float(l.abs().sum())


def scaled_err(got, ref, S):
    """max |got - ref| / S over the elements with S > 0; elements with
    S = 0 received only exact zeros and must be exactly equal."""
    got, ref = got.cpu(), ref.cpu()
    live = S > 0
    assert torch.equal(got[~live], ref[~live])
    if not bool(live.any()):
        return 0.0
    return float(((got - ref).abs()[live] / S[live]).max())


def assert_sgrad_close(got, ref, S, fabs, what, tol=TOL):
    """got, ref: (fhat | None, grads)."""
    worst = 0.0
    for t, (G, R) in enumerate(zip(got[1], ref[1])):
        assert G.dtype == F64 and G.shape == R.shape, (what, t)
        worst = max(worst, scaled_err(G, R, S[t]))
    if ref[0] is not None and got[0] is not None:
        fe = abs(float(got[0]) - float(ref[0])) / max(fabs, 1e-300)
        worst = max(worst, fe)
    print(f"{what}: max|delta|/S = {worst:.3e} (bound {tol:.1e})")
    assert worst <= tol, (what, worst)
    return worst


# The cases of tests/test_sgcp_gpu.py; here the torch path runs them. The
# ranks cover every group width W = 1, 2, 4, 8, 16, 32, 64 and both sides of
# each boundary; the (p, q) a single sample, a tail group, the stored/cell
# boundary inside a wave step, and more than one wave.
GRID_RANKS = [1, 2, 3, 7, 16, 17, 32, 33, 64]
GRID_PQ = [(1, 1), (1, 63), (31, 33), (64, 1), (1000, 999)]
GRID_LOSSES = ["gaussian", "bernoulli-logit"]
# kept small: every rank at 3 modes and every (p, q); every mode count at
# the ranks on both sides of a width boundary and two (p, q)
GRID_CASES = ([(3, r, pq) for r in GRID_RANKS for pq in GRID_PQ]
              + [(nm, r, pq) for nm in (4, 5, 8) for r in (3, 17, 64)
                 for pq in ((31, 33), (1000, 999))])
ALL_LOSS_CASES = [(4, 17, (150, 171))]


@functools.lru_cache(maxsize=None)
def grid_case(nm, rank, pq, loss):
    """(sample, mats, reference (fhat, grads) by the CPU torch path, S,
    fabs): computed once, shared, never modified."""
    dims = DIMS[nm]
    s = make_sample(dims, pq[0], pq[1], VALUE_KIND[loss],
                    seed=1000 * nm + rank)
    mats = make_mats(dims, rank, loss in BOUNDED)
    ref = sp.gcp_sgrad(s, mats, loss, param=param_of(loss), want_loss=True,
                       impl="torch")
    S, fabs = abs_sums(s, mats, loss, param_of(loss))
    return s, mats, ref, S, fabs


# ----------------------------------------------------------------- sampler

def small_tensor(dims=(6, 5, 7), nnz=40, seed=3, kind="count"):
    g = torch.Generator().manual_seed(seed)
    total = math.prod(dims)
    cells = torch.randperm(total, generator=g)[:nnz]
    cols, rem = [], cells
    for d in reversed(dims):
        cols.append(rem % d)
        rem = rem // d
    inds = torch.stack(list(reversed(cols)), 0)
    return sp.SpTensor(inds, draw_values(kind, nnz, g) + 10.0, list(dims))


def test_sampler_shapes_determinism_and_membership():
    t = small_tensor()
    g = torch.Generator().manual_seed(11)
    s = sp.gcp_sample(t, 50, 70, g)
    assert isinstance(s, sp.GcpSample)
    assert s.inds.dtype == I32 and tuple(s.inds.shape) == (3, 120)
    assert s.inds.is_contiguous()
    assert s.vals.dtype == F64 and tuple(s.vals.shape) == (120,)
    assert (s.p, s.q) == (50, 70)
    assert s.wnz == t.nnz / 50 and s.wz == (6 * 5 * 7) / 70
    # deterministic in the generator
    s2 = sp.gcp_sample(t, 50, 70, torch.Generator().manual_seed(11))
    assert torch.equal(s.inds, s2.inds) and torch.equal(s.vals, s2.vals)
    s3 = sp.gcp_sample(t, 50, 70, g)      # the generator has moved on
    assert not torch.equal(s.inds, s3.inds)
    # stored draws: a stored coordinate with its value (values are >= 11)
    stored = {tuple(t.inds[:, k].tolist()): float(t.vals[k])
              for k in range(t.nnz)}
    for j in range(50):
        assert stored[tuple(s.inds[:, j].tolist())] == float(s.vals[j])
    assert len({tuple(s.inds[:, j].tolist()) for j in range(50)}) > 1
    # cell draws: inside dims, value 0, whether stored or not
    for m, d in enumerate(t.dims):
        assert int(s.inds[m].min()) >= 0 and int(s.inds[m].max()) < d
    assert bool((s.vals[50:] == 0).all())
    # with this many draws every index of every mode shows up
    big = sp.gcp_sample(t, 1, 4000, torch.Generator().manual_seed(5))
    for m, d in enumerate(t.dims):
        assert big.inds[m, 1:].unique().numel() == d


def test_sampler_errors():
    t = small_tensor()
    g = torch.Generator().manual_seed(1)
    with pytest.raises(ValueError, match="p and q must be >= 1"):
        sp.gcp_sample(t, 0, 5, g)
    with pytest.raises(ValueError, match="p and q must be >= 1"):
        sp.gcp_sample(t, 5, 0, g)
    t32 = sp.SpTensor(t.inds, t.vals.float(), list(t.dims))
    with pytest.raises(ValueError, match="float64"):
        sp.gcp_sample(t32, 5, 5, g)
    wide = sp.SpTensor(t.inds, t.vals, [1 << 31, 5, 7])
    with pytest.raises(ValueError, match="below 2\\^31"):
        sp.gcp_sample(wide, 5, 5, g)
    huge = sp.SpTensor(t.inds, t.vals, [(1 << 31) - 1] * 3)
    with pytest.raises(ValueError, match="too many cells"):
        sp.gcp_sample(huge, 5, 5, g)
    empty = sp.SpTensor(torch.zeros(3, 0, dtype=torch.int64),
                        torch.zeros(0, dtype=F64), list(t.dims))
    with pytest.raises(ValueError, match="no stored entries"):
        sp.gcp_sample(empty, 5, 5, g)


def test_sampler_large_cell_space():
    """total just under 2^62: the cell decode stays in 64 bits."""
    dims = [(1 << 21) - 1, (1 << 21) - 1, (1 << 20) - 1]
    inds = torch.tensor([[5], [6], [7]])
    t = sp.SpTensor(inds, torch.ones(1, dtype=F64), dims)
    s = sp.gcp_sample(t, 3, 2000, torch.Generator().manual_seed(2))
    for m, d in enumerate(dims):
        assert int(s.inds[m].min()) >= 0 and int(s.inds[m].max()) < d
    assert int(s.inds[0].max()) > 1 << 19
    assert s.wz == math.prod(dims) / 2000


# ------------------------------------------ estimator algebra, enumerated

ENUM_DIMS = {3: [4, 3, 5], 4: [3, 2, 3, 2], 5: [2, 3, 2, 2, 2]}


def enum_case(nm, loss):
    """A tiny tensor with 20 stored entries and the sample that holds every
    stored entry once (p = nnz) and every cell once (q = total)."""
    dims = ENUM_DIMS[nm]
    total = math.prod(dims)
    t = small_tensor(tuple(dims), 20, seed=40 + nm, kind=VALUE_KIND[loss])
    t = sp.SpTensor(t.inds, t.vals - 10.0, dims)
    cells = torch.arange(total)
    cols, rem = [], cells
    for d in reversed(dims):
        cols.append(rem % d)
        rem = rem // d
    ci = torch.stack(list(reversed(cols)), 0)
    inds = torch.cat([t.inds, ci], 1).to(I32).contiguous()
    vals = torch.cat([t.vals, torch.zeros(total, dtype=F64)])
    return t, sp.GcpSample(inds, vals, t.nnz, total, 1.0, 1.0)


def dense_of(t):
    X = torch.zeros(t.dims, dtype=F64)
    X[tuple(t.inds)] = t.vals
    return X


def dense_autograd(t, mats, loss):
    letters = "abcdefgh"[:t.nmodes]
    eq = ",".join(f"{c}z" for c in letters) + "->" + letters
    leaves = [A.clone().requires_grad_(True) for A in mats]
    f = o_loss(loss, dense_of(t), torch.einsum(eq, *leaves),
               param_of(loss)).sum()
    f.backward()
    return float(f.detach()), [A.grad for A in leaves]


def dense_second(t, mats, loss):
    """The dense side again: the model cell by cell from gathered rows, the
    analytic derivative, index_add_."""
    nm, dims = t.nmodes, list(t.dims)
    grid = torch.cartesian_prod(*[torch.arange(d) for d in dims]).T
    rows = [mats[m][grid[m]] for m in range(nm)]
    prod = rows[0]
    for r in rows[1:]:
        prod = prod * r
    mdl = prod.sum(1)
    x = dense_of(t).reshape(-1)
    y = o_dloss(loss, x, mdl, param_of(loss))
    grads = []
    for m in range(nm):
        pi = torch.ones_like(rows[0])
        for u in range(nm):
            if u != m:
                pi = pi * rows[u]
        grads.append(torch.zeros_like(mats[m]).index_add_(
            0, grid[m], y.unsqueeze(1) * pi))
    return float(o_loss(loss, x, mdl, param_of(loss)).sum()), grads


def enum_err(a, b):
    """max relative to max(1, max|b|) over the loss and every gradient."""
    worst = abs(a[0] - b[0]) / max(1.0, abs(b[0]))
    for G, R in zip(a[1], b[1]):
        worst = max(worst, float((G - R).abs().max())
                    / max(1.0, float(R.abs().max())))
    return worst


def enum_measure(nm, loss):
    t, s = enum_case(nm, loss)
    mats = make_mats(t.dims, 3, loss in BOUNDED, seed=9)
    dense = dense_autograd(t, mats, loss)
    second = dense_second(t, mats, loss)
    fhat, grads = sp.gcp_sgrad(s, mats, loss, param=param_of(loss),
                               want_loss=True)
    return enum_err(second, dense), enum_err((float(fhat), grads), dense)


@pytest.mark.parametrize("nm", [3, 4, 5])
@pytest.mark.parametrize("loss", LOSSES)
def test_estimator_is_exact_by_enumeration(loss, nm):
    """With every stored entry once and every cell once, weights 1, the
    estimate IS the full-tensor loss and gradient, zeros as data: catches a
    wrong weight or a wrong correction term."""
    spread, err = enum_measure(nm, loss)
    print(f"{loss} {nm} modes: dense twice {spread:.3e}, estimator vs dense "
          f"{err:.3e} (bound {ENUM_TOL:.1e})")
    assert 1e2 * spread <= ENUM_TOL
    assert err <= ENUM_TOL


# ------------------------------------------- torch path vs per-sample loop

@pytest.mark.parametrize("loss", LOSSES)
def test_torch_path_matches_sample_loop(loss):
    nm, rank = 4, 5
    s = make_sample(DIMS[nm], 40, 55, VALUE_KIND[loss], seed=77)
    mats = make_mats(DIMS[nm], rank, loss in BOUNDED)
    fhat, grads, S, fabs = loop_oracle(s, mats, loss, param_of(loss))
    # duplicates: fewer distinct coordinates than samples
    assert s.inds[0].unique().numel() < 95
    got = sp.gcp_sgrad(s, mats, loss, param=param_of(loss), want_loss=True,
                       impl="torch")
    assert_sgrad_close(got, (fhat, grads), S, fabs, f"torch vs loop {loss}")
    none, g2 = sp.gcp_sgrad(s, mats, loss, param=param_of(loss))
    assert none is None
    for a, b in zip(g2, got[1]):
        assert torch.equal(a, b)


def test_two_sample_orders_agree_within_tol():
    """The figure TOL is derived from, on a few of its cases (the module's
    __main__ block prints it for all); asserted with two of the three orders
    of margin."""
    worst = 0.0
    for loss in GRID_LOSSES:
        for case in [(3, 16, (1000, 999)), (8, 17, (1000, 999)),
                     (4, 3, (31, 33))]:
            worst = max(worst, order_spread(*case, loss))
    print(f"two sample orders differ by {worst:.3e} * S")
    assert 1e2 * worst <= TOL


def order_spread(nm, rank, pq, loss):
    s, mats, ref, S, fabs = grid_case(nm, rank, pq, loss)
    rev = sp.gcp_sgrad(reversed_sample(s), mats, loss, param=param_of(loss),
                       want_loss=True, impl="torch")
    worst = abs(float(rev[0]) - float(ref[0])) / fabs
    for t in range(nm):
        worst = max(worst, scaled_err(rev[1][t], ref[1][t], S[t]))
    return worst


def test_out_views_are_zeroed_and_filled():
    nm, rank = 3, 4
    dims = DIMS[nm]
    s = make_sample(dims, 9, 11, "any", seed=5)
    mats = make_mats(dims, rank, False)
    _, ref = sp.gcp_sgrad(s, mats, "gaussian")
    flat = torch.full((sum(dims) * rank + 2,), 7.0, dtype=F64)
    views, o = [], 1
    for d in dims:
        views.append(flat[o:o + d * rank].view(d, rank))
        o += d * rank
    _, out = sp.gcp_sgrad(s, mats, "gaussian", out=views)
    assert all(a is b for a, b in zip(out, views))
    for a, b in zip(views, ref):
        assert torch.equal(a, b)
    assert flat[0] == 7.0 and flat[-1] == 7.0


def test_sgrad_errors():
    dims = DIMS[3]
    s = make_sample(dims, 4, 4, "any", seed=1)
    mats = make_mats(dims, 4, False)
    with pytest.raises(ValueError, match="3..8 modes"):
        sp.gcp_sgrad(s, mats[:2], "gaussian")
    with pytest.raises(ValueError, match="rank 1..64"):
        sp.gcp_sgrad(s, [torch.ones(d, 65, dtype=F64) for d in dims],
                     "gaussian")
    with pytest.raises(ValueError, match="dtype/device"):
        sp.gcp_sgrad(s, [m.float() for m in mats], "gaussian")
    with pytest.raises(ValueError, match="unknown loss"):
        sp.gcp_sgrad(s, mats, "hinge")
    with pytest.raises(ValueError, match="huber needs param"):
        sp.gcp_sgrad(s, mats, "huber")
    with pytest.raises(ValueError, match="unknown impl"):
        sp.gcp_sgrad(s, mats, "gaussian", impl="triton")
    with pytest.raises(ValueError, match="needs a device tensor"):
        sp.gcp_sgrad(s, mats, "gaussian", impl="hip")
    with pytest.raises(ValueError, match="values 0 or 1"):
        sp.gcp_sgrad(make_sample(dims, 4, 4, "any", seed=1), mats,
                     "bernoulli-logit")
    with pytest.raises(ValueError, match="values >= 0"):
        sp.gcp_sgrad(make_sample(dims, 4, 4, "any", seed=1),
                     [m.abs() for m in mats], "poisson")
    bad = sp.GcpSample(s.inds.clone(), s.vals, 4, 4, 1.0, 1.0)
    bad.inds[1, 3] = dims[1]
    with pytest.raises(ValueError, match="indices outside"):
        sp.gcp_sgrad(bad, mats, "gaussian")
    with pytest.raises(ValueError, match="int32"):
        sp.gcp_sgrad(sp.GcpSample(s.inds.long(), s.vals, 4, 4, 1.0, 1.0),
                     mats, "gaussian")
    with pytest.raises(ValueError, match="out\\[0\\]"):
        sp.gcp_sgrad(s, mats, "gaussian",
                     out=[torch.zeros(d, 5, dtype=F64) for d in dims])


# -------------------------------------------------------------------- Adam

ADAM = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8)


def adam_buffers(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=F64)
    grad = torch.randn(n, generator=g, dtype=F64) * 3.0
    m = torch.randn(n, generator=g, dtype=F64) * 0.1
    v = torch.rand(n, generator=g, dtype=F64) * 0.01
    if n > 2:
        grad[1] = 0.0
        v[2] = 0.0
    return x, grad, m, v


def adam_scalar(x, g, m, v, step, lower, lr, beta1, beta2, eps):
    """The formula one element at a time in Python floats (IEEE double,
    every operation rounded once)."""
    c1 = 1.0 / (1.0 - beta1 ** step)
    c2 = 1.0 / (1.0 - beta2 ** step)
    xs, ms, vs = [], [], []
    for xi, gi, mi, vi in zip(x.tolist(), g.tolist(), m.tolist(),
                              v.tolist()):
        mi = beta1 * mi + (1.0 - beta1) * gi
        vi = beta2 * vi + ((1.0 - beta2) * gi) * gi
        xi = xi - (lr * (mi * c1)) / (math.sqrt(vi * c2) + eps)
        if lower is not None:
            xi = max(xi, lower)
        xs.append(xi)
        ms.append(mi)
        vs.append(vi)
    return (torch.tensor(xs, dtype=F64), torch.tensor(ms, dtype=F64),
            torch.tensor(vs, dtype=F64))


# Bound on x in units of 2^-52 * max(|x before|, |update|). m and v are
# products and sums only and must be bitwise equal. In x the one operation
# that is not correctly rounded everywhere is the square root (torch's CPU
# sqrt goes through a vector math library and was seen one ulp off
# math.sqrt): one ulp there moves the denominator by at most 2 ulp, the
# quotient by at most 3, and the subtraction rounds once more: 4. Measured
# torch path vs scalar loop here: 1.0 (one element of 257).
ADAM_ULPS = 4.0


def adam_x_ulps(got, ref, before):
    scale = torch.maximum(before.abs(), (before - ref).abs()) * 2.0 ** -52
    d = (got.cpu() - ref).abs()
    assert torch.equal(d[scale == 0], torch.zeros_like(d[scale == 0]))
    live = scale > 0
    return float((d[live] / scale[live]).max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize("lower", [None, 0.0])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_torch_matches_scalar_loop(step, lower):
    x, g, m, v = adam_buffers(257)
    before = x.clone()
    want = adam_scalar(x, g, m, v, step, lower, **ADAM)
    sp.adam_step(x, g, m, v, step=step, lower=lower, **ADAM)
    err = adam_x_ulps(x, want[0], before)
    print(f"adam torch vs scalar loop, step {step}: {err:.2f} ulp "
          f"(bound {ADAM_ULPS}), {int((x != want[0]).sum())} of 257 differ")
    assert err <= ADAM_ULPS
    assert torch.equal(m, want[1]) and torch.equal(v, want[2])
    assert bool((g == 0).all())
    if lower is not None:
        assert bool((x >= 0).all()) and int((x == 0).sum()) > 10


def test_adam_errors():
    x, g, m, v = adam_buffers(8)
    with pytest.raises(ValueError, match="step counts from 1"):
        sp.adam_step(x, g, m, v, step=0, lr=0.1)
    with pytest.raises(ValueError, match="g must be a flat"):
        sp.adam_step(x, g.float(), m, v, step=1, lr=0.1)
    with pytest.raises(ValueError, match="v must be a flat"):
        sp.adam_step(x, g, m, v[:4], step=1, lr=0.1)
    with pytest.raises(ValueError, match="needs a device tensor"):
        sp.adam_step(x, g, m, v, step=1, lr=0.1, impl="hip")


# ------------------------------------------------------------------ driver

PLANTED_DIMS = [30, 25, 20]
PLANTED_RANK = 3
PLANTED_OPTS = dict(lr=1e-2, p=2000, q=2000, p_loss=15000, q_loss=15000,
                    iters_per_epoch=200, seed=7)
PLANTED_EPOCHS = {"bernoulli-logit": 5, "poisson": 10}
# final exact loss / initial exact loss, measured on the CPU path: 0.625
# (logit; 10422.0 -> 6511.4 in 5 epochs, one of them undone; the planted
# logits themselves give 5778.2) and 0.466 (poisson; 8354.3 -> 3896.4, ended
# by its second failed epoch after 9); the bounds are 1.25 x that
PLANTED_FRACTION = {"bernoulli-logit": 0.78, "poisson": 0.583}
# mean fitted probability on the ones minus on the zeros, measured 0.351
# (0.561 / 0.210); the bound is that / 1.25
LOGIT_GAP = 0.28


@functools.lru_cache(maxsize=None)
def planted(loss):
    """Dense data of a planted rank-3 model, all 15000 cells, stored as the
    nonzero cells only. Returns (tensor, dense array)."""
    g = torch.Generator().manual_seed(2027)
    if loss == "poisson":
        # sparse nonnegative factors: most cells have a rate near 0
        A = [torch.rand(d, PLANTED_RANK, generator=g, dtype=F64) ** 3 * 1.6
             for d in PLANTED_DIMS]
        X = torch.poisson(torch.einsum("if,jf,kf->ijk", *A), generator=g)
    else:
        A = [torch.randn(d, PLANTED_RANK, generator=g, dtype=F64) * 1.3
             for d in PLANTED_DIMS]
        m = torch.einsum("if,jf,kf->ijk", *A) - 1.3
        X = (torch.rand(m.shape, generator=g, dtype=F64)
             < torch.sigmoid(m)).double()
    inds = X.nonzero().T.contiguous()
    return sp.SpTensor(inds, X[tuple(inds)].clone(), list(PLANTED_DIMS)), X


def exact_loss(X, factors, lam, loss):
    """The objective itself: the loss over ALL cells, densely."""
    fs = [f.cpu() for f in factors]
    m = torch.einsum("if,jf,kf,f->ijk", *fs, lam.cpu())
    return float(o_loss(loss, X, m).sum()), m


def initial_factors(loss, seed):
    out = []
    for k, d in enumerate(PLANTED_DIMS):
        A = sp.seeded_init(d, PLANTED_RANK, k, seed)
        out.append(A.abs() if loss in BOUNDED else A * 0.3)
    return out


def check_planted(device, loss, gap=True, **over):
    t, X = planted(loss)
    opts = sp.SgcpOptions(max_epochs=PLANTED_EPOCHS[loss],
                          **{**PLANTED_OPTS, **over})
    r = sp.cpd_sgcp(t.to(device), PLANTED_RANK, loss, opts)
    assert all(A.device.type == device for A in r.factors)
    f0, _ = exact_loss(X, initial_factors(loss, opts.seed),
                       torch.ones(PLANTED_RANK, dtype=F64), loss)
    f1, m = exact_loss(X, r.factors, r.lam, loss)
    print(f"{loss} on {device}: exact loss {f0:.1f} -> {f1:.1f} "
          f"(fraction {f1 / f0:.4f}, bound {PLANTED_FRACTION[loss]}) in "
          f"{r.nepochs} epochs, {r.nsteps} steps, {r.nfails} failures")
    assert r.nepochs == len(r.loss_trace) - 1 == len(r.lr_trace)
    assert r.nepochs <= PLANTED_EPOCHS[loss]
    assert f1 <= PLANTED_FRACTION[loss] * f0
    for A in r.factors:
        nrm = A.norm(dim=0).cpu()
        assert bool(((nrm - 1).abs() < 1e-12).logical_or(nrm == 0).all())
        if loss in BOUNDED:
            assert bool((A >= 0).all())
    if loss == "bernoulli-logit":
        prob = torch.sigmoid(m)
        p1, p0 = float(prob[X == 1].mean()), float(prob[X == 0].mean())
        print(f"  mean probability on ones / zeros: {p1:.3f} / {p0:.3f} "
              f"(gap bound {LOGIT_GAP})")
        if gap:
            assert p1 - p0 >= LOGIT_GAP
    return r


def test_planted_data_is_as_described():
    t, X = planted("bernoulli-logit")
    assert 0.25 <= t.nnz / X.numel() <= 0.35
    t, X = planted("poisson")
    assert t.nnz / X.numel() <= 0.35 and bool((t.vals >= 1).all())


@pytest.mark.parametrize("loss", ["bernoulli-logit", "poisson"])
def test_cpd_sgcp_planted(loss):
    check_planted("cpu", loss)


def test_driver_is_deterministic_on_cpu():
    t, _ = planted("bernoulli-logit")
    opts = sp.SgcpOptions(max_epochs=1, **{**PLANTED_OPTS,
                                           "iters_per_epoch": 5})
    a = sp.cpd_sgcp(t, 3, "bernoulli-logit", opts)
    b = sp.cpd_sgcp(t, 3, "bernoulli-logit", opts)
    assert a.loss_trace == b.loss_trace
    assert all(torch.equal(x, y) for x, y in zip(a.factors, b.factors))
    assert a.nsteps == 5


def test_failed_epoch_is_rolled_back_and_lr_decays():
    t, _ = planted("bernoulli-logit")
    base = dict(p=200, q=200, p_loss=1000, q_loss=1000, iters_per_epoch=3,
                seed=7)
    start = sp.cpd_sgcp(t, 3, "bernoulli-logit",
                        sp.SgcpOptions(max_epochs=0, **base))
    assert start.nepochs == 0 and len(start.loss_trace) == 1
    # an absurd lr: every epoch fails
    r = sp.cpd_sgcp(t, 3, "bernoulli-logit",
                    sp.SgcpOptions(lr=1e3, decay=0.5, max_fails=2,
                                   max_epochs=50, **base))
    assert r.nfails == 3 and r.nepochs == 3 and r.nsteps == 0
    assert r.lr_trace == [1e3, 5e2, 2.5e2]
    assert len(r.loss_trace) == 4
    assert all(f >= r.loss_trace[0] for f in r.loss_trace[1:])
    # undone: the factors are the initial ones
    for a, b in zip(r.factors, start.factors):
        assert torch.equal(a, b)
    assert torch.equal(r.lam, start.lam)
    # max_fails ends the run: the default allows two failures
    r = sp.cpd_sgcp(t, 3, "bernoulli-logit",
                    sp.SgcpOptions(lr=1e3, max_epochs=50, **base))
    assert r.nfails == 2 and r.nepochs == 2
    # a good epoch after a failed one goes on from the restored state with
    # the decayed lr
    r = sp.cpd_sgcp(t, 3, "bernoulli-logit",
                    sp.SgcpOptions(lr=1e3, decay=1e-5, max_fails=1,
                                   max_epochs=3, **base))
    assert r.nfails == 1 and r.nepochs == 3 and r.nsteps == 6
    assert r.lr_trace == [1e3, 1e3 * 1e-5, 1e3 * 1e-5]
    assert r.loss_trace[3] < r.loss_trace[2] < r.loss_trace[0]


def test_driver_defaults_and_errors():
    o = sp.SgcpOptions()
    assert (o.lr, o.beta1, o.beta2, o.eps, o.decay, o.max_fails,
            o.iters_per_epoch, o.max_epochs) == (1e-3, 0.9, 0.999, 1e-8, 0.1,
                                                 1, 1000, 1000)
    assert o.p is None and o.q is None and o.p_loss is None
    t, _ = planted("poisson")
    with pytest.raises(ValueError, match="takes an SpTensor"):
        sp.cpd_sgcp(sp.csf_alloc(t, "all"), 3, "poisson")
    with pytest.raises(ValueError, match="rank 1..64"):
        sp.cpd_sgcp(t, 65, "poisson")
    with pytest.raises(ValueError, match="values 0 or 1"):
        sp.cpd_sgcp(t, 3, "bernoulli-logit")
    with pytest.raises(ValueError, match="float64"):
        sp.cpd_sgcp(sp.SpTensor(t.inds, t.vals.float(), list(t.dims)), 3,
                    "poisson")
    # the defaults of p, q and the loss sample
    r = sp.cpd_sgcp(t, 2, "poisson",
                    sp.SgcpOptions(max_epochs=1, iters_per_epoch=2))
    assert r.nepochs == 1


# ----------------------------------------------------------- CLI, example

def test_cli_sgcp(tmp_path, capsys):
    from splatt_amd import cli
    t, _ = planted("bernoulli-logit")
    path = str(tmp_path / "ones.tns")
    t.save(path)
    stem = str(tmp_path / "out" / "s_")
    rc = cli.main(["sgcp", path, "-r", "4", "--loss", "bernoulli-logit",
                   "-e", "2", "--iters-per-epoch", "5", "-p", "300", "-q",
                   "300", "--lr", "0.01", "--seed", "77", "--device", "cpu",
                   "--stem", stem])
    assert rc == 0
    out = capsys.readouterr().out
    assert "epoch = 0 loss = " in out and "epoch = 2 loss = " in out
    assert "Final loss estimate:" in out
    loaded = sp.SpTensor.load(path)
    for m in range(3):
        rows = open(f"{stem}mode{m + 1}.mat").read().strip().splitlines()
        assert len(rows) == loaded.dims[m] and len(rows[0].split()) == 4
    assert len(open(f"{stem}lambda.mat").read().split()) == 4
    rc = cli.main(["sgcp", path, "-r", "2", "--loss", "huber", "--param",
                   "0.5", "-e", "1", "--iters-per-epoch", "2", "--device",
                   "cpu", "--nowrite"])
    assert rc == 0
    assert not os.path.exists(str(tmp_path / "mode1.mat"))


def test_example_runs(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runpy.run_path(os.path.join(root, "examples", "sgcp_binary.py"),
                   run_name="__main__")
    out = capsys.readouterr().out
    assert "exact loss" in out


# ---------------------------------------------------------- binding checks

def _grad_args():
    nm, rank, n = 3, 8, 12
    return [torch.zeros(nm, n, dtype=I32), torch.ones(n, dtype=F64), 5,
            [torch.ones(4, rank, dtype=F64) for _ in range(nm)],
            [torch.zeros(4, rank, dtype=F64) for _ in range(nm)],
            0, 0.0, 1.0, 1.0, None]


def _adam_args():
    return [torch.zeros(16, dtype=F64) for _ in range(4)] + [
        1e-3, 0.9, 0.999, 1e-8, 10.0, 1000.0, None]


def test_bindings_are_not_gpu_names():
    """tests/test_binding_checks.py owns the table of gpu_* bindings."""
    for name in ("hip_sgcp_grad", "hip_adam_step"):
        assert hasattr(native(), name)


@pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="host tensors must never reach a device; needs a GPU-less box")
def test_bindings_reject_host_tensors_and_wrong_dtype():
    fn = native().hip_sgcp_grad
    with pytest.raises(RuntimeError, match="inds must be a device tensor"):
        fn(*_grad_args(), 0)
    args = _grad_args()
    args[0] = args[0].to(torch.int16)
    with pytest.raises(RuntimeError, match="inds has dtype Short"):
        fn(*args, 0)
    args = _grad_args()
    args[0] = args[0].long()
    with pytest.raises(RuntimeError, match="inds has dtype Long"):
        fn(*args, 0)
    fn = native().hip_adam_step
    with pytest.raises(RuntimeError, match="x must be a device tensor"):
        fn(*_adam_args(), 0)
    args = _adam_args()
    args[0] = args[0].to(torch.int16)
    with pytest.raises(RuntimeError, match="x has dtype Short"):
        fn(*args, 0)


# ------------------------------------------------ re-measuring the bounds

if __name__ == "__main__":
    worst = 0.0
    for loss in GRID_LOSSES:
        for nm, rank, pq in GRID_CASES:
            worst = max(worst, order_spread(nm, rank, pq, loss))
    for loss in LOSSES:
        for nm, rank, pq in ALL_LOSS_CASES:
            worst = max(worst, order_spread(nm, rank, pq, loss))
    print(f"two sample orders: {worst:.3e} * S  (TOL {TOL:.1e})")
    w1 = w2 = 0.0
    for loss in LOSSES:
        for nm in (3, 4, 5):
            a, b = enum_measure(nm, loss)
            w1, w2 = max(w1, a), max(w2, b)
    print(f"dense twice: {w1:.3e}; estimator vs dense: {w2:.3e}  "
          f"(ENUM_TOL {ENUM_TOL:.1e})")
    for loss in ("bernoulli-logit", "poisson"):
        check_planted("cpu", loss)
