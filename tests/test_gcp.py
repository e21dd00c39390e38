"""Generalized CPD (GCP): the torch path against a row-by-row CPU oracle, the
tail / stored-zero rules, the quasi-Newton driver on planted cases, zero
sampling, errors, the CLI and the example.

The oracles, inputs and bounds here are shared with tests/test_gcp_gpu.py.

Bounds. Float comparisons use  max|delta| <= TOL * max(1, max|oracle|).
Two independent CPU f64 evaluations of the gradient pass (the oracle:
`H @ a` and `H.T @ y` per row with the formulas of the loss table written
out plainly; the second evaluation: numpy, the entries of a row in reversed
order, every sum accumulated one term at a time) differ by at most 1.2e-14
relative to max(1, max|oracle|) over G and frow on the `heavy` input, all
eight losses, ranks 7/16/32/64, all modes; TOL is that figure with about
three orders of margin. DRV_TOL bounds the relative difference of the
driver's loss trace on the fixed schedule FIXED_DRV of the `4-mode` input
over the losses of FIXED_LOSSES: the torch path and the oracle-driven driver
differ by at most 1.6e-15 there; DRV_TOL is that with three orders of
margin. `PYTHONPATH=. python tests/test_gcp.py` re-measures both figures and
re-runs the seed / cap choice of the planted cases.
"""
import functools
import math
import os
import runpy

import numpy as np
import pytest
import torch

import splatt_amd as sp
from splatt_amd import completion, gcp
from splatt_amd._ext import native

from test_apr import exact_case, four_mode, heavy, row_counts, thin

TOL = 1.2e-11
DRV_TOL = 1.6e-12
EPS = 1e-10
RANKS = [1, 7, 16, 17, 32, 64]
LOSSES = ["gaussian", "huber", "poisson", "poisson-log", "bernoulli-odds",
          "bernoulli-logit", "gamma", "rayleigh"]
BOUNDED = {"poisson", "bernoulli-odds", "gamma", "rayleigh"}
DOMAIN = {"gaussian": "any", "huber": "any", "poisson": "count",
          "poisson-log": "count", "bernoulli-odds": "binary",
          "bernoulli-logit": "binary", "gamma": "positive",
          "rayleigh": "count"}
HUBER_DELTA = 0.75


def param_of(loss):
    return HUBER_DELTA if loss == "huber" else None


# ------------------------------------------------------------------ inputs

EDGE_COUNTS = [1, 2, 63, 64, 65, 0, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def edges():
    """dims [10, 60, 50]; mode-0 rows of 1, 2, 63, 64, 65, 0, 1023, 1024,
    1025 and 2049 entries at distinct random cells: every length around a
    64-entry batch and around SEG, one empty row, two multi-segment rows
    whose last segment holds a single entry."""
    g = torch.Generator().manual_seed(99)
    rows, cols = [], []
    for i, n in enumerate(EDGE_COUNTS):
        cell = torch.randperm(60 * 50, generator=g)[:n]
        rows.append(torch.full((n,), i, dtype=torch.int64))
        cols.append(cell)
    i0, cell = torch.cat(rows), torch.cat(cols)
    inds = torch.stack([i0, cell // 50, cell % 50], 0)
    return sp.SpTensor(inds, torch.ones(inds.shape[1], dtype=torch.float64),
                       [10, 60, 50])


COORDS = {"heavy": heavy, "thin": thin, "4-mode": four_mode, "edges": edges}


@functools.lru_cache(maxsize=None)
def make_input(name, domain):
    """The coordinates of `name` with values for a loss domain: any =
    normal, count = 0..3 (a third zeros), binary = 0/1, positive = 0.1..2.1."""
    t = COORDS[name]()
    g = torch.Generator().manual_seed(7 + len(name) + len(domain))
    if domain == "any":
        v = torch.randn(t.nnz, generator=g, dtype=torch.float64)
    elif domain == "count":
        v = torch.randint(0, 4, (t.nnz,), generator=g).double()
        v = v * (torch.rand(t.nnz, generator=g) > 1 / 3)
    elif domain == "binary":
        v = (torch.rand(t.nnz, generator=g) < 0.5).double()
    else:
        v = 0.1 + 2.0 * torch.rand(t.nnz, generator=g, dtype=torch.float64)
    return sp.SpTensor(t.inds.clone(), v, list(t.dims))


def check_preconditions(name):
    """The inputs must keep covering the branches they were chosen for."""
    t = COORDS[name]()
    if name == "heavy":
        for m in range(t.nmodes):
            cnt = row_counts(t, m)
            assert int((cnt == 0).sum()) >= 1, m
            assert int((cnt > completion.SEG).sum()) == 7, m
    elif name == "thin":
        for m in range(t.nmodes):
            cnt = row_counts(t, m)
            assert int((cnt == 0).sum()) >= 1, m
            assert int(cnt.max()) < 16, m
    elif name == "edges":
        assert row_counts(t, 0).tolist() == EDGE_COUNTS
        lin = (t.inds[0] * 60 + t.inds[1]) * 50 + t.inds[2]
        assert int(torch.unique(lin).numel()) == t.nnz


def check_edges_plan(cs):
    """7 single segments of exactly the short lengths, and two multi-segment
    rows cut as 1024 + 1 and 1024 + 1024 + 1."""
    check_preconditions("edges")
    assert completion.SEG == 1024
    plan = gcp.gcp_plan(cs, 0)
    ns = plan["nsingle"]
    assert ns == 7
    assert plan["seg_len"][:ns].tolist() == [1, 2, 63, 64, 65, 1023, 1024]
    assert plan["seg_row"][:ns].tolist() == [0, 1, 2, 3, 4, 6, 7]
    assert plan["seg_len"][ns:].tolist() == [1024, 1, 1024, 1024, 1]
    assert plan["seg_row"][ns:].tolist() == [8, 8, 9, 9, 9]
    assert plan["seg_slot"].tolist() == [-1] * 7 + [0, 1, 2, 3, 4]
    assert plan["mrow"].tolist() == [8, 9]
    assert plan["mslot"].tolist() == [0, 2, 5]


@functools.lru_cache(maxsize=None)
def make_mats(name, rank, bounded, seed=123):
    """Factors in the domain of the loss: positive for the bounded losses
    (model values > 0), signed and scaled for the free ones (model values of
    a few units at most, so that exp stays finite)."""
    t = COORDS[name]()
    out = []
    for m, d in enumerate(t.dims):
        A = sp.seeded_init(d, rank, m, seed)
        out.append(A.abs() + 0.05 if bounded
                   else (A - A.mean()) * (1.5 / math.sqrt(rank)))
    return tuple(out)


_CSF = {}


def csf_of(name, domain, device="cpu"):
    key = (name, domain, device)
    if key not in _CSF:
        _CSF[key] = sp.csf_alloc(make_input(name, domain).to(device), "all")
    return _CSF[key]


# ----------------------------------------------------------------- oracles

def o_loss(loss, x, m, param=None):
    """l(x, m) of the issue's table, written out plainly (torch, f64)."""
    if loss == "gaussian":
        return (m - x) ** 2
    if loss == "huber":
        r = (x - m).abs()
        return torch.where(r <= param, r ** 2, 2 * param * r - param ** 2)
    if loss == "poisson":
        return m - x * torch.log(m + EPS)
    if loss == "poisson-log":
        return torch.exp(m) - x * m
    if loss == "bernoulli-odds":
        return torch.log(m + 1) - x * torch.log(m + EPS)
    if loss == "bernoulli-logit":
        # log(1 + exp(m)) without overflow at the fitted models' large m
        return torch.logaddexp(torch.zeros_like(m), m) - x * m
    if loss == "gamma":
        return x / (m + EPS) + torch.log(m + EPS)
    if loss == "rayleigh":
        return 2 * torch.log(m + EPS) + (math.pi / 4) * (x / (m + EPS)) ** 2
    raise KeyError(loss)


def o_dloss(loss, x, m, param=None):
    """dl/dm of the issue's table."""
    if loss == "gaussian":
        return 2 * (m - x)
    if loss == "huber":
        r = x - m
        return torch.where(r.abs() <= param, -2 * r,
                           -2 * param * torch.sign(r))
    if loss == "poisson":
        return 1 - x / (m + EPS)
    if loss == "poisson-log":
        return torch.exp(m) - x
    if loss == "bernoulli-odds":
        return 1 / (m + 1) - x / (m + EPS)
    if loss == "bernoulli-logit":
        return torch.sigmoid(m) - x
    if loss == "gamma":
        return -x / (m + EPS) ** 2 + 1 / (m + EPS)
    if loss == "rayleigh":
        return 2 / (m + EPS) - (math.pi / 2) * x ** 2 / (m + EPS) ** 3
    raise KeyError(loss)


def _pi(t, mats, mode):
    H = torch.ones(t.nnz, mats[0].shape[1], dtype=torch.float64)
    for m in range(t.nmodes):
        if m != mode:
            H = H * mats[m][t.inds[m]]
    return H


def oracle_grad(t, mats, mode, loss, param=None):
    """Row by row on the COO indices: m = H_i a_i, G[i] = H_i^T dl(x, m),
    frow[i] = sum l(x, m). Rows without entries stay zero."""
    H = _pi(t, mats, mode)
    A = mats[mode]
    G = torch.zeros_like(A)
    frow = torch.zeros(t.dims[mode], dtype=torch.float64)
    order = torch.argsort(t.inds[mode], stable=True)
    cnt = row_counts(t, mode).tolist()
    p = 0
    for i, n in enumerate(cnt):
        if n == 0:
            continue
        sel = order[p:p + n]
        p += n
        Hi, x = H[sel], t.vals[sel].double()
        m = Hi @ A[i]
        G[i] = Hi.T @ o_dloss(loss, x, m, param)
        frow[i] = o_loss(loss, x, m, param).sum()
    return G, frow


def second_grad(t, mats, mode, loss, param=None):
    """The independent second evaluation: numpy, the entries of a row in
    reversed order, the model value accumulated one column at a time and
    G / frow one entry at a time (a sequential cumsum)."""
    H = _pi(t, mats, mode).numpy()
    vals = t.vals.double().numpy()
    key = t.inds[mode].numpy()
    A = mats[mode].numpy()
    G = np.zeros_like(A)
    frow = np.zeros(t.dims[mode])
    for i in range(t.dims[mode]):
        sel = np.nonzero(key == i)[0][::-1]
        if sel.size == 0:
            continue
        Hi, x = H[sel], vals[sel]
        m = np.zeros(sel.size)
        for f in range(A.shape[1]):
            m = m + Hi[:, f] * A[i, f]
        mt, xt = torch.from_numpy(m), torch.from_numpy(x.copy())
        y = o_dloss(loss, xt, mt, param).numpy()
        l = o_loss(loss, xt, mt, param).numpy()
        G[i] = np.cumsum(y[:, None] * Hi, axis=0)[-1]
        frow[i] = np.cumsum(l)[-1]
    return torch.from_numpy(G), torch.from_numpy(frow)


@functools.lru_cache(maxsize=None)
def oracle_case(name, rank, mode, loss):
    """Computed once per case, shared, never modified."""
    t = make_input(name, DOMAIN[loss])
    mats = list(make_mats(name, rank, loss in BOUNDED))
    return oracle_grad(t, mats, mode, loss, param_of(loss))


def max_rel(got, ref):
    """max|got - ref| / max(1, max|ref|)."""
    return ((got.cpu().double() - ref).abs().max().item()
            / max(1.0, ref.abs().max().item()))


def assert_close(got, ref, what):
    worst = 0.0
    for nm, g, r in (("G", got[0], ref[0]), ("frow", got[1], ref[1])):
        assert g.dtype == torch.float64 and g.shape == r.shape, (what, nm)
        err = max_rel(g, r)
        worst = max(worst, err)
        print(f"{what} {nm}: max|delta|/max(1,|ref|) = {err:.3e} "
              f"(bound {TOL:.1e})")
        assert err <= TOL, (what, nm, err)
    return worst


def test_oracle_matches_autograd():
    """The derivative column of the table against autograd of the loss
    column, through the whole model."""
    for loss in LOSSES:
        t = make_input("4-mode", DOMAIN[loss])
        mats = [m.clone().requires_grad_(True)
                for m in make_mats("4-mode", 7, loss in BOUNDED)]
        H = torch.ones(t.nnz, 7, dtype=torch.float64)
        for m in range(t.nmodes):
            H = H * mats[m][t.inds[m]]
        f = o_loss(loss, t.vals, H.sum(1), param_of(loss)).sum()
        f.backward()
        f = float(f.detach())
        plain = [m.detach() for m in mats]
        for mode in range(t.nmodes):
            G, frow = oracle_grad(t, plain, mode, loss, param_of(loss))
            err = max_rel(G, mats[mode].grad)
            print(f"{loss} mode {mode}: oracle vs autograd {err:.3e}")
            assert err <= 1e-13, (loss, mode, err)
            assert abs(float(frow.sum()) - f) <= 1e-13 * abs(f)


def test_two_evaluations_agree_within_tol():
    """The figure TOL is derived from, on the smallest rank of its cases;
    the module's __main__ block prints it for all of them. Asserted with two
    of the three orders of margin: the last bits of a CPU sum depend on the
    host's BLAS and thread count."""
    worst = 0.0
    for loss in LOSSES:
        t = make_input("heavy", DOMAIN[loss])
        mats = list(make_mats("heavy", 7, loss in BOUNDED))
        ref = oracle_case("heavy", 7, 0, loss)
        G, frow = second_grad(t, mats, 0, loss, param_of(loss))
        worst = max(worst, max_rel(G, ref[0]), max_rel(frow, ref[1]))
    print(f"two CPU evaluations differ by {worst:.3e}")
    assert 1e2 * worst <= TOL


# ---------------------------------------------------------- the exact case

EXACT_SHAPES = [([9, 11, 13], 3000), ([3, 11, 13], 5000)]


def check_exact(impl, device, rank):
    """gaussian on dyadic inputs (test_apr.exact_case): every model value is
    a power of two or 0 and every partial sum a short dyadic, so G and frow
    are exact in any summation order."""
    for dims, nnz in EXACT_SHAPES:
        t, mats, Bs = exact_case(dims, nnz, rank, False)
        if dims[0] == 3:
            assert int(row_counts(t, 0).min()) > completion.SEG
        cs = sp.csf_alloc(t.to(device), "all")
        for mode in range(3):
            ms = list(mats)
            ms[mode] = Bs[mode]
            G0, f0 = oracle_grad(t, ms, mode, "gaussian")
            assert float(G0.abs().max()) > 0 and float(f0.max()) > 0
            G, frow = sp.gcp_grad(cs, [m.to(device) for m in ms], mode,
                                  "gaussian", want_loss=True, impl=impl)
            what = (impl, dims, rank, mode)
            assert torch.equal(G.cpu(), G0), what
            assert torch.equal(frow.cpu(), f0), what
            G2, none = sp.gcp_grad(cs, [m.to(device) for m in ms], mode,
                                   "gaussian", impl=impl)
            assert none is None and torch.equal(G2.cpu(), G0), what


@pytest.mark.parametrize("rank", RANKS)
def test_exact_torch(rank):
    check_exact("torch", "cpu", rank)


# -------------------------------------------------------------- edge rows

EDGE_RANKS = [1, 3, 16, 64]
EDGE_LOSSES = ["gaussian", "bernoulli-logit"]


def check_edges(impl, device, rank, loss):
    """dl(0, m) != 0 and l(0, m) != 0 for both losses: a tail step that
    leaks, or a loss counted once per lane, is a wrong number here."""
    cs = csf_of("edges", DOMAIN[loss], device)
    check_edges_plan(cs)
    t = make_input("edges", DOMAIN[loss])
    mats = [m.to(device) for m in make_mats("edges", rank, False)]
    for mode in range(3):
        ref = oracle_case("edges", rank, mode, loss)
        got = sp.gcp_grad(cs, mats, mode, loss, want_loss=True, impl=impl)
        assert_close(got, ref, f"{impl} edges {loss} rank {rank} mode {mode}")
        only_g = sp.gcp_grad(cs, mats, mode, loss, impl=impl)
        assert only_g[1] is None
        assert max_rel(only_g[0], ref[0]) <= TOL
        empty = row_counts(t, mode) == 0
        assert bool((got[0].cpu()[empty] == 0).all())
        assert bool((got[1].cpu()[empty] == 0).all())
    assert int((row_counts(t, 0) == 0).sum()) == 1


@pytest.mark.parametrize("loss", EDGE_LOSSES)
@pytest.mark.parametrize("rank", EDGE_RANKS)
def test_edges_torch(rank, loss):
    check_edges("torch", "cpu", rank, loss)


def test_edges_plan():
    check_edges_plan(csf_of("edges", "any"))


# -------------------------------------------------------------- all losses

ALL_INPUTS = ["heavy", "thin", "4-mode"]


def check_losses(impl, device, name, rank, loss):
    check_preconditions(name)
    cs = csf_of(name, DOMAIN[loss], device)
    t = make_input(name, DOMAIN[loss])
    mats = [m.to(device) for m in make_mats(name, rank, loss in BOUNDED)]
    worst = 0.0
    for mode in range(t.nmodes):
        ref = oracle_case(name, rank, mode, loss)
        assert bool(torch.isfinite(ref[0]).all())
        assert bool(torch.isfinite(ref[1]).all())
        got = sp.gcp_grad(cs, mats, mode, loss, param=param_of(loss),
                          want_loss=True, impl=impl)
        worst = max(worst, assert_close(
            got, ref, f"{impl} {name} {loss} rank {rank} mode {mode}"))
    print(f"{impl} {name} {loss} rank {rank}: worst relative error "
          f"{worst:.3e}")
    return worst


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", ALL_INPUTS)
def test_losses_torch(name, rank, loss):
    check_losses("torch", "cpu", name, rank, loss)


def check_fg(impl, device, loss):
    """f comes from mode 0's pass; frow.sum() of any other pass agrees."""
    name, rank = "heavy", 16
    cs = csf_of(name, DOMAIN[loss], device)
    mats = [m.to(device) for m in make_mats(name, rank, loss in BOUNDED)]
    f, grads = sp.gcp_fg(cs, mats, loss, param=param_of(loss), impl=impl)
    f0 = float(oracle_case(name, rank, 0, loss)[1].sum())
    scale = max(1.0, abs(f0))
    assert f.dim() == 0 and abs(float(f) - f0) <= TOL * scale, (float(f), f0)
    for mode in range(3):
        ref = oracle_case(name, rank, mode, loss)
        assert max_rel(grads[mode], ref[0]) <= TOL
        _, frow = sp.gcp_grad(cs, mats, mode, loss, param=param_of(loss),
                              want_loss=True, impl=impl)
        assert abs(float(frow.sum()) - f0) <= TOL * scale, (mode, loss)


@pytest.mark.parametrize("loss", LOSSES)
def test_fg_torch(loss):
    check_fg("torch", "cpu", loss)


def check_stored_zeros(impl, device):
    """A stored 0 is an observation of zero: it counts; dropping it changes
    the answer."""
    t = make_input("4-mode", "count")
    g = torch.Generator().manual_seed(3)
    v = torch.where(torch.rand(t.nnz, generator=g) < 0.5,
                    torch.zeros(t.nnz, dtype=torch.float64), t.vals + 1.0)
    tz = sp.SpTensor(t.inds.clone(), v, list(t.dims))
    assert 0.4 < float((v == 0).double().mean()) < 0.6
    keep = v != 0
    tc = sp.SpTensor(t.inds[:, keep].clone(), v[keep].clone(), list(t.dims))
    # l(0, m) = exp(m) and m: neither is small next to the other entries
    for loss in ("poisson-log", "poisson"):
        mats = list(make_mats("4-mode", 7, loss in BOUNDED))
        dm = [m.to(device) for m in mats]
        csz = sp.csf_alloc(tz.to(device), "all")
        csc = sp.csf_alloc(tc.to(device), "all")
        for mode in range(4):
            assert int(completion._stream(completion._resolve(csz, mode))
                       ["vals"].numel()) == t.nnz
            ref = oracle_grad(tz, mats, mode, loss)
            got = sp.gcp_grad(csz, dm, mode, loss, want_loss=True, impl=impl)
            assert_close(got, ref, f"{impl} stored zeros {loss} mode {mode}")
            refc = oracle_grad(tc, mats, mode, loss)
            gotc = sp.gcp_grad(csc, dm, mode, loss, want_loss=True, impl=impl)
            assert_close(gotc, refc, f"{impl} compressed {loss} mode {mode}")
            assert max_rel(gotc[0], ref[0]) > 1e-3
            assert max_rel(gotc[1], ref[1]) > 1e-3


def test_stored_zeros_torch():
    check_stored_zeros("torch", "cpu")


def test_grad_on_a_single_csf():
    cs = csf_of("4-mode", "any")
    mats = list(make_mats("4-mode", 7, False))
    got = sp.gcp_grad(cs.csfs[1], mats, 1, "gaussian", want_loss=True)
    assert_close(got, oracle_case("4-mode", 7, 1, "gaussian"), "single csf")


# ------------------------------------------------------------------ errors

DOMAIN_BAD = {
    "poisson": -1.0, "poisson-log": -1.0, "rayleigh": -1.0,
    "bernoulli-odds": 2.0, "bernoulli-logit": 0.5, "gamma": 0.0,
}


def check_domain_rejections(device):
    t = make_input("4-mode", "binary")
    mats = [m.to(device) for m in make_mats("4-mode", 7, True)]
    for loss, bad in DOMAIN_BAD.items():
        v = t.vals.clone() + (1.0 if loss == "gamma" else 0.0)
        v[5] = bad
        cs = sp.csf_alloc(sp.SpTensor(t.inds.clone(), v,
                                      list(t.dims)).to(device), "all")
        with pytest.raises(ValueError, match="needs tensor values"):
            sp.gcp_grad(cs, mats, 0, loss)
        with pytest.raises(ValueError, match="needs tensor values"):
            sp.cpd_gcp(cs, 4, loss)
        # gaussian and huber take anything
        sp.gcp_grad(cs, mats, 0, "gaussian")
        sp.gcp_grad(cs, mats, 0, "huber", param=1.0)


def test_domain_rejections_cpu():
    check_domain_rejections("cpu")


def test_grad_errors():
    t = make_input("4-mode", "any")
    cs = csf_of("4-mode", "any")
    mats = list(make_mats("4-mode", 16, False))
    for rank in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            sp.gcp_grad(
                cs, [torch.ones(d, rank, dtype=torch.float64) for d in t.dims],
                0, "gaussian")
        with pytest.raises(ValueError, match="rank"):
            sp.cpd_gcp(t, rank)
    with pytest.raises(ValueError, match="factor 2 has shape"):
        sp.gcp_grad(cs, mats[:2] + [mats[2][:-1]] + mats[3:], 0, "gaussian")
    with pytest.raises(ValueError, match="factor 0 has shape"):
        sp.gcp_grad(cs, [mats[0][:-1]] + mats[1:], 0, "gaussian")
    with pytest.raises(ValueError, match="factor 1: dtype"):
        sp.gcp_grad(cs, [mats[0], mats[1].float()] + mats[2:], 0, "gaussian")
    with pytest.raises(ValueError, match="factor matrices"):
        sp.gcp_grad(cs, mats[:3], 0, "gaussian")
    with pytest.raises(ValueError, match="hip"):
        sp.gcp_grad(cs, mats, 0, "gaussian", impl="hip")     # CPU tensor
    with pytest.raises(ValueError, match="unknown impl"):
        sp.gcp_grad(cs, mats, 0, "gaussian", impl="triton")
    with pytest.raises(ValueError, match="unknown loss"):
        sp.gcp_grad(cs, mats, 0, "cauchy")
    with pytest.raises(ValueError, match="unknown loss"):
        sp.cpd_gcp(t, 4, "cauchy")
    for bad in (None, 0.0, -1.0):
        with pytest.raises(ValueError, match="huber needs param"):
            sp.gcp_grad(cs, mats, 0, "huber", param=bad)
    with pytest.raises(ValueError, match="huber needs param"):
        sp.cpd_gcp(t, 4, "huber")
    with pytest.raises(IndexError):
        sp.gcp_grad(cs, mats, 4, "gaussian")

    t32 = sp.SpTensor.synthetic([20, 15, 25], 500, dtype=torch.float32,
                                seed=3)
    m32 = [torch.ones(d, 16, dtype=torch.float32) for d in t32.dims]
    with pytest.raises(ValueError, match="float64"):
        sp.gcp_grad(sp.csf_alloc(t32, "all"), m32, 0, "gaussian")
    with pytest.raises(ValueError, match="float64"):
        sp.cpd_gcp(t32, 4)

    two = sp.csf_alloc(t, "two")
    nonroot = [m for m in range(t.nmodes) if two.mode_depth[m] != 0]
    assert nonroot
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.gcp_grad(two, mats, nonroot[0], "gaussian")
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.cpd_gcp(two, 4)


# ---------------------------------------------------------- binding checks

_GCP_BINDING = "hip_gcp_grad"


def _binding_args():
    F, NNZ, ROWS = 8, 12, 5
    I32, I64, F64 = torch.int32, torch.int64, torch.float64
    return [
        [torch.zeros(NNZ, dtype=I32) for _ in range(2)],         # idx
        [torch.ones(4, F, dtype=F64) for _ in range(2)],         # mats
        torch.ones(NNZ, dtype=F64),                              # vals
        torch.tensor([0], dtype=I64), torch.tensor([NNZ], dtype=I32),
        torch.tensor([0], dtype=I32), torch.tensor([-1], dtype=I32),
        1, torch.zeros(0, dtype=I32), torch.zeros(1, dtype=I64),
        0, 0.0,                                                  # loss, param
        torch.ones(ROWS, F, dtype=F64),                          # A
        torch.zeros(1, dtype=F64),                               # ws
        torch.zeros(ROWS, F, dtype=F64),                         # G
        torch.zeros(ROWS, dtype=F64)]                            # frow


def test_binding_is_not_a_gpu_name():
    """tests/test_binding_checks.py owns the table of gpu_* bindings."""
    assert hasattr(native(), _GCP_BINDING)
    assert not _GCP_BINDING.startswith("gpu_")


@pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="host tensors must never reach a device; needs a GPU-less box")
def test_binding_rejects_host_tensors_and_wrong_dtype():
    fn = getattr(native(), _GCP_BINDING)
    with pytest.raises(RuntimeError, match="vals must be a device tensor"):
        fn(*_binding_args(), 0)
    args = _binding_args()
    args[2] = args[2].to(torch.int16)
    with pytest.raises(RuntimeError, match="vals has dtype Short"):
        fn(*args, 0)
    args = _binding_args()
    args[10] = 8
    with pytest.raises(RuntimeError, match="loss id"):
        fn(*args, 0)
    args = _binding_args()
    args[10] = 1                                   # huber, param 0
    with pytest.raises(RuntimeError, match="huber needs param"):
        fn(*args, 0)


# ------------------------------------------------------------------ driver

PLANTED_DIMS = [30, 25, 20]
PLANTED_LOSSES = ["gaussian", "bernoulli-logit", "poisson"]
# seed and iteration cap chosen on the CPU torch path so that the final
# loss is below the loss of the planted parameters (the module's __main__
# block prints the runs they were chosen from)
PLANTED_OPTS = {
    "gaussian": dict(seed=1, max_iters=100, tolerance=0.0),
    "bernoulli-logit": dict(seed=1, max_iters=100, tolerance=0.0),
    "poisson": dict(seed=1, max_iters=100, tolerance=0.0),
}


@functools.lru_cache(maxsize=None)
def planted(loss):
    """30x25x20, rank 4, half the cells stored (zeros included). Returns
    (tensor, planted factors)."""
    g = torch.Generator().manual_seed(2026)
    A = []
    for d in PLANTED_DIMS:
        if loss == "poisson":
            A.append(2.0 * torch.rand(d, 4, generator=g,
                                      dtype=torch.float64) ** 2)
        else:
            A.append(torch.randn(d, 4, generator=g, dtype=torch.float64)
                     * 0.9)
    m = torch.einsum("if,jf,kf->ijk", *A)
    if loss == "gaussian":
        x = m + 0.1 * torch.randn(m.shape, generator=g, dtype=torch.float64)
    elif loss == "poisson":
        x = torch.poisson(m, generator=g)
    else:
        x = (torch.rand(m.shape, generator=g, dtype=torch.float64)
             < torch.sigmoid(m)).double()
    n = m.numel()
    cells = torch.randperm(n, generator=g)[:n // 2]
    inds = torch.stack([cells // (25 * 20), (cells // 20) % 25, cells % 20],
                       0)
    return sp.SpTensor(inds, x.reshape(-1)[cells].clone(),
                       list(PLANTED_DIMS)), A


def loss_at(t, factors, loss, lam=None, param=None):
    H = torch.ones(t.nnz, factors[0].shape[1], dtype=torch.float64)
    if lam is not None:
        H = H * lam.cpu()
    for m in range(t.nmodes):
        H = H * factors[m].cpu()[t.inds[m]]
    return float(o_loss(loss, t.vals, H.sum(1), param).sum())


def check_driver_result(r, t, loss, param=None):
    """What holds for every run: a non-increasing trace, the bounds, and
    lam x factors reproducing the final loss."""
    tr = r.loss_trace
    assert r.niters == len(tr) == len(r.pg_trace) and r.nfev > r.niters
    for a, b in zip(tr, tr[1:]):
        assert b <= a, (loss, a, b)
    for A in r.factors:
        assert bool(torch.isfinite(A).all())
        if loss in BOUNDED:
            assert bool((A >= 0).all()), loss
        nrm = A.norm(dim=0).cpu()
        assert bool(((nrm - 1).abs() < 1e-12).logical_or(nrm == 0).all())
    if loss in BOUNDED:
        assert bool((r.lam >= 0).all())
    f = loss_at(t, r.factors, loss, lam=r.lam, param=param)
    assert abs(f - tr[-1]) <= 1e-9 * max(1.0, abs(tr[-1])), (loss, f, tr[-1])
    pred = sp.kruskal_predict(r.factors, t.inds.to(r.lam.device), r.lam)
    assert abs(float(o_loss(loss, t.vals, pred.cpu(), param).sum())
               - tr[-1]) <= 1e-9 * max(1.0, abs(tr[-1]))


def check_planted(device, loss):
    t, truth = planted(loss)
    r = sp.cpd_gcp(t.to(device), 4, loss,
                   sp.GcpOptions(**PLANTED_OPTS[loss]))
    assert all(A.device.type == device for A in r.factors)
    check_driver_result(r, t, loss)
    at_truth = loss_at(t, truth, loss)
    print(f"{loss}: final {r.loss_trace[-1]:.8e} after {r.niters} "
          f"iterations / {r.nfev} evaluations vs planted parameters "
          f"{at_truth:.8e}")
    assert r.loss_trace[-1] < at_truth
    return r


@pytest.mark.parametrize("loss", PLANTED_LOSSES)
def test_cpd_gcp_planted(loss):
    check_planted("cpu", loss)


SHORT = dict(max_iters=12, tolerance=0.0, seed=5)


def check_every_loss_driver(device, loss):
    t = make_input("4-mode", DOMAIN[loss])
    r = sp.cpd_gcp(t.to(device), 5, loss,
                   sp.GcpOptions(param=param_of(loss), **SHORT))
    assert r.niters >= 3
    check_driver_result(r, t, loss, param_of(loss))
    return r


@pytest.mark.parametrize("loss", LOSSES)
def test_every_loss_driver_torch(loss):
    check_every_loss_driver("cpu", loss)


FIXED_DRV = dict(max_iters=8, tolerance=0.0, seed=77)
FIXED_LOSSES = ["gaussian", "bernoulli-logit", "poisson"]


def oracle_driver(t, rank, loss, opts):
    """cpd_gcp's optimiser with the row-by-row oracle as loss and gradient."""
    lower = 0.0 if loss in BOUNDED else None
    sizes = [d * rank for d in t.dims]
    parts = []
    for m, d in enumerate(t.dims):
        A = sp.seeded_init(d, rank, m, opts.seed)
        parts.append((A.abs() if loss in BOUNDED else A * 0.3).reshape(-1))
    x = torch.cat(parts)

    def fg(v):
        mats, o = [], 0
        for m, d in enumerate(t.dims):
            mats.append(v[o:o + sizes[m]].view(d, rank))
            o += sizes[m]
        gs, f = [], None
        for m in range(t.nmodes):
            G, frow = oracle_grad(t, mats, m, loss, opts.param)
            gs.append(G.reshape(-1))
            if m == 0:
                f = float(frow.sum())
        return f, torch.cat(gs)

    return gcp.gcp_minimize(fg, x, lower, opts)


@functools.lru_cache(maxsize=None)
def fixed_schedule_cpu(loss):
    return sp.cpd_gcp(make_input("4-mode", DOMAIN[loss]), 8, loss,
                      sp.GcpOptions(**FIXED_DRV))


def trace_err(a, b):
    return max(abs(x - y) / abs(y) for x, y in zip(a, b))


@pytest.mark.parametrize("loss", FIXED_LOSSES)
def test_fixed_schedule_matches_oracle_driver(loss):
    r = fixed_schedule_cpu(loss)
    assert r.niters == FIXED_DRV["max_iters"] and not r.converged
    trace, _, nfev, niters, _ = oracle_driver(
        make_input("4-mode", DOMAIN[loss]), 8, loss,
        sp.GcpOptions(**FIXED_DRV))
    assert (niters, nfev) == (r.niters, r.nfev)
    err = trace_err(r.loss_trace, trace)
    print(f"{loss} driver trace, torch vs oracle: {err:.3e} "
          f"(DRV_TOL {DRV_TOL:.1e})")
    assert 1e2 * err <= DRV_TOL


def test_converged_flag_and_prefix():
    t, _ = planted("gaussian")
    tol = 1e-3
    r = sp.cpd_gcp(t, 4, "gaussian",
                   sp.GcpOptions(max_iters=200, tolerance=tol, seed=1))
    assert r.converged and r.niters < 200
    tr = r.loss_trace
    assert (tr[-2] - tr[-1]) <= tol * abs(tr[-2])
    assert all((a - b) > tol * abs(a) for a, b in zip(tr[:-2], tr[1:-1]))
    # a budget too short to get there
    r2 = sp.cpd_gcp(t, 4, "gaussian",
                    sp.GcpOptions(max_iters=3, tolerance=tol, seed=1))
    assert not r2.converged and r2.niters == 3
    assert r2.loss_trace == tr[:3] and r2.pg_trace == r.pg_trace[:3]


# ------------------------------------------------------------ sample_zeros

def check_sample_zeros(device):
    t = make_input("thin", "binary")
    ones = sp.SpTensor(t.inds.clone(), torch.ones_like(t.vals),
                       list(t.dims)).fixed().to(device)
    n = 2 * ones.nnz
    z = sp.sample_zeros(ones, n, seed=11)
    assert z.nnz == ones.nnz + n and z.device.type == device
    assert torch.equal(z.inds[:, :ones.nnz], ones.inds)
    assert torch.equal(z.vals[:ones.nnz], ones.vals)
    assert bool((z.vals[ones.nnz:] == 0).all())
    for m, d in enumerate(z.dims):
        assert 0 <= int(z.inds[m].min()) and int(z.inds[m].max()) < d
    lin = torch.zeros(z.nnz, dtype=torch.int64, device=device)
    for m, d in enumerate(z.dims):
        lin = lin * d + z.inds[m]
    assert int(torch.unique(lin).numel()) == z.nnz      # no collisions
    z2 = sp.sample_zeros(ones, n, seed=11)
    assert torch.equal(z2.inds, z.inds) and torch.equal(z2.vals, z.vals)
    z3 = sp.sample_zeros(ones, n, seed=12)
    assert not torch.equal(z3.inds, z.inds)
    # the enumerating path: a tensor small enough to fill completely
    small = sp.SpTensor(torch.tensor([[0, 1], [0, 2], [1, 0]]).to(device),
                        torch.ones(2, dtype=torch.float64, device=device),
                        [2, 3, 2])
    full = sp.sample_zeros(small, 10, seed=0)
    assert full.nnz == 12
    assert int(torch.unique((full.inds[0] * 3 + full.inds[1]) * 2
                            + full.inds[2]).numel()) == 12
    with pytest.raises(ValueError, match="empty cells"):
        sp.sample_zeros(small, 11, seed=0)
    assert sp.sample_zeros(small, 0, seed=0).nnz == 2


def test_sample_zeros_cpu():
    check_sample_zeros("cpu")


def test_sample_zeros_rejection_path(monkeypatch):
    """Tensors with more cells than the enumeration limit draw and reject."""
    monkeypatch.setattr(gcp, "_ENUMERATE_MAX", 1000)
    t = make_input("thin", "binary").fixed()
    z = sp.sample_zeros(t, 5000, seed=4)
    lin = (z.inds[0] * 250 + z.inds[1]) * 400 + z.inds[2]
    assert z.nnz == t.nnz + 5000
    assert int(torch.unique(lin).numel()) == z.nnz
    z2 = sp.sample_zeros(t, 5000, seed=4)
    assert torch.equal(z2.inds, z.inds)


# ----------------------------------------------------------- CLI, example

def test_cli_gcp(tmp_path, capsys):
    from splatt_amd import cli
    t, _ = planted("bernoulli-logit")
    pos = t.vals == 1
    tp = sp.SpTensor(t.inds[:, pos].clone(), t.vals[pos].clone(),
                     list(t.dims))
    path = str(tmp_path / "pos.tns")
    tp.save(path)
    stem = str(tmp_path / "out" / "g_")
    rc = cli.main(["gcp", path, "-r", "4", "--loss", "bernoulli-logit",
                   "-i", "4", "--tol", "0", "--zeros", "500", "--seed", "77",
                   "--device", "cpu", "--stem", stem])
    assert rc == 0
    out = capsys.readouterr().out
    assert "its = 4 loss = " in out and "Final loss:" in out
    loaded = sp.SpTensor.load(path)
    tz = sp.sample_zeros(loaded, 500, 77)
    r = sp.cpd_gcp(tz, 4, "bernoulli-logit",
                   sp.GcpOptions(max_iters=4, tolerance=0.0, seed=77))
    assert f"its = 4 loss = {r.loss_trace[3]:.8e}" in out
    for m in range(3):
        rows = open(f"{stem}mode{m + 1}.mat").read().strip().splitlines()
        assert len(rows) == loaded.dims[m] and len(rows[0].split()) == 4
        got = torch.tensor([[float(x) for x in row.split()] for row in rows],
                           dtype=torch.float64)
        assert torch.equal(got, r.factors[m])
    lam = [float(x) for x in open(f"{stem}lambda.mat").read().split()]
    assert lam == r.lam.tolist()
    # huber through --param, no files
    rc = cli.main(["gcp", path, "-r", "2", "--loss", "huber", "--param",
                   "0.5", "-i", "2", "--device", "cpu", "--nowrite"])
    assert rc == 0
    assert not os.path.exists(str(tmp_path / "mode1.mat"))


def test_example_runs(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runpy.run_path(os.path.join(root, "examples", "gcp_binary.py"),
                   run_name="__main__")
    out = capsys.readouterr().out
    assert "final loss" in out


# ------------------------------------------------ re-measuring the bounds

if __name__ == "__main__":
    worst = 0.0
    for loss in LOSSES:
        t = make_input("heavy", DOMAIN[loss])
        lw = 0.0
        for rank in (7, 16, 32, 64):
            mats = list(make_mats("heavy", rank, loss in BOUNDED))
            for mode in range(3):
                ref = oracle_case("heavy", rank, mode, loss)
                G, frow = second_grad(t, mats, mode, loss, param_of(loss))
                lw = max(lw, max_rel(G, ref[0]), max_rel(frow, ref[1]))
        print(f"heavy {loss}: {lw:.3e}")
        worst = max(worst, lw)
    print(f"two CPU evaluations, worst: {worst:.3e}  (TOL {TOL:.1e})")
    worst = 0.0
    for loss in FIXED_LOSSES:
        r = fixed_schedule_cpu(loss)
        trace = oracle_driver(make_input("4-mode", DOMAIN[loss]), 8, loss,
                              sp.GcpOptions(**FIXED_DRV))[0]
        err = trace_err(r.loss_trace, trace)
        print(f"{loss} driver trace torch vs oracle: {err:.3e}")
        worst = max(worst, err)
    print(f"driver trace, worst: {worst:.3e}  (DRV_TOL {DRV_TOL:.1e})")
    for loss in PLANTED_LOSSES:
        t, truth = planted(loss)
        at_truth = loss_at(t, truth, loss)
        for seed in (1, 2, 3):
            r = sp.cpd_gcp(t, 4, loss, sp.GcpOptions(
                seed=seed, max_iters=300, tolerance=0.0))
            first = next((i + 1 for i, f in enumerate(r.loss_trace)
                          if f < at_truth), None)
            print(f"planted {loss} seed {seed}: {r.niters} iterations, "
                  f"final {r.loss_trace[-1]:.6e}, planted {at_truth:.6e}, "
                  f"first below at iteration {first}")
