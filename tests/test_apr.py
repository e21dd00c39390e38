"""Poisson CPD (CP-APR): the torch path against a row-by-row CPU oracle, the
stopping rule, the driver on a planted Poisson case, errors, the CLI.

The oracles, inputs and bounds here are shared with tests/test_apr_gpu.py.

Bounds. Float comparisons use  max|delta| <= TOL * max(1, max|oracle|).
Two independent CPU f64 evaluations of the update (the oracle: `H @ b` and
`H.T @ w` per row; the second evaluation: nonzeros in reversed order, every
sum accumulated one term at a time) differ by at most 1.8e-14 relative to
max(1, max|oracle|) over B, Phi and viol0 on the `heavy` input, five
iterations, inner_tol = 0, ranks 7/16/32/64, all modes; TOL is that figure
with about three orders of margin. DRV_TOL bounds the relative difference
of the driver's log-likelihood trace on the fixed 5 x 5 schedule of the
`4-mode` input: the torch path and the oracle-driven driver differ by at
most 1.4e-16 there; DRV_TOL is that with three orders of margin.
`PYTHONPATH=. python tests/test_apr.py` re-measures both figures.
"""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import splatt_amd as sp
from splatt_amd import apr, completion
from splatt_amd._ext import native

TOL = 2e-11
DRV_TOL = 1.4e-13
EPS = 1e-10
RANKS = [1, 7, 16, 17, 32, 64]


# ------------------------------------------------------------------ inputs

def _counts(t):
    """The same coordinates with count values ceil(5 |v|) >= 1."""
    return sp.SpTensor(t.inds.clone(), torch.ceil(5 * t.vals.abs()),
                       list(t.dims))


@functools.lru_cache(maxsize=None)
def heavy():
    return _counts(sp.SpTensor.synthetic([200, 150, 180], 40_000, seed=17,
                                         dist="zipf"))


@functools.lru_cache(maxsize=None)
def thin():
    return _counts(sp.SpTensor.synthetic([300, 250, 400], 900, seed=17))


@functools.lru_cache(maxsize=None)
def four_mode():
    return _counts(sp.SpTensor.synthetic([20, 15, 25, 12], 8_000, seed=17))


INPUTS = {"heavy": heavy, "thin": thin, "4-mode": four_mode}


def row_counts(t, mode):
    return torch.bincount(t.inds[mode], minlength=t.dims[mode])


def check_preconditions(name):
    """The inputs must keep covering the branches they were chosen for."""
    t = INPUTS[name]()
    assert bool((t.vals >= 1).all()) and bool((t.vals == t.vals.round()).all())
    if name == "heavy":
        for m in range(t.nmodes):
            cnt = row_counts(t, m)
            assert int((cnt == 0).sum()) >= 1, m
            assert int((cnt > completion.SEG).sum()) == 7, m
            assert 6000 < int(cnt.max()) < 7000, (m, int(cnt.max()))
    elif name == "thin":
        for m in range(t.nmodes):
            cnt = row_counts(t, m)
            assert int((cnt == 0).sum()) >= 1, m
            assert int(cnt.max()) < 16, m


@functools.lru_cache(maxsize=None)
def make_mats(name, rank, seed=123):
    """Nonnegative factors, columns summing to 1 (what the driver holds)."""
    t = INPUTS[name]()
    out = []
    for m, d in enumerate(t.dims):
        A = sp.seeded_init(d, rank, m, seed).abs()
        out.append(A / A.sum(0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def make_b(name, rank, mode):
    """The start B = A diag(lambda) with lambda = sum(vals) / rank."""
    t = INPUTS[name]()
    return make_mats(name, rank)[mode] * (float(t.vals.sum()) / rank)


# ----------------------------------------------------------------- oracles

def _pi(t, mats, mode):
    H = torch.ones(t.nnz, mats[0].shape[1], dtype=torch.float64)
    for m in range(t.nmodes):
        if m != mode:
            H = H * mats[m][t.inds[m]]
    return H


def oracle_update(t, mats, mode, B0, inner_tol, max_inner, eps_div=EPS):
    """Row by row on the COO indices, as in the algorithm box of apr.py.
    Returns (B, Phi, iters, viol0, vs) with vs every violation evaluated."""
    rank = B0.shape[1]
    H = _pi(t, mats, mode)
    B = B0.clone()
    Phi = torch.zeros_like(B)
    iters = torch.zeros(t.dims[mode], dtype=torch.int32)
    viol0 = torch.zeros(t.dims[mode], dtype=torch.float64)
    vs = []
    for i in range(t.dims[mode]):
        mask = t.inds[mode] == i
        if not bool(mask.any()):
            B[i] = 0.0
            continue
        Hi, x = H[mask], t.vals[mask].double()
        b = B[i].clone()
        for l in range(1, max_inner + 1):
            mdl = torch.clamp_min(Hi @ b, eps_div)
            phi = Hi.T @ (x / mdl)
            v = float(torch.minimum(b, 1.0 - phi).abs().max())
            vs.append(v)
            iters[i] = l
            if l == 1:
                viol0[i] = v
            Phi[i] = phi
            if inner_tol > 0 and v < inner_tol:
                break
            b = b * phi
        B[i] = b
    assert rank == Phi.shape[1]
    return B, Phi, iters, viol0, torch.tensor(vs, dtype=torch.float64)


def second_update(t, mats, mode, B0, max_inner, eps_div=EPS):
    """The independent second evaluation (fixed iteration count): numpy, the
    nonzeros of a row in reversed order, the model value accumulated one
    column at a time and Phi one nonzero at a time (a sequential cumsum)."""
    H = _pi(t, mats, mode).numpy()
    vals = t.vals.double().numpy()
    key = t.inds[mode].numpy()
    B = B0.clone().numpy()
    Phi = np.zeros_like(B)
    viol0 = np.zeros(t.dims[mode])
    for i in range(t.dims[mode]):
        sel = np.nonzero(key == i)[0][::-1]
        if sel.size == 0:
            B[i] = 0.0
            continue
        Hi, x = H[sel], vals[sel]
        b = B[i].copy()
        for l in range(1, max_inner + 1):
            mdl = np.zeros(sel.size)
            for f in range(b.size):
                mdl = mdl + Hi[:, f] * b[f]
            w = x / np.maximum(mdl, eps_div)
            phi = np.cumsum(w[:, None] * Hi, axis=0)[-1]
            if l == 1:
                viol0[i] = np.abs(np.minimum(b, 1.0 - phi)).max()
            Phi[i] = phi
            b = b * phi
        B[i] = b
    return (torch.from_numpy(B), torch.from_numpy(Phi),
            torch.from_numpy(viol0))


FIXED_INNER = 5


@functools.lru_cache(maxsize=None)
def oracle_fixed(name, rank, mode):
    """inner_tol = 0, FIXED_INNER iterations. Computed once per case,
    shared, never modified."""
    return oracle_update(INPUTS[name](), list(make_mats(name, rank)), mode,
                         make_b(name, rank, mode), 0.0, FIXED_INNER)


@functools.lru_cache(maxsize=None)
def oracle_stop(name, rank, mode, inner_tol, max_inner):
    return oracle_update(INPUTS[name](), list(make_mats(name, rank)), mode,
                         make_b(name, rank, mode), inner_tol, max_inner)


def max_rel(got, ref):
    """max|got - ref| / max(1, max|ref|)."""
    return ((got.cpu().double() - ref).abs().max().item()
            / max(1.0, ref.abs().max().item()))


def assert_close(got, ref, what):
    """got = (B, Phi, iters, viol0) against an oracle tuple: floats within
    TOL, iteration counts equal. Returns the largest relative error."""
    B, Phi, iters, viol0 = got
    worst = 0.0
    for nm, g, r in (("B", B, ref[0]), ("Phi", Phi, ref[1]),
                     ("viol0", viol0, ref[3])):
        err = max_rel(g, r)
        worst = max(worst, err)
        print(f"{what} {nm}: max|delta|/max(1,|ref|) = {err:.3e} "
              f"(bound {TOL:.1e})")
        assert err <= TOL, (what, nm, err)
    assert iters.dtype == torch.int32
    assert torch.equal(iters.cpu(), ref[2]), what
    return worst


def run_update(cs, mats, mode, B0, impl, **kw):
    B = B0.clone()
    Phi, iters, viol0 = sp.apr_update(cs, mats, mode, B, impl=impl, **kw)
    return B, Phi, iters, viol0


# ---------------------------------------------------------- the exact case

def exact_case(dims, nnz, rank, zeros, seed=5):
    """Powers of two throughout, so that every model value is a power of two
    (or 0) and every partial sum a short dyadic: one iteration is exact in
    any summation order. Other factors hold one nonzero per row, 2^-3..2^0;
    B holds 2^0..2^3 (with `zeros`, a quarter of its entries 0, so that the
    model value 0 occurs next to nonzero pi and eps_div — a power of two
    here — is what divides); values 1..7. Coordinates repeat: fine for a
    stream."""
    g = torch.Generator().manual_seed(seed + rank)
    inds = torch.stack([torch.randint(0, d, (nnz,), generator=g)
                        for d in dims], 0)
    vals = torch.randint(1, 8, (nnz,), generator=g).double()
    t = sp.SpTensor(inds, vals, list(dims))
    mats, Bs = [], []
    for d in dims:
        # most rows use one of the first two columns, so that the products
        # of the other modes' rows are often nonzero at any rank
        col = torch.randint(0, rank, (d,), generator=g)
        low = torch.randint(0, min(rank, 2), (d,), generator=g)
        col = torch.where(torch.rand(d, generator=g) < 0.7, low, col)
        A = torch.zeros(d, rank, dtype=torch.float64)
        A[torch.arange(d), col] = 2.0 ** -torch.randint(
            0, 4, (d,), generator=g).double()
        mats.append(A)
        B = 2.0 ** torch.randint(0, 4, (d, rank), generator=g).double()
        if zeros:
            B = B * (torch.rand(d, rank, generator=g) >= 0.25)
            B[0, 0] = 0.0       # at rank 1 chance alone may leave none
        Bs.append(B)
    return t, mats, Bs


EXACT_SHAPES = [([9, 11, 13], 3000), ([3, 11, 13], 5000)]
EXACT_EPS = {False: EPS, True: 2.0 ** -30}


def check_exact(impl, device, rank, zeros):
    for dims, nnz in EXACT_SHAPES:
        t, mats, Bs = exact_case(dims, nnz, rank, zeros)
        if dims[0] == 3:
            assert int(row_counts(t, 0).min()) > completion.SEG
        eps = EXACT_EPS[zeros]
        cs = sp.csf_alloc(t.to(device), "all")
        dmats = [m.to(device) for m in mats]
        for mode in range(3):
            ref = oracle_update(t, mats, mode, Bs[mode], 0.0, 1, eps_div=eps)
            if zeros:
                mdl = (_pi(t, mats, mode) * Bs[mode][t.inds[mode]]).sum(1)
                hit = (mdl == 0) & (_pi(t, mats, mode).sum(1) > 0)
                assert int(hit.sum()) > 0, (dims, rank, mode)
            assert float(ref[1].max()) > 0
            B, Phi, iters, viol0 = run_update(
                cs, dmats, mode, Bs[mode].to(device), impl, inner_tol=0.0,
                max_inner=1, eps_div=eps)
            what = (impl, dims, rank, mode, zeros)
            assert torch.equal(B.cpu(), ref[0]), what
            assert torch.equal(Phi.cpu(), ref[1]), what
            assert torch.equal(viol0.cpu(), ref[3]), what
            assert torch.equal(iters.cpu(), ref[2]), what


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("rank", RANKS)
def test_exact_torch(rank, zeros):
    check_exact("torch", "cpu", rank, zeros)


# ------------------------------------------------------------- fixed count

@functools.lru_cache(maxsize=None)
def cpu_csf(name):
    return sp.csf_alloc(INPUTS[name](), "all")


def check_fixed(cs, device, name, rank, impl):
    check_preconditions(name)
    t = INPUTS[name]()
    mats = [m.to(device) for m in make_mats(name, rank)]
    worst = 0.0
    for mode in range(t.nmodes):
        got = run_update(cs, mats, mode, make_b(name, rank, mode).to(device),
                         impl, inner_tol=0.0, max_inner=FIXED_INNER)
        ref = oracle_fixed(name, rank, mode)
        worst = max(worst, assert_close(
            got, ref, f"{impl} {name} rank {rank} mode {mode}"))
        empty = row_counts(t, mode) == 0
        assert bool((got[2].cpu()[~empty] == FIXED_INNER).all())
        assert bool((got[2].cpu()[empty] == 0).all())
        assert bool((got[0].cpu()[empty] == 0).all())
        assert bool((got[1].cpu()[empty] == 0).all())
        assert bool((got[3].cpu()[empty] == 0).all())
    return worst


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_fixed_count_torch(name, rank):
    check_fixed(cpu_csf(name), "cpu", name, rank, "torch")


def test_two_evaluations_agree_within_tol():
    """The figure TOL is derived from, on the smallest rank of its cases;
    the module's __main__ block prints it for all of them."""
    t = heavy()
    ref = oracle_fixed("heavy", 7, 0)
    B, Phi, viol0 = second_update(t, list(make_mats("heavy", 7)), 0,
                                  make_b("heavy", 7, 0), FIXED_INNER)
    err = max(max_rel(B, ref[0]), max_rel(Phi, ref[1]),
              max_rel(viol0, ref[3]))
    print(f"two CPU evaluations differ by {err:.3e}")
    assert 1e3 * err <= TOL


# ----------------------------------------------------------- stopping rule

STOP_INNER = 50
THIN_STOP = [(rank, tol) for rank in (7, 16) for tol in (1e-1, 1e-2)]


def check_stop_preconditions(ref, inner_tol, rows=None):
    B, Phi, iters, viol0, vs = ref
    near = ((vs - inner_tol).abs() <= 1e-6 * inner_tol)
    assert not bool(near.any()), vs[near]
    return iters if rows is None else iters[rows]


def check_stop_thin(cs, device, rank, inner_tol, impl):
    t = thin()
    mats = [m.to(device) for m in make_mats("thin", rank)]
    for mode in range(t.nmodes):
        ref = oracle_stop("thin", rank, mode, inner_tol, STOP_INNER)
        it = check_stop_preconditions(ref, inner_tol)
        assert len(set(it.tolist()) - {0}) >= 3, set(it.tolist())
        got = run_update(cs, mats, mode, make_b("thin", rank, mode).to(device),
                         impl, inner_tol=inner_tol, max_inner=STOP_INNER)
        assert_close(got, ref, f"{impl} stop thin rank {rank} mode {mode} "
                               f"tol {inner_tol}")


@functools.lru_cache(maxsize=None)
def heavy_stop_case():
    """heavy mode 0, rank 16, inner_tol 0.1 from a warm start: B after 20
    fixed iterations, as a later outer iteration of the driver sees it. From
    the cold start of make_b the long rows all need about 50 iterations;
    from here they stop between 29 and 50. Returns (B0, oracle)."""
    mats = list(make_mats("heavy", 16))
    B0 = oracle_update(heavy(), mats, 0, make_b("heavy", 16, 0), 0.0, 20)[0]
    return B0, oracle_update(heavy(), mats, 0, B0, 0.1, STOP_INNER)


def check_stop_heavy(cs, device, impl):
    """The multi-segment rows of heavy mode 0 stop at different rounds."""
    t = heavy()
    rank, inner_tol = 16, 0.1
    B0, ref = heavy_stop_case()
    multi = row_counts(t, 0) > completion.SEG
    it = check_stop_preconditions(ref, inner_tol, multi)
    between = {x for x in it.tolist() if 1 < x < STOP_INNER}
    assert len(between) >= 2, it.tolist()
    print("multi-segment row counts:", sorted(it.tolist()))
    mats = [m.to(device) for m in make_mats("heavy", rank)]
    got = run_update(cs, mats, 0, B0.to(device), impl, inner_tol=inner_tol,
                     max_inner=STOP_INNER)
    assert_close(got, ref, f"{impl} stop heavy")


@pytest.mark.parametrize("rank,inner_tol", THIN_STOP)
def test_stopping_rule_torch_thin(rank, inner_tol):
    check_stop_thin(cpu_csf("thin"), "cpu", rank, inner_tol, "torch")


def test_stopping_rule_torch_heavy():
    check_stop_heavy(cpu_csf("heavy"), "cpu", "torch")


# ------------------------------------------------------------------ driver

PLANTED_LAM = (4000.0, 3000.0, 2000.0, 1000.0)
PLANTED_OPTS = dict(max_iters=60, seed=77)
# smallest column congruence the oracle-driven CPU run reaches on the
# planted case (0.9768), minus 0.05
CONGRUENCE_MIN = 0.9768 - 0.05


@functools.lru_cache(maxsize=None)
def planted():
    """A [30,25,20] rank-4 Poisson sample: factors rand^3 with columns
    summing to 1. Returns (tensor, planted factors, planted lambda)."""
    g = torch.Generator().manual_seed(2025)
    dims = [30, 25, 20]
    A = []
    for d in dims:
        M = torch.rand(d, 4, generator=g, dtype=torch.float64) ** 3
        A.append(M / M.sum(0))
    lam = torch.tensor(PLANTED_LAM, dtype=torch.float64)
    mean = torch.einsum("f,if,jf,kf->ijk", lam, *A)
    x = torch.poisson(mean, generator=g)
    inds = x.nonzero().T.contiguous()
    return sp.SpTensor(inds, x[tuple(inds)].clone(), dims), A, lam


def congruence(factors, truth):
    """Smallest over columns of the product over modes of the cosines, under
    the best column permutation."""
    rank = truth[0].shape[1]
    C = torch.ones(rank, rank, dtype=torch.float64)
    for A, T in zip(factors, truth):
        A = A.cpu()
        C = C * ((A / A.norm(dim=0).clamp_min(1e-300)).T @ (T / T.norm(dim=0)))
    return max(min(float(C[p[j], j]) for j in range(rank))
               for p in itertools.permutations(range(rank)))


def oracle_driver(t, rank, opts):
    """cpd_apr with the row-by-row oracle in place of apr_update."""
    factors = []
    for m, d in enumerate(t.dims):
        A = sp.seeded_init(d, rank, m, opts.seed).abs()
        factors.append(A / A.sum(0))
    lam = torch.full((rank,), float(t.vals.sum()) / rank, dtype=torch.float64)
    phi_prev = [None] * t.nmodes
    trace = []
    for it in range(opts.max_iters):
        kkt = 0.0
        for m in range(t.nmodes):
            A = factors[m]
            if it > 0:
                A = A + opts.kappa * ((A < opts.kappa_tol)
                                      & (phi_prev[m] > 1.0)).double()
            B, phi_prev[m], _, viol0, _ = oracle_update(
                t, factors, m, A * lam, opts.tolerance, opts.max_inner,
                opts.eps_div)
            lam = B.sum(0)
            factors[m] = B / torch.where(lam > 0, lam, torch.ones_like(lam))
            kkt = max(kkt, float(viol0.max()))
        trace.append(apr.poisson_loglik(factors, lam, t.inds, t.vals,
                                        opts.eps_div))
        if kkt < opts.tolerance:
            break
    return factors, lam, trace


def check_planted_result(r):
    t, truth, lam = planted()
    ll = r.loglik_trace
    assert r.niters == len(ll) == len(r.kkt_trace) == len(r.inner_trace)
    print("loglik:", " ".join(f"{x:.8e}" for x in ll))
    for a, b in zip(ll, ll[1:]):
        assert b <= a + 1e-9 * abs(a), (a, b)
    at_truth = apr.poisson_loglik(truth, lam, t.inds, t.vals)
    print(f"final {ll[-1]:.8e} vs planted parameters {at_truth:.8e}")
    assert ll[-1] <= at_truth
    c = congruence(r.factors, truth)
    print(f"smallest congruence {c:.4f} (required {CONGRUENCE_MIN:.4f})")
    assert c >= CONGRUENCE_MIN
    for A in r.factors:
        assert bool((A >= 0).all())
        assert (A.sum(0).cpu() - 1).abs().max().item() < 1e-12
    # at a stationary point the model's mass equals the data's
    assert float(r.lam.sum()) == pytest.approx(float(t.vals.sum()), rel=1e-2)


def test_cpd_apr_planted():
    t, _, _ = planted()
    r = sp.cpd_apr(t, 4, sp.AprOptions(**PLANTED_OPTS))
    check_planted_result(r)


def test_oracle_driver_reaches_recorded_congruence():
    """CONGRUENCE_MIN is derived from this run."""
    t, truth, _ = planted()
    factors, _, _ = oracle_driver(t, 4, sp.AprOptions(**PLANTED_OPTS))
    c = congruence(factors, truth)
    print(f"oracle-driven congruence {c:.4f}")
    assert abs(c - (CONGRUENCE_MIN + 0.05)) < 5e-4


FIXED_DRV = dict(max_iters=5, max_inner=5, tolerance=0.0, seed=77)


@functools.lru_cache(maxsize=None)
def fixed_schedule_cpu():
    """The 5 x 5 fixed schedule on `4-mode`, CPU torch path."""
    return sp.cpd_apr(four_mode(), 8, sp.AprOptions(**FIXED_DRV))


def test_fixed_schedule_matches_oracle_driver():
    r = fixed_schedule_cpu()
    assert r.niters == 5 and not r.converged
    nrows = sum(int((row_counts(four_mode(), m) > 0).sum())
                for m in range(4))
    assert r.inner_trace == [5 * nrows] * 5
    _, _, trace = oracle_driver(four_mode(), 8, sp.AprOptions(**FIXED_DRV))
    err = max(abs(a - b) / abs(b) for a, b in zip(r.loglik_trace, trace))
    print(f"driver trace, torch vs oracle: {err:.3e} (DRV_TOL {DRV_TOL:.1e})")
    assert 1e3 * err <= DRV_TOL


def test_converged_flag():
    t, _, _ = planted()
    tol = 5e-2
    r = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=200, tolerance=tol, seed=77))
    assert r.converged and r.niters < 200
    assert r.kkt_trace[-1] < tol
    assert all(k >= tol for k in r.kkt_trace[:-1])
    # a budget too short to get there
    r2 = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=2, tolerance=tol, seed=77))
    assert not r2.converged and r2.niters == 2
    assert r2.loglik_trace == r.loglik_trace[:2]


# ------------------------------------------------------------------ errors

def test_update_errors():
    t = four_mode()
    cs = cpu_csf("4-mode")
    mats = list(make_mats("4-mode", 16))
    kw = dict(inner_tol=0.0, max_inner=2)
    B = make_b("4-mode", 16, 0).clone()
    for rank in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            sp.apr_update(
                cs, [torch.ones(d, rank, dtype=torch.float64) for d in t.dims],
                0, torch.ones(t.dims[0], rank, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match="B must be"):
        sp.apr_update(cs, mats, 0, B[:-1].contiguous(), **kw)
    with pytest.raises(ValueError, match="B must be"):
        sp.apr_update(cs, mats, 0, B.float(), **kw)
    with pytest.raises(ValueError, match="factor 2 has shape"):
        sp.apr_update(cs, mats[:2] + [mats[2][:-1]] + mats[3:], 0, B, **kw)
    with pytest.raises(ValueError, match="factor matrices"):
        sp.apr_update(cs, mats[:3], 0, B, **kw)
    with pytest.raises(ValueError, match="max_inner"):
        sp.apr_update(cs, mats, 0, B, inner_tol=0.0, max_inner=0)
    with pytest.raises(ValueError, match="hip"):
        sp.apr_update(cs, mats, 0, B, impl="hip", **kw)     # CPU tensor
    with pytest.raises(ValueError, match="unknown impl"):
        sp.apr_update(cs, mats, 0, B, impl="triton", **kw)

    neg = sp.SpTensor(t.inds.clone(), t.vals - 2.0, list(t.dims))
    assert bool((neg.vals < 0).any())
    with pytest.raises(ValueError, match=">= 0"):
        sp.apr_update(sp.csf_alloc(neg, "all"), mats, 0, B, **kw)
    with pytest.raises(ValueError, match=">= 0"):
        sp.cpd_apr(neg, 4)

    t32 = sp.SpTensor.synthetic([20, 15, 25], 500, dtype=torch.float32,
                                seed=3)
    m32 = [torch.ones(d, 16, dtype=torch.float32) for d in t32.dims]
    with pytest.raises(ValueError, match="float64"):
        sp.apr_update(sp.csf_alloc(t32, "all"), m32, 0, m32[0].clone(), **kw)
    with pytest.raises(ValueError, match="float64"):
        sp.cpd_apr(t32, 4)

    two = sp.csf_alloc(t, "two")
    nonroot = [m for m in range(t.nmodes) if two.mode_depth[m] != 0]
    assert nonroot
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.apr_update(two, mats, nonroot[0],
                      make_b("4-mode", 16, nonroot[0]).clone(), **kw)
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.cpd_apr(two, 4)
    for rank in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            sp.cpd_apr(t, rank)


def test_update_on_a_single_csf_and_in_place():
    cs = cpu_csf("4-mode")
    mats = list(make_mats("4-mode", 7))
    B = make_b("4-mode", 7, 1).clone()
    keep = B
    Phi, iters, viol0 = sp.apr_update(cs.csfs[1], mats, 1, B, inner_tol=0.0,
                                      max_inner=FIXED_INNER)
    assert B is keep
    assert_close((B, Phi, iters, viol0), oracle_fixed("4-mode", 7, 1),
                 "single csf")


# ---------------------------------------------------------- binding checks

_APR_BINDING = "hip_apr_update"


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
        1e-10, 0.0, 3,
        torch.zeros(1, dtype=F64),                               # ws
        torch.zeros(ROWS, dtype=I32),                            # done
        torch.ones(ROWS, F, dtype=F64), torch.zeros(ROWS, F, dtype=F64),
        torch.zeros(ROWS, dtype=I32), torch.zeros(ROWS, dtype=F64)]


def test_binding_is_not_a_gpu_name():
    """tests/test_binding_checks.py owns the table of gpu_* bindings."""
    assert hasattr(native(), _APR_BINDING)
    assert not _APR_BINDING.startswith("gpu_")


@pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="host tensors must never reach a device; needs a GPU-less box")
def test_binding_rejects_host_tensors_and_wrong_dtype():
    args = _binding_args()
    with pytest.raises(RuntimeError, match="vals must be a device tensor"):
        getattr(native(), _APR_BINDING)(*args, 0)
    args = _binding_args()
    args[2] = args[2].to(torch.int16)
    with pytest.raises(RuntimeError, match="vals has dtype Short"):
        getattr(native(), _APR_BINDING)(*args, 0)


# --------------------------------------------------------------------- CLI

def test_cli_apr(tmp_path, capsys):
    from splatt_amd import cli
    t, _, _ = planted()
    path = str(tmp_path / "counts.tns")
    t.save(path)
    stem = str(tmp_path / "out" / "p_")
    rc = cli.main(["apr", path, "-r", "4", "-i", "3", "--tol", "1e-4",
                   "--inner", "4", "--seed", "77", "--device", "cpu",
                   "--stem", stem])
    assert rc == 0
    out = capsys.readouterr().out
    assert "its = 3 loglik = " in out and "Final log-likelihood:" in out
    r = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=3, max_inner=4, seed=77))
    assert f"its = 3 loglik = {r.loglik_trace[2]:.8e}" in out
    for m in range(3):
        rows = open(f"{stem}mode{m + 1}.mat").read().strip().splitlines()
        assert len(rows) == t.dims[m] and len(rows[0].split()) == 4
        got = torch.tensor([[float(x) for x in row.split()] for row in rows],
                           dtype=torch.float64)
        assert torch.equal(got, r.factors[m])
    lam = [float(x) for x in open(f"{stem}lambda.mat").read().split()]
    assert lam == r.lam.tolist()
    assert os.path.exists(f"{stem}lambda.mat")


# ------------------------------------------------ re-measuring the bounds

if __name__ == "__main__":
    worst = 0.0
    for rank in (7, 16, 32, 64):
        for mode in range(3):
            ref = oracle_fixed("heavy", rank, mode)
            B, Phi, viol0 = second_update(
                heavy(), list(make_mats("heavy", rank)), mode,
                make_b("heavy", rank, mode), FIXED_INNER)
            err = max(max_rel(B, ref[0]), max_rel(Phi, ref[1]),
                      max_rel(viol0, ref[3]))
            worst = max(worst, err)
            print(f"heavy rank {rank} mode {mode}: {err:.3e}")
    print(f"two CPU evaluations, worst: {worst:.3e}  (TOL {TOL:.1e})")
    r = fixed_schedule_cpu()
    _, _, trace = oracle_driver(four_mode(), 8, sp.AprOptions(**FIXED_DRV))
    err = max(abs(a - b) / abs(b) for a, b in zip(r.loglik_trace, trace))
    print(f"driver trace torch vs oracle: {err:.3e}  (DRV_TOL {DRV_TOL:.1e})")
    t, truth, _ = planted()
    factors, _, tr = oracle_driver(t, 4, sp.AprOptions(**PLANTED_OPTS))
    print(f"oracle-driven planted congruence: {congruence(factors, truth):.4f}"
          f" after {len(tr)} iterations")
