"""Poisson CPD, damped-Newton row solver (PDNR): the torch path against a
row-by-row CPU oracle, the invariants, the driver, errors, the CLI.

The oracle, inputs and bounds here are shared with tests/test_apr_pdnr_gpu.py;
the inputs and helpers are those of tests/test_apr.py.

Bounds. Float comparisons use  max|delta| <= TOL_PDNR * max(1, max|oracle|).
Two independent CPU f64 evaluations of the solver (the oracle: matrix
products per row, its own left-looking Cholesky; the second evaluation: the
nonzeros of a row in reversed order, the model value accumulated one column
at a time, f and Phi one nonzero at a time, H in reversed blocks of 64
nonzeros) took the same branches on every row of every case below and differed,
relative to max(1, max|oracle|) over B, Phi, viol0, f0, f and mu, by at most
2.5e-11 over the one-iteration cases (`thin`, rank 17, mode 0, in B: the
solve amplifies by the condition of H + mu I, and `thin` is singular up to
mu = 1e-5; Phi, viol0 and f0 of that case agree to 4e-16) and by at most
5.5e-13 over the stopping cases (inner_tol = 1e-4, max_inner = 30, ranks
7/16/17/64, first and last mode, three inputs). TOL_PDNR is the larger
figure with three orders of margin. DRV_TOL_PDNR bounds the relative
difference of the driver's log-likelihood trace on `4-mode` (rank 8,
tolerance 1e-4, 5 outer iterations): the torch path and the oracle-driven
driver differ by at most 1.4e-16 there; DRV_TOL_PDNR is that with three
orders of margin. `PYTHONPATH=. python tests/test_apr_pdnr.py`
re-measures all of these figures.
"""
import functools
import math

import numpy as np
import pytest
import torch

import splatt_amd as sp
from splatt_amd import apr
from splatt_amd._ext import native

from test_apr import (EPS, INPUTS, RANKS, _pi, check_planted_result,
                      congruence, cpu_csf, four_mode, make_b, make_mats,
                      max_rel, oracle_update, planted, row_counts)

TOL_PDNR = 2.5e-8
DRV_TOL_PDNR = 1.4e-13
MU0 = 1e-5
LS_MAX = 11
STOP_TOL = 1e-4
STOP_INNER = 30
STOP_RANKS = [7, 16, 17, 64]
# rows whose branches differ from the oracle's may be left out of a stopping
# comparison: at most 2% of a case's rows, never fewer than one allowed
LEFT_OUT = 0.02
FLOATS = ("B", "Phi", "viol0", "f0", "f", "mu")
COUNTS = ("iters", "nback", "nfail")


# ------------------------------------------------------------------ oracle

def _chol_lower(A):
    """Left-looking Cholesky; None if a pivot is <= 0 or NaN."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not s[0] > 0.0:
            return None
        d = math.sqrt(s[0])
        L[j:, j] = s / d
        L[j, j] = d
    return L


def _row_pass(Pi, x, b, eps_div, second, full=True):
    """f (without sum b), Phi and H of one row at b."""
    if not second:
        m = np.maximum(Pi @ b, eps_div)
        fd = -float((x * np.log(m)).sum())
        if not full:
            return fd, None, None
        phi = Pi.T @ (x / m)
        H = Pi.T @ ((x / m ** 2)[:, None] * Pi)
        return fd, phi, H
    m = np.zeros(x.size)
    for c in range(b.size):
        m = m + Pi[:, c] * b[c]
    m = np.maximum(m, eps_div)
    fd = -float(np.cumsum(x * np.log(m))[-1])
    if not full:
        return fd, None, None
    phi = np.cumsum((x / m)[:, None] * Pi, axis=0)[-1]
    H = np.zeros((b.size, b.size))
    for a in range(0, x.size, 64):
        P = Pi[a:a + 64]
        H = H + P.T @ ((x[a:a + 64] / m[a:a + 64] ** 2)[:, None] * P)
    return fd, phi, H


def oracle_pdnr(t, mats, mode, B0, inner_tol, max_inner, eps_div=EPS,
                mu0=MU0, second=False):
    """Row by row on the COO indices, exactly the box of apr.py. Returns a
    dict of per-row B, Phi, viol0, f0, f, mu, iters, nback, nfail, `fs` (a
    list per row: f after every iteration, preceded by the entry value) and
    `viol` (the last violation evaluated)."""
    Pall = _pi(t, mats, mode).numpy()
    vals = t.vals.double().numpy()
    key = t.inds[mode].numpy()
    n, rank = t.dims[mode], B0.shape[1]
    out = {k: np.zeros(n) for k in ("viol0", "f0", "f", "mu", "viol")}
    out.update({k: np.zeros(n, dtype=np.int32) for k in COUNTS})
    B = B0.clone().numpy()
    Phi = np.zeros_like(B)
    fs = [[] for _ in range(n)]
    for i in range(n):
        sel = np.nonzero(key == i)[0]
        if sel.size == 0:
            B[i] = 0.0
            continue
        if second:
            sel = sel[::-1]
        Pi, x = Pall[sel], vals[sel]
        b = B[i].copy()
        mu = mu0
        f = 0.0
        for l in range(1, max_inner + 1):
            fd, phi, H = _row_pass(Pi, x, b, eps_div, second)
            f = float(b.sum()) + fd
            g = 1.0 - phi
            viol = float(np.abs(np.minimum(b, g)).max())
            out["iters"][i] = l
            out["viol"][i] = viol
            Phi[i] = phi
            if l == 1:
                out["viol0"][i] = viol
                out["f0"][i] = f
                fs[i].append(f)
            if inner_tol > 0 and viol < inner_tol:
                break
            eps_act = min(1e-8, float(np.linalg.norm(
                b - np.maximum(b - g, 0.0))))
            fixed = (b == 0) & (g > 0)
            active = (b > 0) & (b <= eps_act) & (g > 0)
            free = ~(fixed | active)
            fi = np.nonzero(free)[0]
            Hff = H[np.ix_(fi, fi)]
            L = _chol_lower(Hff + mu * np.eye(fi.size))
            accepted = False
            if L is not None:
                df = np.linalg.solve(L.T, np.linalg.solve(L, -g[fi]))
                pred = float(g[fi] @ df + 0.5 * (df @ (Hff @ df)))
                d = np.zeros(rank)
                d[fi] = df
                d[active] = -g[active]
                alpha = 1.0
                for _ in range(LS_MAX):
                    bn = np.maximum(b + alpha * d, 0.0)
                    fn = float(bn.sum()) + _row_pass(
                        Pi, x, bn, eps_div, second, full=False)[0]
                    out["nback"][i] += 1
                    if fn <= f + 1e-4 * float(g @ (bn - b)):
                        accepted = True
                        break
                    alpha *= 0.5
            if accepted:
                rho = (fn - f) / pred if pred != 0 else float("nan")
                if pred == 0:
                    mu *= 10.0
                elif rho < 0.25:
                    mu *= 3.5
                elif rho > 0.75:
                    mu *= 2.0 / 7.0
                b, f = bn, fn
            else:
                mu *= 10.0
                out["nfail"][i] += 1
            fs[i].append(f)
        B[i] = b
        out["f"][i] = f
        out["mu"][i] = mu
    res = {k: torch.from_numpy(v) for k, v in out.items()}
    res["B"], res["Phi"] = torch.from_numpy(B), torch.from_numpy(Phi)
    res["fs"] = fs
    return res


@functools.lru_cache(maxsize=None)
def oracle_one(name, rank, mode):
    """One iteration, inner_tol = 0. Computed once per case, shared, never
    modified."""
    return oracle_pdnr(INPUTS[name](), list(make_mats(name, rank)), mode,
                       make_b(name, rank, mode), 0.0, 1)


@functools.lru_cache(maxsize=None)
def oracle_stop(name, rank, mode):
    return oracle_pdnr(INPUTS[name](), list(make_mats(name, rank)), mode,
                       make_b(name, rank, mode), STOP_TOL, STOP_INNER)


def stop_modes(name):
    return (0, INPUTS[name]().nmodes - 1)


def run_pdnr(cs, mats, mode, B0, impl, **kw):
    """The update as a dict shaped like the oracle's."""
    B = B0.clone()
    Phi, iters, viol0, stats = sp.apr_update_pdnr(cs, mats, mode, B,
                                                  impl=impl, **kw)
    got = dict(stats)
    got.update(B=B, Phi=Phi, iters=iters, viol0=viol0)
    return got


def compare(got, ref, what, exact_counts):
    """Floats within TOL_PDNR, counts equal. With `exact_counts` every row is
    compared and the counts must be equal; otherwise rows whose counts
    differ from the oracle's are left out, at most LEFT_OUT of them.
    Returns the largest relative error."""
    for k in COUNTS:
        assert got[k].dtype == torch.int32, k
    same = torch.ones_like(ref["iters"], dtype=torch.bool)
    for k in COUNTS:
        same &= got[k].cpu() == ref[k]
    nrows = same.numel()
    out = int((~same).sum())
    if exact_counts:
        assert out == 0, (what, "rows with other branches:",
                          (~same).nonzero().flatten().tolist())
    else:
        allowed = max(1, int(LEFT_OUT * nrows))
        print(f"{what}: {out} of {nrows} rows left out (allowed {allowed})")
        assert out <= allowed, (what, out, allowed)
    worst = 0.0
    for k in FLOATS:
        g, r = got[k].cpu().double()[same], ref[k][same]
        err = max_rel(g, r)
        worst = max(worst, err)
        print(f"{what} {k}: max|delta|/max(1,|ref|) = {err:.3e} "
              f"(bound {TOL_PDNR:.1e})")
        assert err <= TOL_PDNR, (what, k, err)
    return worst


def check_invariants(got, ref, t, mode, inner_tol, max_inner, what):
    """On every row: b >= 0; f did not increase; a row that stopped early
    has a violation below the tolerance at the B and Phi returned (so that
    Phi is the last pass's); rows without nonzeros are all zero."""
    B, Phi = got["B"].cpu(), got["Phi"].cpu()
    assert bool((B >= 0).all()), what
    f0, f = got["f0"].cpu(), got["f"].cpu()
    assert bool((f <= f0 + 1e-12 * f0.abs().clamp_min(1.0)).all()), what
    empty = row_counts(t, mode) == 0
    for k in FLOATS + COUNTS:
        assert bool((got[k].cpu()[empty] == 0).all()), (what, k)
    iters = got["iters"].cpu()
    assert bool((iters[~empty] >= 1).all()), what
    assert bool((iters <= max_inner).all()), what
    if inner_tol > 0:
        early = ~empty & (iters < max_inner)
        viol = torch.minimum(B, 1.0 - Phi).abs().amax(1)
        assert bool((viol[early] < inner_tol).all()), what
    if ref is not None:
        for fs in ref["fs"]:
            for a, b in zip(fs, fs[1:]):
                assert b <= a + 1e-12 * max(1.0, abs(a)), (what, a, b)


# ----------------------------------------------------------- preconditions

def test_inputs_cover_the_branches():
    """Backtracking, mu on both sides of mu0, failed searches, exact zeros,
    empty rows."""
    ref = oracle_stop("heavy", 16, 0)
    assert bool((ref["nback"] > ref["iters"] - 1).any())
    live = ref["iters"] > 0
    assert bool((ref["mu"][live] < MU0).any())
    assert bool((ref["mu"][live] > MU0).any())
    fails = sum(int(oracle_stop("thin", r, m)["nfail"].sum())
                for r in (7, 16) for m in stop_modes("thin"))
    assert fails > 0
    zeros = sum(int((oracle_stop(n, 16, 0)["B"][
        row_counts(INPUTS[n](), 0) > 0] == 0).sum()) for n in INPUTS)
    assert zeros > 0
    # rows with no nonzero: every mode of `heavy` and `thin` (`4-mode`, with
    # 8000 nonzeros in 20 x 15 x 25 x 12, has none)
    for name in ("heavy", "thin"):
        t = INPUTS[name]()
        for m in range(t.nmodes):
            assert int((row_counts(t, m) == 0).sum()) >= 1, (name, m)


# ------------------------------------------------------------ one iteration

def check_one(cs, device, name, rank, impl):
    t = INPUTS[name]()
    mats = [m.to(device) for m in make_mats(name, rank)]
    worst = 0.0
    for mode in range(t.nmodes):
        what = f"{impl} one {name} rank {rank} mode {mode}"
        got = run_pdnr(cs, mats, mode, make_b(name, rank, mode).to(device),
                       impl, inner_tol=0.0, max_inner=1)
        ref = oracle_one(name, rank, mode)
        worst = max(worst, compare(got, ref, what, exact_counts=True))
        check_invariants(got, ref, t, mode, 0.0, 1, what)
    return worst


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_one_iteration_torch(name, rank):
    check_one(cpu_csf(name), "cpu", name, rank, "torch")


# ------------------------------------------------------------ stopping runs

def check_stop(cs, device, name, rank, impl):
    t = INPUTS[name]()
    mats = [m.to(device) for m in make_mats(name, rank)]
    worst = 0.0
    for mode in stop_modes(name):
        what = f"{impl} stop {name} rank {rank} mode {mode}"
        got = run_pdnr(cs, mats, mode, make_b(name, rank, mode).to(device),
                       impl, inner_tol=STOP_TOL, max_inner=STOP_INNER)
        ref = oracle_stop(name, rank, mode)
        worst = max(worst, compare(got, ref, what, exact_counts=False))
        check_invariants(got, ref, t, mode, STOP_TOL, STOP_INNER, what)
    return worst


@pytest.mark.parametrize("rank", STOP_RANKS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_stopping_runs_torch(name, rank):
    check_stop(cpu_csf(name), "cpu", name, rank, "torch")


def second_vs_oracle(name, rank, mode, inner_tol, max_inner):
    """(rows with other branches, largest relative difference on the rest)
    of the second CPU evaluation against the oracle."""
    ref = (oracle_stop(name, rank, mode) if inner_tol > 0
           else oracle_one(name, rank, mode))
    sec = oracle_pdnr(INPUTS[name](), list(make_mats(name, rank)), mode,
                      make_b(name, rank, mode), inner_tol, max_inner,
                      second=True)
    same = torch.ones_like(ref["iters"], dtype=torch.bool)
    for k in COUNTS:
        same &= sec[k] == ref[k]
    err = max(max_rel(sec[k][same], ref[k][same]) for k in FLOATS)
    return int((~same).sum()), err


def test_two_evaluations_agree_within_tol():
    """The figure TOL_PDNR is derived from, on the case that sets it; the
    module's __main__ block prints it for all of them."""
    out, err = second_vs_oracle("thin", 17, 0, 0.0, 1)
    print(f"two CPU evaluations: {out} rows differ in branches, {err:.3e}")
    assert out == 0
    assert 1e3 * err <= 1.01 * TOL_PDNR
    out, err = second_vs_oracle("thin", 7, 2, STOP_TOL, STOP_INNER)
    print(f"stopping run: {out} rows differ in branches, {err:.3e}")
    assert out <= max(1, int(LEFT_OUT * INPUTS["thin"]().dims[2]))
    assert 1e3 * err <= TOL_PDNR


# ------------------------------------------------------------ thin beats MU

@pytest.mark.parametrize("name", ["thin", "heavy"])
def test_every_row_converges_and_beats_mu(name):
    """Within 30 Newton iterations every row meets inner_tol = 1e-4; from
    the same start 50 multiplicative iterations end higher."""
    t = INPUTS[name]()
    rank, mode = 16, 0
    ref = oracle_stop(name, rank, mode)
    live = row_counts(t, mode) > 0
    assert bool((ref["viol"][live] < STOP_TOL).all())
    print(f"{name}: most Newton iterations in a row {int(ref['iters'].max())}")
    mats = list(make_mats(name, rank))
    Bmu = oracle_update(t, mats, mode, make_b(name, rank, mode), 0.0, 50)[0]
    Pall = _pi(t, mats, mode)

    def objective(B):
        mdl = (B[t.inds[mode]] * Pall).sum(1).clamp_min(EPS)
        return float(B.sum() - (t.vals * mdl.log()).sum())

    f_mu, f_newton = objective(Bmu), objective(ref["B"])
    print(f"{name}: MU x50 {f_mu:.6f}  PDNR {f_newton:.6f}")
    assert f_newton < f_mu
    assert f_newton == pytest.approx(float(ref["f"].sum()), rel=1e-12)


# ------------------------------------------------------------------ driver

PLANTED_PDNR = dict(method="pdnr", max_iters=60, seed=77)
# smallest column congruence the oracle-driven CPU run reaches on the
# planted case (0.9768), minus 0.05
CONGRUENCE_MIN_PDNR = 0.9768 - 0.05
DRV_PDNR = dict(method="pdnr", max_iters=5, tolerance=1e-4, seed=77)


def oracle_driver_pdnr(t, rank, opts):
    """cpd_apr(method="pdnr") with the row-by-row oracle as the update."""
    factors = []
    for m, d in enumerate(t.dims):
        A = sp.seeded_init(d, rank, m, opts.seed).abs()
        factors.append(A / A.sum(0))
    lam = torch.full((rank,), float(t.vals.sum()) / rank, dtype=torch.float64)
    trace = []
    for it in range(opts.max_iters):
        kkt = 0.0
        for m in range(t.nmodes):
            r = oracle_pdnr(t, factors, m, factors[m] * lam, opts.tolerance,
                            opts.max_inner, opts.eps_div, opts.mu0)
            lam = r["B"].sum(0)
            factors[m] = r["B"] / torch.where(lam > 0, lam,
                                              torch.ones_like(lam))
            kkt = max(kkt, float(r["viol0"].max()))
        trace.append(apr.poisson_loglik(factors, lam, t.inds, t.vals,
                                        opts.eps_div))
        if kkt < opts.tolerance:
            break
    return factors, lam, trace


def check_planted_pdnr(r):
    """check_planted_result with this solver's own congruence bound."""
    check_planted_result(r)      # its bound is the same figure today
    c = congruence(r.factors, planted()[1])
    print(f"smallest congruence {c:.4f} (required {CONGRUENCE_MIN_PDNR:.4f})")
    assert c >= CONGRUENCE_MIN_PDNR
    assert r.converged and r.kkt_trace[-1] < 1e-4
    assert len(r.nback_trace) == r.niters
    assert all(n >= 0 for n in r.nback_trace) and sum(r.nback_trace) > 0


def test_cpd_apr_pdnr_planted():
    t, _, _ = planted()
    r = sp.cpd_apr(t, 4, sp.AprOptions(**PLANTED_PDNR))
    check_planted_pdnr(r)
    # keyword overrides are the same call
    r2 = sp.cpd_apr(t, 4, **PLANTED_PDNR)
    assert r2.loglik_trace == r.loglik_trace


def test_oracle_driver_reaches_recorded_congruence():
    """CONGRUENCE_MIN_PDNR is derived from this run."""
    t, truth, _ = planted()
    factors, _, _ = oracle_driver_pdnr(t, 4, sp.AprOptions(**PLANTED_PDNR))
    c = congruence(factors, truth)
    print(f"oracle-driven congruence {c:.4f}")
    assert abs(c - (CONGRUENCE_MIN_PDNR + 0.05)) < 5e-4


@functools.lru_cache(maxsize=None)
def short_schedule_cpu():
    return sp.cpd_apr(four_mode(), 8, sp.AprOptions(**DRV_PDNR))


def test_short_schedule_matches_oracle_driver():
    r = short_schedule_cpu()
    assert r.niters == 5 and len(r.nback_trace) == 5
    _, _, trace = oracle_driver_pdnr(four_mode(), 8,
                                     sp.AprOptions(**DRV_PDNR))
    err = max(abs(a - b) / abs(b) for a, b in zip(r.loglik_trace, trace))
    print(f"driver trace, torch vs oracle: {err:.3e} "
          f"(DRV_TOL_PDNR {DRV_TOL_PDNR:.1e})")
    assert err <= DRV_TOL_PDNR


def test_mu_stays_the_default_and_is_unchanged():
    """AprOptions() is the multiplicative solver, bit for bit what the
    explicit method gives, with no line-search trace."""
    t, _, _ = planted()
    assert sp.AprOptions().method == "mu" and sp.AprOptions().mu0 == MU0
    a = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=4, seed=77))
    b = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=4, seed=77, method="mu",
                                       mu0=3.0))
    assert a.loglik_trace == b.loglik_trace and a.kkt_trace == b.kkt_trace
    assert a.inner_trace == b.inner_trace
    assert a.nback_trace == [] and b.nback_trace == []
    for x, y in zip(a.factors, b.factors):
        assert torch.equal(x, y)
    assert torch.equal(a.lam, b.lam)


# ------------------------------------------------------------------ errors

def test_update_errors():
    t = four_mode()
    cs = cpu_csf("4-mode")
    mats = list(make_mats("4-mode", 16))
    kw = dict(inner_tol=0.0, max_inner=2)
    B = make_b("4-mode", 16, 0).clone()
    up = sp.apr_update_pdnr
    for rank in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            up(cs, [torch.ones(d, rank, dtype=torch.float64) for d in t.dims],
               0, torch.ones(t.dims[0], rank, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match="B must be"):
        up(cs, mats, 0, B[:-1].contiguous(), **kw)
    with pytest.raises(ValueError, match="B must be"):
        up(cs, mats, 0, B.float(), **kw)
    with pytest.raises(ValueError, match="factor 2 has shape"):
        up(cs, mats[:2] + [mats[2][:-1]] + mats[3:], 0, B, **kw)
    with pytest.raises(ValueError, match="factor matrices"):
        up(cs, mats[:3], 0, B, **kw)
    with pytest.raises(ValueError, match="max_inner"):
        up(cs, mats, 0, B, inner_tol=0.0, max_inner=0)
    with pytest.raises(ValueError, match="hip"):
        up(cs, mats, 0, B, impl="hip", **kw)     # CPU tensor
    with pytest.raises(ValueError, match="unknown impl"):
        up(cs, mats, 0, B, impl="triton", **kw)
    for mu0 in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="mu0"):
            up(cs, mats, 0, B, mu0=mu0, **kw)
    with pytest.raises(ValueError, match="mu0"):
        sp.cpd_apr(t, 4, sp.AprOptions(method="pdnr", mu0=0.0))
    with pytest.raises(ValueError, match="unknown method"):
        sp.cpd_apr(t, 4, sp.AprOptions(method="pqnr"))

    neg = sp.SpTensor(t.inds.clone(), t.vals - 2.0, list(t.dims))
    assert bool((neg.vals < 0).any())
    with pytest.raises(ValueError, match=">= 0"):
        up(sp.csf_alloc(neg, "all"), mats, 0, B, **kw)
    with pytest.raises(ValueError, match=">= 0"):
        sp.cpd_apr(neg, 4, method="pdnr")

    t32 = sp.SpTensor.synthetic([20, 15, 25], 500, dtype=torch.float32,
                                seed=3)
    m32 = [torch.ones(d, 16, dtype=torch.float32) for d in t32.dims]
    with pytest.raises(ValueError, match="float64"):
        up(sp.csf_alloc(t32, "all"), m32, 0, m32[0].clone(), **kw)

    two = sp.csf_alloc(t, "two")
    nonroot = [m for m in range(t.nmodes) if two.mode_depth[m] != 0]
    assert nonroot
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        up(two, mats, nonroot[0], make_b("4-mode", 16, nonroot[0]).clone(),
           **kw)


def test_update_on_a_single_csf_and_in_place():
    cs = cpu_csf("4-mode")
    mats = list(make_mats("4-mode", 7))
    B = make_b("4-mode", 7, 1).clone()
    keep = B
    Phi, iters, viol0, stats = sp.apr_update_pdnr(
        cs.csfs[1], mats, 1, B, inner_tol=0.0, max_inner=1)
    assert B is keep
    assert sorted(stats) == ["f", "f0", "mu", "nback", "nfail"]
    got = dict(stats, B=B, Phi=Phi, iters=iters, viol0=viol0)
    compare(got, oracle_one("4-mode", 7, 1), "single csf", exact_counts=True)


# ---------------------------------------------------------- binding checks

_PDNR_BINDING = "hip_apr_pdnr"


def _binding_args():
    F, NNZ, ROWS = 8, 12, 5
    I32, I64, F64 = torch.int32, torch.int64, torch.float64
    return [
        [torch.zeros(NNZ, dtype=I32) for _ in range(2)],         # idx
        [torch.ones(4, F, dtype=F64) for _ in range(2)],         # mats
        torch.ones(NNZ, dtype=F64),                              # vals
        torch.tensor([0, NNZ, NNZ, NNZ, NNZ, NNZ], dtype=I64),   # rowptr
        torch.tensor([0], dtype=I32),                            # rows
        1e-10, 0.0, 3, 1e-5,
        torch.ones(ROWS, F, dtype=F64), torch.zeros(ROWS, F, dtype=F64),
        torch.zeros(ROWS, dtype=I32), torch.zeros(ROWS, dtype=F64),
        torch.zeros(ROWS, dtype=F64), torch.zeros(ROWS, dtype=F64),
        torch.zeros(ROWS, dtype=F64), torch.zeros(ROWS, dtype=I32),
        torch.zeros(ROWS, dtype=I32)]


def test_binding_is_not_a_gpu_name():
    """tests/test_binding_checks.py owns the table of gpu_* bindings."""
    assert hasattr(native(), _PDNR_BINDING)
    assert not _PDNR_BINDING.startswith("gpu_")


@pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="host tensors must never reach a device; needs a GPU-less box")
def test_binding_rejects_host_tensors_and_wrong_dtype():
    args = _binding_args()
    with pytest.raises(RuntimeError, match="vals must be a device tensor"):
        getattr(native(), _PDNR_BINDING)(*args, 0)
    args = _binding_args()
    args[2] = args[2].to(torch.int16)
    with pytest.raises(RuntimeError, match="vals has dtype Short"):
        getattr(native(), _PDNR_BINDING)(*args, 0)


# --------------------------------------------------------------------- CLI

def _cli(tmp_path, capsys, sub, *extra):
    from splatt_amd import cli
    t, _, _ = planted()
    path = str(tmp_path / "counts.tns")
    t.save(path)
    stem = str(tmp_path / sub / "p_")
    rc = cli.main(["apr", path, "-r", "4", "-i", "3", "--tol", "1e-4",
                   "--inner", "4", "--seed", "77", "--device", "cpu",
                   "--stem", stem, *extra])
    assert rc == 0
    out = capsys.readouterr().out
    mats = []
    for m in range(3):
        rows = open(f"{stem}mode{m + 1}.mat").read().strip().splitlines()
        mats.append(torch.tensor(
            [[float(x) for x in row.split()] for row in rows],
            dtype=torch.float64))
    lam = [float(x) for x in open(f"{stem}lambda.mat").read().split()]
    return out, mats, lam


def test_cli_alg_pdnr(tmp_path, capsys):
    out, mats, lam = _cli(tmp_path, capsys, "newton", "--alg", "pdnr")
    t, _, _ = planted()
    r = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=3, max_inner=4, seed=77,
                                       method="pdnr"))
    assert f"its = 3 loglik = {r.loglik_trace[2]:.8e}" in out
    assert f"evals = {r.nback_trace[2]}" in out
    assert f"Line-search evaluations: {sum(r.nback_trace)}" in out
    for got, want in zip(mats, r.factors):
        assert torch.equal(got, want)
    assert lam == r.lam.tolist()


def test_cli_alg_mu_is_the_default(tmp_path, capsys):
    a = _cli(tmp_path, capsys, "plain")
    b = _cli(tmp_path, capsys, "mu", "--alg", "mu")
    lines = lambda o: [x for x in o.splitlines()           # noqa: E731
                       if x.startswith("  its = ") or x.startswith("Final")]
    assert lines(a[0]) == lines(b[0]) and len(lines(a[0])) == 4
    assert "evals" not in a[0] and "Line-search" not in a[0]
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert a[2] == b[2]
    t, _, _ = planted()
    r = sp.cpd_apr(t, 4, sp.AprOptions(max_iters=3, max_inner=4, seed=77))
    for got, want in zip(a[1], r.factors):
        assert torch.equal(got, want)


# ------------------------------------------------ re-measuring the bounds

if __name__ == "__main__":
    worst = 0.0
    for name in INPUTS:
        for rank in RANKS:
            for mode in range(INPUTS[name]().nmodes):
                out, err = second_vs_oracle(name, rank, mode, 0.0, 1)
                worst = max(worst, err)
                if out:
                    print(f"one {name} rank {rank} mode {mode}: {out} rows "
                          f"with other branches")
    print(f"two CPU evaluations, one iteration, worst: {worst:.3e}")
    worst = 0.0
    for name in INPUTS:
        for rank in STOP_RANKS:
            for mode in stop_modes(name):
                out, err = second_vs_oracle(name, rank, mode, STOP_TOL,
                                            STOP_INNER)
                worst = max(worst, err)
                print(f"stop {name} rank {rank} mode {mode}: {out} rows with "
                      f"other branches, {err:.3e}")
    print(f"two CPU evaluations, stopping runs, worst: {worst:.3e}  "
          f"(TOL_PDNR {TOL_PDNR:.1e})")
    r = short_schedule_cpu()
    _, _, trace = oracle_driver_pdnr(four_mode(), 8,
                                     sp.AprOptions(**DRV_PDNR))
    err = max(abs(a - b) / abs(b) for a, b in zip(r.loglik_trace, trace))
    print(f"driver trace torch vs oracle: {err:.3e}  "
          f"(DRV_TOL_PDNR {DRV_TOL_PDNR:.1e})")
    t, truth, _ = planted()
    factors, _, tr = oracle_driver_pdnr(t, 4, sp.AprOptions(**PLANTED_PDNR))
    print(f"oracle-driven planted congruence: {congruence(factors, truth):.4f}"
          f" after {len(tr)} iterations")
