"""Constrained CPD (AO-ADMM): the torch block update against exact integer
oracles, optimality of the converged solve, the driver on a planted
non-negative tensor, the CLI.

The oracles and the inputs here are shared with tests/test_admm_gpu.py.
"""
import functools
import math

import pytest
import torch

import splatt_amd as sp
from splatt_amd import admm
from splatt_amd.cli import parse_constraints

BR = admm.BLOCK_ROWS
LIMIT = 2 ** 52

# the exact cases: w is an integer multiple of rho, the box bounds integers
EXACT_RHO = 2.0
EXACT_CONS = {
    "nonneg": sp.nonneg(),
    "l1": sp.l1(2 * EXACT_RHO),
    "nonneg_l1": sp.nonneg_l1(3 * EXACT_RHO),
    "box": sp.box(-3, 5),
}
EXACT_RANKS = [1, 7, 16, 17, 32, 64]
EXACT_ROWS = [1, 63, 64, 65, 200]


def test_block_rows_constant():
    assert BR == 64


# ------------------------------------------------- 1. exact GEMV and prox

def int_prox(x, con, rho):
    """Elementwise prox on an int64 row; w/rho is an integer here."""
    if con.kind == "nonneg":
        return x.clamp(min=0)
    if con.kind == "box":
        return x.clamp(min=int(con.lo), max=int(con.hi))
    th = int(con.weight / rho)
    assert th * rho == con.weight
    if con.kind == "nonneg_l1":
        return (x - th).clamp(min=0)
    return torch.sign(x) * (x.abs() - th).clamp(min=0)


@functools.lru_cache(maxsize=None)
def exact_inputs(rank, n):
    g = torch.Generator().manual_seed(1000 * rank + n)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g,
                             dtype=torch.int64)

    return (ints(-2, 2, n, rank), ints(-1, 1, rank, rank),
            ints(-2, 2, n, rank), ints(-2, 2, n, rank))


@functools.lru_cache(maxsize=None)
def exact_oracle(rank, n, kind, max_inner=3):
    """int64, one row at a time, no blocks. Returns (H, U, peak) where peak
    bounds every intermediate of any summation order: the absolute-value
    sums of the GEMV and the four squared sums taken over ALL rows."""
    K, G, H, U = (x.clone() for x in exact_inputs(rank, n))
    con = EXACT_CONS[kind]
    rho = int(EXACT_RHO)
    peak = 0
    sq = [[0] * 4 for _ in range(max_inner)]
    for r in range(n):
        k, h, u = K[r], H[r], U[r]
        for it in range(max_inner):
            t = k + rho * (h + u)
            ht = t @ G
            peak = max(peak, int((t.abs() @ G.abs()).max()))
            hold = h
            h = int_prox(ht - u, con, rho)
            u = u + h - ht
            for i, v in enumerate((h - ht, h, h - hold, u)):
                sq[it][i] += int((v * v).sum())
        H[r], U[r] = h, u
    peak = max(peak, max(max(s) for s in sq))
    return H, U, peak


def run_exact(rank, n, kind, impl, device="cpu"):
    K, G, H, U = (x.double().to(device) for x in exact_inputs(rank, n))
    iters = sp.admm_update(K, G, EXACT_RHO, H, U, EXACT_CONS[kind],
                           inner_tol=0.0, max_inner=3, impl=impl)
    Ho, Uo, peak = exact_oracle(rank, n, kind)
    assert peak < LIMIT, (rank, n, kind, peak)
    assert iters.dtype == torch.int32
    assert iters.cpu().tolist() == [3] * ((n + BR - 1) // BR)
    assert torch.equal(H.cpu(), Ho.double()), (impl, rank, n, kind, "H")
    assert torch.equal(U.cpu(), Uo.double()), (impl, rank, n, kind, "U")


@pytest.mark.parametrize("n", EXACT_ROWS)
@pytest.mark.parametrize("rank", EXACT_RANKS)
def test_exact_gemv_prox_torch(rank, n):
    for kind in EXACT_CONS:
        run_exact(rank, n, kind, "torch")


# ------------------------------------------------ 2. exact stopping rule

STOP_TOL = 2.0 ** -6
STOP_MAX = 10
STOP_ROWS = 3 * BR + 20   # K >= 0 | mixed | K < 0 | short mixed block


@functools.lru_cache(maxsize=None)
def stop_inputs(rank):
    g = torch.Generator().manual_seed(77 + rank)

    def ints(lo, hi, rows):
        return torch.randint(lo, hi + 1, (rows, rank), generator=g,
                             dtype=torch.int64)

    K = torch.cat([ints(0, 8, BR), ints(-8, 8, BR), ints(-8, -1, BR),
                   ints(-8, 8, STOP_ROWS - 3 * BR)])
    return K, ints(0, 3, STOP_ROWS)


@functools.lru_cache(maxsize=None)
def stop_oracle(rank):
    """Ginv = I/2, rho = 1, U = 0, nonneg: Ht = (K + H + U)/2. Every value
    after iteration i is a multiple of 2^-i, so everything is carried as an
    int64 multiple of 2^-STOP_MAX and the stopping products are compared as
    integers. Returns (counts, H, U) with H, U as exact doubles."""
    K, H = stop_inputs(rank)
    S = 1 << STOP_MAX
    inv_tol = int(1 / STOP_TOL)
    Hs, Us, counts = [], [], []
    for b0 in range(0, STOP_ROWS, BR):
        k = K[b0:b0 + BR] * S
        h = H[b0:b0 + BR] * S
        u = torch.zeros_like(h)
        it = 0
        while it < STOP_MAX:
            it += 1
            t = k + h + u
            assert bool((t % 2 == 0).all())
            ht = t // 2
            hold = h
            h = (ht - u).clamp(min=0)
            u = u + h - ht
            pr, pn, dr, dn = (int((v * v).sum())
                              for v in (h - ht, h, h - hold, u))
            assert max(pr, pn, dr, dn) < LIMIT
            if pr * inv_tol <= pn and dr * inv_tol <= max(dn, pn):
                break
        counts.append(it)
        Hs.append(h.double() / S)
        Us.append(u.double() / S)
    return counts, torch.cat(Hs), torch.cat(Us)


def run_stop(rank, impl, device="cpu"):
    counts, Ho, Uo = stop_oracle(rank)
    print(f"rank {rank}: oracle counts {counts}")
    assert len(set(counts)) >= 3, counts
    assert counts[2] == STOP_MAX          # the all-zero solution never stops
    assert not bool(Ho[2 * BR:3 * BR].any())
    K, H = (x.double().to(device) for x in stop_inputs(rank))
    U = torch.zeros_like(H)
    Ginv = (0.5 * torch.eye(rank, dtype=torch.float64)).to(device)
    iters = sp.admm_update(K, Ginv, 1.0, H, U, sp.nonneg(),
                           inner_tol=STOP_TOL, max_inner=STOP_MAX, impl=impl)
    assert iters.cpu().tolist() == counts, (impl, rank)
    assert torch.equal(H.cpu(), Ho), (impl, rank, "H")
    assert torch.equal(U.cpu(), Uo), (impl, rank, "U")


@pytest.mark.parametrize("rank", [7, 16])
def test_exact_stopping_rule_torch(rank):
    run_stop(rank, "torch")


# ------------------------------------------------------- realistic inputs

@functools.lru_cache(maxsize=None)
def realistic_gram(rank, seed=5):
    """Hadamard product of two random Grams, as the driver forms it."""
    g = torch.Generator().manual_seed(seed * 100 + rank)
    A = torch.rand(40, rank, generator=g, dtype=torch.float64)
    B = torch.rand(50, rank, generator=g, dtype=torch.float64)
    return (A.T @ A) * (B.T @ B)


@functools.lru_cache(maxsize=None)
def realistic_inputs(rank, n, seed=5):
    """(K, G, H, U): K = H* G + noise for a sparse non-negative H*, so every
    constraint is active on part of the entries; H and U as a few outer
    iterations would leave them."""
    G = realistic_gram(rank, seed)
    g = torch.Generator().manual_seed(seed * 1000 + 7 * rank + n)

    def rnd(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)

    Hstar = rnd(n, rank) * (rnd(n, rank) < 0.5)
    K = Hstar @ G + 0.05 * float(G.abs().max()) * (rnd(n, rank) - 0.5)
    H = rnd(n, rank)
    U = 0.1 * (rnd(n, rank) - 0.5)
    return K, G, H, U


REAL_CONS = {
    "nonneg": sp.nonneg(),
    "l1": sp.l1(5.0),
    "nonneg_l1": sp.nonneg_l1(5.0),
    "box": sp.box(0.1, 0.6),
}


# ---------------------------------------------------------- 3. optimality

# KKT residual bound, relative to max|K|. The converged torch update reaches
# at most 7.0e-13 * max|K| on these inputs (5.1e-10 absolute at max|K| = 734,
# F = 8; 5.8e-10 at max|K| = 1214, F = 16); the bound is that with two
# orders of margin.
KKT_EPS = 7.0e-11


@pytest.mark.parametrize("kind", ["nonneg", "l1", "box", "nonneg_l1"])
@pytest.mark.parametrize("rank", [8, 16])
def test_solve_satisfies_kkt(rank, kind):
    """min 0.5 h G h^T - k h^T + r(h): with g = H G - K the optimum has
    g = 0 on the free entries and the sign conditions at the active ones."""
    K, G, H, U = (x.clone() for x in realistic_inputs(rank, 150))
    con = REAL_CONS[kind]
    iters = sp.admm_solve(K, G, H, U, con, inner_tol=1e-30, max_inner=20000)
    g = H @ G - K
    eps = KKT_EPS * float(K.abs().max())
    w = con.weight

    def worst(mask, viol):
        return float(viol[mask].max()) if bool(mask.any()) else 0.0

    if kind == "nonneg":
        parts = [worst(H == 0, -g), worst(H > 0, g.abs())]
        assert bool((H >= 0).all())
    elif kind == "l1":
        parts = [worst(H == 0, g.abs() - w),
                 worst(H != 0, (g + w * torch.sign(H)).abs())]
    elif kind == "nonneg_l1":
        parts = [worst(H == 0, -(g + w)), worst(H > 0, (g + w).abs())]
        assert bool((H >= 0).all())
    else:
        lo, hi = con.lo, con.hi
        assert bool(((H >= lo) & (H <= hi)).all())
        parts = [worst(H == lo, -g), worst(H == hi, g),
                 worst((H > lo) & (H < hi), g.abs())]
    active = int((H == (con.lo if kind == "box" else 0.0)).sum())
    print(f"{kind} rank {rank}: KKT residual {max(parts):.3e} (bound "
          f"{eps:.3e}, max|K| {float(K.abs().max()):.1f}), active entries "
          f"{active}/{H.numel()}, inner iterations max {int(iters.max())}")
    assert 0 < active < H.numel()          # the constraint does something
    assert max(parts) <= eps, (kind, rank, parts, eps)


# -------------------------------------------------------------- 4. driver

@functools.lru_cache(maxsize=None)
def planted():
    """Rank-4 non-negative 60x50x70 tensor plus noise 0.01, EVERY cell
    stored, so that absent-means-zero changes nothing."""
    g = torch.Generator().manual_seed(2025)
    dims = [60, 50, 70]
    A = [torch.rand(d, 4, generator=g, dtype=torch.float64) for d in dims]
    dense = torch.einsum("if,jf,kf->ijk", *A)
    dense = dense + 0.01 * torch.randn(dense.shape, generator=g,
                                       dtype=torch.float64)
    pos = torch.arange(dense.numel())
    inds = torch.stack([pos // (dims[1] * dims[2]),
                        (pos // dims[2]) % dims[1], pos % dims[2]], 0)
    return sp.SpTensor(inds.contiguous(), dense.reshape(-1).clone(), dims)


DRIVER_ITERS = 30
# cpd_als's fit minus cpd_aoadmm(nonneg)'s after DRIVER_ITERS iterations on
# the CPU is -4.5e-2: from this start ALS sits in a swamp at 0.9306 (0.9316
# after 50 iterations) while the non-negative run is at 0.9751. Ten times a
# negative gap is below the floor, so the margin is the floor 1e-4.
FIT_MARGIN = 1e-4


def driver_opts(**kw):
    kw.setdefault("max_iters", DRIVER_ITERS)
    kw.setdefault("tolerance", 0.0)
    kw.setdefault("seed", 77)
    return sp.AoAdmmOptions(**kw)


@functools.lru_cache(maxsize=None)
def planted_nonneg_cpu():
    return sp.cpd_aoadmm(planted(), 4, sp.nonneg(), driver_opts())


def test_driver_nonneg_planted():
    t = planted()
    k = planted_nonneg_cpu()
    assert isinstance(k, sp.ConstrainedKruskal) and isinstance(k, sp.Kruskal)
    assert k.niters == DRIVER_ITERS == len(k.fit_trace)
    for A in k.factors:
        assert float(A.min()) >= 0.0
    assert torch.equal(k.lam, torch.ones(4, dtype=torch.float64))
    assert abs(sp.kruskal_fit(k, t) - k.fit) < 1e-6
    als = sp.cpd_als(t, 4, sp.CpdOptions(max_iters=DRIVER_ITERS,
                                         tolerance=0.0, seed=77))
    print(f"fit: aoadmm {k.fit:.6f} als {als.fit:.6f} gap "
          f"{als.fit - k.fit:.3e}")
    assert k.fit >= als.fit - FIT_MARGIN
    # duals and inner-iteration bookkeeping
    assert [tuple(u.shape) for u in k.duals] == [(d, 4) for d in t.dims]
    assert len(k.inner_iters) == DRIVER_ITERS
    nblocks = [(d + BR - 1) // BR for d in t.dims]
    for row in k.inner_iters:
        assert len(row) == 3
        for cnt, nb in zip(row, nblocks):
            assert nb <= cnt <= 50 * nb


def test_driver_box_and_sparsity():
    t = planted()
    kb = sp.cpd_aoadmm(t, 4, sp.box(0, 0.8), driver_opts(max_iters=8))
    for A in kb.factors:
        assert float(A.min()) >= 0.0 and float(A.max()) <= 0.8
    kn = sp.cpd_aoadmm(t, 4, sp.nonneg(), driver_opts(max_iters=8))
    ks = sp.cpd_aoadmm(t, 4, sp.nonneg_l1(20.0), driver_opts(max_iters=8))
    zn = sum(int((A == 0).sum()) for A in kn.factors)
    zs = sum(int((A == 0).sum()) for A in ks.factors)
    print(f"exact zeros: nonneg {zn}, nonneg_l1 {zs}")
    assert all(float(A.min()) >= 0.0 for A in ks.factors)
    assert zs > zn


def test_driver_none_mode_is_plain_solve():
    """No constraint anywhere: every mode takes solve_rows(K, inv(G)), i.e.
    un-normalised ALS. One iteration from the same start must reproduce it
    (one MTTKRP thread: the threaded CPU reduction order varies run to run)."""
    from splatt_amd.ops.dense import gram, solve_rows, spd_inverse
    t = planted()
    k = sp.cpd_aoadmm(t, 4, [None, None, None],
                      driver_opts(max_iters=1, nthreads=1))
    cs = sp.csf_alloc(t, "two")
    f = [sp.seeded_init(d, 4, m, 77) for m, d in enumerate(t.dims)]
    for m in range(3):
        G = torch.ones(4, 4, dtype=torch.float64)
        for o in range(3):
            if o != m:
                G *= gram(f[o])
        f[m] = solve_rows(sp.mttkrp(cs, f, m, nthreads=1), spd_inverse(G))
    for a, b in zip(k.factors, f):
        assert torch.equal(a, b)
    assert k.inner_iters == [[0, 0, 0]]
    assert all(not bool(u.any()) for u in k.duals)
    # mixed: the unconstrained mode may go negative, the others may not
    km = sp.cpd_aoadmm(t, 4, [sp.nonneg(), None, sp.nonneg()],
                       driver_opts(max_iters=3))
    assert float(km.factors[0].min()) >= 0 and float(km.factors[2].min()) >= 0
    assert [r[1] for r in km.inner_iters] == [0, 0, 0]


def test_driver_constraint_spellings_agree():
    t = planted()
    c = sp.nonneg_l1(1.0)
    o = driver_opts(max_iters=3, nthreads=1)
    a = sp.cpd_aoadmm(t, 4, c, o)
    b = sp.cpd_aoadmm(t, 4, [c, c, c], o)
    d = sp.cpd_aoadmm(t, 4, {0: c, 1: c, 2: c}, o)
    for x in (b, d):
        assert x.fit_trace == a.fit_trace
        assert x.inner_iters == a.inner_iters
        for fa, fx in zip(a.factors, x.factors):
            assert torch.equal(fa, fx)
    with pytest.raises(ValueError):
        sp.cpd_aoadmm(t, 4, [c, c], o)
    with pytest.raises(ValueError):
        sp.cpd_aoadmm(t, 4, {3: c}, o)
    with pytest.raises(TypeError):
        sp.cpd_aoadmm(t, 4, ["nonneg", None, None], o)


def test_driver_rejects_f32():
    t = sp.SpTensor.synthetic([20, 15, 25], 500, seed=3,
                              dtype=torch.float32)
    with pytest.raises(ValueError, match="float64"):
        sp.cpd_aoadmm(t, 4, sp.nonneg())


# ------------------------------------------------------ 5. CLI and errors

def test_constraint_validation():
    assert sp.nonneg() == sp.Constraint("nonneg")
    assert sp.l1(0.5) == sp.Constraint("l1", weight=0.5)
    assert sp.nonneg_l1(2) == sp.Constraint("nonneg_l1", weight=2)
    assert sp.box(-1, 1) == sp.Constraint("box", lo=-1, hi=1)
    for bad in (lambda: sp.Constraint("simplex"), lambda: sp.l1(0.0),
                lambda: sp.l1(-1.0), lambda: sp.nonneg_l1(0.0),
                lambda: sp.box(1.0, 1.0), lambda: sp.box(2.0, 1.0),
                lambda: sp.l1(float("nan")),
                lambda: sp.box(0.0, float("inf"))):
        with pytest.raises(ValueError):
            bad()


def test_parse_constraints():
    assert parse_constraints(["nonneg"], 3) == [sp.nonneg()] * 3
    assert parse_constraints(["l1:0.1@1,3"], 3) == [sp.l1(0.1), None,
                                                    sp.l1(0.1)]
    assert parse_constraints(["box:0:1@2", "nonneg@1"], 3) == [
        sp.nonneg(), sp.box(0, 1), None]
    assert parse_constraints(["nonneg_l1:2@4"], 4) == [None, None, None,
                                                       sp.nonneg_l1(2.0)]
    for bad in (["simplex"], ["l1"], ["l1:a"], ["l1:0"], ["nonneg:1"],
                ["box:0"], ["box:1:0"], ["box:0:1:2"], ["nonneg@0"],
                ["nonneg@4"], ["nonneg@1,1"], ["nonneg@"], ["nonneg@x"],
                ["nonneg", "l1:1@2"], [""], ["@1"]):
        with pytest.raises(ValueError):
            parse_constraints(bad, 3)


def test_cli_cpd_con(tmp_path, monkeypatch, capsys):
    from splatt_amd.cli import main
    t = sp.SpTensor.synthetic([20, 15, 25], 2000, seed=3)
    path = str(tmp_path / "t.tns")
    t.save(path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["cpd", path, "-r", "4", "-i", "3", "--device", "cpu"]
    assert main(base + ["--con", "nonneg", "--inner-its", "20",
                        "--inner-tol", "1e-3"]) == 0
    out = capsys.readouterr().out
    assert "Final fit:" in out and "inner iterations:" in out
    for m, d in enumerate(t.dims):
        rows = [[float(x) for x in line.split()]
                for line in open(tmp_path / f"mode{m + 1}.mat")]
        assert len(rows) == d and all(len(r) == 4 for r in rows)
        assert min(min(r) for r in rows) >= 0.0
    # the one-line errors
    for extra, word in ((["--con", "nonneg", "--native"], "--native"),
                        (["--con", "nonneg", "--dtype", "f32"], "float64"),
                        (["--con", "bogus"], "unknown kind"),
                        (["--con", "nonneg@7"], "out of range")):
        assert main(base + extra) == 1
        err = capsys.readouterr().err.strip()
        assert word in err and len(err.splitlines()) == 1, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert main(base + ["--con", "nonneg"]) == 1
    assert "WORLD_SIZE" in capsys.readouterr().err


def test_admm_update_errors():
    K, G, H, U = (x.clone() for x in realistic_inputs(8, 70))
    Ginv = torch.linalg.inv(
        G + torch.eye(8, dtype=torch.float64)).contiguous()
    c = sp.nonneg()
    ok = sp.admm_update(K, Ginv, 1.0, H, U, c)
    assert ok.shape == (2,) and ok.dtype == torch.int32
    assert sp.admm_update(K, Ginv, torch.tensor([1.0]), H, U, c,
                          max_inner=0).tolist() == [0, 0]
    with pytest.raises(ValueError, match="float64"):
        sp.admm_update(K.float(), Ginv, 1.0, H, U, c)
    with pytest.raises(ValueError, match="float64"):
        sp.admm_update(K, Ginv, 1.0, H.float(), U, c)
    with pytest.raises(ValueError, match="same shape"):
        sp.admm_update(K[:-1].contiguous(), Ginv, 1.0, H, U, c)
    with pytest.raises(ValueError, match="Ginv"):
        sp.admm_update(K, Ginv[:7, :7].contiguous(), 1.0, H, U, c)
    with pytest.raises(ValueError, match="contiguous"):
        sp.admm_update(K, Ginv, 1.0, H.T.contiguous().T, U, c)
    with pytest.raises(ValueError, match="2-D"):
        sp.admm_update(K, Ginv, 1.0, H, U.reshape(-1), c)
    with pytest.raises(ValueError, match="rank"):
        z = torch.zeros(4, 65, dtype=torch.float64)
        sp.admm_update(z, torch.zeros(65, 65, dtype=torch.float64), 1.0,
                       z.clone(), z.clone(), c)
    with pytest.raises(ValueError, match="rho"):
        sp.admm_update(K, Ginv, 0.0, H, U, c)
    with pytest.raises(ValueError, match="rho"):
        sp.admm_update(K, Ginv, torch.ones(2), H, U, c)
    with pytest.raises(ValueError, match="max_inner"):
        sp.admm_update(K, Ginv, 1.0, H, U, c, max_inner=-1)
    with pytest.raises(ValueError, match="impl"):
        sp.admm_update(K, Ginv, 1.0, H, U, c, impl="triton")
    with pytest.raises(ValueError, match="device"):
        sp.admm_update(K, Ginv, 1.0, H, U, c, impl="hip")
    with pytest.raises(TypeError):
        sp.admm_update(K, Ginv, 1.0, H, U, "nonneg")


# ------------------------------------- float cases shared with the GPU tests

FLOAT_RANKS = [7, 16, 32, 64]
FLOAT_ROWS = 200
FLOAT_ITERS = 20
# max|delta| <= TOL * max(1, max|oracle|). Two independent CPU f64
# evaluations of the same FLOAT_ITERS iterations (library matmul against a
# reversed, one-term-at-a-time summation) differ by at most 9.3e-15 on these
# inputs (relative, F = 64), over every rank and kind; the bound is that figure with about three
# orders of margin.
TOL = 1e-11


@functools.lru_cache(maxsize=None)
def float_inputs(rank, n=FLOAT_ROWS):
    """(K, Ginv, rho, H, U) with rho = trace(G)/F and Ginv = (G + rho I)^-1
    inverted once on the CPU, so every implementation gets the same bits."""
    K, G, H, U = realistic_inputs(rank, n)
    rho = float(G.diagonal().sum()) / rank
    Ginv = torch.linalg.inv(G + rho * torch.eye(rank, dtype=torch.float64))
    return K, Ginv.contiguous(), rho, H, U


def reference_update(K, Ginv, rho, H, U, con, inner_tol, max_inner,
                     reverse=False):
    """One block at a time, nothing vectorised across blocks. Returns
    (counts, H, U, gap) where gap is the smallest relative distance of any
    evaluated stopping ratio from inner_tol. reverse=True sums the GEMV one
    term at a time from the last k to the first."""
    n, F = H.shape
    H, U = H.clone(), U.clone()
    counts, gap = [], math.inf
    for b0 in range(0, n, BR):
        k, h, u = K[b0:b0 + BR], H[b0:b0 + BR], U[b0:b0 + BR]
        it = 0
        while it < max_inner:
            it += 1
            t = k + rho * (h + u)
            if reverse:
                ht = torch.zeros_like(t)
                for j in reversed(range(F)):
                    ht = ht + t[:, j:j + 1] * Ginv[j:j + 1, :]
            else:
                ht = t @ Ginv
            hold = h
            h = con.prox(ht - u, rho)
            u = u + h - ht
            if inner_tol > 0:
                pr, pn, dr, dn = (float(v.square().sum())
                                  for v in (h - ht, h, h - hold, u))
                for lhs, rhs in ((pr, pn), (dr, max(dn, pn))):
                    if rhs > 0:
                        gap = min(gap, abs(lhs / (inner_tol * rhs) - 1.0))
                if pr <= inner_tol * pn and dr <= inner_tol * max(dn, pn):
                    break
        counts.append(it)
        H[b0:b0 + BR], U[b0:b0 + BR] = h, u
    return counts, H, U, gap


@functools.lru_cache(maxsize=None)
def float_oracle(rank, kind):
    """impl="torch" on the CPU at a fixed count: the oracle of the GPU
    float tests. Computed once, shared, never modified."""
    K, Ginv, rho, H, U = float_inputs(rank)
    H, U = H.clone(), U.clone()
    sp.admm_update(K, Ginv, rho, H, U, REAL_CONS[kind], inner_tol=0.0,
                   max_inner=FLOAT_ITERS, impl="torch")
    return H, U


def assert_close(got_h, got_u, ref_h, ref_u, what):
    worst = 0.0
    for name, got, ref in (("H", got_h, ref_h), ("U", got_u, ref_u)):
        err = float((got.cpu() - ref).abs().max())
        scale = max(1.0, float(ref.abs().max()))
        print(f"{what} {name}: max|delta| = {err:.3e} "
              f"(bound {TOL * scale:.3e})")
        assert err <= TOL * scale, (what, name, err, TOL * scale)
        worst = max(worst, err / scale)
    return worst


@pytest.mark.parametrize("kind", list(REAL_CONS))
@pytest.mark.parametrize("rank", FLOAT_RANKS)
def test_float_torch_matches_reversed_summation(rank, kind):
    K, Ginv, rho, H, U = float_inputs(rank)
    _, Hr, Ur, _ = reference_update(K, Ginv, rho, H, U, REAL_CONS[kind], 0.0,
                                    FLOAT_ITERS, reverse=True)
    Ho, Uo = float_oracle(rank, kind)
    rel = assert_close(Hr, Ur, Ho, Uo, f"reversed rank {rank} {kind}")
    print(f"relative difference {rel:.3e}")


STOP_CASES = [(7, "nonneg"), (16, "nonneg"), (32, "nonneg"), (64, "nonneg"),
              (16, "l1"), (16, "box"), (7, "nonneg_l1")]
STOP_TOLS = [1e-2, 1e-4]
STOP_NBLOCKS = 6
FLOAT_STOP_ROWS = (STOP_NBLOCKS - 1) * BR + 37


@functools.lru_cache(maxsize=None)
def float_stop_inputs(rank):
    """The realistic inputs with K changed per block so that the blocks stop
    at different counts: as is | K/50 | K shifted negative (the non-negative
    solution is zero) | 5K | started at H = 0 | a short block."""
    K, Ginv, rho, H, U = float_inputs(rank, FLOAT_STOP_ROWS)
    K, H = K.clone(), H.clone()
    K[BR:2 * BR] /= 50.0
    K[2 * BR:3 * BR] -= 2.0 * float(K.abs().max())
    K[3 * BR:4 * BR] *= 5.0
    H[4 * BR:5 * BR] = 0.0
    return K, Ginv, rho, H, U


@functools.lru_cache(maxsize=None)
def float_stop_oracle(rank, kind, tol):
    K, Ginv, rho, H, U = float_stop_inputs(rank)
    counts, Ho, Uo, gap = reference_update(K, Ginv, rho, H, U,
                                           REAL_CONS[kind], tol, 50)
    print(f"rank {rank} {kind} tol {tol:g}: counts {counts}, closest "
          f"stopping ratio {gap:.2e} away from the tolerance")
    # precondition: no stopping decision is within rounding of flipping
    assert gap > 1e-6, (rank, kind, tol, gap)
    assert len(set(counts)) >= 3, counts
    assert len(counts) == STOP_NBLOCKS
    return counts, Ho, Uo


def run_float_stop(rank, kind, tol, impl, device="cpu"):
    counts, Ho, Uo = float_stop_oracle(rank, kind, tol)
    K, Ginv, rho, H, U = (x.to(device) if isinstance(x, torch.Tensor) else x
                          for x in float_stop_inputs(rank))
    H, U = H.clone(), U.clone()
    iters = sp.admm_update(K, Ginv, rho, H, U, REAL_CONS[kind],
                           inner_tol=tol, max_inner=50, impl=impl)
    assert iters.cpu().tolist() == counts, (impl, rank, kind, tol)
    return assert_close(H, U, Ho, Uo, f"{impl} rank {rank} {kind} tol {tol:g}")


@pytest.mark.parametrize("tol", STOP_TOLS)
@pytest.mark.parametrize("rank,kind", STOP_CASES)
def test_float_stopping_torch_matches_blockwise(rank, kind, tol):
    run_float_stop(rank, kind, tol, "torch")
