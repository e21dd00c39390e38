"""Tensor completion (observed-entries ALS): the torch path against a
row-by-row CPU oracle, the driver on a planted low-rank case, the CLI.

The oracle and the inputs here are shared with tests/test_complete_gpu.py.
"""
import functools
import os

import pytest
import torch

import splatt_amd as sp
from splatt_amd import completion

REG = 1e-2
# max|delta| <= TOL * max(1, max|oracle|): two independent CPU f64
# computations of these updates (one-shot H^T H + LU vs K=4-chunked shuffled
# accumulation + Cholesky) differ by at most 8.4e-13 at reg=1e-2; the bound
# is that figure with about three orders of margin.
TOL = 1e-9


# ------------------------------------------------------------------ inputs

@functools.lru_cache(maxsize=None)
def heavy():
    return sp.SpTensor.synthetic([200, 150, 180], 40_000, seed=17, dist="zipf")


@functools.lru_cache(maxsize=None)
def thin():
    return sp.SpTensor.synthetic([300, 250, 400], 900, seed=17)


@functools.lru_cache(maxsize=None)
def four_mode():
    return sp.SpTensor.synthetic([20, 15, 25, 12], 8_000, seed=17)


INPUTS = {"heavy": heavy, "thin": thin, "4-mode": four_mode}


def row_counts(t, mode):
    return torch.bincount(t.inds[mode], minlength=t.dims[mode])


def check_preconditions(name):
    """The inputs must keep covering the branches they were chosen for."""
    t = INPUTS[name]()
    if name == "heavy":
        for m in range(t.nmodes):
            cnt = row_counts(t, m)
            assert int((cnt == 0).sum()) >= 1, m
            assert int(cnt.max()) > 4 * completion.SEG, (m, int(cnt.max()))
            assert int((cnt % 4 != 0).sum()) > 100, m
    elif name == "thin":
        cnt = row_counts(t, 0)
        assert int((cnt == 0).sum()) >= 1
        assert int((cnt == 1).sum()) >= 1
        for m in range(t.nmodes):
            assert int(row_counts(t, m).max()) < 16  # under-determined rows


@functools.lru_cache(maxsize=None)
def make_mats(name, rank, seed=123):
    t = INPUTS[name]()
    return tuple(sp.seeded_init(d, rank, m, seed)
                 for m, d in enumerate(t.dims))


# ------------------------------------------------------------------ oracle

def oracle_update(t, mats, mode, reg):
    """Row by row: mask Omega_i on the COO indices, N = H^T H + reg*I,
    b = H^T v, LU solve; rows with empty Omega_i are zero."""
    rank = mats[0].shape[1]
    H = torch.ones(t.nnz, rank, dtype=torch.float64)
    for m in range(t.nmodes):
        if m != mode:
            H = H * mats[m][t.inds[m]]
    out = torch.zeros(t.dims[mode], rank, dtype=torch.float64)
    eye = torch.eye(rank, dtype=torch.float64)
    for i in range(t.dims[mode]):
        mask = t.inds[mode] == i
        if not bool(mask.any()):
            continue
        Hi = H[mask]
        out[i] = torch.linalg.solve(Hi.T @ Hi + reg * eye,
                                    Hi.T @ t.vals[mask].double())
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, rank, mode):
    """Computed once per case, shared, never modified."""
    return oracle_update(INPUTS[name](), list(make_mats(name, rank)), mode,
                         REG)


def assert_matches_oracle(got, name, rank, mode, what):
    ref = oracle(name, rank, mode)
    err = (got.cpu() - ref).abs().max().item()
    bound = TOL * max(1.0, ref.abs().max().item())
    print(f"{what} {name} rank {rank} mode {mode}: max|delta| = {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound, (what, name, rank, mode, err, bound)
    empty = row_counts(INPUTS[name](), mode) == 0
    assert bool((got.cpu()[empty] == 0).all()), (what, name, rank, mode)
    return err


# ----------------------------------------------------------- row updates

@pytest.mark.parametrize("rank", [16, 7])
@pytest.mark.parametrize("name", list(INPUTS))
def test_update_torch_matches_oracle(name, rank):
    check_preconditions(name)
    t = INPUTS[name]()
    cs = sp.csf_alloc(t, "all")
    mats = list(make_mats(name, rank))
    for mode in range(t.nmodes):
        got = sp.complete_update(cs, mats, mode, REG, impl="torch")
        assert_matches_oracle(got, name, rank, mode, "torch")


def test_update_auto_is_torch_on_cpu_and_fills_out():
    t = four_mode()
    cs = sp.csf_alloc(t, "all")
    mats = list(make_mats("4-mode", 7))
    out = torch.full((t.dims[1], 7), 3.0, dtype=torch.float64)
    got = sp.complete_update(cs, mats, 1, REG, out=out)
    assert got is out
    assert_matches_oracle(got, "4-mode", 7, 1, "auto")
    # a single root-mode Csf works as well as the set
    got1 = sp.complete_update(cs.csfs[1], mats, 1, REG)
    assert torch.equal(got1, got)


def test_update_errors():
    t = four_mode()
    cs = sp.csf_alloc(t, "all")
    mats = list(make_mats("4-mode", 16))
    for bad in (0.0, -1e-2):
        with pytest.raises(ValueError, match="reg"):
            sp.complete_update(cs, mats, 0, bad)
    with pytest.raises(ValueError, match="rank"):
        sp.complete_update(
            cs, [torch.zeros(d, 65, dtype=torch.float64) for d in t.dims],
            0, REG)
    with pytest.raises(ValueError, match="hip"):
        sp.complete_update(cs, mats, 0, REG, impl="hip")   # CPU tensor

    t32 = sp.SpTensor.synthetic([20, 15, 25], 500, dtype=torch.float32,
                                seed=3)
    cs32 = sp.csf_alloc(t32, "all")
    m32 = [sp.seeded_init(d, 16, m, 1, dtype=torch.float32)
           for m, d in enumerate(t32.dims)]
    with pytest.raises(ValueError, match="float64"):
        sp.complete_update(cs32, m32, 0, REG)
    with pytest.raises(ValueError, match="float64"):
        sp.complete_als(t32, 4)

    two = sp.csf_alloc(t, "two")
    nonroot = [m for m in range(t.nmodes) if two.mode_depth[m] != 0]
    assert nonroot
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.complete_update(two, mats, nonroot[0], REG)
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.complete_als(two, 4)


# ------------------------------------------------------------ evaluation

def test_kruskal_predict_matches_dense():
    g = torch.Generator().manual_seed(5)
    dims = [12, 10, 14]
    factors = [torch.rand(d, 5, generator=g, dtype=torch.float64)
               for d in dims]
    lam = torch.rand(5, generator=g, dtype=torch.float64) + 0.5
    inds = torch.stack([torch.randint(0, d, (300,), generator=g)
                        for d in dims], 0)
    for lm in (None, lam):
        k = sp.Kruskal(factors=factors,
                       lam=torch.ones(5, dtype=torch.float64)
                       if lm is None else lm, fit=0.0, niters=0)
        dense = sp.kruskal_to_dense(k)
        want = dense[inds[0], inds[1], inds[2]]
        got = sp.kruskal_predict(factors, inds, lam=lm)
        assert (got - want).abs().max().item() < 1e-13
    t = sp.SpTensor(inds, want.clone(), dims)
    assert sp.rmse(factors, t) == pytest.approx(
        float((want - sp.kruskal_predict(factors, inds)).square().mean()
              .sqrt()))


# ------------------------------------------------------------------ driver

@functools.lru_cache(maxsize=None)
def planted():
    """Rank-4 60x50x70 tensor, 15% observed, noise 0.01; every tenth
    observation held out for validation. Returns (train, validate)."""
    g = torch.Generator().manual_seed(2024)
    dims = [60, 50, 70]
    A = [torch.rand(d, 4, generator=g, dtype=torch.float64) for d in dims]
    total = dims[0] * dims[1] * dims[2]
    pos = torch.randperm(total, generator=g)[: int(0.15 * total)]
    inds = torch.stack([pos // (dims[1] * dims[2]),
                        (pos // dims[2]) % dims[1], pos % dims[2]], 0)
    vals = (A[0][inds[0]] * A[1][inds[1]] * A[2][inds[2]]).sum(1)
    vals = vals + 0.01 * torch.randn(vals.numel(), generator=g,
                                     dtype=torch.float64)
    hold = torch.arange(vals.numel()) % 10 == 0
    train = sp.SpTensor(inds[:, ~hold].contiguous(), vals[~hold].clone(), dims)
    val = sp.SpTensor(inds[:, hold].contiguous(), vals[hold].clone(), dims)
    return train, val


PLANTED_OPTS = dict(max_iters=12, regularize=REG, tolerance=0.0, seed=77)


def val_rmse(factors, val):
    w = torch.ones(val.nnz, factors[0].shape[1], dtype=torch.float64)
    for m, A in enumerate(factors):
        w = w * A.cpu()[val.inds[m]]
    return float((val.vals - w.sum(1)).square().mean().sqrt())


@functools.lru_cache(maxsize=None)
def planted_oracle_rmse():
    """Final validation RMSE of 12 iterations of the oracle update from the
    same seeded_init start."""
    train, val = planted()
    factors = [sp.seeded_init(d, 4, m, PLANTED_OPTS["seed"])
               for m, d in enumerate(train.dims)]
    for _ in range(PLANTED_OPTS["max_iters"]):
        for m in range(3):
            factors[m] = oracle_update(train, factors, m, REG)
    return val_rmse(factors, val)


def check_planted_result(r, ref_rmse):
    assert r.niters == 12
    assert len(r.objective_trace) == len(r.rmse_train_trace) == 12
    assert len(r.rmse_val_trace) == 12
    obj = r.objective_trace
    print("objective:", " ".join(f"{x:.6e}" for x in obj))
    print("rmse-val :", " ".join(f"{x:.5f}" for x in r.rmse_val_trace))
    for a, b in zip(obj, obj[1:]):
        assert b <= a * (1 + 1e-10), (a, b)
    print(f"final val RMSE {r.rmse_val_trace[-1]:.6f} vs reference "
          f"{ref_rmse:.6f}")
    assert r.rmse_val_trace[-1] <= 1.05 * ref_rmse
    assert r.rmse_val_trace[r.best_iter] == min(r.rmse_val_trace)
    train, val = planted()
    assert val_rmse(r.factors, val) == pytest.approx(
        min(r.rmse_val_trace), rel=1e-9)


def test_complete_als_planted():
    train, val = planted()
    r = sp.complete_als(train, 4, sp.CompleteOptions(**PLANTED_OPTS),
                        validate=val)
    check_planted_result(r, planted_oracle_rmse())


def test_complete_als_stops_on_objective_without_validation():
    train, _ = planted()
    r = sp.complete_als(train, 4, sp.CompleteOptions(
        max_iters=40, regularize=REG, tolerance=1e-2, seed=77))
    assert 2 <= r.niters < 40
    assert r.rmse_val_trace == []
    assert r.best_iter == r.niters - 1
    obj = r.objective_trace
    assert (obj[-2] - obj[-1]) / obj[-2] < 1e-2


# --------------------------------------------------------------------- CLI

def test_cli_complete(tmp_path, capsys):
    from splatt_amd import cli
    train, val = planted()
    ptrain, pval = str(tmp_path / "train.tns"), str(tmp_path / "val.tns")
    train.save(ptrain)
    val.save(pval)
    outdir = tmp_path / "factors"
    rc = cli.main(["complete", ptrain, "--validate", pval, "--test", pval,
                   "-r", "4", "-i", "3", "--reg", "1e-2", "--tol", "0",
                   "--seed", "77", "--device", "cpu",
                   "--write", str(outdir)])
    assert rc == 0
    out = capsys.readouterr().out
    assert "Test RMSE:" in out and "its = 3" in out
    for m in range(3):
        path = outdir / f"mode{m + 1}.mat"
        assert os.path.exists(path)
        rows = open(path).read().strip().splitlines()
        assert len(rows[0].split()) == 4
