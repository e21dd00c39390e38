"""Sparse Tucker: TTMc against a dense tensordot oracle (exact on integer
data, 1e-11 on float data), HOOI against a dense HOOI written here, the CLI.

The inputs, oracles and checks are shared with tests/test_tucker_gpu.py.
"""
import functools
import os

import pytest
import torch

import splatt_amd as sp
from splatt_amd import tucker

from test_complete import INPUTS, check_preconditions, four_mode

# max|delta| <= TOL * max(1, max|oracle|): the bound tests/test_admm.py uses
# for f64 sums of this length (two CPU evaluations differ by ~1e-14 relative)
TOL = 1e-11

RANKS3 = [(16, 16, 16), (32, 16, 32), (7, 5, 3), (17, 1, 9), (1, 1, 1)]
# the last one: P = 4096 = MAX_COLS for mode 0, 512 for the others
RANKS4 = [(4, 3, 5, 2), (16, 4, 4, 4), (2, 16, 16, 16)]
EXACT_CASES = ([("heavy", r) for r in RANKS3]
               + [("thin", (17, 1, 9))]
               + [("4-mode", r) for r in RANKS4])
# the 4-mode input takes the two 3-mode tuples with a fourth rank of 2
FLOAT_CASES = [(name, r) for name in ("heavy", "thin")
               for r in ((16, 16, 16), (7, 5, 3))] \
    + [("4-mode", (16, 16, 16, 2)), ("4-mode", (7, 5, 3, 2))]


def test_segment_length_keeps_preconditions():
    # check_preconditions() sizes `heavy` against completion.SEG
    from splatt_amd import completion
    assert tucker.SEG == completion.SEG <= 1024


# ------------------------------------------------------------------ inputs

@functools.lru_cache(maxsize=None)
def int_tensor(name):
    """The named input with small integer values."""
    t = INPUTS[name]()
    g = torch.Generator().manual_seed(5)
    vals = torch.randint(-3, 4, (t.nnz,), generator=g).double()
    return sp.SpTensor(t.inds.clone(), vals, list(t.dims))


@functools.lru_cache(maxsize=None)
def int_mats(name, ranks):
    t = INPUTS[name]()
    g = torch.Generator().manual_seed(11)
    return tuple(torch.randint(-2, 3, (d, r), generator=g).double()
                 for d, r in zip(t.dims, ranks))


@functools.lru_cache(maxsize=None)
def float_mats(name, ranks, seed=123):
    t = INPUTS[name]()
    return tuple(sp.seeded_init(d, r, m, seed)
                 for m, (d, r) in enumerate(zip(t.dims, ranks)))


# ------------------------------------------------------------------ oracle

def to_dense(t, dtype):
    X = torch.zeros(list(t.dims), dtype=dtype)
    X.index_put_(tuple(t.inds), t.vals.to(dtype), accumulate=True)
    return X


def dense_ttmc(X, mats, mode):
    """Contract every mode but `mode` of the dense X with its matrix: the
    result is [dims[mode], R_t1, .., R_tk], other modes ascending."""
    others = [m for m in range(X.dim()) if m != mode]
    axes = [mode] + others             # tensor mode held by each axis of Y
    Y = X.movedim(mode, 0)
    # smallest rank first: the cheapest order for the big first contraction
    for m in sorted(others, key=lambda m: mats[m].shape[1]):
        a = axes.index(m)
        Y = torch.tensordot(Y, mats[m].to(X.dtype), dims=([a], [0]))
        axes.append(axes.pop(a))
    return Y.permute([axes.index(m) for m in [mode] + others])


@functools.lru_cache(maxsize=None)
def dense_int(name):
    return to_dense(int_tensor(name), torch.int64)


@functools.lru_cache(maxsize=None)
def dense_float(name):
    return to_dense(INPUTS[name](), torch.float64)


@functools.lru_cache(maxsize=None)
def exact_oracle(name, ranks, mode):
    """int64; computed once per case, shared, never modified."""
    return dense_ttmc(dense_int(name), int_mats(name, ranks), mode)


@functools.lru_cache(maxsize=None)
def float_oracle(name, ranks, mode):
    return dense_ttmc(dense_float(name), float_mats(name, ranks), mode)


def assert_exact(got, name, ranks, mode, what):
    ref = exact_oracle(name, ranks, mode)
    assert ref.abs().max().item() < 2 ** 53
    assert got.dtype == torch.float64
    assert tuple(got.shape) == tuple(ref.shape), (what, name, ranks, mode)
    assert torch.equal(got.cpu(), ref.double()), (what, name, ranks, mode)


def assert_close(got, name, ranks, mode, what):
    ref = float_oracle(name, ranks, mode)
    assert tuple(got.shape) == tuple(ref.shape), (what, name, ranks, mode)
    err = (got.cpu() - ref).abs().max().item()
    bound = TOL * max(1.0, ref.abs().max().item())
    print(f"{what} {name} ranks {ranks} mode {mode}: max|delta| = {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound, (what, name, ranks, mode, err, bound)
    cnt = torch.bincount(INPUTS[name]().inds[mode],
                         minlength=INPUTS[name]().dims[mode])
    assert bool((got.cpu()[cnt == 0] == 0).all()), (what, name, ranks, mode)
    return err


# -------------------------------------------------------------------- TTMc

@pytest.mark.parametrize("name,ranks", EXACT_CASES)
def test_ttmc_torch_exact(name, ranks):
    check_preconditions(name)
    t = int_tensor(name)
    cs = sp.csf_alloc(t, "all")
    mats = list(int_mats(name, ranks))
    for mode in range(t.nmodes):
        got = sp.ttmc(cs, mats, mode, impl="torch")
        assert_exact(got, name, ranks, mode, "torch")


@pytest.mark.parametrize("name,ranks", FLOAT_CASES)
def test_ttmc_torch_float(name, ranks):
    t = INPUTS[name]()
    cs = sp.csf_alloc(t, "all")
    mats = list(float_mats(name, ranks))
    for mode in range(t.nmodes):
        got = sp.ttmc(cs, mats, mode)           # auto -> torch on CPU
        assert_close(got, name, ranks, mode, "torch")


def test_ttmc_layout_csf_and_out():
    t = four_mode()
    ranks = (4, 3, 5, 2)
    cs = sp.csf_alloc(t, "all")
    mats = list(float_mats("4-mode", ranks))
    for mode in range(4):
        want = (t.dims[mode],) + tuple(r for m, r in enumerate(ranks)
                                       if m != mode)
        got = sp.ttmc(cs, mats, mode)
        assert tuple(got.shape) == want
        # a single root-mode Csf works as well as the set
        one = sp.ttmc(cs.csfs[cs.mode_csf[mode]], mats, mode)
        assert torch.equal(one, got)
        out = torch.full(want, 3.0, dtype=torch.float64)
        ret = sp.ttmc(cs, mats, mode, out=out)
        assert ret is out
        assert torch.equal(out, got)
        # the matrix of the output mode is not read
        skip = list(mats)
        skip[mode] = None
        assert torch.equal(sp.ttmc(cs, skip, mode), got)


def test_ttmc_errors():
    t = four_mode()
    cs = sp.csf_alloc(t, "all")
    ranks = (4, 3, 5, 2)
    mats = list(float_mats("4-mode", ranks))
    with pytest.raises(ValueError, match="need 4 factor matrices"):
        sp.ttmc(cs, mats[:3], 0)
    bad = list(mats)
    bad[1] = torch.zeros(t.dims[1] + 1, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="shape"):
        sp.ttmc(cs, bad, 0)
    bad[1] = mats[1].float()
    with pytest.raises(ValueError, match="dtype"):
        sp.ttmc(cs, bad, 0)
    bad[1] = mats[1].to("meta")
    with pytest.raises(ValueError, match="device"):
        sp.ttmc(cs, bad, 0)
    for r in (0, 33):
        bad[1] = torch.zeros(t.dims[1], r, dtype=torch.float64)
        with pytest.raises(ValueError, match="rank"):
            sp.ttmc(cs, bad, 0)
    with pytest.raises(ValueError, match="hip"):
        sp.ttmc(cs, mats, 0, impl="hip")            # CPU tensor
    with pytest.raises(ValueError, match="unknown impl"):
        sp.ttmc(cs, mats, 0, impl="triton")
    with pytest.raises(ValueError, match="out must be"):
        sp.ttmc(cs, mats, 0, out=torch.zeros(t.dims[0], 30,
                                             dtype=torch.float64))
    with pytest.raises(IndexError):
        sp.ttmc(cs, mats, 4)

    t32 = sp.SpTensor.synthetic([20, 15, 25], 500, dtype=torch.float32,
                                seed=3)
    cs32 = sp.csf_alloc(t32, "all")
    m32 = [sp.seeded_init(d, 4, m, 1, dtype=torch.float32)
           for m, d in enumerate(t32.dims)]
    with pytest.raises(ValueError, match="float64"):
        sp.ttmc(cs32, m32, 0)
    with pytest.raises(ValueError, match="float64"):
        sp.tucker_hooi(t32, (2, 2, 2))

    two = sp.csf_alloc(t, "two")
    nonroot = [m for m in range(t.nmodes) if two.mode_depth[m] != 0]
    assert nonroot
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.ttmc(two, mats, nonroot[0])
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.tucker_hooi(two, ranks)


def test_tucker_hooi_errors():
    t = four_mode()                       # 20 x 15 x 25 x 12
    with pytest.raises(ValueError, match="need 4 ranks"):
        sp.tucker_hooi(t, (2, 2, 2))
    with pytest.raises(ValueError, match="rank of mode 0"):
        sp.tucker_hooi(t, (0, 2, 2, 2))
    with pytest.raises(ValueError, match="rank of mode 3"):
        sp.tucker_hooi(t, (2, 2, 2, 13))              # > dims[3]
    with pytest.raises(ValueError, match="rank of mode 0"):
        sp.tucker_hooi(t, (9, 2, 2, 2))               # > P_0 = 8
    with pytest.raises(ValueError, match="3..8 modes"):
        sp.tucker_hooi(sp.SpTensor.synthetic([9, 9], 30, seed=1), (2, 2))


# -------------------------------------------------------------------- HOOI

@functools.lru_cache(maxsize=None)
def planted():
    """Dense 12x10x14 tensor of multilinear rank (3,2,4), every entry
    stored. Returns (tensor, factors)."""
    g = torch.Generator().manual_seed(2025)
    dims, ranks = [12, 10, 14], [3, 2, 4]
    core = torch.randn(ranks, generator=g, dtype=torch.float64)
    U = [torch.linalg.qr(torch.randn(d, r, generator=g,
                                     dtype=torch.float64))[0]
         for d, r in zip(dims, ranks)]
    X = torch.einsum("abc,ia,jb,kc->ijk", core, *U)
    inds = torch.cartesian_prod(*[torch.arange(d) for d in dims]).T
    return (sp.SpTensor(inds.contiguous(), X.reshape(-1).clone(), dims),
            tuple(U))


PLANTED_OPTS = dict(max_iters=3, tol=0.0, seed=7)


def check_planted(r):
    t, U0 = planted()
    print("planted fit trace:", " ".join(f"{f:.12f}" for f in r.fit_trace))
    assert r.iters == 3 and len(r.fit_trace) == 3
    assert r.fit >= 1 - 1e-6
    assert tuple(r.core.shape) == (3, 2, 4)
    for m in range(3):
        U = r.factors[m].cpu()
        err = (U @ U.T - U0[m] @ U0[m].T).abs().max().item()
        print(f"planted mode {m}: projector error {err:.3e}")
        assert err <= 1e-8, (m, err)


def test_tucker_hooi_planted():
    t, _ = planted()
    assert t.nnz == 1680
    check_planted(sp.tucker_hooi(t, (3, 2, 4), sp.TuckerOptions(**PLANTED_OPTS)))


@functools.lru_cache(maxsize=None)
def small3():
    return sp.SpTensor.synthetic([50, 40, 60], 5000, seed=3)


RANDOM = {"small3": (small3, (8, 6, 7)), "4-mode": (four_mode, (4, 3, 5, 2))}
RANDOM_OPTS = dict(max_iters=8, tol=0.0, seed=31)


def reconstruct(core, factors):
    X = core
    for m, U in enumerate(factors):
        X = torch.tensordot(X, U, dims=([0], [1]))   # mode m -> last axis
    return X


@functools.lru_cache(maxsize=None)
def dense_hooi_trace(name):
    """Dense HOOI oracle: unfold, direct SVD of the unfolding, same init."""
    make, ranks = RANDOM[name]
    t = make()
    X = to_dense(t, torch.float64)
    nm = t.nmodes
    U = [torch.linalg.qr(sp.seeded_init(t.dims[m], ranks[m], m,
                                        RANDOM_OPTS["seed"]))[0]
         for m in range(nm)]
    xn2 = float(X.square().sum())
    trace = []
    for _ in range(RANDOM_OPTS["max_iters"]):
        for n in range(nm):
            Y = dense_ttmc(X, U, n).reshape(t.dims[n], -1)
            U[n] = torch.linalg.svd(Y, full_matrices=False)[0][:, :ranks[n]]
        G = U[nm - 1].T @ Y
        trace.append(1 - max(xn2 - float(G.square().sum()), 0.0) ** 0.5
                     / xn2 ** 0.5)
    return tuple(trace)


def check_random(r, name, tensor):
    """`r` from tucker_hooi on `name` with RANDOM_OPTS; everything is
    compared on the CPU."""
    _, ranks = RANDOM[name]
    ref = dense_hooi_trace(name)
    print(name, "fit trace:", " ".join(f"{f:.10f}" for f in r.fit_trace))
    assert r.iters == 8 and len(r.fit_trace) == 8
    dmax = max(abs(a - b) for a, b in zip(r.fit_trace, ref))
    print(f"{name}: max trace difference to the dense oracle {dmax:.3e}")
    assert dmax <= 1e-10
    for a, b in zip(r.fit_trace, r.fit_trace[1:]):
        assert b >= a - 1e-12, (a, b)
    assert r.fit == r.fit_trace[-1]
    assert tuple(r.core.shape) == tuple(ranks)
    for m, U in enumerate(r.factors):
        U = U.cpu()
        assert tuple(U.shape) == (tensor.dims[m], ranks[m])
        eye = torch.eye(ranks[m], dtype=torch.float64)
        assert (U.T @ U - eye).abs().max().item() <= 1e-12
    X = to_dense(tensor, torch.float64)
    Xh = reconstruct(r.core.cpu(), [U.cpu() for U in r.factors])
    fit = 1 - float((X - Xh).norm()) / float(X.norm())
    assert abs(fit - r.fit) <= 1e-10, (fit, r.fit)
    pred = r.predict(tensor.inds.to(r.core.device))
    assert pred.device == r.core.device
    want = Xh[tuple(tensor.inds)]
    assert (pred.cpu() - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", list(RANDOM))
def test_tucker_hooi_random(name):
    make, ranks = RANDOM[name]
    t = make()
    r = sp.tucker_hooi(t, ranks, sp.TuckerOptions(**RANDOM_OPTS))
    check_random(r, name, t)
    moved = r.to("cpu")
    assert torch.equal(moved.core, r.core) and moved.fit == r.fit


def test_tucker_hooi_stops_on_tolerance(capsys):
    t = small3()
    r = sp.tucker_hooi(t, (8, 6, 7), sp.TuckerOptions(
        max_iters=40, tol=1e-3, seed=31, verbosity=1))
    assert 2 <= r.iters < 40
    assert abs(r.fit_trace[-1] - r.fit_trace[-2]) < 1e-3
    assert f"its = {r.iters} fit = " in capsys.readouterr().out


# --------------------------------------------------------------------- CLI

def test_cli_tucker(tmp_path, capsys):
    from splatt_amd import cli
    t = small3()
    path = str(tmp_path / "t.tns")
    t.save(path)
    stem = str(tmp_path / "out") + os.sep
    rc = cli.main(["tucker", path, "-r", "8,6,7", "--iters", "3", "--tol",
                   "0", "--seed", "31", "--device", "cpu", "--stem", stem])
    assert rc == 0
    out = capsys.readouterr().out
    assert "its = 3 fit = " in out and "Final fit:" in out
    dims = sp.SpTensor.load(path).dims
    for m, r in enumerate((8, 6, 7)):
        rows = open(stem + f"mode{m + 1}.mat").read().strip().splitlines()
        assert len(rows) == dims[m]
        assert len(rows[0].split()) == r
    core = open(stem + "core.tns").read().strip().splitlines()
    assert len(core) == 8 * 6 * 7
    assert core[0].split()[:3] == ["1", "1", "1"]
    assert core[-1].split()[:3] == ["8", "6", "7"]
    # a rank list that does not fit the tensor is an error, not a crash
    assert cli.main(["tucker", path, "-r", "8,6", "--device", "cpu"]) == 1
