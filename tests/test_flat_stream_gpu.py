"""Unstaged flat MTTKRP: full-line stream staging (v7 kernel) and the
row-pointer root dispatch, against the CPU f64 stream oracle.

Tensors are built directly (distinct coordinates, exact structure) and
allocated with csf_alloc(..., "all"), so every mode is a root dispatch of
a key-sorted stream."""
import functools
import importlib

import pytest
import torch

import splatt_amd as sp

mk = importlib.import_module("splatt_amd.mttkrp")   # sp.mttkrp is the function

pytestmark = pytest.mark.gpu

DIMS3 = [40, 30, 50]
DIMS4 = [20, 15, 25, 10]
NNZ_BIG = 5003          # not a multiple of 32; spans ~20 waves at span 256


def _decode(lin, dims):
    cols = []
    for d in reversed(dims):
        cols.append(lin % d)
        lin = lin // d
    return torch.stack(cols[::-1], 0)


@functools.lru_cache(maxsize=None)
def rand_tensor(dims, nnz, seed=5):
    """nnz DISTINCT coordinates, f64 values in [0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed + nnz)
    total = 1
    for d in dims:
        total *= d
    lin = torch.randperm(total, generator=g)[:nnz]
    vals = torch.rand(nnz, generator=g, dtype=torch.float64) + 0.5
    return sp.SpTensor(_decode(lin, list(dims)), vals, list(dims))


@functools.lru_cache(maxsize=None)
def mats_for(dims, rank):
    return tuple(sp.seeded_init(d, rank, m, 123) for m, d in enumerate(dims))


@functools.lru_cache(maxsize=None)
def oracle(dims, nnz, rank, seed=5):
    t = rand_tensor(dims, nnz, seed)
    return tuple(sp.mttkrp_stream(t, list(mats_for(dims, rank)), m)
                 for m in range(len(dims)))


def gpu_set(t):
    cs = sp.csf_alloc(t.to("cuda"), "all")
    assert all(getattr(c, "_stage", None) is None for c in cs.csfs)
    assert cs.mode_depth == [0] * t.nmodes
    return cs


@functools.lru_cache(maxsize=None)
def gpu_rand_set(dims, nnz):
    return gpu_set(rand_tensor(dims, nnz))


def record_rp(monkeypatch):
    """Record what the row-pointer entry point answers (True = launched)."""
    nat = mk.native()
    orig, calls = nat.gpu_mttkrp_flat_rp, []

    def wrapped(*a):
        calls.append(orig(*a))
        return calls[-1]
    monkeypatch.setattr(nat, "gpu_mttkrp_flat_rp", wrapped)
    return calls


def many_waves(monkeypatch):
    # span = max(256, nnz / waves): the 256 minimum, so NNZ_BIG is ~20 waves
    monkeypatch.setenv("SPLATT_SPAN_WAVES", "1000000")


# ------------------------------------------------------ head / tail sizes
@pytest.mark.parametrize("force_rowptr", [False, True])
@pytest.mark.parametrize("rank", [8, 16, 32])
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
@pytest.mark.parametrize("nnz", [1, 15, 31, 33, 1000, NNZ_BIG])
def test_tail_sizes(monkeypatch, nnz, dims, rank, force_rowptr):
    """force_rowptr drops the run-length gate so the small tensors, mostly
    empty rows and 1-nnz runs, also walk the row-pointer kernel."""
    many_waves(monkeypatch)
    if force_rowptr:
        monkeypatch.setattr(mk, "_ROWPTR_MIN_RUN", 0)
    dims = tuple(dims)
    ref = oracle(dims, nnz, rank)
    cs = gpu_rand_set(dims, nnz)
    mats_g = [m.cuda() for m in mats_for(dims, rank)]
    for mode in range(len(dims)):
        c = cs.csfs[cs.mode_csf[mode]]
        if force_rowptr:
            assert mk.flat_rowptr_ok(c, 0, rank)
        out = sp.mttkrp(cs, mats_g, mode)
        err = (out.cpu() - ref[mode]).abs().max().item()
        print(f"nnz={nnz} dims={dims} rank={rank} mode={mode} "
              f"rowptr={mk.flat_rowptr_ok(c, 0, rank)} err={err:.3e}")
        assert err < 1e-8, (nnz, dims, rank, mode, err)


def test_f32(monkeypatch):
    """test_gpu_mttkrp_f32's recipe: f32 tensor and factors vs the f64
    oracle at 2e-2."""
    many_waves(monkeypatch)
    dims = tuple(DIMS3)
    t = rand_tensor(dims, NNZ_BIG)
    t32 = sp.SpTensor(t.inds, t.vals.float(), t.dims)
    ref = oracle(dims, NNZ_BIG, 16)
    cs = gpu_set(t32)
    mats_g = [m.float().cuda() for m in mats_for(dims, 16)]
    for rowptr in ("1", "0"):
        monkeypatch.setenv("SPLATT_FLAT_ROWPTR", rowptr)
        for mode in range(3):
            out = sp.mttkrp(cs, mats_g, mode)
            err = (out.double().cpu() - ref[mode]).abs().max().item()
            print(f"f32 rowptr={rowptr} mode={mode} err={err:.3e}")
            assert err < 2e-2, (rowptr, mode, err)


# --------------------------------------------- structured rows (mode 0)
# row:      0  1   2   3   4  5  6  7..9  10    11..46   47..49
# nnz:      0  33  31  10  1  1  1  0     1300  20..59   0
# rowptr:   0  0   33  64  74 75 76 77    77    1377 ...
SDIMS = (50, 40, 50)


@functools.lru_cache(maxsize=None)
def structured():
    g = torch.Generator().manual_seed(99)
    counts = [0] * 50
    counts[1], counts[2], counts[3] = 33, 31, 10
    counts[4] = counts[5] = counts[6] = 1
    counts[10] = 1300                       # > 4 x 256: several waves
    for r in range(11, 47):
        counts[r] = 20 + int(torch.randint(0, 40, (1,), generator=g))
    rows, rest = [], []
    for r, n in enumerate(counts):
        if n:
            rows.append(torch.full((n,), r, dtype=torch.long))
            rest.append(torch.randperm(SDIMS[1] * SDIMS[2], generator=g)[:n])
    i0 = torch.cat(rows)
    jk = torch.cat(rest)
    inds = torch.stack([i0, jk // SDIMS[2], jk % SDIMS[2]], 0)
    perm = torch.randperm(inds.shape[1], generator=g)   # unsorted input
    vals = torch.rand(inds.shape[1], generator=g, dtype=torch.float64) + 0.5
    t = sp.SpTensor(inds[:, perm].contiguous(), vals, list(SDIMS))
    rowptr = torch.zeros(51, dtype=torch.long)
    rowptr[1:] = torch.tensor(counts).cumsum(0)
    mats = tuple(sp.seeded_init(d, 16, m, 123) for m, d in enumerate(SDIMS))
    ref = tuple(sp.mttkrp_stream(t, list(mats), m) for m in range(3))
    return t, rowptr, mats, ref


def test_rowptr_edge_cases(monkeypatch):
    many_waves(monkeypatch)
    t, rowptr, mats, ref = structured()
    cs = gpu_set(t)
    mats_g = [m.cuda() for m in mats]
    c0 = cs.csfs[cs.mode_csf[0]]
    assert t.nnz >= 32 * SDIMS[0]
    assert mk.flat_rowptr_ok(c0, 0, 16)
    out = sp.mttkrp(cs, mats_g, 0).cpu()
    assert torch.equal(mk._root_rowptr(c0).cpu(), rowptr)
    err = (out - ref[0]).abs().max().item()
    print(f"structured mode 0 err={err:.3e}")
    assert err < 1e-8
    for r in (0, 7, 8, 9, 47, 48, 49):
        assert torch.all(out[r] == 0.0), r
    for mode in (1, 2):
        o = sp.mttkrp(cs, mats_g, mode).cpu()
        assert (o - ref[mode]).abs().max().item() < 1e-8, mode


def test_sparse_runs_take_key_path(monkeypatch):
    many_waves(monkeypatch)
    dims = tuple(DIMS3)
    t = rand_tensor(dims, 900)
    ref = oracle(dims, 900, 16)
    cs = gpu_set(t)
    mats_g = [m.cuda() for m in mats_for(dims, 16)]
    for mode in range(3):
        c = cs.csfs[cs.mode_csf[mode]]
        assert t.nnz < 32 * dims[mode]
        assert not mk.flat_rowptr_ok(c, 0, 16)
        out = sp.mttkrp(cs, mats_g, mode)
        assert getattr(c, "_rowptr", None) is None
        assert (out.cpu() - ref[mode]).abs().max().item() < 1e-8, mode
    big = gpu_set(rand_tensor(dims, NNZ_BIG))
    for mode in range(3):
        assert mk.flat_rowptr_ok(big.csfs[big.mode_csf[mode]], 0, 16)
    monkeypatch.setenv("SPLATT_FLAT_ROWPTR", "0")
    assert not mk.flat_rowptr_ok(big.csfs[big.mode_csf[0]], 0, 16)


# ---------------------------------------------------- misaligned launches
@pytest.mark.parametrize("rowptr_env", ["1", "0"])
@pytest.mark.parametrize("lo,hi,phase", [
    (2, 40, "odd"),         # p0 = 33
    (4, 30, "even"),        # p0 = 74
    (3, 47, "aligned"),     # p0 = 64
    (11, 12, "odd"),        # p0 = 1377, one short row
    (10, 11, "odd"),        # p0 = 77: the 1300-nnz row alone
])
def test_misaligned_rows(monkeypatch, lo, hi, phase, rowptr_env):
    many_waves(monkeypatch)
    monkeypatch.setenv("SPLATT_FLAT_ROWPTR", rowptr_env)
    t, rowptr, mats, ref = structured()
    cs = gpu_set(t)
    mats_g = [m.cuda() for m in mats]
    c0 = cs.csfs[cs.mode_csf[0]]
    calls = record_rp(monkeypatch)
    p0, p1 = mk._key_bounds(c0, 0, lo, hi)
    assert (p0, p1) == (int(rowptr[lo]), int(rowptr[hi]))
    assert {"odd": p0 % 2 == 1,
            "even": p0 % 2 == 0 and p0 % 32 != 0,
            "aligned": p0 % 32 == 0}[phase]
    sentinel = -7.25
    out = torch.full((SDIMS[0], 16), sentinel, dtype=torch.float64,
                     device="cuda")
    sp.mttkrp(cs, mats_g, 0, out=out, rows=(lo, hi))
    # slices of one allocation stay co-aligned: the launch is not declined
    assert calls == ([True] if rowptr_env == "1" else [])
    out = out.cpu()
    err = (out[lo:hi] - ref[0][lo:hi]).abs().max().item()
    print(f"rows=({lo},{hi}) p0={p0} rowptr={rowptr_env} err={err:.3e}")
    assert err < 1e-8
    assert torch.all(out[:lo] == sentinel) and torch.all(out[hi:] == sentinel)


# ------------------------------------------------------ build equivalence
def _all_modes(cs, mats_g, n):
    return [sp.mttkrp(cs, mats_g, m).clone() for m in range(n)]


@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
def test_levers_equivalent(monkeypatch, dims):
    many_waves(monkeypatch)
    dims = tuple(dims)
    cs = gpu_rand_set(dims, NNZ_BIG)
    mats_g = [m.cuda() for m in mats_for(dims, 16)]
    calls = record_rp(monkeypatch)
    base = _all_modes(cs, mats_g, len(dims))
    monkeypatch.setenv("SPLATT_FLAT_ROWPTR", "0")
    key7 = _all_modes(cs, mats_g, len(dims))
    monkeypatch.delenv("SPLATT_FLAT_ROWPTR")
    monkeypatch.setenv("SPLATT_MTTKRP_U", "1")
    v2 = _all_modes(cs, mats_g, len(dims))
    # default: launched; key lever: not asked; v2 lever: asked and declined
    assert calls == [True] * len(dims) + [False] * len(dims)
    for m in range(len(dims)):
        d1 = (base[m] - key7[m]).abs().max().item()
        d2 = (base[m] - v2[m]).abs().max().item()
        print(f"dims={dims} mode={m} rowptr-vs-key={d1:.3e} vs-v2={d2:.3e}")
        assert d1 < 1e-10 and d2 < 1e-10, (m, d1, d2)


def test_retired_lever_value_is_unset(monkeypatch):
    """SPLATT_MTTKRP_U=8 once selected a kernel that is gone (and made the
    row-pointer launch decline); every value but 1 now means unset."""
    many_waves(monkeypatch)
    dims = tuple(DIMS3)
    cs = gpu_rand_set(dims, NNZ_BIG)
    mats_g = [m.cuda() for m in mats_for(dims, 16)]
    base = _all_modes(cs, mats_g, 3)
    calls = record_rp(monkeypatch)
    monkeypatch.setenv("SPLATT_MTTKRP_U", "8")
    u8 = _all_modes(cs, mats_g, 3)
    assert calls == [True] * 3
    for m in range(3):
        d = (base[m] - u8[m]).abs().max().item()
        print(f"mode={m} unset-vs-U8={d:.3e}")
        assert d < 1e-10, (m, d)


@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16])
def test_factor_store(monkeypatch, store):
    """Same gathered values, f64 accumulation: only the staging differs."""
    many_waves(monkeypatch)
    dims = tuple(DIMS3)
    cs = gpu_rand_set(dims, NNZ_BIG)
    mats_g = [m.cuda().to(store) for m in mats_for(dims, 16)]
    new = _all_modes(cs, mats_g, 3)
    monkeypatch.setenv("SPLATT_FLAT_ROWPTR", "0")
    key7 = _all_modes(cs, mats_g, 3)
    monkeypatch.setenv("SPLATT_MTTKRP_U", "1")
    v2 = _all_modes(cs, mats_g, 3)
    for m in range(3):
        assert new[m].dtype == torch.float64
        d1 = (new[m] - v2[m]).abs().max().item()
        d2 = (key7[m] - v2[m]).abs().max().item()
        print(f"store={store} mode={m} rowptr-vs-v2={d1:.3e} key-vs-v2={d2:.3e}")
        assert d1 < 1e-10 and d2 < 1e-10, (m, d1, d2)


# ------------------------------------------------------------ graph replay
def test_graph_replay(monkeypatch):
    many_waves(monkeypatch)
    dims = tuple(DIMS3)
    cs = gpu_rand_set(dims, NNZ_BIG)
    mats_g = [m.cuda() for m in mats_for(dims, 16)]
    c0 = cs.csfs[cs.mode_csf[0]]
    assert mk.flat_rowptr_ok(c0, 0, 16)
    out = torch.empty(dims[0], 16, dtype=torch.float64, device="cuda")
    eager = sp.mttkrp(cs, mats_g, 0, out=out).clone()   # builds the caches
    assert getattr(c0, "_rowptr", None) is not None
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.mttkrp(cs, mats_g, 0, out=out)
    for _ in range(2):
        out.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        d = (out - eager).abs().max().item()
        print(f"graph replay diff={d:.3e}")
        assert d < 1e-10
