"""f32 value stream of the unstaged flat MTTKRP (v7 kernel, VS = float):
f64 tensors whose values are all f32-exact are narrowed once per CSF and
dispatched on a 4-byte value stream; factors and accumulation stay f64.

Tensors and the oracle follow tests/test_flat_stream_gpu.py: distinct
coordinates, csf_alloc(..., "all") (every mode a root dispatch of a
key-sorted stream), the CPU f64 stream oracle at 1e-8. Values are drawn as
(rand(f32) + 0.5).double(): the sum is formed in f32, so every value is
f32-exact by construction (rand(f32).double() + 0.5 is not: above 1 the f32
spacing is 2^-23 and rand's grid is 2^-24)."""
import functools
import importlib

import pytest
import torch

import splatt_amd as sp

mk = importlib.import_module("splatt_amd.mttkrp")

pytestmark = pytest.mark.gpu

DIMS3 = (40, 30, 50)
DIMS4 = (20, 15, 25, 10)
NNZ_BIG = 5003


def _decode(lin, dims):
    cols = []
    for d in reversed(dims):
        cols.append(lin % d)
        lin = lin // d
    return torch.stack(cols[::-1], 0)


@functools.lru_cache(maxsize=None)
def rand_tensor(dims, nnz, seed=5):
    """nnz DISTINCT coordinates, f32-exact f64 values in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed + nnz)
    total = 1
    for d in dims:
        total *= d
    lin = torch.randperm(total, generator=g)[:nnz]
    vals = (torch.rand(nnz, generator=g, dtype=torch.float32) + 0.5).double()
    assert torch.equal(vals.float().double(), vals)
    return sp.SpTensor(_decode(lin, list(dims)), vals, list(dims))


@functools.lru_cache(maxsize=None)
def mats_for(dims, rank):
    return tuple(sp.seeded_init(d, rank, m, 123) for m, d in enumerate(dims))


@functools.lru_cache(maxsize=None)
def oracle(dims, nnz, rank):
    t = rand_tensor(dims, nnz)
    return tuple(sp.mttkrp_stream(t, list(mats_for(dims, rank)), m)
                 for m in range(len(dims)))


def gpu_set(t):
    cs = sp.csf_alloc(t.to("cuda"), "all")
    assert all(getattr(c, "_stage", None) is None for c in cs.csfs)
    assert cs.mode_depth == [0] * t.nmodes
    return cs


def record(monkeypatch, name):
    """Record what a native entry point answers (None for void ones)."""
    nat = mk.native()
    orig, calls = getattr(nat, name), []

    def wrapped(*a):
        calls.append(orig(*a))
        return calls[-1]
    monkeypatch.setattr(nat, name, wrapped)
    return calls


def many_waves(monkeypatch):
    monkeypatch.setenv("SPLATT_SPAN_WAVES", "1000000")


# -------------------------------------------------------- plain dispatch
@pytest.mark.parametrize("force_rowptr", [False, True])
@pytest.mark.parametrize("rank", [8, 16, 32, 64])
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
@pytest.mark.parametrize("nnz", [1, 15, 31, 33, 1000, NNZ_BIG])
def test_plain_dispatch(monkeypatch, nnz, dims, rank, force_rowptr):
    many_waves(monkeypatch)
    if force_rowptr:
        monkeypatch.setattr(mk, "_ROWPTR_MIN_RUN", 0)
    ref = oracle(dims, nnz, rank)
    cs = gpu_set(rand_tensor(dims, nnz))
    mats_g = [m.cuda() for m in mats_for(dims, rank)]
    v32 = record(monkeypatch, "gpu_mttkrp_flat_v32")
    wide_rp = record(monkeypatch, "gpu_mttkrp_flat_rp")
    wide = record(monkeypatch, "gpu_mttkrp_flat")
    for mode in range(len(dims)):
        c = cs.csfs[cs.mode_csf[mode]]
        out = sp.mttkrp(cs, mats_g, mode)
        assert c._vals32.dtype == torch.float32
        err = (out.cpu() - ref[mode]).abs().max().item()
        print(f"nnz={nnz} dims={dims} rank={rank} mode={mode} "
              f"rowptr={mk.flat_rowptr_ok(c, 0, rank)} err={err:.3e}")
        assert err < 1e-8, (nnz, dims, rank, mode, err)
    # the f32 stream ran for every mode; the 8-byte stream never did
    assert v32 == [True] * len(dims)
    assert wide_rp == [] and wide == []


# ------------------------------------------------ rows-restricted launches
# mode-0 rows whose first stream position lands on phases 0, 1, 16, 31 of a
# 32-element window (and a few more), one row long enough for several waves
SDIMS = (50, 40, 50)
COUNTS = [32, 33, 47, 47, 1300, 5, 0, 0, 27] + [20 + (7 * r) % 40
                                                 for r in range(9, 47)]
COUNTS += [0] * (50 - len(COUNTS))


@functools.lru_cache(maxsize=None)
def structured():
    g = torch.Generator().manual_seed(99)
    rows, rest = [], []
    for r, n in enumerate(COUNTS):
        if n:
            rows.append(torch.full((n,), r, dtype=torch.long))
            rest.append(torch.randperm(SDIMS[1] * SDIMS[2], generator=g)[:n])
    i0, jk = torch.cat(rows), torch.cat(rest)
    inds = torch.stack([i0, jk // SDIMS[2], jk % SDIMS[2]], 0)
    perm = torch.randperm(inds.shape[1], generator=g)
    vals = (torch.rand(inds.shape[1], generator=g, dtype=torch.float32)
            + 0.5).double()
    t = sp.SpTensor(inds[:, perm].contiguous(), vals, list(SDIMS))
    mats = tuple(sp.seeded_init(d, 16, m, 123) for m, d in enumerate(SDIMS))
    ref = sp.mttkrp_stream(t, list(mats), 0)
    rowptr = [0]
    for n in COUNTS:
        rowptr.append(rowptr[-1] + n)
    return t, rowptr, mats, ref


@pytest.mark.parametrize("rowptr_env", ["1", "0"])
def test_rows_partition_sums_to_full(monkeypatch, rowptr_env):
    many_waves(monkeypatch)
    monkeypatch.setenv("SPLATT_FLAT_ROWPTR", rowptr_env)
    t, rowptr, mats, ref = structured()
    cs = gpu_set(t)
    mats_g = [m.cuda() for m in mats]
    v32 = record(monkeypatch, "gpu_mttkrp_flat_v32")
    cuts = [0, 1, 2, 3, 4, 5, 8, 9, 20, 21, 33, 50]
    phases = {rowptr[r] % 32 for r in cuts[:-1]}
    assert {0, 1, 16, 31} <= phases, sorted(phases)
    out = torch.full((SDIMS[0], 16), -7.25, dtype=torch.float64,
                     device="cuda")
    launched = 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sp.mttkrp(cs, mats_g, 0, out=out, rows=(lo, hi))
        launched += rowptr[hi] > rowptr[lo]
    assert v32 == [True] * launched     # slices of the copy stay co-aligned
    err = (out.cpu() - ref).abs().max().item()
    full = sp.mttkrp(cs, mats_g, 0)
    d = (out - full).abs().max().item()
    print(f"rows partition rowptr={rowptr_env} phases={sorted(phases)} "
          f"err={err:.3e} vs-full={d:.3e}")
    assert err < 1e-8 and d < 1e-10


# ------------------------------------------------------------ no narrowing
def _wide_runs(monkeypatch, cs, mats_g, ref, tol=1e-8, det=False):
    v32 = record(monkeypatch, "gpu_mttkrp_flat_v32")
    wide_rp = record(monkeypatch, "gpu_mttkrp_flat_rp")
    for mode in range(len(ref)):
        out = sp.mttkrp(cs, mats_g, mode)
        err = (out.double().cpu() - ref[mode]).abs().max().item()
        assert err < tol, (mode, err)
    assert v32 == []
    assert wide_rp == ([] if det else [True] * len(ref))


def test_inexact_value_keeps_the_wide_stream(monkeypatch):
    many_waves(monkeypatch)
    t = rand_tensor(DIMS3, NNZ_BIG)
    vals = t.vals.clone()
    vals[1234] = 0.1                      # not an f32 value
    t2 = sp.SpTensor(t.inds, vals, t.dims)
    mats = list(mats_for(DIMS3, 16))
    ref = [sp.mttkrp_stream(t2, mats, m) for m in range(3)]
    cs = gpu_set(t2)
    _wide_runs(monkeypatch, cs, [m.cuda() for m in mats], ref)
    assert all(c._vals32 is False for c in cs.csfs)


def test_env_disables(monkeypatch):
    many_waves(monkeypatch)
    monkeypatch.setenv("SPLATT_VALS32", "0")
    cs = gpu_set(rand_tensor(DIMS3, NNZ_BIG))
    mats_g = [m.cuda() for m in mats_for(DIMS3, 16)]
    _wide_runs(monkeypatch, cs, mats_g, oracle(DIMS3, NNZ_BIG, 16))
    assert all(getattr(c, "_vals32", None) is None for c in cs.csfs)


def test_f32_tensor_is_not_narrowed(monkeypatch):
    many_waves(monkeypatch)
    t = rand_tensor(DIMS3, NNZ_BIG)
    cs = gpu_set(sp.SpTensor(t.inds, t.vals.float(), t.dims))
    mats_g = [m.float().cuda() for m in mats_for(DIMS3, 16)]
    _wide_runs(monkeypatch, cs, mats_g, oracle(DIMS3, NNZ_BIG, 16), tol=2e-2)
    assert all(getattr(c, "_vals32", None) is None for c in cs.csfs)


def test_deterministic_is_not_narrowed(monkeypatch):
    many_waves(monkeypatch)
    monkeypatch.setenv("SPLATT_DETERMINISTIC", "1")
    cs = gpu_set(rand_tensor(DIMS3, NNZ_BIG))
    mats_g = [m.cuda() for m in mats_for(DIMS3, 16)]
    _wide_runs(monkeypatch, cs, mats_g, oracle(DIMS3, NNZ_BIG, 16), det=True)
    assert all(getattr(c, "_vals32", None) is None for c in cs.csfs)


def test_capture_without_an_answer_takes_the_wide_stream(monkeypatch):
    """No exactness check (a host sync) inside stream capture: a Csf that
    has not been dispatched yet runs the 8-byte stream in the graph."""
    many_waves(monkeypatch)
    cs = gpu_set(rand_tensor(DIMS3, NNZ_BIG))
    mats_g = [m.cuda() for m in mats_for(DIMS3, 16)]
    c0 = cs.csfs[cs.mode_csf[0]]
    for lvl in range(3):                  # every other cache of a dispatch
        c0.ancestor_expand(lvl)           # is built outside capture
    mk._root_rowptr(c0)
    mk._key_sorted(c0, 0)
    out = torch.empty(DIMS3[0], 16, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.mttkrp(cs, mats_g, 0, out=out)
    assert getattr(c0, "_vals32", None) is None
    g.replay()
    torch.cuda.synchronize()
    err = (out.cpu() - oracle(DIMS3, NNZ_BIG, 16)[0]).abs().max().item()
    assert err < 1e-8


# ------------------------------------------------------ storage accounting
def test_storage_bytes_counts_the_copy(monkeypatch):
    many_waves(monkeypatch)
    cs = gpu_set(rand_tensor(DIMS3, NNZ_BIG))
    mats_g = [m.cuda() for m in mats_for(DIMS3, 16)]
    monkeypatch.setenv("SPLATT_VALS32", "0")
    for mode in range(3):
        sp.mttkrp(cs, mats_g, mode)       # row pointers exist from here on
    before = cs.storage_bytes()
    monkeypatch.delenv("SPLATT_VALS32")
    for k, mode in enumerate(range(3)):
        sp.mttkrp(cs, mats_g, mode)
        assert cs.storage_bytes() == before + 4 * NNZ_BIG * (k + 1)
