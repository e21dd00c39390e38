"""Paced strip MTTKRP (csrc/hip/mttkrp_strip.hip): one launch per dispatch,
its workgroups waiting for each other after each group of windows on a
counter in the CSF's pace words.

The layout is forced as in tests/test_strip_gpu.py (4-row strips, a
64-nonzero cap, 7-row windows, 3 workgroups), with 1, 3 and 8 groups of
windows (the window levels have 3 to 8 windows, so 8 reaches or exceeds the
window count): fewer strips than workgroups, a partial last pass, empty
groups and group edges inside a 32-nonzero line all occur. Values and
factors are small integers (f32-exact values) or small integers plus a
multiple of 2^-30 (f64 values): every product and partial sum is exact in
f64 — at most 33 bits of value, 2 bits per factor and 13 bits for 5003 terms
— so the result must be `torch.equal` to an int64 oracle whatever the order
of the adds. The random-input cases use the CPU f64 stream oracle at 1e-8.

The waits are for speed only, so they have nothing to fail on but the
counts: arrivals must be workgroups x passes x groups after every dispatch.
The time-out path is tested with a budget of 0 and in no other way."""
import functools
import importlib

import pytest
import torch

import splatt_amd as sp

mk = importlib.import_module("splatt_amd.mttkrp")

gpu = pytest.mark.gpu

DIMS3 = (40, 30, 50)
DIMS4 = (20, 15, 25, 10)
WGS = 3
SCALE = 1 << 30


def force(groups):
    return dict(strip_rows=4, strip_cap=64, strip_window=7, strip_wgs=WGS,
                strip_groups=groups)


def _decode(lin, dims):
    cols = []
    for d in reversed(dims):
        cols.append(lin % d)
        lin = lin // d
    return torch.stack(cols[::-1], 0)


@functools.lru_cache(maxsize=None)
def int_tensor(dims, nnz, exact):
    """nnz distinct coordinates; (tensor, values x 2^30 as int64). Values are
    1..4, f32-exact, or 1..4 + (1..3) x 2^-30, which f32 does not hold."""
    g = torch.Generator().manual_seed(17 + nnz)
    total = 1
    for d in dims:
        total *= d
    lin = torch.randperm(total, generator=g)[:nnz]
    iv = torch.randint(1, 5, (nnz,), generator=g) * SCALE
    if not exact:
        iv = iv + torch.randint(1, 4, (nnz,), generator=g)
    vals = iv.double() / SCALE
    assert torch.equal(vals.float().double(), vals) == exact
    return sp.SpTensor(_decode(lin, list(dims)), vals, list(dims)), iv


@functools.lru_cache(maxsize=None)
def int_mats(dims, rank):
    """factors of integers in [-2, 2], as int64"""
    g = torch.Generator().manual_seed(1000 + rank)
    return tuple(torch.randint(-2, 3, (d, rank), generator=g) for d in dims)


@functools.lru_cache(maxsize=None)
def int_oracle(dims, nnz, exact, rank):
    """per mode, the exact MTTKRP as f64, from int64 arithmetic"""
    t, iv = int_tensor(dims, nnz, exact)
    mats = int_mats(dims, rank)
    outs = []
    for mode in range(len(dims)):
        prod = iv.unsqueeze(1).expand(nnz, rank).clone()
        for m in range(len(dims)):
            if m != mode:
                prod *= mats[m][t.inds[m]]
        acc = torch.zeros(dims[mode], rank, dtype=torch.int64)
        acc.index_add_(0, t.inds[mode], prod)
        assert int(acc.abs().max()) < 2 ** 53
        outs.append(acc.double() / SCALE)
    return tuple(outs)


def strip_set(t, rank, groups):
    tg = t.to("cuda")
    nm = t.nmodes
    csfs = [sp.build_csf(tg, sp.order_modes(t.dims, "root", m),
                         flat_only=True, stage_rank=rank, **force(groups))
            for m in range(nm)]
    for c in csfs:
        st = c._strip
        assert st["tile_rows"] == 4 and st["wgs"] == WGS
        assert 1 <= st["groups"] <= groups
        assert st["pace"].numel() == 96 and st["pace"].is_cuda
    return sp.CsfSet(csfs, list(range(nm)), [0] * nm)


def expected_arrivals(c):
    st = c._strip
    ns = int(st["row0"].numel())
    grid = min(st["wgs"], ns)
    return grid * -(-ns // grid) * st["groups"]


def record(monkeypatch, name):
    nat = mk.native()
    orig, calls = getattr(nat, name), []

    def wrapped(*a):
        calls.append(orig(*a))
        return calls[-1]
    monkeypatch.setattr(nat, name, wrapped)
    return calls


def run_exact(cs, dims, nnz, exact, rank, label):
    """every mode against the int64 oracle; returns the pace statistics"""
    ref = int_oracle(dims, nnz, exact, rank)
    mats_g = [m.double().cuda() for m in int_mats(dims, rank)]
    stats = []
    for mode in range(len(dims)):
        c = cs.csfs[mode]
        out = sp.mttkrp(cs, mats_g, mode)
        v32 = getattr(c, "_vals32", None)
        assert (v32 is not False and v32 is not None) == exact
        diff = (out.cpu() - ref[mode]).abs().max().item()
        stats.append(sp.strip_pace_stats(c))
        print(f"{label} nnz={nnz} dims={dims} rank={rank} exact={exact} "
              f"mode={mode} strips={c._strip['row0'].numel()} "
              f"groups={c._strip['groups']} diff={diff:.3e} "
              f"pace={stats[-1]}")
        assert torch.equal(out.cpu(), ref[mode]), (nnz, dims, rank, mode, diff)
    return stats


# ------------------------------------------------------------------ groups
@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["vals32", "vals64"])
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
@pytest.mark.parametrize("nnz", [1, 31, 33, 1000, 5003])
@pytest.mark.parametrize("groups", [1, 3, 8])
def test_paced_groups_are_exact_and_arrivals_add_up(monkeypatch, groups, nnz,
                                                    dims, exact):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    t, _ = int_tensor(dims, nnz, exact)
    ran = record(monkeypatch, "mttkrp_strip_gpu")
    other = record(monkeypatch, "gpu_mttkrp_flat")
    for rank in (16, 32, 64):
        cs = strip_set(t, rank, groups)
        if groups == 8:
            # reaches or exceeds the window count of every window level
            assert all(c._strip["groups"] == c._strip["nbuckets"] <= 8
                       for c in cs.csfs)
        stats = run_exact(cs, dims, nnz, exact, rank, f"groups={groups}")
        for c, (arrivals, timeouts, _) in zip(cs.csfs, stats):
            assert arrivals == expected_arrivals(c)
            # the default budget (milliseconds) is far above any wait of
            # three resident workgroups (microseconds)
            assert timeouts == 0
    assert ran == [True] * (3 * len(dims)) and other == []


# --------------------------------------------------------------- heavy row
# tests/test_strip_gpu.py's case: one row holding most nonzeros (split over
# 20+ strips), empty rows inside strips, whole empty strips, an empty tail
HDIMS = (50, 40, 50)
HCOUNTS = [5, 0, 0, 9, 70, 1, 0, 1300, 33, 0, 2, 64] + [0] * 8 \
    + [20 + (7 * r) % 40 for r in range(20, 41)] + [0] * 9


@functools.lru_cache(maxsize=None)
def heavy():
    g = torch.Generator().manual_seed(99)
    rows, rest = [], []
    for r, n in enumerate(HCOUNTS):
        if n:
            rows.append(torch.full((n,), r, dtype=torch.long))
            rest.append(torch.randperm(HDIMS[1] * HDIMS[2], generator=g)[:n])
    i0, jk = torch.cat(rows), torch.cat(rest)
    inds = torch.stack([i0, jk // HDIMS[2], jk % HDIMS[2]], 0)
    perm = torch.randperm(inds.shape[1], generator=g)
    vals = torch.rand(inds.shape[1], generator=g, dtype=torch.float64) + 0.5
    t = sp.SpTensor(inds[:, perm].contiguous(), vals, list(HDIMS))
    mats = tuple(sp.seeded_init(d, 16, m, 123) for m, d in enumerate(HDIMS))
    return t, mats, sp.mttkrp_stream(t, list(mats), 0)


@gpu
@pytest.mark.parametrize("groups", [1, 3, 8])
def test_heavy_row_twice_into_a_dirty_buffer(monkeypatch, groups):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    assert len(HCOUNTS) == HDIMS[0]
    t, mats, ref = heavy()
    cs = strip_set(t, 16, groups)
    c = cs.csfs[0]
    shared = int(((c._strip["flags"] & 2) != 0).sum())
    assert shared >= 1300 // 64
    mats_g = [m.cuda() for m in mats]
    ran = record(monkeypatch, "mttkrp_strip_gpu")
    # the caller's zeroing is the only thing that clears `out`
    out = torch.full((HDIMS[0], 16), -7.25, dtype=torch.float64,
                     device="cuda")
    errs = []
    for _ in range(2):                      # must not accumulate
        sp.mttkrp(cs, mats_g, 0, out=out)
        errs.append((out.cpu() - ref).abs().max().item())
        assert sp.strip_pace_stats(c)[0] == expected_arrivals(c)
    print(f"heavy row groups={groups}: shared strips={shared} errs={errs}")
    assert max(errs) < 1e-8
    assert ran == [True, True]
    empty = [r for r, n in enumerate(HCOUNTS) if n == 0]
    assert (out[empty] == 0).all()


# ------------------------------------------------------------------- knobs
@gpu
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
def test_budget_zero_gives_up_and_stays_exact(monkeypatch, dims):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.setenv("SPLATT_STRIP_PACE_US", "0")
    t, _ = int_tensor(dims, 5003, False)
    cs = strip_set(t, 16, 3)
    stats = run_exact(cs, dims, 5003, False, 16, "budget=0")
    for c, (arrivals, timeouts, longest) in zip(cs.csfs, stats):
        # an unmet wait gives up at once and the workgroup stops waiting, so
        # there is at most one time-out per workgroup; it goes on arriving
        assert arrivals == expected_arrivals(c)
        assert timeouts <= min(WGS, int(c._strip["row0"].numel()))
        assert timeouts <= arrivals
        assert longest < 1000.0


@gpu
def test_pace_off_leaves_the_pace_words_alone(monkeypatch):
    monkeypatch.setenv("SPLATT_STRIP_PACE", "0")
    t, _ = int_tensor(DIMS3, 5003, True)
    cs = strip_set(t, 16, 3)
    for c in cs.csfs:
        c._strip["pace"].fill_(0x5A5A)
    ref = int_oracle(DIMS3, 5003, True, 16)
    mats_g = [m.double().cuda() for m in int_mats(DIMS3, 16)]
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        assert torch.equal(out.cpu(), ref[mode])
        assert (cs.csfs[mode]._strip["pace"] == 0x5A5A).all()


@gpu
def test_graph_replay_counts_one_dispatch(monkeypatch):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    t, _ = int_tensor(DIMS3, 5003, True)
    cs = strip_set(t, 16, 3)
    c = cs.csfs[0]
    mats_g = [m.cuda() for m in
              (sp.seeded_init(d, 16, m, 123) for m, d in enumerate(DIMS3))]
    eager = sp.mttkrp(cs, mats_g, 0).clone()   # also settles every cache
    ran = record(monkeypatch, "mttkrp_strip_gpu")
    out = torch.full((DIMS3[0], 16), 3.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.mttkrp(cs, mats_g, 0, out=out)
    assert ran == [True]
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    d = (out - eager).abs().max().item()
    arrivals, timeouts, longest = sp.strip_pace_stats(c)
    print(f"graph replay vs-eager={d:.3e} pace={(arrivals, timeouts, longest)}")
    assert d < 1e-12
    assert arrivals == expected_arrivals(c)    # of ONE dispatch, not three


# ----------------------------------------------------------------- binding
def _binding_args(dev):
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    return [z(8, i32), [z(8, i32), z(8, i32)],
            [torch.ones(4, 16, dtype=f64, device=dev) for _ in range(2)],
            torch.ones(8, dtype=f64, device=dev), z(1, i32),
            torch.ones(1, dtype=i32, device=dev), z(1, i32),
            torch.tensor([[0, 8]], dtype=i64, device=dev), 4, 1,
            z(64, f64).view(4, 16), 0]


@gpu
def test_binding_checks_the_pace_tensor():
    nat = mk.native()
    z = lambda n, dt, dev="cuda": torch.zeros(n, dtype=dt, device=dev)
    with pytest.raises(RuntimeError, match="pace has dtype Short"):
        nat.mttkrp_strip_gpu(*_binding_args("cuda"), z(96, torch.int16), 100)
    with pytest.raises(RuntimeError, match="pace must be a device tensor"):
        nat.mttkrp_strip_gpu(*_binding_args("cuda"),
                             z(96, torch.int32, "cpu"), 100)
    with pytest.raises(RuntimeError, match="at least 96 words"):
        nat.mttkrp_strip_gpu(*_binding_args("cuda"), z(95, torch.int32), 100)
    with pytest.raises(RuntimeError, match="pace must be contiguous"):
        nat.mttkrp_strip_gpu(*_binding_args("cuda"),
                             z(192, torch.int32)[::2], 100)
    with pytest.raises(RuntimeError, match="pace_us out of range"):
        nat.mttkrp_strip_gpu(*_binding_args("cuda"), z(96, torch.int32), -1)
    # both word types, and the twelve-argument form, are accepted
    for pace in (z(96, torch.int32), z(96, torch.int32).view(torch.uint32)):
        args = _binding_args("cuda")
        assert nat.mttkrp_strip_gpu(*args, pace, 100)
        torch.cuda.synchronize()
        assert int(pace.view(torch.int32)[0]) == 1      # 1 wg, 1 pass, 1 group
        assert torch.equal(args[10].cpu()[0], torch.full((16,), 8.0,
                                                        dtype=torch.float64))
    assert nat.mttkrp_strip_gpu(*_binding_args("cuda"))
    torch.cuda.synchronize()
