"""Strip/window MTTKRP (csrc/hip/mttkrp_strip.hip): root output kept in LDS
tiles over a stream sorted by (strip, window of one gathered level).

The planner, the layout and the gate are checked on the CPU. The kernel
tests follow tests/test_flat_vals32_gpu.py: distinct coordinates, the CPU f64
stream oracle at 1e-8. The layout is forced through the build_csf parameters
with 4-row strips, a 64-nonzero strip cap, 7-row windows and 3 workgroups per
launch: many strips, several passes, partial 32-nonzero windows at both ends
of a strip, strips of one row and rows split over several strips."""
import functools
import importlib

import pytest
import torch

import splatt_amd as sp
from splatt_amd.csf import strip_gate, strip_layout

mk = importlib.import_module("splatt_amd.mttkrp")

gpu = pytest.mark.gpu

DIMS3 = (40, 30, 50)
DIMS4 = (20, 15, 25, 10)
FORCE = dict(strip_rows=4, strip_cap=64, strip_window=7, strip_wgs=3,
             strip_groups=3)


# ------------------------------------------------------------------ planner
def _check_plan(rowptr, tile_rows, cap):
    s = mk.native().plan_strips(torch.tensor(rowptr, dtype=torch.int64),
                                tile_rows, cap)
    row0, nrows, flags = (s[k].tolist() for k in ("row0", "nrows", "flags"))
    p0, p1 = s["p0"].tolist(), s["p1"].tolist()
    ns = len(row0)
    # every nonzero in exactly one strip, in stream order
    assert p0[0] == 0 and p1[-1] == rowptr[-1]
    assert all(p1[i] == p0[i + 1] for i in range(ns - 1))
    nr = len(rowptr) - 1
    owners = [0] * nr
    for i in range(ns):
        assert 1 <= nrows[i] <= tile_rows
        assert 0 <= p1[i] - p0[i] <= cap
        last = row0[i] + nrows[i] - 1
        # the stream range lies inside the strip's rows
        assert rowptr[row0[i]] <= p0[i] and p1[i] <= rowptr[last + 1]
        for r in range(row0[i], last + 1):
            owners[r] += 1
        # a strip starts inside a row iff bit 0, ends inside one iff bit 1
        assert bool(flags[i] & 1) == (p0[i] > rowptr[row0[i]])
        assert bool(flags[i] & 2) == (p1[i] < rowptr[last + 1])
        if flags[i] & 1:
            assert i > 0 and flags[i - 1] & 2 \
                and row0[i - 1] + nrows[i - 1] - 1 == row0[i]
        if flags[i] & 2:
            assert i + 1 < ns and flags[i + 1] & 1 and row0[i + 1] == last
    # every row is in a strip; only rows heavier than the cap are shared
    for r in range(nr):
        assert owners[r] >= 1
        if owners[r] > 1:
            assert rowptr[r + 1] - rowptr[r] > cap
    return s


def test_planner_caps_and_shared_rows():
    counts = [3, 0, 0, 70, 64, 65, 1, 0, 500, 0, 0, 0, 0, 0, 2, 63, 1, 1, 1,
              1, 1, 0]
    rowptr = [0]
    for n in counts:
        rowptr.append(rowptr[-1] + n)
    s = _check_plan(rowptr, 4, 64)
    # the 500-nonzero row spans ceil(500/64) strips
    assert sum(1 for r, n in zip(s["row0"].tolist(), s["nrows"].tolist())
               if r <= 8 < r + n) == 8
    _check_plan(rowptr, 1, 64)
    _check_plan(rowptr, 1000, 1)
    _check_plan(rowptr, 1000, 10 ** 9)
    _check_plan([0, 0, 0], 4, 64)
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        c = torch.randint(0, 40, (57,), generator=g)
        c[torch.randint(0, 57, (1,), generator=g)] = 900
        rp = [0] + torch.cumsum(c, 0).tolist()
        _check_plan(rp, 5, 97)


def test_layout_is_sorted_by_strip_window_row():
    g = torch.Generator().manual_seed(11)
    nrows, wdim, nnz = 37, 45, 3000
    root = torch.sort(torch.randint(0, nrows, (nnz,), generator=g)).values
    root[500:1400] = 9                     # one heavy row
    root = torch.sort(root).values
    widx = torch.randint(0, wdim, (nnz,), generator=g)
    strips, order = strip_layout(root, widx, nrows, wdim, 4, 64, 7, groups=3)
    # launch groups cut every strip at the same window boundaries
    nb, bounds = strips["nbuckets"], strips["bounds"]
    assert nb == 7 and tuple(bounds.shape) == (strips["p0"].numel(), 4)
    assert torch.equal(bounds[:, 0], strips["p0"])
    assert torch.equal(bounds[:, 3], strips["p1"])
    swin_all = widx[order] // 7
    for row in bounds.tolist():
        for g in range(3):
            seg = swin_all[row[g]:row[g + 1]]
            assert row[g] <= row[g + 1]
            assert ((seg >= -(-g * nb // 3)) & (seg < -(-(g + 1) * nb // 3))).all()
    assert torch.equal(torch.sort(order).values, torch.arange(nnz))
    sroot, swin = root[order], widx[order] // 7
    last = None
    for p0, p1, r0, n in zip(strips["p0"].tolist(), strips["p1"].tolist(),
                             strips["row0"].tolist(),
                             strips["nrows"].tolist()):
        # the sort moves nonzeros inside their strip only
        assert torch.equal(torch.sort(order[p0:p1]).values,
                           torch.arange(p0, p1))
        assert ((sroot[p0:p1] >= r0) & (sroot[p0:p1] < r0 + n)).all()
        key = swin[p0:p1] * nrows + sroot[p0:p1]
        assert (key[1:] >= key[:-1]).all()
        # stable: equal (window, row) keep their stream order
        same = key[1:] == key[:-1]
        assert (order[p0:p1][1:][same] > order[p0:p1][:-1][same]).all()
        assert last is None or p0 == last
        last = p1
    assert last == nnz


# --------------------------------------------------------------------- gate
AMAZON = ([4_821_207, 1_774_269, 1_805_187], 1_741_809_018, 16)
NELL2 = ([12092, 9184, 28818], 76_879_419, 16)
NETFLIX = ([480_189, 17_770, 2182], 100_480_507, 32)
DELICIOUS = ([532_924, 17_262_471, 2_480_308, 1443], 140_126_181, 32)


def _roots(dims):
    for m in range(len(dims)):
        yield m, [m] + sorted((x for x in range(len(dims)) if x != m),
                              key=lambda x: dims[x])


def test_gate_selects_amazon_only():
    dims, nnz, rank = AMAZON
    for m, perm in _roots(dims):
        got = strip_gate(dims, perm, nnz, rank)
        assert got is not None, m
        assert got["tile_rows"] == 1024 and got["window_rows"] == 8192
        assert dims[perm[got["level"]]] >= 4 * (4 << 20) // (rank * 8)
        assert got["lines_strip"] <= 0.8 * got["lines_v7"]
        # the model figures of docs/KERNELS.md
        want = 1.27 if m == 0 else 1.19
        assert abs(got["lines_strip"] - want) < 0.02, (m, got)
        assert abs(got["lines_v7"] - 2.09) < 0.01
        assert strip_gate(dims, perm, nnz, 0) is None
    for dims, nnz, rank in (NELL2, NETFLIX, DELICIOUS):
        for m, perm in _roots(dims):
            assert strip_gate(dims, perm, nnz, rank) is None, (dims, m)
            assert strip_gate(dims, perm, nnz, 0) is None


def test_gate_leaves_factors_under_four_l2_alone():
    # every gathered factor just under 4x the 4 MiB L2 at rank 16
    d = 4 * (4 << 20) // (16 * 8) - 1
    for root in (10 ** 6, 10 ** 7):
        assert strip_gate([root, d, d], [0, 1, 2], 10 ** 9, 16) is None
    assert strip_gate([10 ** 6, d + 1, d], [0, 1, 2], 10 ** 9, 16) is not None
    for dims in (DIMS3, DIMS4, (1200, 900, 1500)):
        for m, perm in _roots(dims):
            assert strip_gate(dims, perm, 300_000, 16) is None


# ------------------------------------------------------------------ binding
def _binding_args(dev="cpu"):
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    return [z(8, i32), [z(8, i32), z(8, i32)],
            [torch.ones(4, 16, dtype=f64, device=dev) for _ in range(2)],
            torch.ones(8, dtype=f64, device=dev), z(1, i32),
            torch.ones(1, dtype=i32, device=dev), z(1, i32),
            torch.tensor([[0, 8]], dtype=i64, device=dev), 4, 1,
            z(64, f64).view(4, 16), 0]


def test_binding_rejects_host_tensors():
    with pytest.raises(RuntimeError, match="out must be a device tensor"):
        mk.native().mttkrp_strip_gpu(*_binding_args())


@gpu
def test_binding_rejects_wrong_dtypes():
    for pos, name in ((0, "key"), (4, "strip row0"), (7, "strip bounds")):
        args = _binding_args("cuda")
        args[pos] = args[pos].to(torch.int16)
        with pytest.raises(RuntimeError, match=f"{name} has dtype Short"):
            mk.native().mttkrp_strip_gpu(*args)
    args = _binding_args("cuda")
    args[3] = args[3].to(torch.int16)
    with pytest.raises(RuntimeError, match="vals has dtype Short"):
        mk.native().mttkrp_strip_gpu(*args)
    args = _binding_args("cuda")
    args[1][1] = args[1][1].cpu()
    with pytest.raises(RuntimeError, match="idx must be a device tensor"):
        mk.native().mttkrp_strip_gpu(*args)


# ------------------------------------------------------------------- kernel
def _decode(lin, dims):
    cols = []
    for d in reversed(dims):
        cols.append(lin % d)
        lin = lin // d
    return torch.stack(cols[::-1], 0)


@functools.lru_cache(maxsize=None)
def rand_tensor(dims, nnz, exact, seed=5):
    """nnz DISTINCT coordinates; f64 values in [0.5, 1.5], f32-exact or not"""
    g = torch.Generator().manual_seed(seed + nnz)
    total = 1
    for d in dims:
        total *= d
    lin = torch.randperm(total, generator=g)[:nnz]
    if exact:
        vals = (torch.rand(nnz, generator=g, dtype=torch.float32)
                + 0.5).double()
        assert torch.equal(vals.float().double(), vals)
    else:
        vals = torch.rand(nnz, generator=g, dtype=torch.float64) + 0.5
        assert not torch.equal(vals.float().double(), vals)
    return sp.SpTensor(_decode(lin, list(dims)), vals, list(dims))


@functools.lru_cache(maxsize=None)
def mats_for(dims, rank):
    return tuple(sp.seeded_init(d, rank, m, 123) for m, d in enumerate(dims))


@functools.lru_cache(maxsize=None)
def oracle(dims, nnz, exact, rank):
    t = rand_tensor(dims, nnz, exact)
    return tuple(sp.mttkrp_stream(t, list(mats_for(dims, rank)), m)
                 for m in range(len(dims)))


def strip_set(t, rank):
    tg = t.to("cuda")
    nm = t.nmodes
    csfs = [sp.build_csf(tg, sp.order_modes(t.dims, "root", m),
                         flat_only=True, stage_rank=rank, **FORCE)
            for m in range(nm)]
    for c in csfs:
        st = c._strip
        assert getattr(c, "_stage", None) is None
        assert st["tile_rows"] == 4 and st["wgs"] == 3 and st["cap"] == 64
        assert int((st["p1"] - st["p0"]).sum()) == t.nnz
    return sp.CsfSet(csfs, list(range(nm)), [0] * nm)


def record(monkeypatch, name):
    nat = mk.native()
    orig, calls = getattr(nat, name), []

    def wrapped(*a):
        calls.append(orig(*a))
        return calls[-1]
    monkeypatch.setattr(nat, name, wrapped)
    return calls


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["vals32", "vals64"])
@pytest.mark.parametrize("rank", [16, 32, 64])
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
@pytest.mark.parametrize("nnz", [1, 31, 33, 1000, 5003])
def test_strip_matches_oracle(monkeypatch, nnz, dims, rank, exact):
    ref = oracle(dims, nnz, exact, rank)
    cs = strip_set(rand_tensor(dims, nnz, exact), rank)
    mats_g = [m.cuda() for m in mats_for(dims, rank)]
    ran = record(monkeypatch, "mttkrp_strip_gpu")
    other = record(monkeypatch, "gpu_mttkrp_flat")
    for mode in range(len(dims)):
        c = cs.csfs[mode]
        assert not mk.mttkrp_rows_ok(cs, mode, rank)
        out = sp.mttkrp(cs, mats_g, mode)
        v32 = getattr(c, "_vals32", None)
        assert (v32 is not False and v32 is not None) == exact
        err = (out.cpu() - ref[mode]).abs().max().item()
        print(f"nnz={nnz} dims={dims} rank={rank} exact={exact} mode={mode} "
              f"strips={c._strip['row0'].numel()} err={err:.3e}")
        assert err < 1e-8, (nnz, dims, rank, mode, err)
    assert ran == [True] * len(dims) and other == []


# one row holding most nonzeros (split over many strips), empty rows inside
# strips (rows 1, 2), whole empty strips (rows 12..19) and an empty tail
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
def test_heavy_row_empty_rows_and_reused_buffers(monkeypatch):
    assert len(HCOUNTS) == HDIMS[0]
    t, mats, ref = heavy()
    cs = strip_set(t, 16)
    st = cs.csfs[0]._strip
    shared = int(((st["flags"] & 2) != 0).sum())
    assert shared >= 1300 // 64            # the heavy row's strips
    mats_g = [m.cuda() for m in mats]
    ran = record(monkeypatch, "mttkrp_strip_gpu")
    # the caller's zeroing is the only thing that clears `out`
    out = torch.full((HDIMS[0], 16), -7.25, dtype=torch.float64,
                     device="cuda")
    sp.mttkrp(cs, mats_g, 0, out=out)
    err1 = (out.cpu() - ref).abs().max().item()
    sp.mttkrp(cs, mats_g, 0, out=out)      # must not accumulate
    err2 = (out.cpu() - ref).abs().max().item()
    print(f"heavy row: shared strips={shared} err={err1:.3e} again={err2:.3e}")
    assert err1 < 1e-8 and err2 < 1e-8
    assert ran == [True, True]
    empty = [r for r, n in enumerate(HCOUNTS) if n == 0]
    assert (out[empty] == 0).all()
    with pytest.raises(ValueError, match="key-sorted"):
        sp.mttkrp(cs, mats_g, 0, out=out, rows=(0, 10))


@gpu
def test_graph_capture_replays_the_eager_result(monkeypatch):
    t = rand_tensor(DIMS3, 5003, True)
    cs = strip_set(t, 16)
    mats_g = [m.cuda() for m in mats_for(DIMS3, 16)]
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
    ref = oracle(DIMS3, 5003, True, 16)[0]
    err = (out.cpu() - ref).abs().max().item()
    d = (out - eager).abs().max().item()
    print(f"graph replay err={err:.3e} vs-eager={d:.3e}")
    assert err < 1e-8 and d < 1e-8
