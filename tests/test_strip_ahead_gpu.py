"""Run-ahead pacing of the strip MTTKRP (csrc/hip/mttkrp_strip.hip): the
workgroups of the one launch wait on a ring of 8 slot counters and may lead
the slowest by SPLATT_STRIP_AHEAD groups.

Layout, inputs and oracle are those of tests/test_strip_paced_gpu.py: the
forced tiny layout (4-row strips, a 64-nonzero cap, 7-row windows, 3
workgroups) with 1, 3 and 8 groups of windows, small-integer values and
factors whose products and sums are exact in f64, so the result must be
`torch.equal` to the int64 oracle whatever the order of the adds and
whatever the waits do. Run-ahead 0, 1, 2 and 7; the strips have at most 8
groups and up to a few passes, so 7 reaches or exceeds the group count and
with one pass no workgroup waits at all.

The waits are for speed only, so beyond the results there are only counts to
check: arrivals = workgroups x passes x groups after every dispatch (added
once per workgroup at the end of the kernel), no time-outs, and no more
polled waits than arrivals. The time-out path is tested with a budget of 0
and in no other way."""
import importlib
import os
import sys

import pytest
import torch

import splatt_amd as sp

mk = importlib.import_module("splatt_amd.mttkrp")
# tensors, oracles and helpers are shared with the paced tests (cached there)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
paced = importlib.import_module("test_strip_paced_gpu")

gpu = pytest.mark.gpu

DIMS3, DIMS4, WGS = paced.DIMS3, paced.DIMS4, paced.WGS
AHEADS = [0, 1, 2, 7]


def strip_set(t, rank, groups):
    cs = paced.strip_set(t, rank, groups)
    for c in cs.csfs:
        sl = c._strip["slots"]
        assert sl.numel() == 256 and sl.is_cuda and sl.dtype == torch.int32
    return cs


def check_counts(c, ahead):
    """pace words and slot ring after a dispatch of CSF c"""
    arrivals, timeouts, _ = sp.strip_pace_stats(c)
    wait_us, polled = sp.strip_pace_waits(c)
    expected = paced.expected_arrivals(c)
    assert arrivals == expected
    assert timeouts == 0
    assert polled <= arrivals and wait_us >= 0.0
    st = c._strip
    grid = min(st["wgs"], int(st["row0"].numel()))
    per_wg = expected // grid
    slots = st["slots"].cpu().view(8, 32)
    # slot s counts the calls t = s, s + 8, ... of every workgroup
    assert slots[:, 0].tolist() == [grid * len(range(s, per_wg, 8))
                                    for s in range(8)]
    assert int(slots[:, 1:].abs().sum()) == 0
    if ahead >= per_wg:
        assert polled == 0                  # nothing to wait for


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["vals32", "vals64"])
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
@pytest.mark.parametrize("nnz", [1, 33, 5003])
@pytest.mark.parametrize("groups", [1, 3, 8])
def test_run_ahead_is_exact_and_counts_add_up(monkeypatch, groups, nnz, dims,
                                              exact):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_TRACE", raising=False)
    t, _ = paced.int_tensor(dims, nnz, exact)
    ran = paced.record(monkeypatch, "mttkrp_strip_gpu")
    other = paced.record(monkeypatch, "gpu_mttkrp_flat")
    ref = {rank: paced.int_oracle(dims, nnz, exact, rank)
           for rank in (16, 32, 64)}
    for rank in (16, 32, 64):
        cs = strip_set(t, rank, groups)
        mats_g = [m.double().cuda() for m in paced.int_mats(dims, rank)]
        for ahead in AHEADS:
            monkeypatch.setenv("SPLATT_STRIP_AHEAD", str(ahead))
            for mode in range(len(dims)):
                c = cs.csfs[mode]
                out = sp.mttkrp(cs, mats_g, mode)
                diff = (out.cpu() - ref[rank][mode]).abs().max().item()
                print(f"groups={groups} ahead={ahead} nnz={nnz} rank={rank} "
                      f"mode={mode} diff={diff:.3e} "
                      f"pace={sp.strip_pace_stats(c)} "
                      f"waits={sp.strip_pace_waits(c)}")
                assert torch.equal(out.cpu(), ref[rank][mode]), \
                    (ahead, rank, mode, diff)
                check_counts(c, ahead)
    assert ran == [True] * (3 * len(AHEADS) * len(dims)) and other == []


@gpu
@pytest.mark.parametrize("groups", [1, 3, 8])
def test_heavy_row_twice_into_a_dirty_buffer(monkeypatch, groups):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    monkeypatch.setenv("SPLATT_STRIP_AHEAD", "2")
    t, mats, ref = paced.heavy()
    cs = strip_set(t, 16, groups)
    c = cs.csfs[0]
    mats_g = [m.cuda() for m in mats]
    ran = paced.record(monkeypatch, "mttkrp_strip_gpu")
    out = torch.full((paced.HDIMS[0], 16), -7.25, dtype=torch.float64,
                     device="cuda")
    errs = []
    for _ in range(2):                      # must not accumulate
        sp.mttkrp(cs, mats_g, 0, out=out)
        errs.append((out.cpu() - ref).abs().max().item())
        check_counts(c, 2)
    print(f"heavy row groups={groups} ahead=2: errs={errs}")
    assert max(errs) < 1e-8
    assert ran == [True, True]
    empty = [r for r, n in enumerate(paced.HCOUNTS) if n == 0]
    assert (out[empty] == 0).all()


@gpu
@pytest.mark.parametrize("dims", [DIMS3, DIMS4], ids=["3mode", "4mode"])
def test_budget_zero_gives_up_and_stays_exact(monkeypatch, dims):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.setenv("SPLATT_STRIP_PACE_US", "0")
    monkeypatch.setenv("SPLATT_STRIP_AHEAD", "2")
    t, _ = paced.int_tensor(dims, 5003, False)
    cs = strip_set(t, 16, 3)
    stats = paced.run_exact(cs, dims, 5003, False, 16, "ahead=2 budget=0")
    for c, (arrivals, timeouts, longest) in zip(cs.csfs, stats):
        assert arrivals == paced.expected_arrivals(c)
        # sticky: at most one time-out per workgroup
        assert timeouts <= min(WGS, int(c._strip["row0"].numel()))
        assert longest < 1000.0
        _, polled = sp.strip_pace_waits(c)
        assert timeouts <= polled <= arrivals


@gpu
def test_pace_off_leaves_both_buffers_alone(monkeypatch):
    monkeypatch.setenv("SPLATT_STRIP_PACE", "0")
    monkeypatch.setenv("SPLATT_STRIP_AHEAD", "2")
    t, _ = paced.int_tensor(DIMS3, 5003, True)
    cs = strip_set(t, 16, 3)
    for c in cs.csfs:
        c._strip["pace"].fill_(0x5A5A)
        c._strip["slots"].fill_(0x3C3C)
    ref = paced.int_oracle(DIMS3, 5003, True, 16)
    mats_g = [m.double().cuda() for m in paced.int_mats(DIMS3, 16)]
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        assert torch.equal(out.cpu(), ref[mode])
        assert (cs.csfs[mode]._strip["pace"] == 0x5A5A).all()
        assert (cs.csfs[mode]._strip["slots"] == 0x3C3C).all()


@gpu
def test_graph_replay_counts_one_dispatch(monkeypatch):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    monkeypatch.setenv("SPLATT_STRIP_AHEAD", "2")
    t, _ = paced.int_tensor(DIMS3, 5003, True)
    cs = strip_set(t, 16, 3)
    c = cs.csfs[0]
    mats_g = [m.cuda() for m in
              (sp.seeded_init(d, 16, m, 123) for m, d in enumerate(DIMS3))]
    eager = sp.mttkrp(cs, mats_g, 0).clone()   # also settles every cache
    ran = paced.record(monkeypatch, "mttkrp_strip_gpu")
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
    print(f"graph replay ahead=2 vs-eager={d:.3e} "
          f"pace={sp.strip_pace_stats(c)}")
    assert d < 1e-12
    check_counts(c, 2)                         # of ONE dispatch, not three


@gpu
def test_trace_holds_one_row_per_workgroup(monkeypatch):
    monkeypatch.delenv("SPLATT_STRIP_PACE", raising=False)
    monkeypatch.delenv("SPLATT_STRIP_PACE_US", raising=False)
    monkeypatch.setenv("SPLATT_STRIP_AHEAD", "1")
    monkeypatch.setenv("SPLATT_STRIP_TRACE", "1")
    t, _ = paced.int_tensor(DIMS3, 5003, True)
    cs = strip_set(t, 16, 3)
    c = cs.csfs[0]
    ref = paced.int_oracle(DIMS3, 5003, True, 16)
    mats_g = [m.double().cuda() for m in paced.int_mats(DIMS3, 16)]
    assert torch.equal(sp.mttkrp(cs, mats_g, 0).cpu(), ref[0])
    tr = c._strip["trace"].cpu()
    assert tuple(tr.shape) == (WGS, 4)
    khz = mk.native().strip_wall_khz()
    wait_us, polled = sp.strip_pace_waits(c)
    _, _, longest = sp.strip_pace_stats(c)
    assert ((tr[:, 0] >= 0) & (tr[:, 0] < 16)).all()          # XCC id
    assert int(tr[:, 2].sum()) == polled
    assert abs(int(tr[:, 1].sum()) * 1000.0 / khz - wait_us) < 1e-6
    assert abs(int(tr[:, 3].max()) * 1000.0 / khz - longest) < 1e-6


# ----------------------------------------------------------------- binding
@gpu
def test_binding_checks_slots_and_run_ahead():
    nat = mk.native()
    args = lambda: paced._binding_args("cuda")
    z = lambda n, dt=torch.int32, dev="cuda": torch.zeros(n, dtype=dt,
                                                          device=dev)
    with pytest.raises(RuntimeError, match="slots has dtype Short"):
        nat.mttkrp_strip_gpu(*args(), z(96), 100, z(256, torch.int16), 0)
    with pytest.raises(RuntimeError, match="slots must be a device tensor"):
        nat.mttkrp_strip_gpu(*args(), z(96), 100, z(256, dev="cpu"), 0)
    with pytest.raises(RuntimeError, match="at least 256 words"):
        nat.mttkrp_strip_gpu(*args(), z(96), 100, z(255), 0)
    with pytest.raises(RuntimeError, match="slots must be contiguous"):
        nat.mttkrp_strip_gpu(*args(), z(96), 100, z(512)[::2], 0)
    for bad in (-1, 8):
        with pytest.raises(RuntimeError, match="ahead out of range"):
            nat.mttkrp_strip_gpu(*args(), z(96), 100, z(256), bad)
    with pytest.raises(RuntimeError, match="ahead > 0 needs"):
        nat.mttkrp_strip_gpu(*args(), z(96), 100, None, 1)
    with pytest.raises(RuntimeError, match="slots need a pace tensor"):
        nat.mttkrp_strip_gpu(*args(), None, 100, z(256), 0)
    with pytest.raises(RuntimeError, match="at least 4 words"):
        nat.mttkrp_strip_gpu(*args(), z(96), 100, z(256), 0, z(3))
    row = torch.full((16,), 8.0, dtype=torch.float64)
    # both word types, every run-ahead; 1 workgroup, 1 pass, 1 group
    for slots in (z(256), z(256).view(torch.uint32)):
        for ahead in (0, 1, 7):
            a, pace = args(), z(96)
            slots.view(torch.int32).fill_(9)       # the launcher clears it
            assert nat.mttkrp_strip_gpu(*a, pace, 100, slots, ahead)
            torch.cuda.synchronize()
            assert int(pace[0]) == 1
            assert slots.view(torch.int32).cpu().nonzero().tolist() == [[0]]
            assert int(slots.view(torch.int32)[0]) == 1
            assert torch.equal(a[10].cpu()[0], row)
    # the 12- and 14-argument forms: as before, the slots are not needed
    a = args()
    assert nat.mttkrp_strip_gpu(*a)
    torch.cuda.synchronize()
    assert torch.equal(a[10].cpu()[0], row)
    a, pace = args(), z(96)
    assert nat.mttkrp_strip_gpu(*a, pace, 100)
    torch.cuda.synchronize()
    assert int(pace[0]) == 1 and torch.equal(a[10].cpu()[0], row)
