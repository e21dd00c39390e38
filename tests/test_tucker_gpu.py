"""Sparse Tucker on the MI355X: the HIP TTMc kernel against the dense
oracles of tests/test_tucker.py (same inputs, same bounds), and HOOI on
device against HOOI on the CPU."""
import pytest
import torch

import splatt_amd as sp
from splatt_amd import tucker

from test_complete import INPUTS, check_preconditions, four_mode, heavy
from test_tucker import (EXACT_CASES, FLOAT_CASES, PLANTED_OPTS, RANDOM,
                         RANDOM_OPTS, TOL, assert_close, assert_exact,
                         check_planted, check_random, float_mats,
                         float_oracle, int_mats, int_tensor, planted)

pytestmark = pytest.mark.gpu

_CSF = {}


def device_csf(name, exact):
    key = (name, exact)
    if key not in _CSF:
        t = int_tensor(name) if exact else INPUTS[name]()
        _CSF[key] = sp.csf_alloc(t.to("cuda"), "all")
    return _CSF[key]


@pytest.mark.parametrize("name,ranks", EXACT_CASES)
def test_ttmc_hip_exact(name, ranks):
    check_preconditions(name)
    cs = device_csf(name, True)
    mats = [m.cuda() for m in int_mats(name, ranks)]
    for mode in range(cs.nmodes):
        got = sp.ttmc(cs, mats, mode, impl="hip")
        assert got.is_cuda
        assert_exact(got, name, ranks, mode, "hip")
        # auto picks the kernel on device tensors
        assert torch.equal(sp.ttmc(cs, mats, mode), got)


@pytest.mark.parametrize("name,ranks", FLOAT_CASES)
def test_ttmc_hip_float_reproducible(name, ranks):
    cs = device_csf(name, False)
    mats = [m.cuda() for m in float_mats(name, ranks)]
    for mode in range(cs.nmodes):
        got = sp.ttmc(cs, mats, mode, impl="hip")
        assert_close(got, name, ranks, mode, "hip")
        again = sp.ttmc(cs, mats, mode, impl="hip")
        assert torch.equal(again, got)


def test_ttmc_torch_on_device_matches_hip():
    """impl='torch' on device tensors is the benchmark's baseline."""
    for name, ranks in (("heavy", (7, 5, 3)), ("4-mode", (16, 4, 4, 4))):
        cs = device_csf(name, True)
        mats = [m.cuda() for m in int_mats(name, ranks)]
        for mode in range(cs.nmodes):
            a = sp.ttmc(cs, mats, mode, impl="torch")
            assert a.is_cuda
            assert_exact(a, name, ranks, mode, "torch-on-device")
            assert torch.equal(a, sp.ttmc(cs, mats, mode, impl="hip"))
    name, ranks = "heavy", (16, 16, 16)
    cs = device_csf(name, False)
    mats = [m.cuda() for m in float_mats(name, ranks)]
    for mode in range(3):
        a = sp.ttmc(cs, mats, mode, impl="torch")
        assert_close(a, name, ranks, mode, "torch-on-device")
        err = (a - sp.ttmc(cs, mats, mode, impl="hip")).abs().max().item()
        bound = TOL * max(1.0, float_oracle(name, ranks, mode).abs().max()
                          .item())
        assert err <= bound, (mode, err, bound)


def test_ttmc_hip_batched_workspace(monkeypatch):
    """A byte budget too small for all multi-segment rows at once: the rows
    go through the workspace in several batches, same exact result."""
    check_preconditions("heavy")
    name, ranks = "heavy", (16, 16, 16)
    cols = 256
    cs = device_csf(name, True)
    mats = [m.cuda() for m in int_mats(name, ranks)]
    for mode in range(3):
        monkeypatch.delenv("SPLATT_TTMC_MB", raising=False)
        plan = tucker.ttmc_plan(cs, mode, cols)
        ms = plan["mslot"].cpu()
        widest = int((ms[1:] - ms[:-1]).max())
        assert int(ms[-1]) > widest              # more than one such row
        mb = (widest + 0.5) * tucker.slot_bytes(cols) / (1 << 20)
        monkeypatch.setenv("SPLATT_TTMC_MB", repr(mb))
        plan = tucker.ttmc_plan(cs, mode, cols)
        cap = tucker.workspace_budget_bytes() // tucker.slot_bytes(cols)
        assert len(plan["batches"]) > 1, (mode, plan["batches"])
        assert all(s1 - s0 <= cap for _, _, s0, s1 in plan["batches"])
        got = sp.ttmc(cs, mats, mode, impl="hip")
        assert_exact(got, name, ranks, mode, "hip-batched")


def test_ttmc_hip_rejects_staged_stream():
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t = heavy()
    cs = build_shard_csf(t.to("cuda"), list(t.dims), "all", flat_only=True,
                         stage_rank=16)
    staged = [m for m in range(t.nmodes)
              if getattr(cs.csfs[cs.mode_csf[m]], "_stage", None) is not None]
    assert staged
    mats = [m.cuda() for m in float_mats("heavy", (16, 16, 16))]
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.ttmc(cs, mats, staged[0])


def test_ttmc_hip_rejects_wide_rows_and_host_factors():
    t = four_mode()
    cs = device_csf("4-mode", False)
    ranks = (2, 32, 32, 32)                      # P_0 = 32768 > MAX_COLS
    mats = [sp.seeded_init(d, r, m, 5).cuda()
            for m, (d, r) in enumerate(zip(t.dims, ranks))]
    with pytest.raises(ValueError, match="impl='torch'"):
        sp.ttmc(cs, mats, 0, impl="hip")
    wide = sp.ttmc(cs, mats, 0)                  # auto -> torch
    assert tuple(wide.shape) == (t.dims[0], 32, 32, 32)
    # index_add_ on device sums in no fixed order: compare to the bound
    err = (wide - sp.ttmc(cs, mats, 0, impl="torch")).abs().max().item()
    assert err <= TOL * max(1.0, wide.abs().max().item())
    host = [m.cpu() for m in mats]
    with pytest.raises(ValueError, match="device"):
        sp.ttmc(cs, host, 1)


def test_tucker_hooi_device_planted():
    t, _ = planted()
    opts = sp.TuckerOptions(**PLANTED_OPTS)
    cpu = sp.tucker_hooi(t, (3, 2, 4), opts)
    dev = sp.tucker_hooi(t.to("cuda"), (3, 2, 4), opts)
    assert dev.core.is_cuda and all(U.is_cuda for U in dev.factors)
    check_planted(dev)
    assert max(abs(a - b) for a, b in zip(cpu.fit_trace, dev.fit_trace)) \
        <= 1e-10


def test_tucker_hooi_device_four_mode():
    make, ranks = RANDOM["4-mode"]
    t = make()
    opts = sp.TuckerOptions(**RANDOM_OPTS)
    cpu = sp.tucker_hooi(t, ranks, opts)
    dev = sp.tucker_hooi(t.to("cuda"), ranks, opts)
    assert dev.core.is_cuda and all(U.is_cuda for U in dev.factors)
    dmax = max(abs(a - b) for a, b in zip(cpu.fit_trace, dev.fit_trace))
    print(f"device vs CPU fit trace: max difference {dmax:.3e}")
    assert dmax <= 1e-10
    check_random(dev, "4-mode", t)               # includes U^T U = I to 1e-12
