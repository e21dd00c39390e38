"""Tensor completion on the MI355X: the HIP row-solve and predict kernels
against the CPU oracle of tests/test_complete.py (same inputs, same bound)."""
import pytest
import torch

import splatt_amd as sp
from splatt_amd import completion

from test_complete import (INPUTS, PLANTED_OPTS, REG, TOL,
                           assert_matches_oracle, check_planted_result,
                           check_preconditions, heavy, make_mats, oracle,
                           planted, row_counts)

pytestmark = pytest.mark.gpu

_CSF = {}


def device_csf(name):
    if name not in _CSF:
        _CSF[name] = sp.csf_alloc(INPUTS[name]().to("cuda"), "all")
    return _CSF[name]


def device_mats(name, rank):
    return [m.cuda() for m in make_mats(name, rank)]


@pytest.mark.parametrize("name,rank", [
    ("heavy", 16), ("heavy", 32), ("heavy", 64),   # MFMA path
    ("heavy", 7),                                  # generic path
    ("thin", 16), ("thin", 32), ("4-mode", 16)])
def test_update_hip_matches_oracle(name, rank):
    check_preconditions(name)
    t = INPUTS[name]()
    cs = device_csf(name)
    mats = device_mats(name, rank)
    for mode in range(t.nmodes):
        got = sp.complete_update(cs, mats, mode, REG)   # auto -> hip
        assert_matches_oracle(got, name, rank, mode, "hip")


def test_update_hip_batched_workspace(monkeypatch):
    """A byte budget too small for all multi-segment rows at once: the rows
    go through the workspace in several batches, same result."""
    check_preconditions("heavy")
    rank = 32
    t = heavy()
    cs = device_csf("heavy")
    mats = device_mats("heavy", rank)
    for mode in range(t.nmodes):
        monkeypatch.setenv("SPLATT_COMPLETE_MB", "1")
        plan = completion.completion_plan(cs, mode, rank)
        if len(plan["batches"]) < 2:
            # 1 MB still holds every slot: budget = the widest row's slots
            ms = plan["mslot"].cpu()
            widest = int((ms[1:] - ms[:-1]).max())
            assert int(ms[-1]) > widest          # more than one such row
            mb = (widest + 0.5) * completion.slot_bytes(rank) / (1 << 20)
            monkeypatch.setenv("SPLATT_COMPLETE_MB", repr(mb))
            plan = completion.completion_plan(cs, mode, rank)
        cap = completion.workspace_budget_bytes() // completion.slot_bytes(rank)
        assert len(plan["batches"]) > 1, (mode, plan["batches"])
        assert all(s1 - s0 <= cap for _, _, s0, s1 in plan["batches"])
        got = sp.complete_update(cs, mats, mode, REG, impl="hip")
        assert_matches_oracle(got, "heavy", rank, mode, "hip-batched")


@pytest.mark.parametrize("rank", [16, 7])
def test_update_torch_on_device_matches_hip(rank):
    """impl='torch' on device tensors is the benchmark's baseline."""
    t = heavy()
    cs = device_csf("heavy")
    mats = device_mats("heavy", rank)
    for mode in range(t.nmodes):
        a = sp.complete_update(cs, mats, mode, REG, impl="torch")
        b = sp.complete_update(cs, mats, mode, REG, impl="hip")
        assert_matches_oracle(a, "heavy", rank, mode, "torch-on-device")
        err = (a - b).abs().max().item()
        bound = TOL * max(1.0, oracle("heavy", rank, mode).abs().max().item())
        assert err <= bound, (rank, mode, err, bound)


@pytest.mark.parametrize("rank", [16, 7])
def test_kruskal_predict_device(rank):
    t = heavy()
    g = torch.Generator().manual_seed(9)
    inds = torch.stack([torch.randint(0, d, (10_000,), generator=g)
                        for d in t.dims], 0)
    mats = list(make_mats("heavy", rank))
    lam = torch.rand(rank, generator=g, dtype=torch.float64) + 0.5
    for lm in (None, lam):
        want = sp.kruskal_predict(mats, inds, lam=lm)
        got = sp.kruskal_predict([m.cuda() for m in mats], inds.cuda(),
                                 lam=None if lm is None else lm.cuda())
        assert got.is_cuda
        err = (got.cpu() - want).abs().max().item()
        print(f"predict rank {rank}: max|delta| = {err:.3e}")
        assert err <= 1e-12
    # a length that is no multiple of the 64-entry wave chunk
    got = sp.kruskal_predict([m.cuda() for m in mats], inds[:, :77].cuda())
    assert (got.cpu() - sp.kruskal_predict(mats, inds[:, :77])
            ).abs().max().item() <= 1e-12
    th = sp.SpTensor(inds, want.clone(), list(t.dims))
    assert sp.rmse([m.cuda() for m in mats], th.to("cuda")) == pytest.approx(
        sp.rmse(mats, th), abs=1e-12)


def test_complete_als_device_planted():
    train, val = planted()
    opts = sp.CompleteOptions(**PLANTED_OPTS)
    cpu = sp.complete_als(train, 4, opts, validate=val)
    dev = sp.complete_als(train.to("cuda"), 4, opts, validate=val.to("cuda"))
    assert all(f.is_cuda for f in dev.factors)
    check_planted_result(dev, cpu.rmse_val_trace[-1])


def test_update_hip_rejects_staged_stream():
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t = heavy()
    cs = build_shard_csf(t.to("cuda"), list(t.dims), "all", flat_only=True,
                         stage_rank=16)
    staged = [m for m in range(t.nmodes)
              if getattr(cs.csfs[cs.mode_csf[m]], "_stage", None) is not None]
    assert staged
    with pytest.raises(ValueError, match="csf_alloc='all'"):
        sp.complete_update(cs, device_mats("heavy", 16), staged[0], REG)
