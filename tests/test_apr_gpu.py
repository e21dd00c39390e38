"""Poisson CPD (CP-APR) on the MI355X: the HIP row-update kernels against the
CPU oracles of tests/test_apr.py (same inputs, same bounds).

Largest device errors observed, relative to max(1, max|oracle|): 1.3e-13
over the fixed-count cases (heavy, rank 1, mode 1, Phi) and 8.1e-15 over
the stopping cases (bound TOL = 2e-11); the driver's log-likelihood trace
on the fixed 5 x 5 schedule differed from the CPU run by 1.3e-16 relative
(bound DRV_TOL = 1.4e-13).
"""
import pytest
import torch

import splatt_amd as sp
from splatt_amd import apr, completion

from test_apr import (DRV_TOL, FIXED_DRV, FIXED_INNER, INPUTS, PLANTED_OPTS,
                      RANKS, THIN_STOP, assert_close, check_exact,
                      check_fixed, check_planted_result, check_stop_heavy,
                      check_stop_thin, fixed_schedule_cpu, four_mode, heavy,
                      make_b, make_mats, oracle_fixed, planted, run_update)

pytestmark = pytest.mark.gpu

_CSF = {}


def device_csf(name):
    if name not in _CSF:
        _CSF[name] = sp.csf_alloc(INPUTS[name]().to("cuda"), "all")
    return _CSF[name]


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("rank", RANKS)
def test_exact_hip(rank, zeros):
    """Bit for bit, single- and multi-segment rows."""
    check_exact("hip", "cuda", rank, zeros)


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_fixed_count_hip(name, rank):
    worst = check_fixed(device_csf(name), "cuda", name, rank, "hip")
    print(f"hip {name} rank {rank}: worst relative error {worst:.3e}")


def test_plan_has_both_kinds_of_rows():
    """heavy exercises the in-wave loop and the slot / fold rounds at once."""
    for mode in range(3):
        plan = apr.apr_plan(device_csf("heavy"), mode)
        assert plan["nsingle"] > 100
        assert plan["mrow"].numel() == 7
        assert len(plan["batches"]) == 1
        assert int(plan["seg_len"].max()) == completion.SEG


@pytest.mark.parametrize("rank,inner_tol", THIN_STOP)
def test_stopping_rule_hip_thin(rank, inner_tol):
    check_stop_thin(device_csf("thin"), "cuda", rank, inner_tol, "hip")


def test_stopping_rule_hip_heavy():
    check_stop_heavy(device_csf("heavy"), "cuda", "hip")


@pytest.mark.parametrize("rank", [16, 7])
def test_update_is_reproducible(rank):
    cs = device_csf("heavy")
    mats = [m.cuda() for m in make_mats("heavy", rank)]
    for mode in range(3):
        B0 = make_b("heavy", rank, mode).cuda()
        a = run_update(cs, mats, mode, B0, "hip", inner_tol=1e-2,
                       max_inner=8)
        b = run_update(cs, mats, mode, B0, "hip", inner_tol=1e-2,
                       max_inner=8)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("rank", [16, 7])
def test_update_auto_is_hip_and_torch_on_device_matches(rank):
    """impl='torch' on device tensors is the benchmark's baseline."""
    cs = device_csf("thin")
    mats = [m.cuda() for m in make_mats("thin", rank)]
    for mode in range(3):
        B0 = make_b("thin", rank, mode).cuda()
        kw = dict(inner_tol=0.0, max_inner=FIXED_INNER)
        got = run_update(cs, mats, mode, B0, "torch", **kw)
        assert all(x.is_cuda for x in got)
        assert_close(got, oracle_fixed("thin", rank, mode),
                     f"torch-on-device thin rank {rank} mode {mode}")
        auto = run_update(cs, mats, mode, B0, "auto", **kw)
        hip = run_update(cs, mats, mode, B0, "hip", **kw)
        for x, y in zip(auto, hip):
            assert torch.equal(x, y)


def test_cpd_apr_device_planted():
    t, _, _ = planted()
    r = sp.cpd_apr(t.to("cuda"), 4, sp.AprOptions(**PLANTED_OPTS))
    assert all(f.is_cuda for f in r.factors) and r.lam.is_cuda
    check_planted_result(r)


def test_cpd_apr_device_fixed_schedule_matches_cpu():
    cpu = fixed_schedule_cpu()
    dev = sp.cpd_apr(four_mode().to("cuda"), 8, sp.AprOptions(**FIXED_DRV))
    assert dev.niters == cpu.niters == 5
    assert dev.inner_trace == cpu.inner_trace
    err = max(abs(a - b) / abs(b)
              for a, b in zip(dev.loglik_trace, cpu.loglik_trace))
    print(f"driver trace, device vs CPU: {err:.3e} (DRV_TOL {DRV_TOL:.1e})")
    assert err <= DRV_TOL


def test_update_hip_rejects_negative_values():
    t = heavy()
    neg = sp.SpTensor(t.inds.clone(), t.vals - 2.0, list(t.dims)).to("cuda")
    mats = [m.cuda() for m in make_mats("heavy", 16)]
    with pytest.raises(ValueError, match=">= 0"):
        sp.apr_update(sp.csf_alloc(neg, "all"), mats, 0,
                      make_b("heavy", 16, 0).cuda(), inner_tol=0.0,
                      max_inner=1)
