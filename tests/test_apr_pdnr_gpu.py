"""Poisson CPD, damped-Newton row solver (PDNR) on the MI355X: the fused HIP
kernel against the CPU oracle of tests/test_apr_pdnr.py (same inputs, same
bounds, the same cap on rows left out).

Largest device errors observed, relative to max(1, max|oracle|): 3.6e-11
over the one-iteration cases (thin, rank 16, mode 0, B; 5.2e-14 outside the
thin input), iters / nback / nfail equal to the oracle's on every row;
5.8e-13 over the stopping cases (thin, rank 7, mode 2, Phi) with no row
left out in any case (bound TOL_PDNR = 2.5e-8); the driver's log-likelihood
trace on the 5-iteration schedule of `4-mode` differed from the CPU run by
1.3e-16 relative (bound DRV_TOL_PDNR = 1.4e-13).
"""
import pytest
import torch

import splatt_amd as sp

from test_apr import INPUTS, RANKS, heavy, make_b, make_mats, planted
from test_apr_pdnr import (DRV_PDNR, DRV_TOL_PDNR, PLANTED_PDNR, STOP_RANKS,
                           check_one, check_planted_pdnr, check_stop, compare,
                           oracle_one, run_pdnr, short_schedule_cpu)

pytestmark = pytest.mark.gpu

_CSF = {}


def device_csf(name):
    if name not in _CSF:
        _CSF[name] = sp.csf_alloc(INPUTS[name]().to("cuda"), "all")
    return _CSF[name]


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_one_iteration_hip(name, rank):
    worst = check_one(device_csf(name), "cuda", name, rank, "hip")
    print(f"hip one {name} rank {rank}: worst relative error {worst:.3e}")


@pytest.mark.parametrize("rank", STOP_RANKS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_stopping_runs_hip(name, rank):
    worst = check_stop(device_csf(name), "cuda", name, rank, "hip")
    print(f"hip stop {name} rank {rank}: worst relative error {worst:.3e}")


@pytest.mark.parametrize("rank", [16, 7])
def test_update_is_reproducible(rank):
    """No atomics and a fixed summation order: bit for bit."""
    cs = device_csf("heavy")
    mats = [m.cuda() for m in make_mats("heavy", rank)]
    keys = ("B", "Phi", "iters", "viol0", "f0", "f", "mu", "nback", "nfail")
    for mode in range(3):
        B0 = make_b("heavy", rank, mode).cuda()
        a = run_pdnr(cs, mats, mode, B0, "hip", inner_tol=1e-3, max_inner=8)
        b = run_pdnr(cs, mats, mode, B0, "hip", inner_tol=1e-3, max_inner=8)
        assert int(a["iters"].max()) > 1
        for k in keys:
            assert torch.equal(a[k], b[k]), (mode, k)


@pytest.mark.parametrize("rank", [16, 7])
def test_update_auto_is_hip_and_torch_on_device_matches(rank):
    """impl='torch' on device tensors is the benchmark's baseline."""
    cs = device_csf("thin")
    mats = [m.cuda() for m in make_mats("thin", rank)]
    for mode in range(3):
        B0 = make_b("thin", rank, mode).cuda()
        kw = dict(inner_tol=0.0, max_inner=1)
        got = run_pdnr(cs, mats, mode, B0, "torch", **kw)
        assert all(x.is_cuda for x in got.values())
        compare(got, oracle_one("thin", rank, mode),
                f"torch-on-device thin rank {rank} mode {mode}",
                exact_counts=True)
        auto = run_pdnr(cs, mats, mode, B0, "auto", **kw)
        hip = run_pdnr(cs, mats, mode, B0, "hip", **kw)
        for k in auto:
            assert torch.equal(auto[k], hip[k]), k


def test_cpd_apr_pdnr_device_planted():
    t, _, _ = planted()
    r = sp.cpd_apr(t.to("cuda"), 4, sp.AprOptions(**PLANTED_PDNR))
    assert all(f.is_cuda for f in r.factors) and r.lam.is_cuda
    check_planted_pdnr(r)


def test_cpd_apr_pdnr_device_short_schedule_matches_cpu():
    cpu = short_schedule_cpu()
    dev = sp.cpd_apr(INPUTS["4-mode"]().to("cuda"), 8,
                     sp.AprOptions(**DRV_PDNR))
    assert dev.niters == cpu.niters == 5
    err = max(abs(a - b) / abs(b)
              for a, b in zip(dev.loglik_trace, cpu.loglik_trace))
    print(f"driver trace, device vs CPU: {err:.3e} "
          f"(DRV_TOL_PDNR {DRV_TOL_PDNR:.1e})")
    assert err <= DRV_TOL_PDNR


def test_update_hip_rejects_negative_values():
    t = heavy()
    neg = sp.SpTensor(t.inds.clone(), t.vals - 2.0, list(t.dims)).to("cuda")
    mats = [m.cuda() for m in make_mats("heavy", 16)]
    with pytest.raises(ValueError, match=">= 0"):
        sp.apr_update_pdnr(sp.csf_alloc(neg, "all"), mats, 0,
                           make_b("heavy", 16, 0).cuda(), inner_tol=0.0,
                           max_inner=1)
