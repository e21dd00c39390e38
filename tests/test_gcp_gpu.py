"""Generalized CPD (GCP) on the MI355X: the HIP loss-gradient kernels against
the CPU oracles of tests/test_gcp.py (same inputs, same bounds).

Largest device errors observed, relative to max(1, max|oracle|): 3.4e-14
over the all-losses cases (heavy, rayleigh, rank 1; per loss between 4.1e-15
for gaussian and 3.4e-14, so the device's exp and log do not show) and
4.1e-15 over the edge-row cases (bound TOL = 1.2e-11); the driver's loss
trace on the fixed schedule differed from the CPU run by at most 1.5e-15
relative (gaussian; bound DRV_TOL = 1.6e-12), with equal iteration and
evaluation counts.
"""
import pytest
import torch

import splatt_amd as sp
from splatt_amd import completion, gcp

from test_gcp import (ALL_INPUTS, BOUNDED, DOMAIN, DRV_TOL, EDGE_LOSSES,
                      EDGE_RANKS, FIXED_DRV, FIXED_LOSSES, LOSSES,
                      PLANTED_LOSSES, RANKS, assert_close,
                      check_domain_rejections, check_edges,
                      check_every_loss_driver, check_exact,
                      check_fg, check_losses, check_planted,
                      check_sample_zeros, check_stored_zeros, csf_of,
                      fixed_schedule_cpu, make_input, make_mats, oracle_case,
                      param_of, trace_err)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rank", RANKS)
def test_exact_hip(rank):
    """Bit for bit, single- and multi-segment rows, G and frow."""
    check_exact("hip", "cuda", rank)


@pytest.mark.parametrize("loss", EDGE_LOSSES)
@pytest.mark.parametrize("rank", EDGE_RANKS)
def test_edges_hip(rank, loss):
    check_edges("hip", "cuda", rank, loss)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", ALL_INPUTS)
def test_losses_hip(name, rank, loss):
    check_losses("hip", "cuda", name, rank, loss)


def test_plan_has_both_kinds_of_rows():
    for mode in range(3):
        plan = gcp.gcp_plan(csf_of("heavy", "any", "cuda"), mode)
        assert plan["nsingle"] > 100
        assert plan["mrow"].numel() == 7
        assert len(plan["batches"]) == 1
        assert int(plan["seg_len"].max()) == completion.SEG


@pytest.mark.parametrize("loss", LOSSES)
def test_fg_hip(loss):
    check_fg("hip", "cuda", loss)


def test_stored_zeros_hip():
    check_stored_zeros("hip", "cuda")


@pytest.mark.parametrize("loss", ["gaussian", "bernoulli-logit", "rayleigh"])
@pytest.mark.parametrize("rank", [16, 7])
def test_grad_is_reproducible(rank, loss):
    cs = csf_of("heavy", DOMAIN[loss], "cuda")
    mats = [m.cuda() for m in make_mats("heavy", rank, loss in BOUNDED)]
    for mode in range(3):
        a = sp.gcp_grad(cs, mats, mode, loss, want_loss=True, impl="hip")
        b = sp.gcp_grad(cs, mats, mode, loss, want_loss=True, impl="hip")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("rank", [16, 7])
def test_grad_auto_is_hip_and_torch_on_device_matches(rank):
    """impl='torch' on device tensors is the benchmark's baseline."""
    loss = "bernoulli-logit"
    cs = csf_of("thin", DOMAIN[loss], "cuda")
    mats = [m.cuda() for m in make_mats("thin", rank, False)]
    for mode in range(3):
        got = sp.gcp_grad(cs, mats, mode, loss, want_loss=True, impl="torch")
        assert all(x.is_cuda for x in got)
        assert_close(got, oracle_case("thin", rank, mode, loss),
                     f"torch-on-device thin rank {rank} mode {mode}")
        auto = sp.gcp_grad(cs, mats, mode, loss, want_loss=True)
        hip = sp.gcp_grad(cs, mats, mode, loss, want_loss=True, impl="hip")
        assert torch.equal(auto[0], hip[0]) and torch.equal(auto[1], hip[1])


def test_grad_on_a_single_csf_hip():
    cs = csf_of("4-mode", "any", "cuda")
    mats = [m.cuda() for m in make_mats("4-mode", 7, False)]
    got = sp.gcp_grad(cs.csfs[1], mats, 1, "gaussian", want_loss=True)
    assert_close(got, oracle_case("4-mode", 7, 1, "gaussian"), "single csf")


def test_domain_rejections_device():
    check_domain_rejections("cuda")


@pytest.mark.parametrize("loss", PLANTED_LOSSES)
def test_cpd_gcp_device_planted(loss):
    check_planted("cuda", loss)


@pytest.mark.parametrize("loss", LOSSES)
def test_every_loss_driver_hip(loss):
    check_every_loss_driver("cuda", loss)


@pytest.mark.parametrize("loss", FIXED_LOSSES)
def test_cpd_gcp_device_fixed_schedule_matches_cpu(loss):
    cpu = fixed_schedule_cpu(loss)
    dev = sp.cpd_gcp(make_input("4-mode", DOMAIN[loss]).to("cuda"), 8, loss,
                     sp.GcpOptions(param=param_of(loss), **FIXED_DRV))
    assert (dev.niters, dev.nfev) == (cpu.niters, cpu.nfev)
    err = trace_err(dev.loss_trace, cpu.loss_trace)
    print(f"{loss} driver trace, device vs CPU: {err:.3e} "
          f"(DRV_TOL {DRV_TOL:.1e})")
    assert err <= DRV_TOL


def test_sample_zeros_device():
    check_sample_zeros("cuda")
