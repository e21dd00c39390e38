"""Constrained CPD (AO-ADMM) on the MI355X: the fused block-ADMM kernel
against the oracles of tests/test_admm.py (same inputs, same bounds), then
the driver on device against its CPU run."""
import math

import pytest
import torch

import splatt_amd as sp

from test_admm import (BR, DRIVER_ITERS, EXACT_CONS, EXACT_RANKS, EXACT_ROWS,
                       FLOAT_ITERS, FLOAT_RANKS, REAL_CONS, STOP_CASES,
                       STOP_TOLS, assert_close, driver_opts, float_inputs,
                       float_oracle, float_stop_inputs, planted,
                       planted_nonneg_cpu, run_exact, run_float_stop,
                       run_stop)

pytestmark = pytest.mark.gpu


def hip_impls(rank):
    """The default kernel instance and, where a rank has two, both."""
    if rank in (16, 32, 64):
        return ["hip", "hip_valu", "hip_mfma"]
    return ["hip"]


# ------------------------------------------------------- 1. exact cases

@pytest.mark.parametrize("n", EXACT_ROWS)
@pytest.mark.parametrize("rank", EXACT_RANKS)
def test_exact_gemv_prox_hip(rank, n):
    for impl in hip_impls(rank):
        for kind in EXACT_CONS:
            run_exact(rank, n, kind, impl, "cuda")


@pytest.mark.parametrize("rank", [7, 16, 32, 64])
def test_exact_stopping_rule_hip(rank):
    for impl in hip_impls(rank):
        run_stop(rank, impl, "cuda")


# ------------------------------------- 2. float inputs at a fixed count

def run_fixed(rank, kind, impl):
    K, Ginv, rho, H, U = float_inputs(rank)
    K, Ginv, H, U = K.cuda(), Ginv.cuda(), H.cuda(), U.cuda()
    iters = sp.admm_update(K, Ginv, rho, H, U, REAL_CONS[kind],
                           inner_tol=0.0, max_inner=FLOAT_ITERS, impl=impl)
    assert iters.cpu().tolist() == [FLOAT_ITERS] * math.ceil(H.shape[0] / BR)
    return H, U


@pytest.mark.parametrize("kind", list(REAL_CONS))
@pytest.mark.parametrize("rank", FLOAT_RANKS)
def test_float_fixed_count_hip(rank, kind):
    Ho, Uo = float_oracle(rank, kind)
    for impl in hip_impls(rank):
        H, U = run_fixed(rank, kind, impl)
        assert_close(H, U, Ho, Uo, f"{impl} rank {rank} {kind}")


# ------------------------------- 3. float inputs with the stopping rule

@pytest.mark.parametrize("tol", STOP_TOLS)
@pytest.mark.parametrize("rank,kind", STOP_CASES)
def test_float_stopping_hip(rank, kind, tol):
    for impl in hip_impls(rank):
        run_float_stop(rank, kind, tol, impl, "cuda")


# --------------------------------------------------- 4. reproducibility

@pytest.mark.parametrize("rank", [7, 16, 64])
def test_hip_is_reproducible(rank):
    K, Ginv, rho, H0, U0 = float_stop_inputs(rank)
    K, Ginv = K.cuda(), Ginv.cuda()
    runs = []
    for _ in range(2):
        H, U = H0.cuda(), U0.cuda()
        it = sp.admm_update(K, Ginv, rho, H, U, sp.nonneg(), inner_tol=1e-4)
        runs.append((H, U, it))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------- 5. the torch baseline on device

@pytest.mark.parametrize("rank,kind", [(7, "box"), (16, "nonneg"),
                                       (32, "l1")])
def test_torch_on_device_matches_hip(rank, kind):
    Hh, Uh = run_fixed(rank, kind, "hip")
    Ht, Ut = run_fixed(rank, kind, "torch")
    assert_close(Ht, Ut, Hh.cpu(), Uh.cpu(), f"torch-on-device rank {rank}")
    # and the stopping counts: same oracle as the kernel's
    run_float_stop(rank, kind, 1e-2, "torch", "cuda")


def test_auto_is_hip_on_device():
    """impl="auto" on device tensors is the kernel: bit-equal to "hip"."""
    Ha, Ua = run_fixed(16, "nonneg", "auto")
    Hh, Uh = run_fixed(16, "nonneg", "hip")
    assert torch.equal(Ha, Hh) and torch.equal(Ua, Uh)


# ------------------------------------------------------ 6. the driver

def test_driver_on_device_matches_cpu():
    ref = planted_nonneg_cpu()
    k = sp.cpd_aoadmm(planted().to("cuda"), 4, sp.nonneg(), driver_opts())
    assert k.niters == DRIVER_ITERS
    for it, (a, b) in enumerate(zip(ref.fit_trace, k.fit_trace)):
        assert abs(a - b) < 1e-6, (it, a, b)
    for A in k.factors:
        assert A.is_cuda and float(A.min()) >= 0.0
    assert torch.equal(k.lam.cpu(), torch.ones(4, dtype=torch.float64))
    assert k.inner_iters == ref.inner_iters


def test_driver_4mode_on_device(med4):
    k = sp.cpd_aoadmm(med4.to("cuda"), 8, sp.nonneg(),
                      driver_opts(max_iters=15))
    assert len(k.fit_trace) == 15
    assert all(math.isfinite(f) for f in k.fit_trace)
    assert k.fit_trace[-1] >= k.fit_trace[0] - 1e-9
    assert all(float(A.min()) >= 0.0 for A in k.factors)


def test_cli_cpd_con_on_device(tmp_path, monkeypatch, capsys):
    """`splatt cpd --con` on the production device build (flat streams +
    LDS-staged buckets at rank 16) writes non-negative modeN.mat files."""
    from splatt_amd.cli import main
    t = sp.SpTensor.synthetic([300, 250, 400], 20_000, seed=17)
    path = str(tmp_path / "t.tns")
    t.save(path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert main(["cpd", path, "-r", "16", "-i", "3", "--device", "cuda",
                 "--con", "nonneg"]) == 0
    out = capsys.readouterr().out
    assert "Final fit:" in out and "inner iterations:" in out
    for m, d in enumerate(t.dims):
        rows = [[float(x) for x in line.split()]
                for line in open(tmp_path / f"mode{m + 1}.mat")]
        assert len(rows) == d and all(len(r) == 16 for r in rows)
        assert min(min(r) for r in rows) >= 0.0
