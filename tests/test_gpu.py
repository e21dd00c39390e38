"""GPU numerics: every HIP kernel against the plain CPU fp64 oracle.
All tests require an MI355X (run via gpurun / the round-end driver)."""
import pytest
import torch

import splatt_amd as sp
from splatt_amd.csf import build_csf

pytestmark = pytest.mark.gpu

POLICIES = ["one", "two", "all"]


@pytest.fixture(scope="module")
def t3():
    return sp.SpTensor.synthetic([300, 250, 400], 120_000, seed=17)


def make_mats(dims, rank, seed=123, device="cpu"):
    return [sp.seeded_init(d, rank, m, seed).to(device)
            for m, d in enumerate(dims)]


def test_native_arch():
    from splatt_amd._ext import native
    assert native().hip_arch() == 950


@pytest.mark.parametrize("alg", ["flat", "csf"])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rank", [16, 32, 64])
def test_gpu_mttkrp_matches_oracle(t3, policy, rank, alg):
    mats_c = make_mats(t3.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t3.to("cuda"), policy)
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode, alg=alg)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        err = (out.cpu() - ref).abs().max().item()
        assert err < 1e-8, (policy, rank, mode, alg, err)


@pytest.mark.parametrize("nm_dims,nnz", [([60, 50, 70, 40], 80_000),
                                         ([30, 25, 35, 20, 15], 60_000)])
def test_gpu_mttkrp_flat_nmode(nm_dims, nnz):
    t = sp.SpTensor.synthetic(nm_dims, nnz, seed=31)
    mats_c = make_mats(t.dims, 16)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t.to("cuda"), "two")
    for mode in range(len(nm_dims)):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode


def test_gpu_mttkrp_generic_rank(t3):
    """rank 7 exercises the generic fallback kernel."""
    mats_c = make_mats(t3.dims, 7)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t3.to("cuda"), "two")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8


def test_gpu_mttkrp_f32(t3):
    t32 = sp.SpTensor(t3.inds, t3.vals.float(), t3.dims)
    mats_c = [m.float() for m in make_mats(t3.dims, 16)]
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t32.to("cuda"), "two")
    ref64 = [sp.mttkrp_stream(t3, make_mats(t3.dims, 16), m) for m in range(3)]
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        assert (out.double().cpu() - ref64[mode]).abs().max().item() < 2e-2


def test_gpu_csf_build_matches_cpu(t3):
    perm = sp.order_modes(t3.dims, "smallfirst")
    a = build_csf(t3, perm)
    b = build_csf(t3.to("cuda"), perm)
    for l in range(3):
        for x, y in ((a.fptr[l], b.fptr[l]), (a.fids[l], b.fids[l])):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x, y.cpu())
    assert torch.equal(a.vals, b.vals.cpu())


def test_gpu_cpd_matches_cpu(t3):
    opts = sp.CpdOptions(max_iters=5, tolerance=0.0)
    k_cpu = sp.cpd_als(t3, 16, opts)
    k_gpu = sp.cpd_als(sp.csf_alloc(t3.to("cuda"), "two"), 16, opts)
    assert abs(k_cpu.fit - k_gpu.fit) < 1e-6
    for a, b in zip(k_cpu.fit_trace, k_gpu.fit_trace):
        assert abs(a - b) < 1e-6


def test_gpu_atomic_heavy_small_dims():
    """Tiny output dims -> maximal atomic contention on every kernel."""
    t = sp.SpTensor.synthetic([8, 6, 2000], 200_000, seed=23)
    mats_c = make_mats(t.dims, 16)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t.to("cuda"), "one")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-7


@pytest.mark.parametrize("rank", [8, 16, 32, 64])
def test_gpu_gram_matches_blas(rank):
    from splatt_amd.ops.dense import gram
    A = torch.rand(29818, rank, dtype=torch.float64).cuda()
    G = gram(A)
    ref = (A.T @ A)
    assert (G - ref).abs().max().item() < 1e-8


def test_gpu_flat_only_build_matches(t3):
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    mats_c = make_mats(t3.dims, 16)
    mats_g = [m.cuda() for m in mats_c]
    td = t3.to("cuda")
    cs = build_shard_csf(td, list(t3.dims), "all", flat_only=True)
    for c in cs.csfs:
        assert all(fp is None for fp in c.fptr)
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8


def test_gpu_gather_tiled_build_matches(t3):
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    mats_c = make_mats(t3.dims, 16)
    mats_g = [m.cuda() for m in mats_c]
    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                         flat_only=True, gather_tiles=4)
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8


@pytest.mark.parametrize("rank", [16, 32])
def test_gpu_lds_staged_matches(t3, rank):
    """LDS-staged kernel vs oracle (bucketed stage_rank build)."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    mats_c = make_mats(t3.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                         flat_only=True, stage_rank=rank)
    assert any(getattr(c, "_stage", None) is not None for c in cs.csfs)
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode


def test_gpu_lds_staged_4mode():
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t = sp.SpTensor.synthetic([60, 900, 70, 40], 120_000, seed=31)
    mats_c = make_mats(t.dims, 16)
    mats_g = [m.cuda() for m in mats_c]
    cs = build_shard_csf(t.to("cuda"), list(t.dims), "all",
                         flat_only=True, stage_rank=16)
    for mode in range(4):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode


@pytest.mark.parametrize("rank", [8, 16, 32, 64])
def test_gpu_spd_inverse(rank):
    from splatt_amd.ops.dense import spd_inverse
    A = torch.rand(500, rank, dtype=torch.float64).cuda()
    G = A.T @ A + 0.1 * torch.eye(rank, dtype=torch.float64).cuda()
    Ginv = spd_inverse(G)
    err = (G @ Ginv - torch.eye(rank, dtype=torch.float64).cuda()).abs().max()
    assert float(err) < 1e-9


def test_gpu_graph_step_matches_eager(t3):
    """hipGraph-captured iteration == eager iteration (same fit)."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    from splatt_amd.parallel.grid import GridDecomp, grid_cpd_init, grid_cpd_step
    from splatt_amd.parallel.graph_exec import GraphStepRunner
    opts = sp.CpdOptions(max_iters=6, tolerance=0.0)
    dec = GridDecomp.create(list(t3.dims))

    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all", flat_only=True,
                         stage_rank=16)
    st = grid_cpd_init(cs, dec, 16, opts)
    grid_cpd_step(st, 0)
    runner = GraphStepRunner(st)
    assert runner.capture(), runner.capture_error
    for _ in range(3):
        runner.replay()
    fit_graph = runner.finalize(st.norm_x)

    st2 = grid_cpd_init(cs, dec, 16, opts)
    for it in range(6):  # 1 eager + 2 warmup-in-capture + 3 replays
        fit_eager = grid_cpd_step(st2, it)
    assert abs(fit_graph - fit_eager) < 1e-6, (fit_graph, fit_eager)


def test_gpu_mttkrp_flat_8mode():
    """8-mode tensors (SPLATT_MAX_NMODES) on the generic device path."""
    dims = [8, 9, 10, 7, 6, 8, 5, 9]
    t = sp.SpTensor.synthetic(dims, 30_000, seed=77)
    mats_c = make_mats(t.dims, 6)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t.to("cuda"), "one")
    for mode in (0, 3, 7):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode


def test_gpu_lowrank_recovery():
    """Device ALS must actually factorize: a rank-3 tensor reaches
    fit > 0.99 (quality, not just numerics-vs-oracle)."""
    g = torch.Generator().manual_seed(42)
    mats = [torch.rand(d, 3, generator=g, dtype=torch.float64)
            for d in (40, 30, 25)]
    dense = torch.einsum("ir,jr,kr->ijk", *mats)
    inds = (dense.abs() > -1).nonzero().T
    t = sp.SpTensor(inds, dense.flatten(), [40, 30, 25]).to("cuda")
    k = sp.cpd_als(sp.csf_alloc(t, "all"), 3,
                   sp.CpdOptions(max_iters=60, tolerance=1e-10))
    assert k.fit > 0.99


def test_gpu_mttkrp_rank128(t3):
    """Ranks beyond the 64-lane spec set use the generic column-chunked
    kernel."""
    mats_c = make_mats(t3.dims, 128)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t3.to("cuda"), "one")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8


def test_gpu_event_timer():
    from splatt_amd.utils.timers import CudaEventTimer
    t = CudaEventTimer()
    x = torch.rand(1 << 20, device="cuda")
    with t.time():
        for _ in range(4):
            x = x * 1.0001
    assert t.elapsed_ms() > 0.0


@pytest.mark.parametrize("rank", [16, 32, 64])
def test_gpu_gram_f32_mfma(rank):
    from splatt_amd.ops.dense import gram
    A = (torch.rand(20011, rank, dtype=torch.float32).cuda() - 0.5)
    G = gram(A)
    ref = A.double().T @ A.double()
    assert (G.double() - ref).abs().max().item() < 0.05  # f32 accumulation


def test_gpu_rccl_rs_ag_helpers(tmp_path):
    """Exercise the RCCL collective signatures used by the owned-row
    update path on a 1-rank NCCL group (validates the nccl code path the
    multi-GPU round-end run takes)."""
    import torch.distributed as dist
    from splatt_amd.parallel.grid import _all_gather_rows, _reduce_scatter_rows
    dist.init_process_group(
        "nccl", init_method=f"file://{tmp_path}/store1", rank=0, world_size=1)
    try:
        full = torch.rand(103, 16, dtype=torch.float64).cuda()
        want = full.clone()
        own, work = _reduce_scatter_rows(full, 0, 103, dist.group.WORLD, 1)
        if work is not None:
            work.wait()
        assert torch.allclose(own, want)
        out = torch.empty(103, 16, dtype=torch.float64).cuda()
        _all_gather_rows(own, 103, dist.group.WORLD, 1, out)
        assert torch.allclose(out, want)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("rank", [16, 32])
def test_gpu_deterministic_matches_oracle(t3, rank):
    """Deterministic (atomic-free) kernel vs the CPU oracle, all modes."""
    mats_c = make_mats(t3.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t3.to("cuda"), "all")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        err = (out.cpu() - ref).abs().max().item()
        assert err < 1e-8, (rank, mode, err)


def test_gpu_deterministic_bitwise_repeatable():
    """Two runs (with unrelated GPU work in between) must be torch.equal —
    the property the atomic path cannot give."""
    t = sp.SpTensor.synthetic([40, 60, 3000], 400_000, seed=31)
    mats = [m.cuda() for m in make_mats(t.dims, 16)]
    cs = sp.csf_alloc(t.to("cuda"), "all")
    for mode in range(3):
        a = sp.mttkrp(cs, mats, mode, deterministic=True).clone()
        _ = torch.rand(2048, 2048, device="cuda") @ \
            torch.rand(2048, 2048, device="cuda")   # unrelated traffic
        b = sp.mttkrp(cs, mats, mode, deterministic=True)
        assert torch.equal(a, b), mode


def test_gpu_deterministic_4mode():
    t = sp.SpTensor.synthetic([90, 120, 80, 40], 150_000, seed=41)
    mats_c = make_mats(t.dims, 32)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t.to("cuda"), "all")
    for mode in range(4):
        out = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode
        again = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        assert torch.equal(out, again)


def test_gpu_deterministic_rejects_unsupported(t3):
    mats = [m.cuda() for m in make_mats(t3.dims, 16)]
    cs2 = sp.csf_alloc(t3.to("cuda"), "one")   # non-root output depths
    deep_mode = next(m for m in range(3)
                     if cs2.mode_depth[m] != 0)
    with pytest.raises(ValueError, match="depth-0"):
        sp.mttkrp(cs2, mats, deep_mode, deterministic=True)
    mats7 = [m.cuda() for m in make_mats(t3.dims, 7)]
    csa = sp.csf_alloc(t3.to("cuda"), "all")
    with pytest.raises(ValueError, match="rank"):
        sp.mttkrp(csa, mats7, 0, deterministic=True)


def test_gpu_deterministic_cpd_repeatable():
    """SPLATT_DETERMINISTIC=1 -> whole device CPD is run-to-run identical."""
    import os
    t = sp.SpTensor.synthetic([150, 200, 180], 90_000, seed=53)
    os.environ["SPLATT_DETERMINISTIC"] = "1"
    try:
        opts = sp.CpdOptions(max_iters=4, tolerance=0.0, seed=9)
        k1 = sp.cpd_als(sp.csf_alloc(t.to("cuda"), "all"), 16, opts)
        k2 = sp.cpd_als(sp.csf_alloc(t.to("cuda"), "all"), 16, opts)
    finally:
        del os.environ["SPLATT_DETERMINISTIC"]
    assert k1.fit == k2.fit
    for a, b in zip(k1.factors, k2.factors):
        assert torch.equal(a, b)


def test_gpu_deterministic_on_staged_build():
    """LDS-bucketed builds reorder the stream bucket-major (the bench.py
    path); the det dispatch must detect that and run on a key-sorted copy."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t = sp.SpTensor.synthetic([500, 4000, 900], 300_000, seed=67).to("cuda")
    cs = build_shard_csf(t, [500, 4000, 900], "all", flat_only=True,
                         stage_rank=16)
    tc = sp.SpTensor.synthetic([500, 4000, 900], 300_000, seed=67)
    mats_c = make_mats(tc.dims, 16)
    mats_g = [m.cuda() for m in mats_c]
    assert any(getattr(c, "_stage", None) is not None for c in cs.csfs)
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        ref = sp.mttkrp_stream(tc, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode
        again = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        assert torch.equal(out, again), mode


@pytest.mark.parametrize("rank", [16, 32])
def test_gpu_rowsolve_matches_matmul(rank):
    from splatt_amd.ops.dense import solve_rows
    import os
    A = torch.rand(37813, rank, dtype=torch.float64).cuda()
    B = torch.rand(rank, rank, dtype=torch.float64).cuda()
    os.environ["SPLATT_DETERMINISTIC"] = "1"
    try:
        C = solve_rows(A, B)
        C2 = solve_rows(A, B)
    finally:
        del os.environ["SPLATT_DETERMINISTIC"]
    assert (C - A @ B).abs().max().item() < 1e-10
    assert torch.equal(C, C2)


def test_gpu_gram_det_matches():
    import os
    from splatt_amd.ops.dense import gram
    A = torch.rand(29818, 16, dtype=torch.float64).cuda()
    os.environ["SPLATT_DETERMINISTIC"] = "1"
    try:
        G = gram(A)
        G2 = gram(A)
    finally:
        del os.environ["SPLATT_DETERMINISTIC"]
    assert (G - A.T @ A).abs().max().item() < 1e-8
    assert torch.equal(G, G2)


def test_gpu_deterministic_graph_replay():
    """hipGraph-captured iteration under SPLATT_DETERMINISTIC=1: two
    independent capture+replay sequences must produce bitwise-equal
    factors (the graph path routes solve/gram through the det kernels)."""
    import os
    from splatt_amd.parallel.grid import GridDecomp, grid_cpd_init, \
        grid_cpd_step
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    from splatt_amd.parallel.graph_exec import GraphStepRunner

    def run():
        t = sp.SpTensor.synthetic([300, 260, 420], 150_000, seed=71,
                                  device="cuda")
        dec = GridDecomp.create([300, 260, 420])
        cs = build_shard_csf(t, [300, 260, 420], "all", flat_only=True)
        st = grid_cpd_init(cs, dec, 16, sp.CpdOptions(seed=5))
        grid_cpd_step(st, 0)   # iteration 0 eager (2-norm schedule)
        r = GraphStepRunner(st)
        assert r.capture(), r.capture_error
        for _ in range(3):
            r.replay()
        r.finalize(st.norm_x)
        return [a.clone() for a in st.factors], st.fit

    os.environ["SPLATT_DETERMINISTIC"] = "1"
    try:
        f1, fit1 = run()
        f2, fit2 = run()
    finally:
        del os.environ["SPLATT_DETERMINISTIC"]
    assert fit1 == fit2
    for a, b in zip(f1, f2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rank", [16, 32, 64])
def test_gpu_deterministic_cpd_matches_cpu(monkeypatch, rank):
    """SPLATT_DETERMINISTIC=1 routes gram/solve through the atomic-free
    dense kernels; the fit trace must still be the CPU's, at every spec
    rank (F*F > 256 above rank 16)."""
    t = sp.SpTensor.synthetic([60, 50, 70], 20_000, seed=53)
    opts = sp.CpdOptions(max_iters=4, tolerance=0.0)
    k_cpu = sp.cpd_als(t, rank, opts)
    monkeypatch.setenv("SPLATT_DETERMINISTIC", "1")
    k_gpu = sp.cpd_als(sp.csf_alloc(t.to("cuda"), "all"), rank, opts)
    assert len(k_cpu.fit_trace) == len(k_gpu.fit_trace) == 4
    for it, (a, b) in enumerate(zip(k_cpu.fit_trace, k_gpu.fit_trace)):
        print(f"det cpd rank {rank} it {it}: cpu {a:.12f} gpu {b:.12f}")
        assert abs(a - b) < 1e-6, (rank, it, a, b)


def test_gpu_deterministic_graph_step_matches_eager(monkeypatch, t3):
    """Deterministic twin of test_gpu_graph_step_matches_eager at rank 32:
    the captured iteration keeps its Gram buffers across replays, so an
    element gram_det does not rewrite stays at its iteration-0 value."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    from splatt_amd.parallel.grid import GridDecomp, grid_cpd_init, grid_cpd_step
    from splatt_amd.parallel.graph_exec import GraphStepRunner
    monkeypatch.setenv("SPLATT_DETERMINISTIC", "1")
    opts = sp.CpdOptions(max_iters=6, tolerance=0.0)
    dec = GridDecomp.create(list(t3.dims))

    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all", flat_only=True,
                         stage_rank=32)
    st = grid_cpd_init(cs, dec, 32, opts)
    grid_cpd_step(st, 0)
    runner = GraphStepRunner(st)
    assert runner.det
    assert runner.capture(), runner.capture_error
    for _ in range(3):
        runner.replay()
    fit_graph = runner.finalize(st.norm_x)
    # the Gram buffers the replays kept must describe the final factors
    # (dot-product forward bound, as in test_dense_gpu.py)
    for m in range(3):
        A = st.factors[m].cpu()
        bound = 2 * A.shape[0] * 2.0 ** -53 * (A.abs().T @ A.abs())
        err = (st.grams[m].cpu() - A.T @ A).abs()
        assert bool((err <= bound).all()), (m, float((err / bound).max()))

    st2 = grid_cpd_init(cs, dec, 32, opts)
    for it in range(6):  # 1 eager + 2 warmup-in-capture + 3 replays
        fit_eager = grid_cpd_step(st2, it)
    assert abs(fit_graph - fit_eager) < 1e-6, (fit_graph, fit_eager)


@pytest.mark.parametrize("rank", [4, 8, 64])
def test_gpu_deterministic_matches_oracle_other_ranks(rank):
    """Ranks 4 and 64 have 16 and 1 sub-spans per wave."""
    t = sp.SpTensor.synthetic([40, 30, 50], 6_000, seed=31)
    mats_c = make_mats(t.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    cs = sp.csf_alloc(t.to("cuda"), "all")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        err = (out.cpu() - ref).abs().max().item()
        assert err < 1e-8, (rank, mode, err)
        again = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        assert torch.equal(out, again), (rank, mode)


def test_gpu_cpd_regularize():
    t = sp.SpTensor.synthetic([100, 80, 120], 30_000, seed=19)
    o0 = sp.CpdOptions(max_iters=5, tolerance=0.0, seed=3)
    ob = sp.CpdOptions(max_iters=5, tolerance=0.0, seed=3, regularize=20.0)
    k0 = sp.cpd_als(sp.csf_alloc(t.to("cuda"), "all"), 8, o0)
    kb = sp.cpd_als(sp.csf_alloc(t.to("cuda"), "all"), 8, ob)
    assert kb.fit < k0.fit and kb.fit == kb.fit


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("rank", [16, 32])
def test_gpu_mttkrp_rows_restricted(t3, staged, rank):
    """rows=(lo,hi) partial launches (the chunked comm pipeline's building
    block) tile the full result exactly, on both the plain flat kernel
    (key-sorted stream) and the LDS-staged bucketed build."""
    from splatt_amd.mttkrp import mttkrp_rows_ok
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                         flat_only=True, stage_rank=rank if staged else 0)
    mats_c = make_mats(t3.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    for mode in range(3):
        assert mttkrp_rows_ok(cs, mode, rank)
        full = sp.mttkrp(cs, mats_g, mode)
        out = torch.empty_like(full)
        n = t3.dims[mode]
        bounds = [0, n // 4, n // 2, (3 * n) // 4, n]
        for i in range(4):
            sp.mttkrp(cs, mats_g, mode, out=out,
                      rows=(bounds[i], bounds[i + 1]))
        err = (out - full).abs().max().item()
        assert err < 1e-10, (staged, rank, mode, err)
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        err2 = (out.cpu() - ref).abs().max().item()
        assert err2 < 1e-8, (staged, rank, mode, err2)


def test_gpu_generic_rank_graph_capturable(t3):
    """The generic-rank fallback must be hipGraph-capturable (ADVICE r1:
    no hipStreamSynchronize/blocking copies inside the launch path)."""
    rank = 10   # not in the spec set -> generic kernel
    cs = sp.csf_alloc(t3.to("cuda"), "all")
    mats_g = make_mats(t3.dims, rank, device="cuda")
    ref = sp.mttkrp(cs, mats_g, 0)
    out = torch.empty_like(ref)
    sp.mttkrp(cs, mats_g, 0, out=out)   # warm
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.mttkrp(cs, mats_g, 0, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert (out - ref).abs().max().item() < 1e-10


@pytest.mark.parametrize("rank", [16, 32])
def test_gpu_packed_stream_matches(t3, rank):
    """v6 packed-stream LDS kernel == v5 separate-stream kernel == oracle
    on staged builds (3- and 4-mode)."""
    import os
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    for t in (t3, sp.SpTensor.synthetic([120, 90, 150, 40], 60_000, seed=9)):
        cs = build_shard_csf(t.to("cuda"), list(t.dims), "all",
                             flat_only=True, stage_rank=rank)
        assert any(getattr(c, "_pack", None) is not None for c in cs.csfs)
        mats_c = make_mats(t.dims, rank)
        mats_g = [m.cuda() for m in mats_c]
        for mode in range(t.nmodes):
            out6 = sp.mttkrp(cs, mats_g, mode)
            os.environ["SPLATT_NO_PACK"] = "1"
            try:
                out5 = sp.mttkrp(cs, mats_g, mode)
            finally:
                del os.environ["SPLATT_NO_PACK"]
            assert (out6 - out5).abs().max().item() < 1e-10
            ref = sp.mttkrp_stream(t, mats_c, mode)
            assert (out6.cpu() - ref).abs().max().item() < 1e-8


@pytest.mark.parametrize("staged", [True, False])
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_gpu_factor_store_mttkrp(t3, store, staged):
    """Reduced-precision factor STORAGE (SPLATT_FACTOR_STORE): gathers
    read f32/bf16 rows, accumulation stays f64; result tracks the f64
    oracle within storage precision (ROADMAP 2b documented mode), on
    both the LDS-staged packed path and the plain v2 path."""
    import os
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    rank = 16
    os.environ["SPLATT_FACTOR_STORE"] = store
    try:
        cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                             flat_only=True,
                             stage_rank=rank if staged else 0)
        mats_c = make_mats(t3.dims, rank)
        qdt = {"f32": torch.float32, "bf16": torch.bfloat16}[store]
        mats_q = [m.cuda().to(qdt) for m in mats_c]
        tol = {"f32": 5e-5, "bf16": 2e-1}[store]
        for mode in range(3):
            out = sp.mttkrp(cs, mats_q, mode)
            assert out.dtype == torch.float64
            ref = sp.mttkrp_stream(t3, mats_c, mode)
            rel = ((out.cpu() - ref).abs().max()
                   / ref.abs().max()).item()
            assert rel < tol, (store, mode, rel)
    finally:
        del os.environ["SPLATT_FACTOR_STORE"]


def test_gpu_factor_store_cpd_converges(t3):
    """bf16-store CPD-ALS reaches a fit close to the f64 run."""
    import os
    ref = sp.cpd_als(sp.csf_alloc(t3.to("cuda"), "all"), 16,
                     sp.CpdOptions(max_iters=4, tolerance=0.0))
    os.environ["SPLATT_FACTOR_STORE"] = "bf16"
    try:
        from splatt_amd.parallel.dist_cpd import build_shard_csf
        cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                             flat_only=True, stage_rank=16)
        k = sp.cpd_als(cs, 16, sp.CpdOptions(max_iters=4, tolerance=0.0))
    finally:
        del os.environ["SPLATT_FACTOR_STORE"]
    assert abs(k.fit - ref.fit) < 5e-3, (k.fit, ref.fit)


def test_gpu_det6_staged_deterministic(t3):
    """The LDS-staged deterministic kernel (det6: bucket-privatized
    outputs + ordered fixup + ascending-bucket fold) matches the oracle,
    matches the key-sorted det kernel bitwise-relevantly (both exact),
    and is bitwise-repeatable."""
    import os
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    rank = 16
    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                         flat_only=True, stage_rank=rank)
    assert any(getattr(c, "_pack", None) is not None for c in cs.csfs)
    mats_c = make_mats(t3.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    for mode in range(3):
        a = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        b = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        assert torch.equal(a, b), mode          # bitwise repeatable
        ref = sp.mttkrp_stream(t3, mats_c, mode)
        assert (a.cpu() - ref).abs().max().item() < 1e-8, mode
        # force the fallback key-sorted det kernel; values agree to fp
        os.environ["SPLATT_NO_DET6"] = "1"
        try:
            d = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        finally:
            del os.environ["SPLATT_NO_DET6"]
        assert (a - d).abs().max().item() < 1e-9, mode


def test_gpu_det6_small_budget_fallback(t3):
    """With a tiny SPLATT_DET_MB the dispatcher falls back to the
    key-sorted det kernel and stays correct."""
    import os
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    rank = 16
    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all",
                         flat_only=True, stage_rank=rank)
    mats_c = make_mats(t3.dims, rank)
    mats_g = [m.cuda() for m in mats_c]
    os.environ["SPLATT_DET_MB"] = "0"
    try:
        a = sp.mttkrp(cs, mats_g, 0, deterministic=True)
    finally:
        del os.environ["SPLATT_DET_MB"]
    ref = sp.mttkrp_stream(t3, mats_c, 0)
    assert (a.cpu() - ref).abs().max().item() < 1e-8


@pytest.mark.timeout(420)
def test_gpu_chunked_pipeline_two_ranks_one_gpu(tmp_path):
    """Composition test for the chunked comm/compute pipeline with REAL
    device tensors and kernels: two ranks share this GPU over gloo
    (SPLATT_BENCH_BACKEND=gloo), running bench.py's exact distributed
    code path (medium grid, chunked RS/AG, rows-restricted launches).
    RCCL semantics are exercised by the driver's multi-GPU run; this
    pins the GPU-side math and launch plumbing beforehand."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1",
               SPLATT_BENCH_CONFIG="small",
               SPLATT_BENCH_BACKEND="gloo",
               SPLATT_FORCE_RS_PRIMS="1",
               SPLATT_COMM_CHUNK_MIN_MB="0")
    # one retry: torchrun rendezvous on a busy box can transiently fail
    for attempt in range(2):
        r = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--standalone",
             "--nnodes=1", "--nproc-per-node", "2", "--local-addr",
             "127.0.0.1", "bench.py", "--gpus", "2", "--steps", "2",
             "--warmup", "1"],
            capture_output=True, text=True, cwd=root, env=env, timeout=400)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr[-1500:]
    j = json.loads([l for l in r.stdout.strip().splitlines()
                    if l.startswith("{")][0])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong"
    # single-process fit on the same global tensor must match (the
    # rank-invariance property, reference mpi_mat_rand)
    assert 0.0 <= j["config"]["fit"] < 1.0


def test_gpu_bench_harness_lds_alg(t3):
    """`bench` harness's 'lds' algorithm (the production staged path)
    validates against the oracle and beats/equals plain flat."""
    from splatt_amd.benchmarks import bench_mttkrp
    r = bench_mttkrp(t3, 16, ["flat", "lds"], 2, device="cuda",
                     validate=True)
    assert r["flat"]["validated"] and r["lds"]["validated"]


# ------------------------------------------------------------------------
# One case per launcher x element type that nothing above drives, at the
# smallest shapes that still take each path: [40, 30, 150] with 2400
# nonzeros (SPLATT_LDS_KB=1 cuts the 150-row mode into three 64-row LDS
# buckets, one block each), rank 8 for the specialised kernels and rank 5
# for the generic ones.

SMALL_DIMS = [40, 30, 150]


@pytest.fixture(scope="module")
def small3():
    """(tensor, {rank: (f64 factors, f64 oracle per mode, f32 bound per
    mode)}). The bound is test_gpu_mttkrp_f32's 2e-2, tightened elementwise
    by the forward bound of an f32 sum of products in any order:
    |err| <= k u sum|terms| with u = 2^-24 and k < nnz + 2 nmodes roundings
    per term (value, factor entries, products) and per partial sum."""
    t = sp.SpTensor.synthetic(SMALL_DIMS, 2400, seed=5)
    tabs = sp.SpTensor(t.inds, t.vals.abs(), t.dims)
    k = t.nnz + 2 * t.nmodes
    cases = {}
    for rank in (8, 5):
        mats_c = make_mats(t.dims, rank)
        refs = [sp.mttkrp_stream(t, mats_c, m) for m in range(3)]
        mags = [sp.mttkrp_stream(tabs, [a.abs() for a in mats_c], m)
                for m in range(3)]
        bounds = [torch.clamp(k * 2.0 ** -24 * g, max=2e-2) for g in mags]
        cases[rank] = (mats_c, refs, bounds)
    return t, cases


def _as_f32(t, mats_c):
    return (sp.SpTensor(t.inds, t.vals.float(), t.dims).to("cuda"),
            [m.float().cuda() for m in mats_c])


def _assert_f32_close(out, ref, bound, what):
    assert out.dtype == torch.float32
    err = (out.double().cpu() - ref).abs()
    print(f"{what}: max err {float(err.max()):.3e}, "
          f"max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("alg,policy,rank", [("csf", "one", 8),
                                             ("csf", "one", 5),
                                             ("flat", "two", 5)])
def test_gpu_mttkrp_f32_small(small3, alg, policy, rank):
    """f32 through gpu_mttkrp3 (root/internal/leaf of one CSF; spec and
    generic kernels) and through the generic-rank flat kernel."""
    t, cases = small3
    mats_c, refs, bounds = cases[rank]
    t32, mats_g = _as_f32(t, mats_c)
    cs = sp.csf_alloc(t32, policy)
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode, alg=alg)
        _assert_f32_close(out, refs[mode], bounds[mode], (alg, rank, mode))


@pytest.mark.parametrize("packed", [True, False], ids=["flat6", "flat5"])
def test_gpu_lds_staged_f32_small(small3, monkeypatch, packed):
    """f32 through the LDS-staged kernels, packed and separate streams."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t, cases = small3
    mats_c, refs, bounds = cases[8]
    t32, mats_g = _as_f32(t, mats_c)
    monkeypatch.setenv("SPLATT_LDS_KB", "1")
    cs = build_shard_csf(t32, SMALL_DIMS, "all", flat_only=True, stage_rank=8)
    assert all(getattr(c, "_pack", None) is not None for c in cs.csfs)
    assert any(c._stage["nbuckets"] == 3 for c in cs.csfs)
    if not packed:
        monkeypatch.setenv("SPLATT_NO_PACK", "1")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode)
        _assert_f32_close(out, refs[mode], bounds[mode], (packed, mode))


@pytest.mark.parametrize("staged", [True, False], ids=["det6", "flat_det"])
def test_gpu_deterministic_f32_small(small3, monkeypatch, staged):
    """f32 through both deterministic kernels: oracle + bitwise repeat."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t, cases = small3
    mats_c, refs, bounds = cases[8]
    t32, mats_g = _as_f32(t, mats_c)
    if staged:
        monkeypatch.setenv("SPLATT_LDS_KB", "1")
        cs = build_shard_csf(t32, SMALL_DIMS, "all", flat_only=True,
                             stage_rank=8)
        assert all(getattr(c, "_pack", None) is not None for c in cs.csfs)
    else:
        cs = sp.csf_alloc(t32, "all")
    for mode in range(3):
        out = sp.mttkrp(cs, mats_g, mode, deterministic=True).clone()
        _assert_f32_close(out, refs[mode], bounds[mode], (staged, mode))
        again = sp.mttkrp(cs, mats_g, mode, deterministic=True)
        assert torch.equal(out, again), mode


def test_gpu_lds_staged_5mode():
    """Five modes: the staged separate-stream kernel with four other modes
    (no packed stream above four modes)."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    t = sp.SpTensor.synthetic([8, 12, 9, 11, 10], 2000, seed=7)
    mats_c = make_mats(t.dims, 8)
    mats_g = [m.cuda() for m in mats_c]
    cs = build_shard_csf(t.to("cuda"), list(t.dims), "all", flat_only=True,
                         stage_rank=8)
    for c in cs.csfs:
        assert getattr(c, "_stage", None) is not None
        assert getattr(c, "_pack", None) is None
    for mode in range(5):
        out = sp.mttkrp(cs, mats_g, mode)
        ref = sp.mttkrp_stream(t, mats_c, mode)
        assert (out.cpu() - ref).abs().max().item() < 1e-8, mode
