"""Dense ALS kernels (csrc/hip/dense_kernels.hip) at the shapes where their
launch arithmetic changes: Gram (MFMA, generic, deterministic), row solve,
SPD inverse and the column helpers of the C-API driver.

Exact-integer method: inputs are small integers stored as floats, chosen so
that every product and every partial sum is exactly representable. Any
summation order (atomic or not, MFMA or scalar) then gives the same bits,
the reference is an int64 CPU computation and the comparison is
torch.equal. Each case asserts its own no-rounding precondition on the CPU.
Every buffer a kernel must fully write is NaN-prefilled, so an element the
kernel skips cannot pass by luck. One float-input case per kernel family
covers rounding, against a derived forward-error bound."""
import functools
import math

import pytest
import torch

from splatt_amd._ext import native
from splatt_amd.ops import dense

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]

# launch_gram: ceil(n/128) blocks (cap 2048), 32-row LDS tiles, 16 rows per
# MFMA loop trip of a block. 2051 is prime (16+ blocks, no aligned range);
# 300001 is past the block cap (147 rows per block).
GRAM_RANKS = [1, 4, 7, 8, 16, 17, 24, 32, 48, 64]
GRAM_NS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 130, 2051]
N_CAPPED = 300001


def stream():
    return torch.cuda.current_stream().cuda_stream


def unit_roundoff(dtype):
    return 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24


def int_limit(dtype):
    return 8 if dtype == torch.float64 else 4


def assert_exact_premise(nterms, amax, bmax, dtype):
    """A sum of `nterms` products |a*b| <= amax*bmax stays an exactly
    representable integer at every partial sum."""
    cap = 2 ** 53 if dtype == torch.float64 else 2 ** 24
    assert nterms * amax * bmax < cap, (nterms, amax, bmax, dtype)


@functools.lru_cache(maxsize=None)
def int_matrix(n, F, dtype, seed=0):
    """int64 CPU matrix with entries in {-lim..lim} (lim 8 for f64, 4 for
    f32), seeded per shape."""
    lim = int_limit(dtype)
    g = torch.Generator().manual_seed(1000003 * seed + 131 * n + F)
    return torch.randint(-lim, lim + 1, (n, F), generator=g,
                         dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def gram_case(n, F, dtype):
    """(device A, exact reference G as `dtype` on the CPU)."""
    Ai = int_matrix(n, F, dtype)
    amax = int(Ai.abs().max())
    assert_exact_premise(n, amax, amax, dtype)
    ref = Ai.T @ Ai                                   # int64, exact
    return Ai.to(dtype).cuda(), ref.to(dtype)


def det_nparts(n):
    """The partial count ops.dense.gram and GraphStepRunner use."""
    return max(1, min(256, (n + 63) // 64))


def run_gram(A):
    F = A.shape[1]
    G = torch.zeros(F, F, dtype=A.dtype, device="cuda")
    native().gpu_gram(A, G, stream())
    return G


def run_gram_det(A, nparts):
    """Direct call with NaN-prefilled workspace and output."""
    F = A.shape[1]
    Gpart = torch.full((nparts * F * F,), float("nan"), dtype=A.dtype,
                       device="cuda")
    G = torch.full((F, F), float("nan"), dtype=A.dtype, device="cuda")
    native().gpu_gram_det(A, Gpart, G, stream())
    return G, Gpart.view(nparts, F, F)


# ------------------------------------------------------------------ Gram

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rank", GRAM_RANKS)
def test_gram_exact(rank, dtype):
    """gpu_gram (MFMA at 16/32/64, gram_kern PAIRS 1/4/16 otherwise)."""
    for n in GRAM_NS:
        A, ref = gram_case(n, rank, dtype)
        assert torch.equal(run_gram(A).cpu(), ref), (n, rank)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rank", GRAM_RANKS)
def test_gram_det_exact(rank, dtype):
    """gpu_gram_det on both sides of F*F = 256. Besides the partial count
    the library uses, small n also runs with 1 part and with 256 parts
    (n < nparts: blocks with an empty row range contribute exact zeros)."""
    for n in GRAM_NS:
        A, ref = gram_case(n, rank, dtype)
        counts = {det_nparts(n)}
        if n <= 130:
            counts |= {1, 256}
        for nparts in sorted(counts):
            G, Gpart = run_gram_det(A, nparts)
            assert torch.equal(G.cpu(), ref), (n, rank, nparts)
            # every partial is written, and they add up to the reference
            assert torch.equal(Gpart.sum(dim=0).cpu(), ref), (n, rank, nparts)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rank", [16, 64, 24])
def test_gram_exact_past_block_cap(rank, dtype):
    A, ref = gram_case(N_CAPPED, rank, dtype)
    assert torch.equal(run_gram(A).cpu(), ref)
    G, _ = run_gram_det(A, det_nparts(N_CAPPED))
    assert torch.equal(G.cpu(), ref)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rank", GRAM_RANKS)
def test_ops_gram_exact(monkeypatch, rank, dtype, det):
    """ops.dense.gram in both modes (allocates its own output)."""
    if det:
        monkeypatch.setenv("SPLATT_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("SPLATT_DETERMINISTIC", raising=False)
    for n in GRAM_NS:
        A, ref = gram_case(n, rank, dtype)
        # stale allocator blocks must not be able to stand in for a result
        junk = torch.full((rank, rank), float("nan"), dtype=dtype,
                          device="cuda")
        del junk
        assert torch.equal(dense.gram(A).cpu(), ref), (n, rank)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rank", [24, 32, 64])
def test_gram_det_bitwise_repeatable(rank, dtype):
    g = torch.Generator().manual_seed(7 + rank)
    A = (torch.rand(2051, rank, generator=g, dtype=torch.float64) - 0.5) \
        .to(dtype).cuda()
    G1, P1 = run_gram_det(A, det_nparts(2051))
    G2, P2 = run_gram_det(A, det_nparts(2051))
    assert torch.isfinite(G1).all()
    assert torch.equal(G1, G2) and torch.equal(P1, P2)


@pytest.mark.parametrize("kernel", ["gram", "gram_det"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rank", [16, 24, 64])
def test_gram_float_forward_bound(rank, dtype, kernel):
    """Rounding: A = rand - 0.5 against the f64 CPU product, elementwise
    |G - ref| <= 2 n u (|A|^T |A|) — the dot-product forward bound, with
    the factor 2 covering the reference's own rounding."""
    n = 2051
    g = torch.Generator().manual_seed(11 + rank)
    A = (torch.rand(n, rank, generator=g, dtype=torch.float64) - 0.5) \
        .to(dtype)
    A64 = A.double()
    ref = A64.T @ A64
    bound = 2 * n * unit_roundoff(dtype) * (A64.abs().T @ A64.abs())
    if kernel == "gram":
        G = run_gram(A.cuda())
    else:
        G, _ = run_gram_det(A.cuda(), det_nparts(n))
    err = (G.double().cpu() - ref).abs()
    print(f"gram float {kernel} F={rank} {dtype}: max err/bound = "
          f"{float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------- row solve

ROWSOLVE_NS = [1, 2, 63, 64, 65, 257]


def rowsolve_case(n, F, dtype):
    Ai = int_matrix(n, F, dtype, seed=1)
    Bi = int_matrix(F, F, dtype, seed=2)
    assert_exact_premise(F, int(Ai.abs().max()), int(Bi.abs().max()), dtype)
    return Ai.to(dtype).cuda(), Bi.to(dtype).cuda(), (Ai @ Bi).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("F", [4, 8, 16, 32, 64])
def test_rowsolve_exact(F, dtype):
    ns = list(ROWSOLVE_NS)
    if F == 64:
        # more rows than 8192 blocks x (256 // F) rows: second grid-stride trip
        ns.append(8192 * (256 // F) + 5)
    for n in ns:
        A, B, ref = rowsolve_case(n, F, dtype)
        C = torch.full((n, F), float("nan"), dtype=dtype, device="cuda")
        native().gpu_rowsolve(A, B, C, stream())
        assert torch.equal(C.cpu(), ref), (n, F)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("F", [4, 8, 16, 32, 64])
def test_solve_rows_deterministic_exact(monkeypatch, F, dtype):
    monkeypatch.setenv("SPLATT_DETERMINISTIC", "1")
    for n in (1, 65, 257):
        A, B, ref = rowsolve_case(n, F, dtype)
        assert torch.equal(dense.solve_rows(A, B).cpu(), ref), (n, F)


def test_rowsolve_rejects_generic_rank():
    A = torch.ones(5, 7, dtype=torch.float64, device="cuda")
    B = torch.eye(7, dtype=torch.float64, device="cuda")
    C = torch.empty_like(A)
    with pytest.raises(RuntimeError, match="rowsolve supports"):
        native().gpu_rowsolve(A, B, C, stream())


# ----------------------------------------------------------- SPD inverse

SPD_RANKS = [1, 2, 7, 8, 16, 17, 32, 33, 64]


def spd_matrix(F, kappa):
    """G = Q diag(s) Q^T in f64, s log-spaced in [1, kappa], symmetrised."""
    g = torch.Generator().manual_seed(97 + F)
    Q, _ = torch.linalg.qr(torch.randn(F, F, generator=g,
                                       dtype=torch.float64))
    s = torch.logspace(0, math.log10(kappa), F, dtype=torch.float64)
    G = (Q * s) @ Q.T
    return (G + G.T) / 2


def inv_residual(G, Ginv):
    """max |G Ginv - I|, evaluated in f64 on the CPU."""
    F = G.shape[0]
    return float((G.double() @ Ginv.double()
                  - torch.eye(F, dtype=torch.float64)).abs().max())


@pytest.mark.parametrize("dtype,kappa", [(torch.float64, 1e2),
                                         (torch.float64, 1e6),
                                         (torch.float32, 1e2)],
                         ids=["f64-1e2", "f64-1e6", "f32-1e2"])
@pytest.mark.parametrize("F", SPD_RANKS)
def test_spd_inverse_vs_lapack(F, dtype, kappa):
    """Residual relative to torch.linalg.inv at the kernel's precision:
    r_dev <= 16 r_ref + 4 F u. The kernel forms X^T X from an explicit
    triangular inverse, a constant factor less accurate than potri."""
    u = unit_roundoff(dtype)
    G = spd_matrix(F, kappa).to(dtype)        # what both solvers are given
    Ginv = torch.full((F, F), float("nan"), dtype=dtype, device="cuda")
    native().gpu_spd_inverse(G.cuda(), Ginv, stream())
    Ginv = Ginv.cpu()
    assert torch.isfinite(Ginv).all()
    r_dev = inv_residual(G, Ginv)
    r_ref = inv_residual(G, torch.linalg.inv(G))
    print(f"spd_inverse F={F} {dtype} kappa={kappa:g}: r_dev={r_dev:.3e} "
          f"r_ref={r_ref:.3e} ratio={r_dev / max(r_ref, 1e-300):.2f}")
    assert r_dev <= 16 * r_ref + 4 * F * u, (r_dev, r_ref)
    asym = float((Ginv - Ginv.T).abs().max())
    assert asym <= 4 * F * u * float(Ginv.abs().max()), asym


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("F", SPD_RANKS)
def test_spd_inverse_power_of_two_diagonal(F, dtype):
    """G = diag(1, 2, 4, ...). Off-diagonals are exact zeros. Even powers
    have an exact square root, so those entries invert exactly. For odd
    powers sqrt(2) is not representable and no Cholesky route can be
    exact: the three roundings (sqrt, reciprocal, square) give a relative
    error of at most 2u + 2u + u = 5u to first order; 6u is required."""
    u = unit_roundoff(dtype)
    d = torch.tensor([2.0 ** k for k in range(F)], dtype=dtype)
    Ginv = torch.full((F, F), float("nan"), dtype=dtype, device="cuda")
    native().gpu_spd_inverse(torch.diag(d).cuda(), Ginv, stream())
    Ginv = Ginv.cpu()
    want = 1.0 / d                                     # exact powers of two
    assert torch.equal(Ginv - torch.diag(Ginv.diagonal()),
                       torch.zeros(F, F, dtype=dtype))
    got = Ginv.diagonal()
    assert torch.equal(got[0::2], want[0::2])
    assert bool(((got - want).abs() <= 6 * u * want).all())
    # all-even powers: the whole inverse is exact
    d4 = torch.tensor([4.0 ** k for k in range(min(F, 60))], dtype=dtype)
    Fe = d4.numel()
    Ginv = torch.full((Fe, Fe), float("nan"), dtype=dtype, device="cuda")
    native().gpu_spd_inverse(torch.diag(d4).cuda(), Ginv, stream())
    assert torch.equal(Ginv.cpu(), torch.diag(1.0 / d4))


# -------------------------------------------------------- column helpers

COL_RANKS = [1, 7, 16, 24, 64]       # 256 % F != 0 leaves idle lanes
COL_NS = [1, 255, 256, 257, 70001]   # n < 256 blocks leaves blocks empty
F64 = torch.float64


@pytest.mark.parametrize("F", COL_RANKS)
def test_colacc_sum_of_squares_exact(F):
    for n in COL_NS:
        Ai = int_matrix(n, F, F64, seed=3)
        amax = int(Ai.abs().max())
        assert_exact_premise(n, amax, amax, F64)
        out = torch.zeros(F, dtype=F64, device="cuda")
        native().gpu_colacc(Ai.to(F64).cuda(), 0, out, stream())
        assert torch.equal(out.cpu(), (Ai * Ai).sum(dim=0).to(F64)), (n, F)


@pytest.mark.parametrize("F", COL_RANKS)
def test_colacc_max_abs_exact(F):
    """max |x| is exact for any input: a negative entry holds the column
    maximum in column 0, and the last column (F > 1) is all zero."""
    for n in COL_NS:
        g = torch.Generator().manual_seed(41 * n + F)
        A = torch.randn(n, F, generator=g, dtype=F64)
        A[n // 2, 0] = -(float(A.abs().max()) + 1.5)
        if F > 1:
            A[:, F - 1] = 0.0
        out = torch.zeros(F, dtype=F64, device="cuda")
        native().gpu_colacc(A.cuda(), 1, out, stream())
        ref = A.abs().amax(dim=0)
        assert ref[0] == -A[n // 2, 0] and (F == 1 or ref[F - 1] == 0.0)
        assert torch.equal(out.cpu(), ref), (n, F)


@pytest.mark.parametrize("F", COL_RANKS)
def test_coldot_exact(F):
    for n in COL_NS:
        Xi = int_matrix(n, F, F64, seed=4)
        Ai = int_matrix(n, F, F64, seed=5)
        assert_exact_premise(n, int(Xi.abs().max()), int(Ai.abs().max()),
                             F64)
        out = torch.zeros(F, dtype=F64, device="cuda")
        native().gpu_coldot(Xi.to(F64).cuda(), Ai.to(F64).cuda(), out,
                            stream())
        assert torch.equal(out.cpu(), (Xi * Ai).sum(dim=0).to(F64)), (n, F)


@pytest.mark.parametrize("F", COL_RANKS)
def test_colscale(F):
    """Power-of-two lam: exact. General lam: within 1 ulp of the CPU f64
    division."""
    for n in COL_NS:
        g = torch.Generator().manual_seed(59 * n + F)
        A = torch.randn(n, F, generator=g, dtype=F64)
        sign = torch.randint(0, 2, (F,), generator=g).to(F64) * 2 - 1
        lam2 = sign * 2.0 ** torch.randint(-3, 4, (F,), generator=g).to(F64)
        dev = A.cuda()
        native().gpu_colscale(dev, lam2.cuda(), stream())
        assert torch.equal(dev.cpu(), A / lam2), (n, F)

        lam = torch.rand(F, generator=g, dtype=F64) + 0.5
        dev = A.cuda()
        native().gpu_colscale(dev, lam.cuda(), stream())
        ref = A / lam
        ulp = torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) \
            - ref.abs()
        assert bool(((dev.cpu() - ref).abs() <= ulp).all()), (n, F)


def test_column_helpers_reject_bad_arguments():
    A = torch.ones(4, 8, dtype=F64, device="cuda")
    out = torch.zeros(8, dtype=F64, device="cuda")
    wide = torch.ones(4, 65, dtype=F64, device="cuda")
    out65 = torch.zeros(65, dtype=F64, device="cuda")
    with pytest.raises(RuntimeError):
        native().gpu_colacc(wide, 0, out65, stream())
    with pytest.raises(RuntimeError):
        native().gpu_colacc(A.float(), 0, out.float(), stream())
    with pytest.raises(RuntimeError):
        native().gpu_colacc(A, 2, out, stream())
    with pytest.raises(RuntimeError):
        native().gpu_colacc(A, 0, out[:7], stream())
    with pytest.raises(RuntimeError):
        native().gpu_colscale(A.T, out[:4], stream())      # not contiguous
    with pytest.raises(RuntimeError):
        native().gpu_colscale(wide, out65, stream())
    with pytest.raises(RuntimeError):
        native().gpu_coldot(A[:3], A, out, stream())
    with pytest.raises(RuntimeError):
        native().gpu_coldot(A.cpu(), A, out, stream())
