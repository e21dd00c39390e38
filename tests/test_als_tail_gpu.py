"""Fused dense ALS tail (csrc/hip/als_tail.hip) against CPU oracles.

Exact cases use small integers scaled by powers of two, built so that every
column maximum of |T| = |K @ Ginv| is a power of two: T, lam, A, gram and
inner are then exactly representable, every partial sum on the device is
exact whatever its order, and the outputs must be torch.equal to an int64
oracle. The float case takes error bounds from the f64 unit roundoff."""
import functools

import pytest
import torch

import splatt_amd as sp
from splatt_amd._ext import native
from splatt_amd.ops import dense

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RANKS = [16, 32, 64]
# wave-tile (16 rows), block (64 rows) and grid edges
NS = [1, 3, 4, 15, 16, 17, 63, 64, 65, 1000, 2051]
SMALL_COL, ZERO_COL, ODD_COL = 3, 5, 6     # special columns (all < 16)


@functools.lru_cache(maxsize=None)
def exact_case(F, n, odd=False):
    """K (n x F) integers in [-8, 8], Ginv integers in [-4, 4] times a
    power of two per column, and the int64 oracle.

    Row 0 is the planted row: K[0, k] = 8 on the first F/2 columns k, and
    Ginv[k, f] = g_f in {+-1, +-2, +-4} there, so T[0, f] = 4 F g_f, a power
    of two. Every other row has sum_k |K[i, k]| <= F, hence |T[i, f]| <= 4 F
    <= |T[0, f]|: the column maximum is that power of two for every n >= 1.
    Column SMALL_COL is scaled by 2^-12 (every |T| < 1, lam = 1), column
    ZERO_COL is zero; odd=True makes g = 3 in column ODD_COL, a lam that is
    no power of two."""
    g = torch.Generator().manual_seed(1000 * F + n)
    half = F // 2
    K = torch.zeros(n, F, dtype=torch.int64)
    K[0, :half] = 8
    if n > 1:
        # dense rows in [-1, 1] and sparse rows of F/8 entries in [-8, 8]
        dense_rows = torch.randint(-1, 2, (n - 1, F), generator=g)
        sparse = torch.zeros(n - 1, F, dtype=torch.int64)
        cols = torch.stack([torch.randperm(F, generator=g)[: F // 8]
                            for _ in range(n - 1)])
        sparse.scatter_(1, cols, torch.randint(-8, 9, (n - 1, F // 8),
                                               generator=g))
        pick = torch.rand(n - 1, generator=g) < 0.5
        K[1:] = torch.where(pick[:, None], dense_rows, sparse)
    assert int(K[1:].abs().sum(1).max() if n > 1 else 0) <= F
    Gi = torch.randint(-4, 5, (F, F), generator=g)
    gf = (2 ** torch.randint(0, 3, (F,), generator=g)) \
        * (2 * torch.randint(0, 2, (F,), generator=g) - 1)
    if odd:
        gf[ODD_COL] = 3
    Gi[:half] = gf
    Gi[:, ZERO_COL] = 0
    e = torch.zeros(F, dtype=torch.int64)          # column exponents
    e[SMALL_COL] = -12
    scale = torch.pow(2.0, e.double())
    T64 = K @ Gi                                   # int64, exact
    T = T64.double() * scale
    lam = T.abs().amax(0).clamp(min=1.0)
    A = T / lam
    if odd:
        gram = inner = None
    else:
        lg = torch.log2(lam)
        assert torch.equal(lg, lg.round())         # powers of two
        s = scale / lam                            # A = T64 * s, s = 2^k
        gram = (T64.T @ T64).double() * torch.outer(s, s)
        inner = (K * T64).sum(0).double() * s
    return K.double(), Gi.double() * scale, lam, A, gram, inner


def run_tail(K, Ginv, want_inner=True, bufs=None):
    n, F = K.shape
    Kg, Gg = K.contiguous().cuda(), Ginv.contiguous().cuda()
    if bufs is None:
        # outputs start as garbage: the op must reset what it accumulates
        bufs = dict(
            A=torch.full((n, F), -7.25, dtype=torch.float64, device="cuda"),
            lam=torch.full((F,), 123.0, dtype=torch.float64, device="cuda"),
            gram=torch.full((F, F), 9.5, dtype=torch.float64, device="cuda"),
            inner=torch.full((F,), -3.0, dtype=torch.float64, device="cuda"))
    dense.als_tail(Kg, Gg, bufs["A"], bufs["lam"], bufs["gram"],
                   inner=bufs["inner"] if want_inner else None)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("want_inner", [True, False])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("F", RANKS)
def test_exact(F, n, want_inner):
    K, Ginv, lam, A, gram, inner = exact_case(F, n)
    b = run_tail(K, Ginv, want_inner)
    assert lam[SMALL_COL] == 1.0 and lam[ZERO_COL] == 1.0
    assert torch.all(A[:, ZERO_COL] == 0)
    assert torch.equal(b["lam"].cpu(), lam)
    assert torch.equal(b["A"].cpu(), A)
    assert torch.equal(b["gram"].cpu(), gram)
    if want_inner:
        assert torch.equal(b["inner"].cpu(), inner)
    else:
        assert torch.all(b["inner"] == -3.0)       # untouched


def test_exact_grid_cap():
    """One row count past the launcher's block cap: waves take more than
    one 16-row tile."""
    n = int(native().als_tail_cap_rows()) + 17
    K, Ginv, lam, A, gram, inner = exact_case(16, n)
    b = run_tail(K, Ginv)
    assert torch.equal(b["lam"].cpu(), lam)
    assert torch.equal(b["A"].cpu(), A)
    assert torch.equal(b["gram"].cpu(), gram)
    assert torch.equal(b["inner"].cpu(), inner)


@pytest.mark.parametrize("F", RANKS)
def test_odd_lam_quotient_is_correctly_rounded(F):
    """lam = 12 F is no power of two: A must be the correctly rounded
    quotient (a true division, no reciprocal multiply), bit for bit; gram
    and inner take the float bounds."""
    n = 1000
    K, Ginv, lam, A, _, _ = exact_case(F, n, odd=True)
    assert lam[ODD_COL] == 12.0 * F
    b = run_tail(K, Ginv)
    assert torch.equal(b["lam"].cpu(), lam)
    Ag = b["A"].cpu()
    assert torch.equal(Ag, A)
    gb = 2 * n * U * (Ag.abs().T @ Ag.abs())
    assert torch.all((b["gram"].cpu() - Ag.T @ Ag).abs() <= gb)
    ib = 2 * n * U * (K.abs() * Ag.abs()).sum(0)
    assert torch.all((b["inner"].cpu() - (K * Ag).sum(0)).abs() <= ib)


@pytest.mark.parametrize("F", RANKS)
def test_float(F):
    """Random data against the f64 CPU evaluation. T is not an output: it
    is read back as A * lam, which adds at most 2u|T| to the F u (|K||Ginv|)
    of the product, inside the bound 2 F u (|K||Ginv|). gram and inner are
    referred to the device's own A, so their bounds are those of the
    reductions alone."""
    n = 2051
    g = torch.Generator().manual_seed(7 + F)
    K = torch.rand(n, F, generator=g, dtype=torch.float64) - 0.5
    B = torch.rand(F, F, generator=g, dtype=torch.float64) - 0.5
    Ginv = torch.linalg.inv(B @ B.T / F + torch.eye(F, dtype=torch.float64))
    Ginv = (Ginv + Ginv.T) * 3.0           # |T| above 1 in most columns
    b = run_tail(K, Ginv)
    Ag, lg = b["A"].cpu(), b["lam"].cpu()
    T = K @ Ginv
    tb = 2 * F * U * (K.abs() @ Ginv.abs())
    rt = ((Ag * lg - T).abs() / tb).max().item()
    lam = T.abs().amax(0).clamp(min=1.0)
    rl = ((lg - lam).abs() / tb.amax(0)).max().item()
    assert (lam > 1.0).any()
    assert torch.equal(Ag.abs().amax(0)[lam > 1.0],
                       torch.ones(int((lam > 1.0).sum()), dtype=torch.float64))
    gb = 2 * n * U * (Ag.abs().T @ Ag.abs())
    rg = ((b["gram"].cpu() - Ag.T @ Ag).abs() / gb).max().item()
    ib = 2 * n * U * (K.abs() * Ag.abs()).sum(0)
    ri = ((b["inner"].cpu() - (K * Ag).sum(0)).abs() / ib).max().item()
    print(f"F={F} error/bound: T={rt:.3f} lam={rl:.3f} gram={rg:.4f} "
          f"inner={ri:.4f}")
    assert rt <= 1.0 and rl <= 1.0 and rg <= 1.0 and ri <= 1.0


@pytest.mark.parametrize("F", RANKS)
def test_second_call_does_not_accumulate(F):
    """Two calls on the same static buffers (what a graph replay does):
    same lam and A, and a gram / inner that are not doubled."""
    K, Ginv, lam, A, gram, inner = exact_case(F, 1000)
    b = run_tail(K, Ginv)
    b = run_tail(K, Ginv, bufs=b)
    assert torch.equal(b["lam"].cpu(), lam)
    assert torch.equal(b["A"].cpu(), A)
    assert torch.equal(b["gram"].cpu(), gram)
    assert torch.equal(b["inner"].cpu(), inner)


def test_prep_forms_hadamard_inverse():
    """With Gram inputs the first launch forms inv(G0 .* G1 + reg I), as
    the copy_/mul_/spd_inverse chain does."""
    F = 16
    g = torch.Generator().manual_seed(3)
    Gs = []
    for _ in range(2):
        X = torch.rand(200, F, generator=g, dtype=torch.float64)
        Gs.append((X.T @ X).cuda())
    want = dense.spd_inverse(Gs[0] * Gs[1]
                             + 0.5 * torch.eye(F, dtype=torch.float64,
                                               device="cuda"))
    K, _, _, _, _, _ = exact_case(F, 64)
    Ginv = torch.empty(F, F, dtype=torch.float64, device="cuda")
    A = torch.empty(64, F, dtype=torch.float64, device="cuda")
    lam = torch.empty(F, dtype=torch.float64, device="cuda")
    gram = torch.empty(F, F, dtype=torch.float64, device="cuda")
    dense.als_tail(K.cuda(), Ginv, A, lam, gram, grams=Gs, reg=0.5)
    assert torch.equal(Ginv, want)
    T = K @ Ginv.cpu()
    lam_ref = T.abs().amax(0).clamp(min=1.0)
    assert (lam.cpu() - lam_ref).abs().max().item() <= 1e-12 * lam_ref.max()


# ------------------------------------------------------------- dispatch
def record_tail(monkeypatch):
    nat = native()
    orig, calls = nat.gpu_als_tail, []

    def wrapped(*a):
        calls.append(tuple(a[0].shape))
        return orig(*a)
    monkeypatch.setattr(nat, "gpu_als_tail", wrapped)
    return calls


@functools.lru_cache(maxsize=None)
def small_set():
    t = sp.SpTensor.synthetic([60, 50, 70], 8000, seed=3)
    return sp.csf_alloc(t.to("cuda"), "all")


def test_fallbacks_take_the_library_chain(monkeypatch):
    calls = record_tail(monkeypatch)
    opts = sp.CpdOptions(max_iters=3, tolerance=0.0)
    sp.cpd_als(small_set(), 16, opts)
    assert len(calls) == 2 * 3          # iterations 1 and 2, three modes
    del calls[:]
    sp.cpd_als(small_set(), 7, opts)
    assert calls == []
    monkeypatch.setenv("SPLATT_FUSED_TAIL", "0")
    sp.cpd_als(small_set(), 16, opts)
    assert calls == []
    monkeypatch.delenv("SPLATT_FUSED_TAIL")
    monkeypatch.setenv("SPLATT_DETERMINISTIC", "1")
    sp.cpd_als(small_set(), 16, opts)
    assert calls == []


# ------------------------------------------------------ whole iteration
@pytest.fixture(scope="module")
def t3():
    return sp.SpTensor.synthetic([300, 250, 400], 120_000, seed=17)


def _graph_and_eager(t3, rank, monkeypatch, fused_calls=None):
    """The recipe of test_gpu.py::test_gpu_graph_step_matches_eager."""
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    from splatt_amd.parallel.grid import (GridDecomp, grid_cpd_init,
                                          grid_cpd_step)
    from splatt_amd.parallel.graph_exec import GraphStepRunner
    opts = sp.CpdOptions(max_iters=6, tolerance=0.0)
    dec = GridDecomp.create(list(t3.dims))
    cs = build_shard_csf(t3.to("cuda"), list(t3.dims), "all", flat_only=True,
                         stage_rank=rank)
    fits, facs = {}, {}
    for fused in ("1", "0"):
        monkeypatch.setenv("SPLATT_FUSED_TAIL", fused)
        st = grid_cpd_init(cs, dec, rank, opts)
        grid_cpd_step(st, 0)
        runner = GraphStepRunner(st)
        assert runner.fused == (fused == "1")
        assert runner.capture(), runner.capture_error
        for _ in range(3):
            runner.replay()
        fits[fused] = runner.finalize(st.norm_x)
        facs[fused] = [f.clone() for f in st.factors] + [st.lam.clone()]
    st2 = grid_cpd_init(cs, dec, rank, opts)
    for it in range(6):  # 1 eager + 2 warmup-in-capture + 3 replays
        fit_eager = grid_cpd_step(st2, it)
    # the factors themselves (max-normalized, entries in [-1, 1]) and lam,
    # relative: the two chains differ by rounding carried through five
    # iterations, far below the fit's 1e-6
    dfac = max(((a - b).abs().max() / b.abs().max()).item()
               for a, b in zip(facs["1"], facs["0"]))
    return fits["1"], fits["0"], fit_eager, dfac


@pytest.mark.parametrize("rank", [16, 32])
def test_graph_step_fused_matches_eager(t3, rank, monkeypatch):
    calls = record_tail(monkeypatch)
    fused, chain, eager, dfac = _graph_and_eager(t3, rank, monkeypatch)
    assert len(calls) == 3 * 3          # 2 warm-up steps + 1 captured
    print(f"rank {rank}: fit={fused:.6f} fused-eager={fused - eager:+.3e} "
          f"fused-chain={fused - chain:+.3e} factors/lam rel diff={dfac:.3e}")
    assert abs(fused - eager) < 1e-6, (fused, eager)
    assert abs(fused - chain) < 1e-6, (fused, chain)
    assert dfac < 1e-6


def test_cpd_als_fit_trace_on_and_off(t3, monkeypatch):
    cs = sp.csf_alloc(t3.to("cuda"), "all")
    opts = sp.CpdOptions(max_iters=6, tolerance=0.0)
    calls = record_tail(monkeypatch)
    on = sp.cpd_als(cs, 16, opts)
    assert len(calls) == 5 * 3
    monkeypatch.setenv("SPLATT_FUSED_TAIL", "0")
    off = sp.cpd_als(cs, 16, opts)
    assert len(calls) == 5 * 3
    d = max(abs(a - b) for a, b in zip(on.fit_trace, off.fit_trace))
    print(f"cpd_als fit trace, fused on vs off: max diff {d:.3e}")
    assert len(on.fit_trace) == len(off.fit_trace) == 6
    assert d < 1e-6
