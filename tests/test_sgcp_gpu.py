"""Stochastic GCP on the MI355X: the HIP sampled-gradient and Adam kernels
against the CPU torch path in f64 (tests/test_sgcp.py: same inputs, same
scaled error, same bound TOL = 1e3 x the spread of two CPU evaluations that
add the samples in opposite orders).

Largest device errors observed, as |delta| / S (S the sum of absolute
contributions per output element, or of the loss estimate's terms; bound
TOL = 1.6e-12):
    shape grid (gaussian, bernoulli-logit)      1.8e-15 (8 modes, rank 17,
                                                p, q = 1000, 999)
    all eight losses at the mid shape           1.1e-15 (bernoulli-odds; per
                                                loss from 3.2e-16)
    5000 samples on 2 x 1 x 3 cells             9.8e-14 (logit, rank 64)
    model value 0 under gamma / rayleigh        6.7e-16
hip_adam_step against the torch formula on the CPU: m and v bitwise equal;
x within 2.2 ulp (bound ADAM_ULPS = 4), at most 293 of 100003 elements
differing, and bitwise equal to the scalar IEEE loop at every size it was
compared at: the differences are the CPU's vectorised sqrt. Twenty driver
steps, hip against torch on the device: 1.1e-16 (bernoulli-logit) and
1.7e-16 (poisson) where the CPU torch path differs from itself by 1.1e-16
and 3.3e-16 with the sample order reversed (bound: 100 x that). The planted
bernoulli-logit run draws other samples on the device than on the CPU; it
meets the CPU run's loss bound (0.78 of the initial exact loss; 0.711 was
recorded with a loss sample of 4000 + 4000, before the tests went to the
less noisy 15000 + 15000).
"""
import math

import pytest
import torch

import splatt_amd as sp
from splatt_amd.gcp import LOSSES as LOSS_TABLE

from test_gcp import BOUNDED, LOSSES, param_of
from test_sgcp import (ADAM, ADAM_ULPS, ALL_LOSS_CASES, DIMS, F64, GRID_CASES,
                       GRID_LOSSES, I32, TOL, VALUE_KIND, abs_sums,
                       adam_buffers, adam_scalar, adam_x_ulps,
                       assert_sgrad_close, check_planted, grid_case,
                       make_mats, make_sample, planted, reversed_sample,
                       to_device)

pytestmark = pytest.mark.gpu


def on_device(s, mats):
    return to_device(s, "cuda"), [m.cuda() for m in mats]


def check_hip(nm, rank, pq, loss):
    s, mats, ref, S, fabs = grid_case(nm, rank, pq, loss)
    sd, md = on_device(s, mats)
    what = f"hip {loss} {nm} modes rank {rank} p,q {pq}"
    got = sp.gcp_sgrad(sd, md, loss, param=param_of(loss), want_loss=True)
    assert got[0].is_cuda and got[0].dim() == 0
    assert all(G.is_cuda for G in got[1])
    assert_sgrad_close(got, ref, S, fabs, what)
    fhat, grads = sp.gcp_sgrad(sd, md, loss, param=param_of(loss),
                               impl="hip")
    assert fhat is None
    assert_sgrad_close((None, grads), ref, S, fabs, what + " gradient only")
    # the loss estimate is summed in a fixed order
    again = sp.gcp_sgrad(sd, md, loss, param=param_of(loss), want_loss=True)
    assert torch.equal(again[0], got[0])


@pytest.mark.parametrize("nm,rank,pq", GRID_CASES)
def test_shape_grid_hip(nm, rank, pq):
    for loss in GRID_LOSSES:
        check_hip(nm, rank, pq, loss)


@pytest.mark.parametrize("loss", LOSSES)
def test_all_losses_hip(loss):
    for nm, rank, pq in ALL_LOSS_CASES:
        check_hip(nm, rank, pq, loss)


def test_torch_on_device_matches():
    """impl='torch' on device tensors is the benchmark's baseline."""
    loss = "bernoulli-logit"
    s, mats, ref, S, fabs = grid_case(4, 17, (1000, 999), loss)
    sd, md = on_device(s, mats)
    got = sp.gcp_sgrad(sd, md, loss, want_loss=True, impl="torch")
    assert got[0].is_cuda and all(G.is_cuda for G in got[1])
    assert_sgrad_close(got, ref, S, fabs, "torch on device")


# -------------------------------------------------------------- exact case

DYADIC = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0], dtype=F64)


def dyadic_mats(dims, rank, seed):
    g = torch.Generator().manual_seed(seed)
    return [DYADIC[torch.randint(0, 6, (d, rank), generator=g)]
            for d in dims]


def check_equal(s, mats):
    ref = sp.gcp_sgrad(s, mats, "gaussian", want_loss=True, impl="torch")
    sd, md = on_device(s, mats)
    got = sp.gcp_sgrad(sd, md, "gaussian", want_loss=True, impl="hip")
    assert float(got[0]) == float(ref[0])
    for G, R in zip(got[1], ref[1]):
        assert torch.equal(G.cpu(), R)
    assert any(bool((R != 0).any()) for R in ref[1])


@pytest.mark.parametrize("rank", [3, 16, 33])
def test_exact_hip(rank):
    """Gaussian loss, dyadic factors, small integer values, both weights 4:
    every contribution is dyadic and every sum exact in any order."""
    g = torch.Generator().manual_seed(rank)
    dims = [8, 8, 8]
    cells = torch.randperm(512, generator=g)[:64]
    inds = torch.stack([cells // 64, (cells // 8) % 8, cells % 8])
    t = sp.SpTensor(inds, torch.randint(1, 5, (64,), generator=g).double(),
                    dims)
    s = sp.gcp_sample(t, 16, 128, g)
    assert s.wnz == 4.0 and s.wz == 4.0
    check_equal(s, dyadic_mats(dims, rank, seed=rank + 50))


# ---------------------------------------------------------- collision case

COLLIDE_DIMS = [2, 1, 3]


@pytest.mark.parametrize("rank", [4, 16, 64])
def test_collisions_hip(rank):
    """p + q = 5000 samples on 2 x 1 x 3 cells: every atomic lands on a
    handful of rows."""
    for loss in GRID_LOSSES:
        s = make_sample(COLLIDE_DIMS, 2500, 2500, VALUE_KIND[loss], seed=rank)
        mats = make_mats(COLLIDE_DIMS, rank, False)
        ref = sp.gcp_sgrad(s, mats, loss, want_loss=True, impl="torch")
        S, fabs = abs_sums(s, mats, loss)
        sd, md = on_device(s, mats)
        got = sp.gcp_sgrad(sd, md, loss, want_loss=True)
        assert_sgrad_close(got, ref, S, fabs, f"collisions {loss} rank {rank}")
    g = torch.Generator().manual_seed(rank)
    inds = torch.stack([torch.randint(0, d, (5000,), generator=g)
                        for d in COLLIDE_DIMS]).to(I32).contiguous()
    vals = torch.cat([torch.randint(1, 5, (2500,), generator=g).double(),
                      torch.zeros(2500, dtype=F64)])
    check_equal(sp.GcpSample(inds, vals, 2500, 2500, 4.0, 0.5),
                dyadic_mats(COLLIDE_DIMS, rank, seed=rank + 9))


# ------------------------------------------- untouched rows, out=, guards

def test_untouched_rows_and_out_views():
    dims, rank = [40, 33, 29], 5
    # rows 0..9 of every mode only
    s = make_sample([10, 10, 10], 37, 45, "any", seed=4)
    mats = make_mats(dims, rank, False)
    ref = sp.gcp_sgrad(s, mats, "gaussian", impl="torch")
    sd, md = on_device(s, mats)
    npar = sum(dims) * rank
    guard = 3
    flat = torch.full((npar + 2 * guard,), 7.25, dtype=F64, device="cuda")
    views, o = [], guard
    for d in dims:
        views.append(flat[o:o + d * rank].view(d, rank))
        o += d * rank
    _, out = sp.gcp_sgrad(sd, md, "gaussian", out=views)
    assert all(a is b for a, b in zip(out, views))
    S, fabs = abs_sums(s, mats, "gaussian")
    assert_sgrad_close((None, views), ref, S, fabs, "out views")
    for G in views:
        assert bool((G[10:] == 0).all())
    assert bool((flat[:guard] == 7.25).all())
    assert bool((flat[-guard:] == 7.25).all())
    # a second call zeroes what the first one left
    _, out = sp.gcp_sgrad(sd, md, "gaussian", out=views)
    assert_sgrad_close((None, views), ref, S, fabs, "out views, again")


# ----------------------------------------- model value 0 on a bounded loss

@pytest.mark.parametrize("loss", ["gamma", "rayleigh"])
@pytest.mark.parametrize("rank,pq", [(3, (5, 8)), (17, (2, 3)), (64, (3, 2))])
def test_zero_model_value_hip(loss, rank, pq):
    """Rows 0 and 1 of the first factor are zero, so the model is exactly 0
    on the samples that hit them — sample 0, which dropped tail groups
    re-read, among them — and dl(0, 0) = 1/eps or 2/eps. Nothing of that
    may leak: not from tail groups, not from masked lanes."""
    dims = DIMS[3]
    s = make_sample(dims, pq[0], pq[1], VALUE_KIND[loss], seed=rank)
    s.inds[0, 0] = 0
    s.inds[0, -1] = 1
    mats = make_mats(dims, rank, True)
    mats[0][:2] = 0.0
    ref = sp.gcp_sgrad(s, mats, loss, want_loss=True, impl="torch")
    S, fabs = abs_sums(s, mats, loss)
    assert max(float(G.abs().max()) for G in ref[1]) > 1e9
    sd, md = on_device(s, mats)
    got = sp.gcp_sgrad(sd, md, loss, want_loss=True)
    assert all(bool(torch.isfinite(G).all()) for G in got[1])
    assert math.isfinite(float(got[0]))
    assert_sgrad_close(got, ref, S, fabs, f"zero model {loss} rank {rank}")


# -------------------------------------------------------------------- Adam

@pytest.mark.parametrize("lower", [None, 0.0])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_adam_step_hip(n, step, lower):
    """Against the torch formula on the CPU with the same c1, c2: m and v
    bitwise, x within ADAM_ULPS (the CPU's vectorised sqrt is not correctly
    rounded; see tests/test_sgcp.py), g zeroed."""
    x, g, m, v = adam_buffers(n, seed=n)
    before = x.clone()
    dev = [b.cuda() for b in (x, g, m, v)]
    sp.adam_step(x, g, m, v, step=step, lower=lower, impl="torch", **ADAM)
    sp.adam_step(*dev, step=step, lower=lower, **ADAM)
    xd, gd, md, vd = [b.cpu() for b in dev]
    assert torch.equal(md, m) and torch.equal(vd, v)
    assert bool((gd == 0).all())
    err = adam_x_ulps(xd, x, before)
    msg = (f"adam hip vs torch formula n {n} step {step} lower {lower}: "
           f"{err:.2f} ulp (bound {ADAM_ULPS}), {int((xd != x).sum())} of "
           f"{n} differ")
    if n <= 257:
        xb, gb, mb, vb = adam_buffers(n, seed=n)
        want = adam_scalar(xb, gb, mb, vb, step, lower, **ADAM)
        msg += f"; {int((xd != want[0]).sum())} differ from the scalar loop"
    print(msg)
    assert err <= ADAM_ULPS
    if lower is not None:
        assert bool((xd >= lower).all())


def test_adam_step_rejects_aliases_and_views():
    x = torch.zeros(16, dtype=F64, device="cuda")
    with pytest.raises(RuntimeError, match="must not alias"):
        sp.adam_step(x, x, x.clone(), x.clone(), step=1, lr=0.1)
    with pytest.raises(ValueError, match="flat contiguous"):
        sp.adam_step(x[::2], x[::2].clone(), x[::2].clone(), x[::2].clone(),
                     step=1, lr=0.1)


# ------------------------------------------------------------------ driver

DRIVER_STEPS = 20
# hip vs torch on device may differ by this many times what the CPU torch
# path differs from itself with the samples added in the opposite order
DRIVER_MARGIN = 100.0


def run_steps(samples, x0, dims, rank, loss, impl, device):
    lower = LOSS_TABLE[loss][1]
    x = x0.to(device).clone()
    g, m, v = (torch.zeros_like(x) for _ in range(3))

    def split(buf):
        out, o = [], 0
        for d in dims:
            out.append(buf[o:o + d * rank].view(d, rank))
            o += d * rank
        return out

    X, G = split(x), split(g)
    for k, s in enumerate(samples):
        sp.gcp_sgrad(s, X, loss, impl=impl, out=G)
        sp.adam_step(x, g, m, v, step=k + 1, lr=1e-2, lower=lower, impl=impl)
    return x.cpu()


@pytest.mark.parametrize("loss", ["bernoulli-logit", "poisson"])
def test_driver_steps_hip_match_torch_on_device(loss):
    """The step the driver takes — gcp_sample, gcp_sgrad into views of the
    flat gradient, adam_step — 20 times with the same device generator,
    hence the same samples."""
    t, _ = planted(loss)
    td = t.to("cuda")
    dims, rank = list(t.dims), 3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    samples = [sp.gcp_sample(td, 500, 500, gen) for _ in range(DRIVER_STEPS)]
    x0 = torch.cat([
        (sp.seeded_init(d, rank, k, 5).abs() if loss in BOUNDED
         else sp.seeded_init(d, rank, k, 5) * 0.3).reshape(-1)
        for k, d in enumerate(dims)])
    hip = run_steps(samples, x0, dims, rank, loss, "hip", "cuda")
    tor = run_steps(samples, x0, dims, rank, loss, "torch", "cuda")
    cpu = [to_device(s, "cpu") for s in samples]
    fwd = run_steps(cpu, x0, dims, rank, loss, "torch", "cpu")
    rev = run_steps([reversed_sample(s) for s in cpu], x0, dims, rank, loss,
                    "torch", "cpu")
    spread = float((fwd - rev).abs().max())
    err = float((hip - tor).abs().max())
    moved = float((hip - x0).abs().max())
    print(f"{loss}: hip vs torch on device {err:.3e}, hip vs CPU "
          f"{float((hip - fwd).abs().max()):.3e}; CPU torch path, two sample "
          f"orders {spread:.3e} (x {DRIVER_MARGIN:.0f} is the bound); "
          f"factors moved by {moved:.3e}")
    assert moved > 0.05
    assert spread > 0
    assert err <= DRIVER_MARGIN * spread


def test_cpd_sgcp_device_planted():
    """The loss-decrease condition of the CPU run. The device generator
    draws other samples, so the run is another one; the gap between ones
    and zeros is printed and asserted on the CPU only."""
    r = check_planted("cuda", "bernoulli-logit", gap=False)
    assert r.nsteps > 0


def test_cpd_sgcp_device_rollback():
    t, _ = planted("bernoulli-logit")
    r = sp.cpd_sgcp(t.to("cuda"), 3, "bernoulli-logit",
                    sp.SgcpOptions(lr=1e3, decay=0.5, max_fails=1,
                                   max_epochs=9, p=200, q=200, p_loss=1000,
                                   q_loss=1000, iters_per_epoch=3, seed=7))
    assert (r.nfails, r.nepochs, r.nsteps) == (2, 2, 0)
    assert r.lr_trace == [1e3, 5e2]
