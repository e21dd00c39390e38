#!/usr/bin/env python3
"""CP-APR damped-Newton (PDNR) row-solver benchmark.

1. Per call, per mode, at ranks 16 and 32 (inner_tol = 0, so every row runs
   every iteration):

  pdnr-1   apr_update_pdnr(impl="hip", max_inner=1)   — one Newton iteration
  pdnr-10  apr_update_pdnr(impl="hip", max_inner=10)  — ten
  mu-pass  apr_update(impl="hip", max_inner=10) / 10   — one multiplicative
           pass of the same mode on the same CsfSet
  cmpl     complete_update(impl="hip") of the same mode on the same CsfSet —
           the same Hessian accumulation and Cholesky, once
  nback    mean line-search evaluations per row and iteration of pdnr-10

  The expectation before measuring: one inner iteration costs about one
  completion update plus nback model-value passes,
      model = cmpl + nback * mu-pass,
  and `ratio` is (pdnr-10 / 10) / model. All figures are medians of
  device-event timings of whole calls after warm-up; every call starts from
  the same B (a [rows, rank] copy inside the timed region).

2. The tail: one workgroup owns a row, so the longest row bounds a launch.
   On a zipf-distributed tensor the whole mode is timed against a tensor
   that holds only the longest row's nonzeros.

3. End to end: cpd_apr with the multiplicative solver against PDNR on a
   planted Poisson tensor, wall time and outer / inner iterations until
   kkt < 1e-4 or max_iters.

Usage: apr_pdnr_bench.py [--size t3|nell2|both] [--skip-tail] [--skip-e2e]
                         [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splatt_amd as sp  # noqa: E402

SIZES = {
    # tests/test_gpu.py's t3
    "t3": dict(dims=[300, 250, 400], nnz=120_000, seed=17, reps=30),
    # the NELL-2 shape of scripts/mttkrp_bench.py
    "nell2": dict(dims=[12092, 9184, 28818], nnz=76_879_419, seed=0xB0B0,
                  reps=5),
}
RANKS = [16, 32]
REG = 1e-2
ZIPF = dict(dims=[2000, 1500, 1800], nnz=4_000_000, seed=17)
PLANTED = dict(dims=[400, 300, 200], rank=8, mass=2.0e6, seed=2025)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def counts(t):
    """The same coordinates with count values ceil(5 |v|) >= 1."""
    return sp.SpTensor(t.inds, torch.ceil(5 * t.vals.abs()), list(t.dims))


def starts(t, rank):
    total = float(t.vals.sum())
    ms = []
    for m, d in enumerate(t.dims):
        A = sp.seeded_init(d, rank, m, 123).cuda().abs()
        ms.append(A / A.sum(0))
    return ms, [(A * (total / rank)).contiguous() for A in ms]


def run(name, emit):
    cfg = SIZES[name]
    dims, nnz = cfg["dims"], cfg["nnz"]
    tic = time.time()
    t = counts(sp.SpTensor.synthetic(dims, nnz, seed=cfg["seed"]).to("cuda"))
    cs = sp.csf_alloc(t, "all")
    torch.cuda.synchronize()
    emit(f"== {name}: dims {dims} nnz {nnz} (tensor + CSF built in "
         f"{time.time() - tic:.0f} s)")
    for rank in RANKS:
        mats, b0 = starts(t, rank)
        for mode in range(len(dims)):
            B = torch.empty_like(b0[mode])
            last = {}

            def pdnr(n):
                B.copy_(b0[mode])
                last["r"] = sp.apr_update_pdnr(
                    cs, mats, mode, B, inner_tol=0.0, max_inner=n, impl="hip")

            def mu(n):
                B.copy_(b0[mode])
                sp.apr_update(cs, mats, mode, B, inner_tol=0.0, max_inner=n,
                              impl="hip")

            p1 = median_ms(lambda: pdnr(1), 2, cfg["reps"])
            p10 = median_ms(lambda: pdnr(10), 1, cfg["reps"])
            _, iters, _, stats = last["r"]
            nb = float(stats["nback"].sum()) / max(1.0, float(iters.sum()))
            m10 = median_ms(lambda: mu(10), 2, cfg["reps"])
            c = median_ms(lambda: sp.complete_update(
                cs, mats, mode, REG, out=B, impl="hip"), 2, cfg["reps"])
            model = c[0] + nb * m10[0] / 10
            emit(f"rank {rank:2d} mode {mode}: pdnr-1 {p1[0]:9.3f} ms "
                 f"[{p1[1]:.3f}..{p1[2]:.3f}]  pdnr-10 {p10[0]:9.3f} ms "
                 f"[{p10[1]:.3f}..{p10[2]:.3f}]  per-iter {p10[0] / 10:8.3f} "
                 f"ms  mu-pass {m10[0] / 10:8.3f} ms  cmpl {c[0]:8.3f} ms  "
                 f"nback/iter {nb:5.2f}  model {model:8.3f} ms  ratio "
                 f"{p10[0] / 10 / model:5.2f}x")


def run_tail(emit):
    dims, nnz = ZIPF["dims"], ZIPF["nnz"]
    t = counts(sp.SpTensor.synthetic(dims, nnz, seed=ZIPF["seed"],
                                     dist="zipf").to("cuda"))
    cs = sp.csf_alloc(t, "all")
    emit(f"== tail: zipf dims {dims} nnz {t.nnz}")
    for rank in RANKS:
        mats, b0 = starts(t, rank)
        for mode in range(len(dims)):
            cnt = torch.bincount(t.inds[mode], minlength=dims[mode])
            top = int(cnt.argmax())
            keep = t.inds[mode] == top
            one = sp.SpTensor(t.inds[:, keep].contiguous(),
                              t.vals[keep].contiguous(), list(dims))
            cs1 = sp.csf_alloc(one, "all")
            B = torch.empty_like(b0[mode])

            def call(src):
                B.copy_(b0[mode])
                sp.apr_update_pdnr(src, mats, mode, B, inner_tol=0.0,
                                   max_inner=10, impl="hip")

            full = median_ms(lambda: call(cs), 1, 5)
            lone = median_ms(lambda: call(cs1), 1, 5)
            emit(f"rank {rank:2d} mode {mode}: rows with nonzeros "
                 f"{int((cnt > 0).sum())}  longest row {int(cnt.max())} nnz "
                 f"({100.0 * int(cnt.max()) / t.nnz:.1f}% of all)  pdnr-10 "
                 f"whole mode {full[0]:8.3f} ms  longest row alone "
                 f"{lone[0]:8.3f} ms  = {100.0 * lone[0] / full[0]:5.1f}% of "
                 f"the launch")


def run_e2e(emit):
    cfg = PLANTED
    g = torch.Generator().manual_seed(cfg["seed"])
    A = []
    for d in cfg["dims"]:
        M = torch.rand(d, cfg["rank"], generator=g, dtype=torch.float64) ** 3
        A.append(M / M.sum(0))
    lam = torch.arange(cfg["rank"], 0, -1, dtype=torch.float64)
    lam = lam * (cfg["mass"] / float(lam.sum()))
    mean = torch.einsum("f,if,jf,kf->ijk", lam, *A)
    x = torch.poisson(mean, generator=g)
    inds = x.nonzero().T.contiguous()
    t = sp.SpTensor(inds, x[tuple(inds)].clone(), cfg["dims"]).to("cuda")
    cs = sp.csf_alloc(t, "all")
    emit(f"== end to end: planted Poisson dims {cfg['dims']} rank "
         f"{cfg['rank']} nnz {t.nnz} counts {float(t.vals.sum()):.0f}")
    for method, inner in (("mu", 10), ("pdnr", 10), ("pdnr", 20)):
        opts = sp.AprOptions(max_iters=200, max_inner=inner, tolerance=1e-4,
                             seed=77, method=method)
        sp.cpd_apr(cs, cfg["rank"], opts, max_iters=1)      # warm-up
        torch.cuda.synchronize()
        tic = time.time()
        r = sp.cpd_apr(cs, cfg["rank"], opts)
        torch.cuda.synchronize()
        wall = time.time() - tic
        emit(f"{method:4s} max_inner {inner:2d}: {wall:8.3f} s  outer "
             f"{r.niters:3d}  inner {sum(r.inner_trace):8d}  evaluations "
             f"{sum(r.nback_trace):8d}  kkt {r.kkt_trace[-1]:.3e}  "
             f"{'converged' if r.converged else 'not converged'}  "
             f"-loglik {r.loglik_trace[-1]:.8e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="both", choices=["t3", "nell2", "both"])
    ap.add_argument("--skip-tail", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("apr_pdnr_bench.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for name in (["t3", "nell2"] if args.size == "both" else [args.size]):
        run(name, emit)
    if not args.skip_tail:
        run_tail(emit)
    if not args.skip_e2e:
        run_e2e(emit)


if __name__ == "__main__":
    main()
