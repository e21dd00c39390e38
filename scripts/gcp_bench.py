#!/usr/bin/env python3
"""GCP loss-gradient benchmark: per mode, at ranks 16 and 32,

  g       gcp_grad(impl="hip", loss="gaussian")                 no transcendental
  g+f     the same with want_loss=True
  l       gcp_grad(impl="hip", loss="bernoulli-logit")          one exp
  l+f     the same with want_loss=True                          exp and log1p
  apr-1   apr_update(impl="hip", max_inner=1) — the same gathers and
          shuffles with a division in place of the subtraction, plus the
          copy of B and the fixed work of its launcher
  mttkrp  mttkrp() of the same mode on the same CsfSet
  torch   gcp_grad(impl="torch", loss="gaussian", want_loss=True) — same
          device tensors, set against g+f

All figures are medians of device-event timings of whole calls after
warm-up, all from one run. The values are 0/1 (valid for every loss timed
here and for apr). The torch path's index_add_ serialises on the few rows a
sorted chunk touches, so at the NELL-2 shape it is timed as single
synchronised calls, shortest rows first, until --torch-wall seconds are
spent; the rest is reported as not measured. hip and torch outputs are
compared at the timed size.

Usage: gcp_bench.py [--size t3|nell2|both] [--torch-wall S] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splatt_amd as sp  # noqa: E402
from splatt_amd import gcp  # noqa: E402

SIZES = {
    # tests/test_gpu.py's t3
    "t3": dict(dims=[300, 250, 400], nnz=120_000, seed=17,
               reps_hip=30, warm_torch=1, reps_torch=10),
    # the NELL-2 shape of scripts/mttkrp_bench.py
    "nell2": dict(dims=[12092, 9184, 28818], nnz=76_879_419, seed=0xB0B0,
                  reps_hip=7, warm_torch=0, reps_torch=1),
}
RANKS = [16, 32]


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


def run(name, emit, torch_wall):
    cfg = SIZES[name]
    dims, nnz = cfg["dims"], cfg["nnz"]
    tic = time.time()
    t = sp.SpTensor.synthetic(dims, nnz, seed=cfg["seed"]).to("cuda")
    # binary observations: the sign of the synthetic value
    t = sp.SpTensor(t.inds, (t.vals > 0).double(), list(dims))
    cs = sp.csf_alloc(t, "all")
    torch.cuda.synchronize()
    emit(f"== {name}: dims {dims} nnz {nnz} (segment {sp.completion.SEG} "
         f"entries; tensor + CSF built in {time.time() - tic:.0f} s)")
    mats = {}
    for rank in RANKS:
        # positive, model values of order 1: valid for apr as well
        mats[rank] = [(sp.seeded_init(d, rank, m, 123).cuda().abs()
                       * rank ** (-1.0 / len(dims))).contiguous()
                      for m, d in enumerate(dims)]
    cases = [(rank, mode) for rank in RANKS for mode in range(len(dims))]
    hipgf = {}
    for rank, mode in cases:
        ms = mats[rank]
        reps = cfg["reps_hip"]

        def grad(loss, want):
            return lambda: sp.gcp_grad(cs, ms, mode, loss, want_loss=want,
                                       impl="hip")

        g = median_ms(grad("gaussian", False), 3, reps)
        gf = median_ms(grad("gaussian", True), 3, reps)
        lg = median_ms(grad("bernoulli-logit", False), 3, reps)
        lf = median_ms(grad("bernoulli-logit", True), 3, reps)
        B = torch.empty_like(ms[mode])

        def apr1():
            B.copy_(ms[mode])
            sp.apr_update(cs, ms, mode, B, inner_tol=0.0, max_inner=1,
                          impl="hip")

        a1 = median_ms(apr1, 3, reps)
        mk = median_ms(lambda: sp.mttkrp(cs, ms, mode, out=B), 3, reps)
        plan = gcp.gcp_plan(cs, mode)
        hipgf[rank, mode] = gf[0]
        emit(f"rank {rank:2d} mode {mode}: g {g[0]:8.3f} ms "
             f"[{g[1]:.3f}..{g[2]:.3f}]  g+f {gf[0]:8.3f} ms "
             f"[{gf[1]:.3f}..{gf[2]:.3f}]  l {lg[0]:8.3f} ms "
             f"[{lg[1]:.3f}..{lg[2]:.3f}]  l+f {lf[0]:8.3f} ms "
             f"[{lf[1]:.3f}..{lf[2]:.3f}]  apr-1 {a1[0]:8.3f} ms  "
             f"mttkrp {mk[0]:8.3f} ms  g/apr-1 {g[0] / a1[0]:5.2f}x  "
             f"g/mttkrp {g[0] / mk[0]:5.2f}x  (g+f)/g {gf[0] / g[0]:5.2f}x  "
             f"l/g {lg[0] / g[0]:5.2f}x  (l+f)/g {lf[0] / g[0]:5.2f}x  "
             f"segments {plan['seg_start'].numel()} multi-segment rows "
             f"{plan['mrow'].numel()}")

    spent = 0.0
    # shortest rows first: the torch path's time grows with the row length
    for rank, mode in sorted(cases, key=lambda rm: (-dims[rm[1]], rm[0])):
        if spent > torch_wall:
            emit(f"rank {rank:2d} mode {mode}: torch not measured "
                 f"(--torch-wall {torch_wall:.0f} s spent)")
            continue
        ms = mats[rank]
        tic = time.time()
        tm = median_ms(lambda: sp.gcp_grad(cs, ms, mode, "gaussian",
                                           want_loss=True, impl="torch"),
                       cfg["warm_torch"], cfg["reps_torch"])
        Gt, ft = sp.gcp_grad(cs, ms, mode, "gaussian", want_loss=True,
                             impl="torch")
        torch.cuda.synchronize()
        spent += time.time() - tic
        Gh, fh = sp.gcp_grad(cs, ms, mode, "gaussian", want_loss=True,
                             impl="hip")
        diff = max(
            ((Gh - Gt).abs().max() / Gt.abs().max().clamp_min(1.0)).item(),
            ((fh - ft).abs().max() / ft.abs().max().clamp_min(1.0)).item())
        emit(f"rank {rank:2d} mode {mode}: torch g+f {tm[0]:10.3f} ms "
             f"[{tm[1]:.3f}..{tm[2]:.3f}] ({cfg['reps_torch']} timed)  "
             f"torch/hip g+f {tm[0] / hipgf[rank, mode]:8.1f}x  "
             f"max|hip-torch|/max|ref| {diff:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="both", choices=["t3", "nell2", "both"])
    ap.add_argument("--torch-wall", type=float, default=60.0,
                    help="seconds of torch-path timing per size")
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gcp_bench.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for name in (["t3", "nell2"] if args.size == "both" else [args.size]):
        run(name, emit, args.torch_wall)


if __name__ == "__main__":
    main()
