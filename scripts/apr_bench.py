#!/usr/bin/env python3
"""CP-APR row-update benchmark: per mode, at ranks 16 and 32,

  hip-1   apr_update(impl="hip", max_inner=1)   — one inner pass
  hip-10  apr_update(impl="hip", max_inner=10)  — ten, inner_tol = 0
  torch   apr_update(impl="torch", max_inner=1) — same device tensors
  mttkrp  mttkrp() of the same mode on the same CsfSet — one inner pass
          does the same gathers plus log2 W shuffles and a division per
          nonzero, so about one MTTKRP per pass is the expectation

All figures are medians of device-event timings of whole calls after
warm-up; every call starts from the same B (a [rows, rank] copy inside the
timed region). `per-pass` is hip-10 / 10. The torch path's index_add_
serialises on the few rows a sorted chunk touches, so at the NELL-2 shape it
is timed as single synchronised calls, shortest rows first, until
--torch-wall seconds are spent; the rest is reported as not measured. hip
and torch outputs are compared at the timed size.

Usage: apr_bench.py [--size t3|nell2|both] [--torch-wall S] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splatt_amd as sp  # noqa: E402
from splatt_amd import apr  # noqa: E402

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
    # counts: ceil(5 |v|)
    t = sp.SpTensor(t.inds, torch.ceil(5 * t.vals.abs()), list(dims))
    cs = sp.csf_alloc(t, "all")
    torch.cuda.synchronize()
    total = float(t.vals.sum())
    emit(f"== {name}: dims {dims} nnz {nnz} (segment {sp.completion.SEG} "
         f"nnz; tensor + CSF built in {time.time() - tic:.0f} s)")
    mats, b0 = {}, {}
    for rank in RANKS:
        ms = []
        for m, d in enumerate(dims):
            A = sp.seeded_init(d, rank, m, 123).cuda().abs()
            ms.append(A / A.sum(0))
        mats[rank] = ms
        b0[rank] = [(A * (total / rank)).contiguous() for A in ms]
    cases = [(rank, mode) for rank in RANKS for mode in range(len(dims))]

    def update(rank, mode, B, impl, max_inner):
        B.copy_(b0[rank][mode])
        return sp.apr_update(cs, mats[rank], mode, B, inner_tol=0.0,
                             max_inner=max_inner, impl=impl)

    hip1 = {}
    for rank, mode in cases:
        B = torch.empty_like(b0[rank][mode])
        h1 = median_ms(lambda: update(rank, mode, B, "hip", 1),
                       3, cfg["reps_hip"])
        h10 = median_ms(lambda: update(rank, mode, B, "hip", 10),
                        2, cfg["reps_hip"])
        m = median_ms(lambda: sp.mttkrp(cs, mats[rank], mode, out=B),
                      3, cfg["reps_hip"])
        plan = apr.apr_plan(cs, mode)
        hip1[rank, mode] = h1[0]
        emit(f"rank {rank:2d} mode {mode}: hip-1 {h1[0]:9.3f} ms "
             f"[{h1[1]:.3f}..{h1[2]:.3f}]  hip-10 {h10[0]:9.3f} ms "
             f"[{h10[1]:.3f}..{h10[2]:.3f}]  per-pass {h10[0] / 10:8.3f} ms  "
             f"mttkrp {m[0]:8.3f} ms  per-pass/mttkrp "
             f"{h10[0] / 10 / m[0]:5.2f}x  hip-1/mttkrp {h1[0] / m[0]:5.2f}x  "
             f"segments {plan['seg_start'].numel()} multi-segment rows "
             f"{plan['mrow'].numel()}")

    spent = 0.0
    # shortest rows first: the torch path's time grows with the row length
    for rank, mode in sorted(cases, key=lambda rm: (-dims[rm[1]], rm[0])):
        if spent > torch_wall:
            emit(f"rank {rank:2d} mode {mode}: torch not measured "
                 f"(--torch-wall {torch_wall:.0f} s spent)")
            continue
        Bt = torch.empty_like(b0[rank][mode])
        Bh = torch.empty_like(b0[rank][mode])
        tic = time.time()
        tm = median_ms(lambda: update(rank, mode, Bt, "torch", 1),
                       cfg["warm_torch"], cfg["reps_torch"])
        spent += time.time() - tic
        update(rank, mode, Bh, "hip", 1)
        diff = ((Bh - Bt).abs().max() / Bt.abs().max().clamp_min(1.0)).item()
        emit(f"rank {rank:2d} mode {mode}: torch {tm[0]:10.3f} ms "
             f"[{tm[1]:.3f}..{tm[2]:.3f}] ({cfg['reps_torch']} timed)  "
             f"torch/hip-1 {tm[0] / hip1[rank, mode]:8.1f}x  "
             f"max|hip-torch|/max|B| {diff:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="both", choices=["t3", "nell2", "both"])
    ap.add_argument("--torch-wall", type=float, default=60.0,
                    help="seconds of torch-path timing per size")
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("apr_bench.py needs a GPU")
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
