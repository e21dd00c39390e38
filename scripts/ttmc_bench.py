#!/usr/bin/env python3
"""TTMc benchmark: per mode, at ranks (16,16,16) and (32,32,32),

  hip    ttmc(impl="hip")    — the gfx950 MFMA kernel
  torch  ttmc(impl="torch")  — same device tensors, chunked gather +
         Kronecker + index_add_
  mttkrp mttkrp() of the same mode on the same CsfSet at F = 16 / 32 — the
         gather-only floor: it reads the same (nmodes-1) factor rows per
         nonzero and does F instead of P = F^2 FMAs with them

hip and mttkrp figures are medians of device-event timings of whole calls
after warm-up. The torch path materialises an nnz x P intermediate chunk by
chunk and its index_add_ serialises on the few rows a sorted chunk touches;
at the NELL-2 shape it is timed as single synchronised calls, shortest rows
first, until --torch-wall seconds are spent; the rest is reported as not
measured. The FMA rate counts the algorithm's nnz * P fused multiply-adds
over the hip time (the kernel issues more: ranks are padded to 16-wide MFMA
tiles and the K tail of every segment is zero-filled). hip and torch outputs
are compared at the timed size.

Usage: ttmc_bench.py [--size t3|nell2|both] [--torch-wall S] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splatt_amd as sp  # noqa: E402
from splatt_amd import tucker  # noqa: E402

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
    cs = sp.csf_alloc(t, "all")
    torch.cuda.synchronize()
    emit(f"== {name}: dims {dims} nnz {nnz} (segment {tucker.SEG} nnz; "
         f"tensor + CSF built in {time.time() - tic:.0f} s)")
    mats = {rank: [sp.seeded_init(d, rank, m, 123).cuda()
                   for m, d in enumerate(dims)] for rank in RANKS}
    cases = [(rank, mode) for rank in RANKS for mode in range(len(dims))]

    hip = {}
    for rank, mode in cases:
        cols = rank * rank
        h = median_ms(lambda: sp.ttmc(cs, mats[rank], mode, impl="hip"),
                      3, cfg["reps_hip"])
        mo = torch.empty(dims[mode], rank, dtype=torch.float64, device="cuda")
        m = median_ms(lambda: sp.mttkrp(cs, mats[rank], mode, out=mo),
                      3, cfg["reps_hip"])
        plan = tucker.ttmc_plan(cs, mode, cols)
        hip[rank, mode] = h[0]
        emit(f"ranks {rank:2d}^3 mode {mode}: hip {h[0]:10.3f} ms "
             f"[{h[1]:.3f}..{h[2]:.3f}]  mttkrp(F={rank}) {m[0]:8.3f} ms  "
             f"hip/mttkrp {h[0] / m[0]:6.1f}x  nnz*P FMA "
             f"{nnz * cols / (h[0] * 1e-3) / 1e9:8.1f} G/s  segments "
             f"{plan['seg_start'].numel()} multi-segment rows "
             f"{plan['mrow'].numel()} batches {len(plan['batches'])}")
        del mo

    spent = 0.0
    # shortest rows first: the torch path's time grows with the row length
    for rank, mode in sorted(cases, key=lambda rm: (-dims[rm[1]], rm[0])):
        if spent > torch_wall:
            emit(f"ranks {rank:2d}^3 mode {mode}: torch not measured "
                 f"(--torch-wall {torch_wall:.0f} s spent)")
            continue
        tic = time.time()
        tm = median_ms(lambda: sp.ttmc(cs, mats[rank], mode, impl="torch"),
                       cfg["warm_torch"], cfg["reps_torch"])
        spent += time.time() - tic
        out_t = sp.ttmc(cs, mats[rank], mode, impl="torch")
        out_h = sp.ttmc(cs, mats[rank], mode, impl="hip")
        diff = (out_h - out_t).abs().max().item()
        emit(f"ranks {rank:2d}^3 mode {mode}: torch {tm[0]:10.3f} ms "
             f"[{tm[1]:.3f}..{tm[2]:.3f}] ({cfg['reps_torch']} timed)  "
             f"torch/hip {tm[0] / hip[rank, mode]:8.1f}x  max|hip-torch| "
             f"{diff:.2e} (max|hip| {out_h.abs().max().item():.2e})")
        del out_t, out_h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="both", choices=["t3", "nell2", "both"])
    ap.add_argument("--torch-wall", type=float, default=60.0,
                    help="seconds of torch-path timing per size")
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ttmc_bench.py needs a GPU")
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
