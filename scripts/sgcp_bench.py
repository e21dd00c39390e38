#!/usr/bin/env python3
"""Stochastic GCP benchmark: the sampled-gradient pass and the Adam step, at
ranks 16 and 32 and samples of p + q = 1e4, 1e5, 1e6 (p = q), on

  nell2   the NELL-2 shape of scripts/gcp_bench.py, coordinates uniform
  zipf    the same shape, every coordinate drawn with probability
          proportional to 1 / (index + 1): a few rows hold most entries

  grad    gcp_sgrad(impl="hip"), gradient only, bernoulli-logit (one exp
          per derivative) and gaussian (none), against impl="torch" on the
          same device tensors, and against the bytes the pass cannot avoid:
          2 * (p+q) * N * F * 8 (every factor row gathered once, every
          gradient row added once)
  stored / cells
          the same pass on a sample that is all stored draws but one, and
          all cell draws but one: on `zipf` the stored draws pile their
          atomics on a few rows and the cell draws do not, so the ratio is
          what same-row atomic contention costs
  adam    adam_step(impl="hip") against impl="torch" on device, on the
          tensor's parameter count and on 2^27 parameters (the Amazon /
          Delicious scale), against seven passes of the buffer

All figures are medians of device-event timings of whole calls (argument
checks and the zeroing of the gradient included) after warm-up, all from one
run. hip and torch gradients are compared at every timed size.

Usage: sgcp_bench.py [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splatt_amd as sp  # noqa: E402

DIMS = [12092, 9184, 28818]
NNZ = {"nell2": 76_879_419, "zipf": 20_000_000}
RANKS = [16, 32]
SAMPLES = [10_000, 100_000, 1_000_000]
BIG_ADAM = 1 << 27


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
    return statistics.median(times)


def make_tensor(name, gen):
    nnz = NNZ[name]
    cols = []
    for d in DIMS:
        u = torch.rand(nnz, generator=gen, device="cuda", dtype=torch.float64)
        if name == "zipf":
            # inverse CDF of p(k) ~ 1 / (k + 1) on [0, d)
            k = torch.exp(u * math.log(d + 1.0)) - 1.0
        else:
            k = u * d
        cols.append(k.long().clamp_(0, d - 1))
    return sp.SpTensor(torch.stack(cols), torch.ones(nnz, dtype=torch.float64,
                                                     device="cuda"),
                       list(DIMS))


def run(name, emit):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xB0B0)
    t = make_tensor(name, gen)
    top = [int(torch.bincount(t.inds[m], minlength=d).max())
           for m, d in enumerate(DIMS)]
    emit(f"== {name}: dims {DIMS} nnz {t.nnz}; entries in the fullest row of "
         f"each mode {top}")
    nm = len(DIMS)
    for rank in RANKS:
        mats = [(sp.seeded_init(d, rank, m, 123).cuda()
                 * rank ** (-1.0 / nm)).contiguous()
                for m, d in enumerate(DIMS)]
        outs = [torch.zeros_like(A) for A in mats]
        for n in SAMPLES:
            s = sp.gcp_sample(t, n // 2, n // 2, gen)
            s_st = sp.gcp_sample(t, n - 1, 1, gen)
            s_ce = sp.gcp_sample(t, 1, n - 1, gen)
            for smp in (s, s_st, s_ce):     # the domain check, once
                sp.gcp_sgrad(smp, mats, "bernoulli-logit", out=outs)

            def grad(smp, loss, impl):
                return lambda: sp.gcp_sgrad(smp, mats, loss, impl=impl,
                                            out=outs)

            reps = 30 if n < 1_000_000 else 15
            hl = median_ms(grad(s, "bernoulli-logit", "hip"), 3, reps)
            hg = median_ms(grad(s, "gaussian", "hip"), 3, reps)
            tl = median_ms(grad(s, "bernoulli-logit", "torch"), 2, 7)
            st = median_ms(grad(s_st, "bernoulli-logit", "hip"), 3, reps)
            ce = median_ms(grad(s_ce, "bernoulli-logit", "hip"), 3, reps)
            _, gh = sp.gcp_sgrad(s, mats, "bernoulli-logit", impl="hip")
            _, gt = sp.gcp_sgrad(s, mats, "bernoulli-logit", impl="torch")
            diff = max(((a - b).abs().max()
                        / b.abs().max().clamp_min(1.0)).item()
                       for a, b in zip(gh, gt))
            gbytes = 2.0 * n * nm * rank * 8 / 1e9
            emit(f"rank {rank:2d} p+q {n:7d}: grad logit {hl:8.3f} ms "
                 f"({gbytes / hl * 1e3:7.1f} GB/s of its byte bound)  "
                 f"gaussian {hg:8.3f} ms  torch logit {tl:8.3f} ms  "
                 f"torch/hip {tl / hl:6.1f}x  stored-only {st:8.3f} ms  "
                 f"cells-only {ce:8.3f} ms  stored/cells {st / ce:5.2f}x  "
                 f"max|hip-torch|/max|ref| {diff:.2e}")
        npar = sum(DIMS) * rank
        for size in (npar, BIG_ADAM):
            bufs = [torch.randn(size, dtype=torch.float64, device="cuda")
                    for _ in range(3)] + [
                torch.rand(size, dtype=torch.float64, device="cuda")]
            step = [0]

            def adam(impl):
                def go():
                    step[0] += 1
                    bufs[1].fill_(0.5)   # g comes back zeroed
                    sp.adam_step(*bufs, step=step[0], lr=1e-3, lower=0.0,
                                 impl=impl)
                return go

            fill = median_ms(lambda: bufs[1].fill_(0.5), 2, 9)
            ah = median_ms(adam("hip"), 2, 9) - fill
            at = median_ms(adam("torch"), 2, 9) - fill
            abytes = 7.0 * size * 8 / 1e9
            emit(f"rank {rank:2d} adam {size:10d} parameters: hip {ah:8.3f} "
                 f"ms ({abytes / ah * 1e3:7.1f} GB/s of seven passes)  torch "
                 f"{at:8.3f} ms ({abytes / at * 1e3:7.1f} GB/s)  torch/hip "
                 f"{at / ah:5.2f}x  (the fill of g that precedes each timed "
                 f"step, {fill:.3f} ms, is subtracted)")
            del bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sgcp_bench.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for name in ("nell2", "zipf"):
        run(name, emit)


if __name__ == "__main__":
    main()
