#!/usr/bin/env python3
"""AO-ADMM block-update benchmark: whole admm_update() calls on synthetic
K/H/U with a realistic G (Hadamard product of two random Grams), nonneg,
at FIXED inner-iteration counts:

  mfma   admm_update(impl="hip_mfma") — the rank-16/32/64 instances (what
         impl="hip" runs at these ranks)
  valu   admm_update(impl="hip_valu") — the generic VALU instance at the
         same rank
  torch  admm_update(impl="torch")    — same device tensors, torch ops

Two ways of fixing the count: inner_tol = 0 (the kernel skips the block
sums and both barriers; the torch path skips its four reductions), and
inner_tol = 1e-300 (the stopping test is evaluated every iteration and never
passes on these inputs) — the second is what a tolerance-driven run pays per
iteration.

Figures are medians of device-event timings after warm-up. H and U are
updated in place, so successive calls continue from the previous state; at a
fixed count the work does not depend on the values. The floor printed with
every shape is the time to stream five n x F f64 arrays (read K, H, U; write
H, U) at 6.3 TB/s, the copy rate an MI355X reaches in practice (8 TB/s peak).

Usage: admm_bench.py [--rows N[,N...]] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splatt_amd as sp  # noqa: E402

ROWS = [28_818, 1 << 20, 1 << 24]   # 28 818: NELL-2's largest mode
RANKS = [16, 32]
COUNTS = [5, 50]
HBM_COPY = 6.3e12


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


def inputs(n, rank):
    g = torch.Generator(device="cuda").manual_seed(1234 + rank)

    def rnd(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64,
                          device="cuda")

    A, B = rnd(4096, rank), rnd(4096, rank)
    G = (A.T @ A) * (B.T @ B)
    rho = G.diagonal().sum() / rank
    Ginv = torch.linalg.inv(
        G + rho * torch.eye(rank, dtype=torch.float64, device="cuda"))
    Hstar = rnd(n, rank) * (rnd(n, rank) < 0.5)
    K = Hstar @ G
    K += 0.05 * G.abs().max() * (rnd(n, rank) - 0.5)
    return K, Ginv.contiguous(), rho.reshape(1), rnd(n, rank), \
        torch.zeros(n, rank, dtype=torch.float64, device="cuda")


def run(n, rank, emit):
    K, Ginv, rho, H0, U0 = inputs(n, rank)
    floor_ms = 5 * n * rank * 8 / HBM_COPY * 1e3
    emit(f"== n {n} rank {rank}: streaming floor {floor_ms:.4f} ms "
         f"(5 x {n * rank * 8 / 1e6:.1f} MB at 6.3 TB/s)")
    con = sp.nonneg()
    big = n >= (1 << 22)
    for count in COUNTS:
        for tol, label in ((0.0, "tol=0     "), (1e-300, "tol=1e-300")):
            res, diff, ref = {}, {}, None
            for name, impl in (("mfma", "hip_mfma"), ("valu", "hip_valu"),
                               ("torch", "torch")):
                H, U = H0.clone(), U0.clone()
                it = sp.admm_update(K, Ginv, rho, H, U, con, inner_tol=tol,
                                    max_inner=count, impl=impl)
                assert int(it.min()) == int(it.max()) == count, (name, count)
                if ref is None:
                    ref = (H.clone(), U.clone())
                else:
                    diff[name] = max(float((H - ref[0]).abs().max()),
                                     float((U - ref[1]).abs().max()))
                reps = (3 if big else 7) if name == "torch" else 15
                res[name] = median_ms(
                    lambda: sp.admm_update(K, Ginv, rho, H, U, con,
                                           inner_tol=tol, max_inner=count,
                                           impl=impl),
                    1 if name == "torch" else 3, reps)
                del H, U
            dv, dt = diff["valu"], diff["torch"]
            del ref
            m, v, t = res["mfma"], res["valu"], res["torch"]
            emit(f"inner {count:2d} {label}: mfma {m[0]:9.4f} ms "
                 f"[{m[1]:.4f}..{m[2]:.4f}]  valu {v[0]:9.4f} ms "
                 f"[{v[1]:.4f}..{v[2]:.4f}]  torch {t[0]:10.3f} ms "
                 f"[{t[1]:.3f}..{t[2]:.3f}]  valu/mfma {v[0] / m[0]:5.2f}x  "
                 f"torch/mfma {t[0] / m[0]:7.1f}x  mfma/floor "
                 f"{m[0] / floor_ms:6.1f}x  max|valu-mfma| {dv:.1e} "
                 f"max|torch-mfma| {dt:.1e}")
    del K, H0, U0
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS))
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("admm_bench.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for n in (int(x) for x in args.rows.split(",")):
        for rank in RANKS:
            run(n, rank, emit)


if __name__ == "__main__":
    main()
