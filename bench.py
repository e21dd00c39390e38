#!/usr/bin/env python3
"""Flagship benchmark: CPD-ALS over the gfx950 HIP MTTKRP on synthetic
tensors shaped like the BASELINE.json configs.

One "step" = one full ALS iteration (all modes: MTTKRP + Cholesky solve +
normalize + Gram update + fit), the reference's headline unit
(cpd_als_iterate, src/cpd.c:271). Reported value = effective MTTKRP GFLOP/s
over the WHOLE step time (3*nnz*rank flops per MTTKRP, nmodes MTTKRPs per
step — the flop convention of BASELINE.md), aggregated across all ranks.

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs. `--dump-outputs DIR`
additionally writes the last timed step's factors/lambda/fit as .npy files
(inputs are seeded, so two builds can be compared output for output);
`--full` adds the measurements beyond the headline (per-phase breakdown).

Default experiment = BASELINE.json config 4: Amazon-Reviews-shaped
(4.8M x 1.8M x 1.8M, 1.74B nnz) rank-16 f64 CPD-ALS, medium-grained
nmodes-D grid over the N GPUs at FIXED global nnz — STRONG scaling, so the
driver's N=1 BENCH and the N=1,2,4,8 SCALE sweep measure one experiment
(config 5 = `--config delicious4d`). `--decomp coarse` gives the weak-
scaling variant (per-GPU work fixed, partitioned mode grows with N).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# avoid fragmentation OOM on billion-nnz builds (must precede torch import)
os.environ.setdefault("PYTORCH_HIP_ALLOC_CONF", "expandable_segments:True")

import torch
import torch.distributed as dist

import splatt_amd as sp
from splatt_amd.parallel.dist_cpd import build_shard_csf
from splatt_amd.parallel.grid import GridDecomp, grid_cpd_init, grid_cpd_step

CONFIGS = {
    # name: (dims, nnz per shard, rank, concentration)
    "nell2": ([12092, 9184, 28818], 76_879_419, 16, 1.5),
    "netflix": ([480_189, 17_770, 2182], 100_480_507, 32, 1.5),
    "amazon": ([4_821_207, 1_774_269, 1_805_187], 1_741_809_018, 16, 1.5),
    "delicious4d": ([532_924, 17_262_471, 2_480_308, 1443], 140_126_181, 32, 1.5),
    "small": ([1200, 900, 1500], 300_000, 16, 1.5),
    # CI-sized 4-mode shape (config 5's mode count at gloo scale)
    "small4": ([500, 1400, 700, 60], 250_000, 8, 1.5),
}


def synth_box_shard(dec, nnz, seed, dtype, device, dist="uniform"):
    """Generate this rank's grid-box shard directly at local size (indices
    already chunk-local)."""
    local_dims = list(dec.chunkn)
    if dist == "zipf":
        return sp.SpTensor.synthetic(local_dims, nnz, dtype=dtype,
                                     device=device, seed=seed, dist="zipf")
    gen_dev = device if nnz > 200_000_000 else "cpu"
    g = torch.Generator(device=gen_dev).manual_seed(seed)
    cols = []
    for m, d in enumerate(local_dims):
        u = torch.rand(nnz, generator=g, dtype=torch.float32, device=gen_dev)
        u = u * u.sqrt()  # mild concentration -> non-uniform fiber lengths
        cols.append((u.double() * d).long().clamp_(0, d - 1))
    inds = torch.stack(cols, 0)
    vals = torch.rand(nnz, generator=g, dtype=torch.float32,
                      device=gen_dev).to(dtype)
    return sp.SpTensor(inds, vals, local_dims).to(device)


DUMP_BUDGET_BYTES = 48 << 20   # all dumped arrays together stay under 64 MB


def dump_outputs(outdir, st, rank, world):
    """Write what the last timed step produced — the factor matrices, lambda
    and the fit, i.e. the Kruskal result a caller of the ALS step receives —
    as <outdir>/<name>.npy. A factor larger than its share of the budget is
    written as a fixed, seeded sample of its rows (sorted row order), so two
    builds run with the same arguments dump the same rows."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    sfx = f".rank{rank}" if world > 1 else ""
    per_factor = DUMP_BUDGET_BYTES // len(st.factors)
    for m, fac in enumerate(st.factors):
        nrows, ncols = fac.shape
        cap = max(1, per_factor // (ncols * fac.element_size()))
        if nrows > cap:
            rows = np.sort(np.random.default_rng(0xD0 + m).choice(
                nrows, size=cap, replace=False))
            fac = fac.index_select(
                0, torch.from_numpy(rows).to(fac.device))
        np.save(os.path.join(outdir, f"factor{m}{sfx}.npy"),
                fac.detach().cpu().numpy())
    np.save(os.path.join(outdir, f"lambda{sfx}.npy"),
            st.lam.detach().cpu().numpy())
    if rank == 0:
        np.save(os.path.join(outdir, "fit.npy"),
                np.array([st.fit], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    # default = BASELINE.json config 4: Amazon-shaped rank-16 CPD-ALS,
    # medium-grained over N GPUs at FIXED global nnz (strong scaling), so
    # the driver's N=1 BENCH and N=1..8 SCALE runs are one experiment.
    # SPLATT_BENCH_* env overrides let CI exercise the default argv at
    # CPU-sized shapes (tests/test_bench_dist.py).
    ap.add_argument("--config",
                    default=os.environ.get("SPLATT_BENCH_CONFIG", "amazon"),
                    choices=list(CONFIGS))
    ap.add_argument("--rank-f", type=int, default=0, help="override CP rank")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--device",
                    default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--csf", default="all", choices=["one", "two", "all"])
    ap.add_argument("--synth", default="uniform", choices=["uniform", "zipf"],
                    help="index distribution of the synthetic tensor")
    ap.add_argument("--profile", action="store_true",
                    help="print a per-phase breakdown (device-synced timers)")
    ap.add_argument("--gather-tiles", type=int, default=-1,
                    help="-1 (default): LDS-staged bucketing sized by "
                         "SPLATT_LDS_KB; 0: off; N>1: plain gather-range "
                         "buckets without LDS staging")
    ap.add_argument("--factor-store", default="f64",
                    choices=["f64", "f32", "bf16"],
                    help="reduced-precision factor STORAGE for the MTTKRP "
                         "gathers (accumulation stays f64). Documented "
                         "experimental mode; the default and all headline "
                         "numbers are full f64")
    ap.add_argument("--deterministic", action="store_true",
                    help="bitwise-reproducible kernels (SPLATT_DETERMINISTIC=1;"
                         " ~84%% of default throughput via the det6 kernel)")
    ap.add_argument("--decomp",
                    default=os.environ.get("SPLATT_BENCH_DECOMP", "medium"),
                    choices=["coarse", "medium"],
                    help="medium = nmodes-D grid, fixed global tensor "
                         "(strong scaling; the BASELINE configs 4/5 shape); "
                         "coarse = 1D layers on the longest mode, per-rank "
                         "work fixed (weak scaling)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the factors, lambda "
                         "and fit of the last timed step as DIR/<name>.npy "
                         "(large factors as a fixed seeded row sample)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure "
                         "(today: the --profile per-phase breakdown); a "
                         "plain run only sets up, warms up, times the steps "
                         "and prints the result line")
    args = ap.parse_args()

    if args.deterministic:
        os.environ["SPLATT_DETERMINISTIC"] = "1"
    if args.factor_store != "f64":
        os.environ["SPLATT_FACTOR_STORE"] = args.factor_store
    dims, nnz_shard, rank_f, _ = CONFIGS[args.config]
    if args.rank_f:
        rank_f = args.rank_f
    dtype = torch.float64 if args.dtype == "f64" else torch.float32

    if args.device != "cpu" and not torch.cuda.is_available():
        print("bench.py: no GPU visible; pass --device cpu for a host run",
              file=sys.stderr)
        return 2

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        if args.device != "cpu":
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        # SPLATT_BENCH_BACKEND=gloo lets CI drive CUDA tensors through
        # gloo with several ranks sharing one GPU (chunked-pipeline
        # composition test); the driver's real runs use RCCL
        backend = os.environ.get(
            "SPLATT_BENCH_BACKEND",
            "nccl" if args.device != "cpu" else "gloo")
        dist.init_process_group(backend)
    device = torch.device(args.device if args.device == "cpu" else
                          f"cuda:{local_rank % torch.cuda.device_count()}")

    t0 = time.time()
    if args.decomp == "coarse":
        # weak scaling: global partitioned-mode dim = N x shard dim; one
        # full-size layer per rank (grid = [.., world, ..])
        part_mode = max(range(len(dims)), key=lambda m: dims[m])
        global_dims = list(dims)
        global_dims[part_mode] *= world
        grid = [1] * len(dims)
        grid[part_mode] = world
        nnz_local = nnz_shard
        scaling = "weak"
    else:
        # medium-grained: fixed global tensor over an auto nmodes-D grid
        global_dims = list(dims)
        grid = None
        nnz_local = nnz_shard // world
        scaling = "strong"
    dec = GridDecomp.create(global_dims, grid=grid)
    shard = synth_box_shard(dec, nnz_local, seed=0xB0B0 + rank, dtype=dtype,
                            device=device, dist=args.synth)
    gt = max(args.gather_tiles, 0)
    stage_rank = rank_f if (args.gather_tiles < 0
                            and device.type == "cuda") else 0
    cs = build_shard_csf(shard, global_dims, args.csf,
                         flat_only=device.type == "cuda",
                         gather_tiles=gt if device.type == "cuda" else 0,
                         stage_rank=stage_rank)
    del shard
    # actual staging outcome (the run-density gate may decline staging,
    # e.g. Amazon/Delicious-scale dims -> plain v2 kernels)
    staged = any(getattr(c, "_stage", None) is not None for c in cs.csfs)
    if rank == 0:
        print(f"# setup: grid={dec.grid} shard_nnz={nnz_local} gt={gt} "
              f"csf_bytes={cs.storage_bytes()} build_s={time.time() - t0:.1f}",
              file=sys.stderr, flush=True)

    opts = sp.CpdOptions(max_iters=args.warmup + args.steps, tolerance=0.0,
                         seed=0x5EED)
    from splatt_amd.parallel.grid import comm_stats
    cstats = comm_stats(dec, nnz_local, rank_f,
                        8 if args.dtype == "f64" else 4, cs=cs)
    if rank == 0:
        print(f"# comm: {cstats}", file=sys.stderr, flush=True)
    st = grid_cpd_init(cs, dec, rank_f, opts)

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    it = 0
    for _ in range(max(args.warmup, 1)):   # iteration 0 must run eager
        grid_cpd_step(st, it)
        it += 1

    # single-GPU steady state: capture the whole ALS iteration as ONE
    # hipGraph (launch-bound dense tail -> one replay per step)
    runner = None
    if world == 1 and device.type == "cuda"             and os.environ.get("SPLATT_NO_GRAPH") != "1":
        from splatt_amd.parallel.graph_exec import GraphStepRunner
        _r = GraphStepRunner(st)
        runner = _r if _r.capture() else None
        if rank == 0:
            print(f"# exec: {'hipGraph-captured' if runner else 'eager'} step",
                  file=sys.stderr, flush=True)
        if runner is None and rank == 0:
            from splatt_amd.parallel import graph_exec  # noqa
            print(f"# graph capture error: "
                  f"{getattr(_r, 'capture_error', None)}",
                  file=sys.stderr, flush=True)

    barrier_sync()
    tic = time.time()
    if runner is not None:
        for _ in range(args.steps):
            runner.replay()
    else:
        for _ in range(args.steps):
            grid_cpd_step(st, it)
            it += 1
    barrier_sync()
    elapsed = time.time() - tic
    if runner is not None:
        runner.finalize(st.norm_x)

    # before any further step touches the state
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, st, rank, world)

    if args.profile or args.full:
        from splatt_amd.utils.timers import TimerRegistry
        reg = TimerRegistry(sync_device=device.type == "cuda")
        for _ in range(3):
            grid_cpd_step(st, it, timers=reg)
            it += 1
        if rank == 0:
            print(reg.report(), file=sys.stderr, flush=True)

    # max over ranks
    if world > 1:
        e = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())

    nmodes = len(global_dims)
    nnz_global = nnz_local * world
    flops = args.steps * nmodes * 3.0 * nnz_global * rank_f
    gflops = flops / elapsed / 1e9
    if rank == 0:
        result = {
            "metric": "mttkrp_gflops",
            "value": round(gflops, 2),
            "unit": "GFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": (args.dtype if args.factor_store == "f64" else
                      f"{args.dtype}+{args.factor_store}-store"),
            "data": "synthetic",
            "config": {
                "model": f"{args.config}-shaped CPD-ALS",
                "dims": global_dims,
                "nnz": nnz_global,
                "cp_rank": rank_f,
                "csf": args.csf,
                "tiling": ("lds-staged buckets" if staged else
                           (f"gather-range x{gt}" if gt > 1 else "none")),
                "parallelism": f"{args.decomp}-grid {dec.grid} x{world} (RCCL/xGMI)",
                "fit": round(st.fit, 6),
            },
        }
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
