"""Command-line interface: `python -m splatt_amd <cmd>` (the native
`bin/splatt` binary covers the host-library surface).

Capability parity: the reference `splatt` binary and its sub-commands
(cmds/splatt_cmds.h:18-27): cpd, bench, check, convert, reorder, stats.
"""
from __future__ import annotations

import argparse
import sys

import torch

import splatt_amd as sp
from splatt_amd.stats import cpd_stats, stats_csf, stats_tt
from splatt_amd.utils.timers import TIMERS


def _add_common(p):
    p.add_argument("tensor", help="input tensor (.tns/.coo text or .bin)")
    p.add_argument("--dtype", default="f64", choices=["f64", "f32"])


def _load(args) -> "sp.SpTensor":
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    with TIMERS.time("IO"):
        t = sp.SpTensor.load(args.tensor, dtype)
    return t


def _write_matrix(path: str, A: torch.Tensor) -> None:
    """Dense matrix as text, one row per line (the `modeN.mat` format)."""
    with open(path, "w") as fh:
        for row in A.cpu().tolist():
            fh.write(" ".join(f"{x:.17g}" for x in row) + "\n")


def cmd_complete(args) -> int:
    """`splatt complete`: regularised ALS over the observed entries, with
    held-out validation / test RMSE."""
    import os
    if args.dtype != "f64":
        raise ValueError("complete supports float64 tensors only "
                         "(--dtype f64)")
    t = _load(args)
    print(stats_tt(t, args.tensor))
    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    val = sp.SpTensor.load(args.validate) if args.validate else None
    test = sp.SpTensor.load(args.test) if args.test else None
    for name, h in (("--validate", val), ("--test", test)):
        if h is not None and (h.nmodes != t.nmodes or any(
                hd > td for hd, td in zip(h.dims, t.dims))):
            raise ValueError(f"{name} tensor {h.dims} does not fit inside "
                             f"the training tensor's dims {t.dims}")
    opts = sp.CompleteOptions(max_iters=args.its, regularize=args.reg,
                              tolerance=args.tol, seed=args.seed,
                              verbose=True)
    with TIMERS.time("COMPLETE"):
        cs = sp.csf_alloc(t.to(dev), "all")
        print(stats_csf(cs))
        r = sp.complete_als(cs, args.rank, opts,
                            validate=val.to(dev) if val is not None else None)
    line = (f"Final objective: {r.objective_trace[-1]:.6e}  train RMSE: "
            f"{r.rmse_train_trace[-1]:.5f}  (iterations: {r.niters}")
    if val is not None:
        line += (f"; best validation RMSE {r.rmse_val_trace[r.best_iter]:.5f}"
                 f" at iteration {r.best_iter + 1}")
    print(line + ")")
    if test is not None:
        print(f"Test RMSE: {sp.rmse(r.factors, test.to(dev)):.5f}")
    if args.write is not None:
        os.makedirs(args.write, exist_ok=True)
        for m, f in enumerate(r.factors):
            _write_matrix(os.path.join(args.write, f"mode{m + 1}.mat"), f)
        print(f"wrote {len(r.factors)} factor matrices to {args.write}")
    print(TIMERS.report())
    return 0


def cmd_tucker(args) -> int:
    """`splatt tucker`: sparse Tucker decomposition by HOOI. Writes
    <stem>modeN.mat per mode and the core as <stem>core.tns (every entry,
    1-based coordinates)."""
    import os
    if args.dtype != "f64":
        raise ValueError("tucker supports float64 tensors only "
                         "(--dtype f64)")
    try:
        ranks = [int(x) for x in args.rank.split(",")]
    except ValueError:
        raise ValueError(f"-r {args.rank!r}: ranks must be a comma list of "
                         "integers, one per mode")
    t = _load(args)
    print(stats_tt(t, args.tensor))
    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    opts = sp.TuckerOptions(max_iters=args.its, tol=args.tol, seed=args.seed,
                            verbosity=1)
    with TIMERS.time("TUCKER"):
        cs = sp.csf_alloc(t.to(dev), "all")
        print(stats_csf(cs))
        r = sp.tucker_hooi(cs, ranks, opts)
    print(f"Final fit: {r.fit:.6f}  (iterations: {r.iters})")
    if not args.nowrite:
        parent = os.path.dirname(args.stem)
        if parent:
            os.makedirs(parent, exist_ok=True)
        for m, f in enumerate(r.factors):
            _write_matrix(f"{args.stem}mode{m + 1}.mat", f)
        core = r.core.cpu()
        coords = torch.cartesian_prod(
            *[torch.arange(n) for n in core.shape]).reshape(-1, core.dim())
        with open(f"{args.stem}core.tns", "w") as fh:
            for idx, x in zip(coords.tolist(), core.reshape(-1).tolist()):
                fh.write(" ".join(str(i + 1) for i in idx) + f" {x:.17g}\n")
        print(f"wrote {len(r.factors)} factor matrices and core.tns "
              f"({'x'.join(str(n) for n in core.shape)}) with stem "
              f"{args.stem!r}")
    print(TIMERS.report())
    return 0


def cmd_apr(args) -> int:
    """`splatt apr`: Poisson CPD (CP-APR) of a count tensor. Writes
    <stem>modeN.mat per mode and <stem>lambda.mat."""
    import os
    if args.dtype != "f64":
        raise ValueError("apr supports float64 tensors only (--dtype f64)")
    t = _load(args)
    print(stats_tt(t, args.tensor))
    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    opts = sp.AprOptions(max_iters=args.its, max_inner=args.inner,
                         tolerance=args.tol, seed=args.seed, verbose=True,
                         method=args.alg)
    with TIMERS.time("APR"):
        cs = sp.csf_alloc(t.to(dev), "all")
        print(stats_csf(cs))
        k = sp.cpd_apr(cs, args.rank, opts)
    print(f"Final log-likelihood: {-k.loglik_trace[-1]:.8e}  KKT violation: "
          f"{k.kkt_trace[-1]:.3e}  (iterations: {k.niters}; inner "
          f"iterations: {sum(k.inner_trace)}; "
          f"{'converged' if k.converged else 'not converged'})")
    if args.alg == "pdnr":
        print(f"Line-search evaluations: {sum(k.nback_trace)}")
    if not args.nowrite:
        parent = os.path.dirname(args.stem)
        if parent:
            os.makedirs(parent, exist_ok=True)
        for m, f in enumerate(k.factors):
            _write_matrix(f"{args.stem}mode{m + 1}.mat", f)
        with open(f"{args.stem}lambda.mat", "w") as fh:
            for x in k.lam.cpu().tolist():
                fh.write(f"{x:.17g}\n")
        print(f"wrote {len(k.factors)} factor matrices and lambda.mat with "
              f"stem {args.stem!r}")
    print(TIMERS.report())
    return 0


def cmd_gcp(args) -> int:
    """`splatt gcp`: generalized CPD of the stored entries under an
    elementwise loss. Writes <stem>modeN.mat per mode and <stem>lambda.mat."""
    import os
    if args.dtype != "f64":
        raise ValueError("gcp supports float64 tensors only (--dtype f64)")
    t = _load(args)
    print(stats_tt(t, args.tensor))
    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    opts = sp.GcpOptions(max_iters=args.its, tolerance=args.tol,
                         seed=args.seed, param=args.param, verbose=True)
    with TIMERS.time("GCP"):
        t = t.to(dev)
        if args.zeros:
            t = sp.sample_zeros(t, args.zeros, args.seed)
            print(f"stored {args.zeros} sampled zeros: {t.nnz} observed "
                  "entries")
        cs = sp.csf_alloc(t, "all")
        print(stats_csf(cs))
        k = sp.cpd_gcp(cs, args.rank, args.loss, opts)
    final = k.loss_trace[-1] if k.loss_trace else float("nan")
    print(f"Final loss: {final:.8e}  ({args.loss}; iterations: {k.niters}; "
          f"evaluations: {k.nfev}; "
          f"{'converged' if k.converged else 'not converged'})")
    if not args.nowrite:
        parent = os.path.dirname(args.stem)
        if parent:
            os.makedirs(parent, exist_ok=True)
        for m, f in enumerate(k.factors):
            _write_matrix(f"{args.stem}mode{m + 1}.mat", f)
        with open(f"{args.stem}lambda.mat", "w") as fh:
            for x in k.lam.cpu().tolist():
                fh.write(f"{x:.17g}\n")
        print(f"wrote {len(k.factors)} factor matrices and lambda.mat with "
              f"stem {args.stem!r}")
    print(TIMERS.report())
    return 0


def cmd_sgcp(args) -> int:
    """`splatt sgcp`: stochastic generalized CPD over ALL cells (unstored
    cells are zeros) by Adam on sampled gradients. Writes <stem>modeN.mat
    per mode and <stem>lambda.mat."""
    import os
    if args.dtype != "f64":
        raise ValueError("sgcp supports float64 tensors only (--dtype f64)")
    t = _load(args)
    print(stats_tt(t, args.tensor))
    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    opts = sp.SgcpOptions(p=args.p, q=args.q, lr=args.lr, decay=args.decay,
                          max_fails=args.fails,
                          iters_per_epoch=args.iters_per_epoch,
                          max_epochs=args.epochs, seed=args.seed,
                          param=args.param, verbose=True)
    with TIMERS.time("SGCP"):
        k = sp.cpd_sgcp(t.to(dev), args.rank, args.loss, opts)
    print(f"Final loss estimate: {min(k.loss_trace):.8e}  ({args.loss}; "
          f"epochs: {k.nepochs}; steps kept: {k.nsteps}; failed epochs: "
          f"{k.nfails})")
    if not args.nowrite:
        parent = os.path.dirname(args.stem)
        if parent:
            os.makedirs(parent, exist_ok=True)
        for m, f in enumerate(k.factors):
            _write_matrix(f"{args.stem}mode{m + 1}.mat", f)
        with open(f"{args.stem}lambda.mat", "w") as fh:
            for x in k.lam.cpu().tolist():
                fh.write(f"{x:.17g}\n")
        print(f"wrote {len(k.factors)} factor matrices and lambda.mat with "
              f"stem {args.stem!r}")
    print(TIMERS.report())
    return 0


def parse_constraints(specs, nmodes: int):
    """`--con` specs -> per-mode list of Constraint / None.

    SPEC = KIND[:ARG[:ARG]][@MODES]; MODES is a comma list of 1-based modes
    (the numbering of the modeN.mat files), default every mode."""
    from splatt_amd.admm import KINDS, Constraint
    nargs = {"nonneg": 0, "l1": 1, "nonneg_l1": 1, "box": 2}
    out = [None] * nmodes
    for spec in specs:
        body, at, modes_s = spec.partition("@")
        parts = body.split(":")
        kind = parts[0]
        if kind not in KINDS:
            raise ValueError(f"--con {spec!r}: unknown kind {kind!r} "
                             f"({', '.join(KINDS)})")
        if len(parts) - 1 != nargs[kind]:
            raise ValueError(f"--con {spec!r}: {kind} takes {nargs[kind]} "
                             f"argument(s), got {len(parts) - 1}")
        try:
            vals = [float(x) for x in parts[1:]]
        except ValueError:
            raise ValueError(f"--con {spec!r}: arguments must be numbers")
        try:
            if kind == "box":
                con = Constraint(kind, lo=vals[0], hi=vals[1])
            elif vals:
                con = Constraint(kind, weight=vals[0])
            else:
                con = Constraint(kind)
        except ValueError as e:
            raise ValueError(f"--con {spec!r}: {e}")
        if at:
            try:
                modes = [int(x) for x in modes_s.split(",")]
            except ValueError:
                raise ValueError(f"--con {spec!r}: modes must be a comma "
                                 "list of integers")
        else:
            modes = list(range(1, nmodes + 1))
        for m in modes:
            if not 1 <= m <= nmodes:
                raise ValueError(f"--con {spec!r}: mode {m} out of range "
                                 f"1..{nmodes}")
            if out[m - 1] is not None:
                raise ValueError(f"--con {spec!r}: mode {m} is constrained "
                                 "twice")
            out[m - 1] = con
    return out


def cmd_cpd(args) -> int:
    import os
    con_specs = getattr(args, "con", None) or []
    if con_specs:
        if args.native:
            raise ValueError("--con cannot be combined with --native")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("--con is not supported by the distributed "
                             "driver (WORLD_SIZE > 1)")
        if args.dtype != "f64":
            raise ValueError("--con supports float64 tensors only "
                             "(--dtype f64)")
    if getattr(args, "csf", None) is None:
        use_cuda = (args.device in ("auto", "cuda")
                    and torch.cuda.is_available())
        args.csf = "all" if use_cuda else "two"
    if getattr(args, "factor_store", "f64") != "f64":
        os.environ["SPLATT_FACTOR_STORE"] = args.factor_store
    if getattr(args, "deterministic", False):
        # bitwise-reproducible device kernels (docs/KERNELS.md); forces
        # ALLMODE so every mode has a root-sorted stream
        os.environ["SPLATT_DETERMINISTIC"] = "1"
        args.csf = "all"
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        return _cmd_cpd_dist(args, world)
    t = _load(args)
    print(stats_tt(t, args.tensor))
    opts = sp.CpdOptions(tolerance=args.tol, max_iters=args.its,
                         seed=args.seed, csf_alloc=args.csf,
                         nthreads=args.nthreads, verbose=args.verbose > 0,
                         regularize=args.reg)
    cons = parse_constraints(con_specs, t.nmodes) if con_specs else None

    def run(cs):
        if cons is None:
            return sp.cpd_als(cs, args.rank, opts)
        aopts = sp.AoAdmmOptions(
            tolerance=args.tol, max_iters=args.its, seed=args.seed,
            csf_alloc=args.csf, nthreads=args.nthreads,
            verbose=args.verbose > 0, regularize=args.reg,
            inner_tol=args.inner_tol, max_inner=args.inner_its)
        return sp.cpd_aoadmm(cs, args.rank, cons, aopts)

    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    with TIMERS.time("CPD"):
        if dev == "cpu" and args.native:
            k = sp.cpd_als_cpu_native(t, args.rank, opts)
        elif dev == "cuda":
            # production device build: flat streams + LDS-staged buckets
            # (the same path bench.py and the distributed driver use)
            from splatt_amd.parallel.dist_cpd import build_shard_csf
            stage = args.rank if args.rank in (4, 8, 16, 32, 64) else 0
            cs = build_shard_csf(t.to(dev), list(t.dims), args.csf,
                                 flat_only=True, stage_rank=stage)
            print(stats_csf(cs))
            print(cpd_stats(cs, args.rank, opts))
            k = run(cs)
        else:
            cs = sp.csf_alloc(t.to(dev), args.csf)
            print(stats_csf(cs))
            print(cpd_stats(cs, args.rank, opts))
            k = run(cs)
    if cons is not None:
        print(f"Final fit: {k.fit:.5f}  (iterations: {k.niters}; inner "
              f"iterations: {sum(sum(r) for r in k.inner_iters)})")
    else:
        print(f"Final fit: {k.fit:.5f}  (iterations: {k.niters})")
    if not args.nowrite:
        for m, f in enumerate(k.factors):
            _write_matrix(f"mode{m + 1}.mat", f)
        with open("lambda.mat", "w") as fh:
            for x in k.lam.cpu().tolist():
                fh.write(f"{x:.17g}\n")
    print(TIMERS.report())
    return 0


def _cmd_cpd_dist(args, world: int) -> int:
    """`torchrun --nproc-per-node N -m splatt_amd cpd ...` — the analog of
    `mpirun splatt cpd` (reference cmds/mpi_cmd_cpd.c:175): grid
    decomposition over RCCL (GPU) or gloo (CPU), rank-0 output."""
    import os
    import torch.distributed as dist
    from splatt_amd.parallel.dist_cpd import build_shard_csf
    from splatt_amd.parallel.grid import (GridDecomp, grid_cpd_als,
                                          load_shard, write_factors)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = args.device in ("auto", "cuda") and torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
    dist.init_process_group("nccl" if use_cuda else "gloo")
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    t = sp.SpTensor.load(args.tensor, dtype)
    dec = GridDecomp.create(list(t.dims))
    shard = dec.localize(t)
    if use_cuda:
        shard = shard.to(f"cuda:{local_rank % torch.cuda.device_count()}")
    stage = args.rank if (use_cuda
                          and args.rank in (4, 8, 16, 32, 64)) else 0
    cs = build_shard_csf(shard, list(t.dims), args.csf,
                         flat_only=use_cuda, stage_rank=stage)
    opts = sp.CpdOptions(tolerance=args.tol, max_iters=args.its,
                         seed=args.seed, csf_alloc=args.csf)
    k = grid_cpd_als(cs, dec, args.rank, opts)
    if rank == 0:
        print(f"Final fit: {k.fit:.5f}  (iterations: {k.niters}; "
              f"grid {dec.grid})")
    if not args.nowrite:
        write_factors(k, dec)
    dist.destroy_process_group()
    return 0


def cmd_check(args) -> int:
    t = _load(args)
    fixed = t.fixed(dedup=True, compress=args.compress)
    ndups = getattr(fixed, "_ndups", 0)
    nempty = getattr(fixed, "_nempty", 0)
    print(f"duplicates merged: {ndups}; empty slices removed: {nempty}")
    if args.fix:
        fixed.save(args.fix)
        print(f"wrote {args.fix}")
    return 0


def cmd_convert(args) -> int:
    t = _load(args)
    kind = args.type
    if kind == "auto":
        kind = "bin" if args.output.endswith(".bin") else "tns"
    if kind in ("bin", "tns"):
        if kind == "bin" and not args.output.endswith(".bin"):
            args.output += ".bin"
        t.save(args.output)
    elif kind == "graph":
        from splatt_amd.graph import graph_mpartite, graph_write
        graph_write(graph_mpartite(t), args.output)
    elif kind == "hgraph":
        from splatt_amd.graph import hgraph_nnz, hgraph_write
        hgraph_write(hgraph_nnz(t), args.output)
    elif kind == "fib_hgraph":
        from splatt_amd.graph import hgraph_fib, hgraph_write
        hgraph_write(hgraph_fib(t, args.mode), args.output)
    elif kind == "csr":
        # mode-`--mode` CSR unfolding (reference CNV_FIB_SPMAT,
        # convert.c:134): "nrows ncols nnz" header then one
        # "col val" pair list per row
        X = t.unfold(args.mode)
        cp = X.crow_indices().tolist()
        ci = X.col_indices().tolist()
        v = X.values().tolist()
        with open(args.output, "w") as f:
            f.write(f"{X.shape[0]} {X.shape[1]} {len(v)}\n")
            for r in range(X.shape[0]):
                f.write(" ".join(f"{ci[i] + 1} {v[i]:g}"
                                 for i in range(cp[r], cp[r + 1])) + "\n")
    print(f"wrote {args.output} ({kind})")
    return 0


def cmd_stats(args) -> int:
    t = _load(args)
    print(stats_tt(t, args.tensor))
    if getattr(args, "part", None):
        from splatt_amd.graph import part_read
        from splatt_amd.stats import stats_hparts
        print(stats_hparts(t, part_read(args.part), args.part))
        return 0
    cs = sp.csf_alloc(t, args.csf)
    print(stats_csf(cs))
    return 0


def cmd_bench(args) -> int:
    from splatt_amd.benchmarks import bench_mttkrp, format_bench
    t = _load(args)
    print(stats_tt(t, args.tensor))
    dev = args.device
    if dev == "auto":
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    threads = [int(x) for x in args.threads.split(",")] if args.threads \
        else None
    res = bench_mttkrp(t, args.rank, args.algs.split(","), args.iters,
                       device=dev, validate=args.validate, threads=threads)
    print(format_bench(res))
    return 0


def cmd_reorder(args) -> int:
    from splatt_amd import reorder as ro
    from splatt_amd.graph import part_read
    t = _load(args)
    if args.type == "rand":
        perm = ro.perm_rand(t.dims, args.seed)
    elif args.type == "bfs":
        perm = ro.perm_bfs(t)
    elif args.type == "graph":
        perm = ro.perm_graph(t, part_read(args.partfile))
    elif args.type == "hgraph":
        perm = ro.perm_hgraph(t, part_read(args.partfile))
    else:
        raise SystemExit(f"unknown reorder type {args.type}")
    out = ro.perm_apply(t, perm)
    out.save(args.output)
    if args.permfile:
        ro.perm_write(perm, args.permfile)
    print(f"wrote {args.output}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        prog="splatt",
        description="MI355X-native sparse tensor factorization "
                    "(CPD-ALS / CSF MTTKRP)")
    ap.add_argument("--version", action="version", version=sp.__version__)
    sub = ap.add_subparsers(dest="cmd", required=True)

    p = sub.add_parser("cpd", help="compute the CPD of a sparse tensor")
    _add_common(p)
    p.add_argument("-r", "--rank", type=int, default=10)
    p.add_argument("-t", "--tol", type=float, default=1e-5)
    p.add_argument("-i", "--its", type=int, default=50)
    p.add_argument("--seed", type=int, default=0x5EED5EED)
    p.add_argument("--reg", type=float, default=0.0,
                   help="ridge regularization on the normal equations")
    p.add_argument("--csf", default=None, choices=["one", "two", "all"],
                   help="CSF allocation policy (default: 'all' on GPU — "
                        "root-output streams for every mode, 3-5x faster "
                        "kernels; 'two' on CPU, the reference default)")
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--nthreads", type=int, default=0)
    p.add_argument("--native", action="store_true",
                   help="use the C++ host driver (CPU reference path)")
    p.add_argument("--nowrite", action="store_true")
    p.add_argument("--factor-store", default="f64",
                   choices=["f64", "f32", "bf16"],
                   help="reduced-precision factor STORAGE for the device "
                        "MTTKRP gathers (accumulation stays f64; "
                        "docs/TUNING.md)")
    p.add_argument("--deterministic", action="store_true",
                   help="bitwise-reproducible device CPD (atomic-free "
                        "kernels, >=80%% throughput; implies --csf all)")
    p.add_argument("--con", action="append", default=[], metavar="SPEC",
                   help="constrained CPD (AO-ADMM); repeatable. SPEC = "
                        "KIND[:ARG[:ARG]][@MODES] with KIND nonneg, l1:W, "
                        "nonneg_l1:W or box:LO:HI and MODES a comma list of "
                        "1-based modes (default: every mode), e.g. "
                        "--con nonneg, --con l1:0.1@1,3, --con box:0:1@2")
    p.add_argument("--inner-its", type=int, default=50,
                   help="ADMM inner iteration bound per block (--con)")
    p.add_argument("--inner-tol", type=float, default=1e-2,
                   help="ADMM inner stopping tolerance (--con)")
    p.add_argument("-v", "--verbose", action="count", default=0)
    p.set_defaults(fn=cmd_cpd)

    p = sub.add_parser("complete",
                       help="tensor completion: ALS over observed entries")
    _add_common(p)
    p.add_argument("--validate", help="held-out tensor: early stopping and "
                                      "best-iteration selection")
    p.add_argument("--test", help="held-out tensor: final RMSE report")
    p.add_argument("-r", "--rank", type=int, default=10)
    p.add_argument("-i", "--iters", "--its", dest="its", type=int,
                   default=50)
    p.add_argument("--reg", type=float, default=1e-2,
                   help="ridge weight on every factor (must be > 0)")
    p.add_argument("-t", "--tol", type=float, default=1e-4,
                   help="stop when the relative improvement of the "
                        "validation RMSE (else the objective) drops below")
    p.add_argument("--seed", type=int, default=0x5EED5EED)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--write", nargs="?", const=".", default=None,
                   metavar="DIR",
                   help="write modeN.mat factor files (into DIR, default .)")
    p.set_defaults(fn=cmd_complete)

    p = sub.add_parser("tucker",
                       help="sparse Tucker decomposition (HOOI)")
    _add_common(p)
    p.add_argument("-r", "--rank", default="8,8,8", metavar="R1,R2,..",
                   help="comma list of ranks, one per mode (each 1..32)")
    p.add_argument("-i", "--iters", "--its", dest="its", type=int,
                   default=50)
    p.add_argument("-t", "--tol", type=float, default=1e-5,
                   help="stop when the fit changes by less than this")
    p.add_argument("--seed", type=int, default=0x5EED5EED)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--stem", default="", metavar="PATH",
                   help="prefix of the output files PATHmodeN.mat and "
                        "PATHcore.tns (end it with / for a directory)")
    p.add_argument("--nowrite", action="store_true")
    p.set_defaults(fn=cmd_tucker)

    p = sub.add_parser("apr",
                       help="Poisson CPD of a count tensor (CP-APR)")
    _add_common(p)
    p.add_argument("-r", "--rank", type=int, default=10)
    p.add_argument("-i", "--iters", "--its", dest="its", type=int,
                   default=100)
    p.add_argument("-t", "--tol", type=float, default=1e-4,
                   help="KKT tolerance, outer and per row (0: run every "
                        "iteration)")
    p.add_argument("--inner", type=int, default=10,
                   help="inner iterations per row and mode update")
    p.add_argument("--alg", default="mu", choices=["mu", "pdnr"],
                   help="row solver: multiplicative updates (mu) or the "
                        "damped-Newton solver (pdnr)")
    p.add_argument("--seed", type=int, default=0x5EED5EED)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--stem", default="", metavar="PATH",
                   help="prefix of the output files PATHmodeN.mat and "
                        "PATHlambda.mat (end it with / for a directory)")
    p.add_argument("--nowrite", action="store_true")
    p.set_defaults(fn=cmd_apr)

    from splatt_amd.gcp import LOSSES as _gcp_losses
    p = sub.add_parser("gcp",
                       help="generalized CPD of the stored entries under an "
                            "elementwise loss (GCP)")
    _add_common(p)
    p.add_argument("-r", "--rank", type=int, default=10)
    p.add_argument("--loss", default="gaussian", choices=list(_gcp_losses))
    p.add_argument("--param", type=float, default=None,
                   help="loss parameter (huber: delta)")
    p.add_argument("-i", "--iters", "--its", dest="its", type=int,
                   default=200)
    p.add_argument("-t", "--tol", type=float, default=1e-6,
                   help="stop when the loss decreases by less than this, "
                        "relatively (0: run every iteration)")
    p.add_argument("--zeros", type=int, default=0, metavar="N",
                   help="store N zeros sampled from the empty cells first "
                        "(binary data: positives plus sampled negatives)")
    p.add_argument("--seed", type=int, default=0x5EED5EED)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--stem", default="", metavar="PATH",
                   help="prefix of the output files PATHmodeN.mat and "
                        "PATHlambda.mat (end it with / for a directory)")
    p.add_argument("--nowrite", action="store_true")
    p.set_defaults(fn=cmd_gcp)

    p = sub.add_parser("sgcp",
                       help="stochastic generalized CPD over all cells "
                            "(unstored cells are zeros): Adam on sampled "
                            "gradients")
    _add_common(p)
    p.add_argument("-r", "--rank", type=int, default=10)
    p.add_argument("--loss", default="bernoulli-logit",
                   choices=list(_gcp_losses))
    p.add_argument("--param", type=float, default=None,
                   help="loss parameter (huber: delta)")
    p.add_argument("-e", "--epochs", type=int, default=1000,
                   help="at most this many epochs")
    p.add_argument("--iters-per-epoch", type=int, default=1000)
    p.add_argument("-p", type=int, default=None, metavar="N",
                   help="stored entries drawn per step")
    p.add_argument("-q", type=int, default=None, metavar="N",
                   help="cells drawn per step")
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--decay", type=float, default=0.1,
                   help="lr multiplier after an epoch that did not improve")
    p.add_argument("--fails", type=int, default=1,
                   help="stop after this many + 1 such epochs")
    p.add_argument("--seed", type=int, default=0x5EED5EED)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--stem", default="", metavar="PATH",
                   help="prefix of the output files PATHmodeN.mat and "
                        "PATHlambda.mat (end it with / for a directory)")
    p.add_argument("--nowrite", action="store_true")
    p.set_defaults(fn=cmd_sgcp)

    p = sub.add_parser("check", help="find/repair duplicates + empty slices")
    _add_common(p)
    p.add_argument("--fix", help="write the repaired tensor here")
    p.add_argument("--compress", action="store_true",
                   help="also remove empty slices")
    p.set_defaults(fn=cmd_check)

    p = sub.add_parser("convert", help="convert tensor/graph formats")
    _add_common(p)
    p.add_argument("output")
    p.add_argument("-t", "--type", default="auto",
                   choices=["auto", "bin", "tns", "graph", "hgraph",
                            "fib_hgraph", "csr"])
    p.add_argument("-m", "--mode", type=int, default=0,
                   help="mode for fib_hgraph/csr conversions")
    p.set_defaults(fn=cmd_convert)

    p = sub.add_parser("stats", help="print tensor statistics")
    _add_common(p)
    p.add_argument("--part", help="nnz partition file: report partition "
                                  "quality (reference --hparts analysis)")
    p.add_argument("--csf", default="two", choices=["one", "two", "all"])
    p.set_defaults(fn=cmd_stats)

    p = sub.add_parser("bench", help="benchmark MTTKRP algorithms")
    _add_common(p)
    p.add_argument("-r", "--rank", type=int, default=16)
    p.add_argument("-a", "--algs", default="flat,csf,stream",
                   help="comma list from: flat, csf, stream, giga, ttbox, lds (production staged device path)")
    p.add_argument("-N", "--iters", type=int, default=3)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--validate", action="store_true")
    p.add_argument("--threads", help="comma list of CPU thread counts to "
                                     "sweep (reference bench scaling mode)")
    p.set_defaults(fn=cmd_bench)

    p = sub.add_parser("reorder", help="reorder a tensor")
    _add_common(p)
    p.add_argument("output")
    p.add_argument("--type", default="bfs",
                   choices=["rand", "bfs", "graph", "hgraph"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--partfile", help="partition file from an external "
                                      "partitioner (graph/hgraph types)")
    p.add_argument("--permfile", help="prefix to write .modeN.perm files")
    p.set_defaults(fn=cmd_reorder)

    args = ap.parse_args(argv)
    try:
        return args.fn(args)
    except (RuntimeError, OSError, ValueError) as e:
        print(f"splatt: {e}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
