"""CSF (Compressed Sparse Fiber) tensors, device-resident.

Capability parity: reference src/csf.{h,c} (csf_alloc policies csf.c:770-814,
mode orders csf.c:694-726, construction csf.c:248-644). Two builders:
  * CPU: the C++ core (parallel filter + prefix sums).
  * GPU: rocPRIM-backed torch primitives — stable radix sorts per level,
    boundary flags, cumsum compaction — the K13 "CSF construction on device"
    path (reference's hybrid counting sort, sort.c:761-905, reimagined as
    GPU radix sort + scans).
The structure is identical on both: flat fptr/fids per level + vals.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import List, Optional, Sequence

import torch

from splatt_amd._ext import native
from splatt_amd.sptensor import SpTensor


class CsfAllocPolicy(str, Enum):
    ONEMODE = "one"
    TWOMODE = "two"
    ALLMODE = "all"


@dataclass
class Csf:
    dims: List[int]                       # tensor dims (mode order)
    dim_perm: List[int]                   # level -> mode
    fptr: List[Optional[torch.Tensor]]    # per level int64; None at leaf
    fids: List[Optional[torch.Tensor]]    # per level int32; None root = dense
    vals: torch.Tensor

    @property
    def nmodes(self) -> int:
        return len(self.dims)

    @property
    def nnz(self) -> int:
        return int(self.vals.numel())

    @property
    def device(self) -> torch.device:
        return self.vals.device

    def level_of_mode(self, mode: int) -> int:
        return self.dim_perm.index(mode)

    def nfibs(self, level: int) -> int:
        if level == self.nmodes - 1:
            return self.nnz
        fp = self.fptr[level]
        return int(fp.numel() - 1) if fp is not None else 0

    def to(self, device) -> "Csf":
        c = Csf(
            list(self.dims), list(self.dim_perm),
            [t.to(device) if t is not None else None for t in self.fptr],
            [t.to(device) if t is not None else None for t in self.fids],
            self.vals.to(device),
        )
        # carry expansions + stage metadata (a frozen flat CSF has no fptr
        # tree to recompute them from)
        pack = getattr(self, "_pack", None)
        if pack is not None:
            p = pack.to(device)
            levels = list(self._pack_levels)  # type: ignore[attr-defined]
            object.__setattr__(c, "_pack", p)
            object.__setattr__(c, "_pack_levels", levels)
            object.__setattr__(c, "_expand_cache",
                               {l: p[:, col] for col, l in enumerate(levels)})
            c.fids[self.nmodes - 1] = c._expand_cache[self.nmodes - 1]  # type: ignore[attr-defined]
        else:
            cache = getattr(self, "_expand_cache", None)
            if cache:
                object.__setattr__(c, "_expand_cache",
                                   {l: t.to(device) for l, t in cache.items()})
        stage = getattr(self, "_stage", None)
        if stage is not None:
            object.__setattr__(c, "_stage", dict(stage))
        # strip/window layout (build_csf): sizes + descriptor tensors
        strip = getattr(self, "_strip", None)
        if strip is not None:
            object.__setattr__(c, "_strip", {
                k: v.to(device) if isinstance(v, torch.Tensor) else v
                for k, v in strip.items()})
        # root row pointers of the flat kernel (mttkrp.py _root_rowptr)
        rowptr = getattr(self, "_rowptr", None)
        if rowptr is not None:
            object.__setattr__(c, "_rowptr", rowptr.to(device))
        # f32 value stream of the flat kernel (mttkrp.py _vals32): the
        # copy, or False when the values are not all f32-exact
        v32 = getattr(self, "_vals32", None)
        if v32 is not None:
            object.__setattr__(c, "_vals32",
                               v32 if v32 is False else v32.to(device))
        return c

    def storage_bytes(self) -> int:
        b = self.vals.numel() * self.vals.element_size()
        rowptr = getattr(self, "_rowptr", None)
        if rowptr is not None:
            b += rowptr.numel() * rowptr.element_size()
        v32 = getattr(self, "_vals32", None)
        if v32 is not None and v32 is not False:
            b += v32.numel() * v32.element_size()
        pack = getattr(self, "_pack", None)
        if pack is not None:
            # expansions/leaf fids are strided views into the pack
            return b + pack.numel() * pack.element_size()
        for t in self.fptr + self.fids:
            if t is not None:
                b += t.numel() * t.element_size()
        # flat builds keep contiguous expansions instead of the tree
        cache = getattr(self, "_expand_cache", None)
        if cache and all(fp is None for fp in self.fptr):
            for l, t in cache.items():
                if t is not self.fids[self.nmodes - 1]:
                    b += t.numel() * t.element_size()
        return b

    def ancestor_expand(self, level: int) -> torch.Tensor:
        """Per-nonzero ancestor label at `level` (int32, length nnz) — the
        sorted coordinate column recovered from the CSF compression. Feeds
        the flat MTTKRP kernels; cached after first use."""
        cache = getattr(self, "_expand_cache", None)
        if cache is None:
            cache = {}
            object.__setattr__(self, "_expand_cache", cache)
        if level in cache:
            return cache[level]
        nm = self.nmodes
        if level == nm - 1:
            t = self.fids[nm - 1]
        else:
            # nnz start of each node at `level`: compose fptr chains down
            nnzstart = self.fptr[nm - 2]
            for l in range(nm - 3, level - 1, -1):
                nnzstart = nnzstart[self.fptr[l]]
            counts = nnzstart[1:] - nnzstart[:-1]
            labels = self.fids[level]
            if labels is None:  # dense root: identity labels
                labels = torch.arange(counts.numel(), dtype=torch.int32,
                                      device=counts.device)
            t = torch.repeat_interleave(labels, counts)
        cache[level] = t
        return t

    def freeze_flat(self) -> "Csf":
        """Materialize every per-level expansion and drop the fptr tree —
        the flat MTTKRP kernels only need expansions + vals. Halves the
        device footprint of billion-nnz ALLMODE sets (fptr is int64 and
        ~nnz-long when fibers are short)."""
        for l in range(self.nmodes):
            self.ancestor_expand(l)
        self.fptr = [None] * self.nmodes
        return self

    def to_dict(self) -> dict:
        return {
            "fptr": [t.cpu() if t is not None else None for t in self.fptr],
            "fids": [t.cpu() if t is not None else None for t in self.fids],
            "vals": self.vals.cpu(),
            "dims": list(self.dims),
            "dim_perm": list(self.dim_perm),
            "nfibs": [self.nfibs(l) for l in range(self.nmodes)],
        }


def order_modes(dims: Sequence[int], policy: str, mode: int = 0) -> List[int]:
    """Mode-order policies: smallfirst / root / leaf."""
    return [int(x) for x in native().order_modes(list(dims), policy, mode)]


L2_BYTES = 4 << 20          # one XCD's L2


def strip_gate(dims: Sequence[int], perm: Sequence[int], nnz: int,
               stage_rank: int, wgs: int = 256, tile_kb: int = 128,
               window_kb: int = 1024) -> Optional[dict]:
    """Line-count model of the strip/window layout (csrc/hip/
    mttkrp_strip.hip) against the unstaged v7 kernel for the root-output CSF
    with level order `perm`; the chosen sizes, or None when the layout is
    not worth building. Lines are 128-B L2 misses per nonzero, f64 factors:

        v7     NOTHER * rowlines + 12/128
        strip  (NOTHER - 1) * rowlines + 16/128
               + passes * 8 * dims[w] * rowlines / nnz

    rowlines = rank * 8 / 128 lines of a factor row, passes = ceil(strips /
    wgs) launches, and the last term every XCD re-reading the window mode's
    factor once per pass. A window level w is eligible when its factor is at
    least 4x the L2 (smaller ones already hit); the one with the smallest
    refetch term is taken, and the layout is chosen when the model predicts
    at most 0.8x the lines of v7. A tensor with fewer strips than one launch
    holds (`wgs`) is left alone: its workgroups would not fill the device,
    which the line model does not see."""
    nm = len(dims)
    if stage_rank <= 0 or not 3 <= nm <= 4 or nnz <= 0:
        return None
    rowbytes = stage_rank * 8
    rowlines = rowbytes / 128.0
    tile_rows = max(1, tile_kb * 1024 // rowbytes)
    window_rows = max(1, window_kb * 1024 // rowbytes)
    nstrips = -(-dims[perm[0]] // tile_rows)
    if nstrips < wgs:
        return None
    passes = -(-nstrips // wgs)
    best = None
    for l in range(1, nm):
        d = dims[perm[l]]
        if d * rowbytes < 4 * L2_BYTES:
            continue
        refetch = passes * 8 * d * rowlines / nnz
        if best is None or refetch < best[1]:
            best = (l, refetch)
    if best is None:
        return None
    nother = nm - 1
    v7 = nother * rowlines + 12 / 128.0
    new = (nother - 1) * rowlines + 16 / 128.0 + best[1]
    if new > 0.8 * v7:
        return None
    return {"level": best[0], "tile_rows": tile_rows,
            "window_rows": window_rows, "wgs": wgs, "passes": passes,
            "lines_v7": v7, "lines_strip": new}


def strip_layout(root: torch.Tensor, widx: torch.Tensor, nrows: int,
                 wdim: int, tile_rows: int, nnz_cap: int,
                 window_rows: int, groups: int = 1) -> tuple:
    """Strips and the strip/window order of a root-sorted stream. `root` is
    the non-decreasing output row per nonzero, `widx` the window level's
    index in the same order. Returns (strips, order): `strips` the host
    descriptors of plan_strips (every nonzero in exactly one strip, strips
    within the row and nnz caps, a row heavier than the cap split and
    flagged), `order` the permutation that stably sorts the stream by
    (strip, widx // window_rows) — inside a (strip, window) cell the order
    stays (row, remaining levels). strips["bounds"] ([strips, groups + 1])
    cuts every strip's range at the same `groups` + 1 window boundaries:
    the kernel's workgroups wait for each other after each group of windows
    of their strips."""
    dev = root.device
    rowptr = torch.searchsorted(
        root.contiguous(),
        torch.arange(nrows + 1, dtype=root.dtype, device=dev)
    ).to(torch.int64).cpu().contiguous()
    strips = native().plan_strips(rowptr, int(tile_rows), int(nnz_cap))
    ns = int(strips["row0"].numel())
    nb = -(-wdim // window_rows)
    kdt = torch.int32 if ns * nb < 2 ** 31 else torch.int64
    lens = (strips["p1"] - strips["p0"]).to(dev)
    cell = torch.repeat_interleave(
        torch.arange(ns, dtype=kdt, device=dev) * nb, lens)
    cell += torch.div(widx, window_rows, rounding_mode="floor").to(kdt)
    strips["nbuckets"] = nb
    cell, order = torch.sort(cell, stable=True)
    groups = max(1, min(int(groups), nb))
    edge = torch.tensor([-(-g * nb // groups) for g in range(groups + 1)],
                        dtype=kdt, device=dev)
    q = (torch.arange(ns, dtype=kdt, device=dev) * nb).unsqueeze(1) + edge
    strips["bounds"] = torch.searchsorted(cell, q.reshape(-1).contiguous()) \
        .to(torch.int64).reshape(ns, groups + 1).cpu()
    return strips, order


def build_csf(t: SpTensor, perm: Sequence[int], flat_only: bool = False,
              gather_tiles: int = 0, stage_rank: int = 0,
              lds_kb: int = 0, strip_rows: int = 0, strip_cap: int = 0,
              strip_window: int = 0, strip_wgs: int = 0,
              strip_groups: int = 0) -> Csf:
    """Build one CSF with level->mode permutation `perm`. `flat_only`
    (device builds): skip the fptr/fids tree — the sorted columns ARE the
    flat kernel's expansions, so billion-nnz ALLMODE sets build ~2x faster
    at half the transient footprint. `gather_tiles` > 1 (flat_only builds):
    the dense-tiling analog for the flat kernel — nonzeros are bucketed by
    the row range of the LARGEST non-root mode (outermost sort key), so
    each phase's random factor-row gathers hit a 1/T-sized working set
    (reference tt_densetile's cache story, tile.c:262, recast for the
    per-XCD L2/L3 hierarchy). Output-key runs stay contiguous per bucket,
    so the kernel is unchanged (one atomic per key run per bucket).
    `stage_rank` > 0 whose LDS staging is declined (run-density gate) may
    take the strip/window layout instead (strip_gate; SPLATT_STRIP=0
    disables, SPLATT_STRIP_TILE_KB / _WINDOW_KB / _WGS size it).
    `strip_rows` > 0 forces that layout with these sizes whatever the gate
    says: rows per strip, `strip_cap` nonzeros per strip (0: the mean strip
    load), `strip_window` rows of the window level per window (0: 1 MiB of
    factor rows), `strip_wgs` workgroups per launch (0: what the device
    holds), `strip_groups` groups of windows per strip, the workgroups of
    the launch pacing each other from group to group (0: the default,
    STRIP_GROUP_KB of factor rows per group)."""
    if any(d > 0xFFFFFFFF for d in t.dims):
        raise ValueError("mode dimensions above 2^32 are not supported "
                         "(CSF node ids are 32-bit; shard the mode first)")
    if t.device.type == "cuda":
        # device streams store labels as SIGNED int32 (the HIP kernels'
        # key/idx width); the host builder's unsigned ids reach 2^32
        if any(d > 0x7FFFFFFF for d in t.dims):
            raise ValueError(
                "device builds support mode dimensions up to 2^31-1 "
                "(int32 stream labels; shard the mode or build on CPU)")
        if t.nnz > 0x7FFFFFFF:
            raise ValueError(
                "device builds support up to 2^31-1 nonzeros per shard "
                "(torch sort limit; shard the tensor or build on CPU)")
        if lds_kb <= 0:
            import os
            lds_kb = int(os.environ.get("SPLATT_LDS_KB", "24"))
        return _build_csf_device(t, list(perm), flat_only, gather_tiles,
                                 stage_rank, lds_kb,
                                 (strip_rows, strip_cap, strip_window,
                                  strip_wgs, strip_groups))
    d = native().csf_build(t.inds, t.vals, list(t.dims), list(perm))
    return Csf(dims=[int(x) for x in d["dims"]],
               dim_perm=[int(x) for x in d["dim_perm"]],
               fptr=[x if isinstance(x, torch.Tensor) else None for x in d["fptr"]],
               fids=[x if isinstance(x, torch.Tensor) else None for x in d["fids"]],
               vals=d["vals"])


def _strip_ok(t: SpTensor, stage_rank: int) -> bool:
    """Tensors the strip kernel exists for: f64, 3 or 4 modes, a kernel
    rank, and no deterministic build (that path needs contiguous keys)."""
    import os
    return (t.vals.dtype == torch.float64 and 3 <= t.nmodes <= 4
            and stage_rank in (16, 32, 64)
            and os.environ.get("SPLATT_DETERMINISTIC") != "1")


def _strip_wgs(rank: int, nother: int, tile_rows: int) -> int:
    """Workgroups per launch the device holds, for both value-stream types
    (asking also prepares both kernel instances before any stream capture);
    0 when the tile does not fit."""
    return min(native().strip_wgs(rank, nother, v32, tile_rows)
               for v32 in (False, True))


# factor bytes of the window level per pace group: the workgroups of the
# launch stay within this much of the factor, times 1 + the run-ahead of
# mttkrp.py STRIP_AHEAD (measured default of the pair,
# profiles/amazon_strip_ahead.md); SPLATT_STRIP_GROUP_KB overrides
STRIP_GROUP_KB = 8192


def _strip_groups(factor_bytes: int) -> int:
    import os
    kb = int(os.environ.get("SPLATT_STRIP_GROUP_KB", str(STRIP_GROUP_KB)))
    return max(1, -(-factor_bytes // (max(1, kb) * 1024)))


def _strip_default(t: SpTensor, perm: List[int], stage_rank: int):
    """The gate of a build whose LDS staging was declined: strip_gate with
    the device's workgroup count and the SPLATT_STRIP_* knobs."""
    import os
    if os.environ.get("SPLATT_STRIP") == "0" or not _strip_ok(t, stage_rank):
        return None
    tile_kb = int(os.environ.get("SPLATT_STRIP_TILE_KB", "128"))
    window_kb = int(os.environ.get("SPLATT_STRIP_WINDOW_KB", "1024"))
    wgs = int(os.environ.get("SPLATT_STRIP_WGS", "0"))
    tile_rows = max(1, tile_kb * 1024 // (stage_rank * 8))
    held = _strip_wgs(stage_rank, t.nmodes - 1, tile_rows)
    if held <= 0:
        return None
    return strip_gate(t.dims, perm, t.nnz, stage_rank, wgs if wgs > 0 else held,
                      tile_kb, window_kb)


def _strip_forced(t: SpTensor, perm: List[int], stage_rank: int,
                  sizes: tuple) -> dict:
    rows, cap, window, wgs, groups = (int(x) for x in sizes)
    if not _strip_ok(t, stage_rank):
        raise ValueError(
            "the strip/window layout needs an f64 tensor of 3 or 4 modes, "
            "stage_rank in {16,32,64} and a non-deterministic build")
    w = max(range(1, t.nmodes), key=lambda l: t.dims[perm[l]])
    if window <= 0:
        window = max(1, (1 << 20) // (stage_rank * 8))
    if wgs <= 0:
        wgs = _strip_wgs(stage_rank, t.nmodes - 1, rows)
        if wgs <= 0:
            raise ValueError(f"a strip of {rows} rows at rank {stage_rank} "
                             "does not fit the device's LDS")
    return {"level": w, "tile_rows": rows, "window_rows": window,
            "wgs": wgs, "cap": cap, "groups": groups}


def _build_csf_device(t: SpTensor, perm: List[int],
                      flat_only: bool = False,
                      gather_tiles: int = 0, stage_rank: int = 0,
                      lds_kb: int = 48,
                      strip_sizes: tuple = (0, 0, 0, 0, 0)) -> Csf:
    """All-device CSF construction with torch/rocPRIM primitives."""
    stage_rank_in = stage_rank
    nm, nnz = t.nmodes, t.nnz
    dev = t.device
    if nnz == 0:
        c = Csf(dims=list(t.dims), dim_perm=list(perm),
                fptr=[torch.zeros(1, dtype=torch.int64, device=dev)
                      if l < nm - 1 else None for l in range(nm)],
                fids=[None if l == 0 else
                      torch.zeros(0, dtype=torch.int32, device=dev)
                      for l in range(nm)],
                vals=t.vals.clone())
        return c
    # lexicographic stable sort: least-significant level first
    order = torch.arange(nnz, device=dev)
    for level in reversed(range(nm)):
        keys = t.inds[perm[level]].index_select(0, order)
        order = order.index_select(0, torch.argsort(keys, stable=True))
    stage_meta = None
    strip_cfg = None
    cache_mb = 0
    if flat_only:
        import os as _os2
        cache_mb = int(_os2.environ.get("SPLATT_CACHE_TILE_MB", "0"))
    if flat_only and strip_sizes[0] > 0:
        # forced strip/window layout (tests, experiments): no staging
        strip_cfg = _strip_forced(t, perm, stage_rank, strip_sizes)
    elif flat_only and cache_mb > 0 and stage_rank > 0:
        # EXPERIMENTAL 3-D cache tiling for HBM-bound shapes: bucket by a
        # cell over ALL modes with per-mode factor windows <= cache_mb, so
        # every stream (output atomics + both gathers) works in an
        # L3-resident window. Output runs shrink to nnz/(ncells*root_dim);
        # the kernel is unchanged (atomic per run).
        vbytes = t.vals.element_size()
        win = cache_mb * 1024 * 1024
        cell = torch.zeros(nnz, dtype=torch.int64, device=dev)
        ncells = 1
        for l in range(nm):
            d = t.dims[perm[l]]
            tl = max(1, (d * stage_rank * vbytes + win - 1) // win)
            ch = (d + tl - 1) // tl
            b = torch.div(t.inds[perm[l]].index_select(0, order), ch,
                          rounding_mode="floor")
            cell = cell * tl + b
            ncells *= tl
        order = order.index_select(0, torch.argsort(cell, stable=True))
        stage_rank = 0  # no LDS staging on this sort order
    elif flat_only and (gather_tiles > 1 or stage_rank > 0):
        big = max(range(1, nm), key=lambda l: t.dims[perm[l]])
        if stage_rank > 0:
            # LDS-staging buckets: rows-per-bucket sized to the LDS budget.
            # Candidate selection: among non-root levels, stage the LARGEST
            # dim whose bucketing keeps the output-key runs dense — the
            # gate (>= min_run nnz per bucket x output row) protects the
            # one-atomic-per-run economy (measured: Netflix +13% at 8-9
            # nnz runs, -28% at ~1 nnz runs).
            import os as _os
            min_run = int(_os.environ.get("SPLATT_STAGE_MIN_RUN", "8"))
            # LDS tile sized by the factor STORAGE width (f32/bf16 store
            # modes fit 2-4x more rows per bucket)
            vbytes = {"f32": 4, "bf16": 2}.get(
                _os.environ.get("SPLATT_FACTOR_STORE", ""),
                t.vals.element_size())
            chunk_cap = max(64, (lds_kb * 1024) // (stage_rank * vbytes))
            root_dim = max(1, t.dims[perm[0]])
            # note: even L2-resident factors profit from staging (the TA
            # tag path, not bandwidth, is the binder — profiles/); the
            # size gate is available for experiments but off by default
            min_bytes = int(_os.environ.get("SPLATT_STAGE_MIN_BYTES", "0"))
            big, chunk, tiles = -1, 0, 1
            for l in sorted(range(1, nm), key=lambda x: -t.dims[perm[x]]):
                d = t.dims[perm[l]]
                if d * stage_rank * vbytes < min_bytes:
                    continue
                ch = min(chunk_cap, d)
                ti = (d + ch - 1) // ch
                if ti <= 1 or nnz // (ti * root_dim) >= min_run:
                    big, chunk, tiles = l, ch, ti
                    break
            if big < 0:
                strip_cfg = _strip_default(t, perm, stage_rank)
                stage_rank = 0
        else:
            dim_big = t.dims[perm[big]]
            tiles = gather_tiles
            chunk = (dim_big + tiles - 1) // tiles
        if tiles > 1:
            bucket = torch.div(t.inds[perm[big]].index_select(0, order),
                               chunk, rounding_mode="floor")
            order = order.index_select(0, torch.argsort(bucket, stable=True))
        if stage_rank > 0:
            stage_meta = {"level": big, "chunk": int(chunk),
                          "nbuckets": int(tiles)}
    strip_meta = None
    if strip_cfg is not None:
        w = strip_cfg["level"]
        nrows = t.dims[perm[0]]
        ns_rows = -(-nrows // strip_cfg["tile_rows"])
        cap = strip_cfg.get("cap") or max(1, -(-nnz // ns_rows))
        strips, sorder = strip_layout(
            t.inds[perm[0]].index_select(0, order),
            t.inds[perm[w]].index_select(0, order), nrows, t.dims[perm[w]],
            strip_cfg["tile_rows"], cap, strip_cfg["window_rows"],
            strip_cfg.get("groups") or _strip_groups(
                t.dims[perm[w]] * stage_rank_in * 8))
        order = order.index_select(0, sorder)
        del sorder
        # the passes take the strips in this order: heaviest first, so the
        # workgroups of one pass carry like loads and finish together
        by_load = torch.argsort(strips["p1"] - strips["p0"], descending=True,
                                stable=True)
        strip_meta = dict(strip_cfg, cap=int(cap),
                          nbuckets=int(strips["nbuckets"]))
        strip_meta["groups"] = int(strips["bounds"].shape[1]) - 1
        for k in ("row0", "nrows", "flags", "p0", "p1", "bounds"):
            strip_meta[k] = strips[k].index_select(0, by_load).to(dev)
        # the kernel's pace words (arrivals, time-outs, longest wait; 96
        # words, csrc/hip/launchers.hpp), cleared by every dispatch
        strip_meta["pace"] = torch.zeros(96, dtype=torch.int32, device=dev)
        # and the ring of 8 arrival counters of its run-ahead pacing, one
        # 128-B line each
        strip_meta["slots"] = torch.zeros(256, dtype=torch.int32, device=dev)
    sinds = [t.inds[perm[l]].index_select(0, order) for l in range(nm)]
    svals = t.vals.index_select(0, order)

    if flat_only:
        c = Csf(dims=list(t.dims), dim_perm=list(perm),
                fptr=[None] * nm, fids=[None] * nm, vals=svals)
        import os as _os3
        if (stage_meta is not None and nm <= 4
                and _os3.environ.get("SPLATT_PACK") != "0"):
            # packed stream: ONE int4 word per nonzero [key, staged level,
            # remaining levels] for the v6 LDS kernel (halves the stream
            # tag lookups, csrc/hip/mttkrp_lds.hip). The per-level
            # expansions become strided VIEWS into the pack — no second
            # copy of the index streams.
            lvl = stage_meta["level"]
            levels = [0, lvl] + [l for l in range(1, nm) if l != lvl]
            pack = torch.zeros(nnz, 4, dtype=torch.int32, device=dev)
            for col, l in enumerate(levels):
                pack[:, col] = sinds[l].to(torch.int32)
            cache = {l: pack[:, col] for col, l in enumerate(levels)}
            object.__setattr__(c, "_pack", pack)
            object.__setattr__(c, "_pack_levels", levels)
        else:
            cache = {l: sinds[l].to(torch.int32) for l in range(nm)}
        c.fids[nm - 1] = cache[nm - 1]
        object.__setattr__(c, "_expand_cache", cache)
        if stage_meta is not None:
            object.__setattr__(c, "_stage", stage_meta)
        if strip_meta is not None:
            object.__setattr__(c, "_strip", strip_meta)
        return c

    # new-node flags per level: node at level l starts where any of levels
    # 0..l changes (diff-level trick, same invariant as the C++ builder)
    fptr: List[Optional[torch.Tensor]] = [None] * nm
    fids: List[Optional[torch.Tensor]] = [None] * nm
    change = torch.zeros(nnz, dtype=torch.bool, device=dev)
    change[0] = True
    starts_per_level: List[torch.Tensor] = []
    for l in range(nm - 1):
        if nnz > 1:
            change[1:] |= sinds[l][1:] != sinds[l][:-1]
        starts = change.nonzero(as_tuple=True)[0]
        starts_per_level.append(starts)
        fids[l] = sinds[l].index_select(0, starts).to(torch.int32)
    for l in range(nm - 1):
        starts = starts_per_level[l]
        if l < nm - 2:
            child = starts_per_level[l + 1]
            ptr = torch.searchsorted(child, starts)
            ptr = torch.cat([ptr, torch.tensor([child.numel()], device=dev)])
        else:
            ptr = torch.cat([starts, torch.tensor([nnz], device=dev)])
        fptr[l] = ptr.to(torch.int64)
    fids[nm - 1] = sinds[nm - 1].to(torch.int32)

    # dense root => identity labels dropped (reference NULL root fids)
    if fids[0] is not None and fids[0].numel() == t.dims[perm[0]]:
        fids[0] = None

    return Csf(dims=list(t.dims), dim_perm=list(perm),
               fptr=fptr, fids=fids, vals=svals)


@dataclass
class CsfSet:
    """One or more CSF copies + the per-output-mode dispatch map
    (reference csf_alloc / mode_csf_map, csf.c:770-814, mttkrp.c:1831-1861)."""
    csfs: List[Csf]
    mode_csf: List[int]
    mode_depth: List[int]

    @property
    def nmodes(self) -> int:
        return len(self.mode_csf)

    @property
    def dims(self) -> List[int]:
        return self.csfs[0].dims

    @property
    def nnz(self) -> int:
        return self.csfs[0].nnz

    def to(self, device) -> "CsfSet":
        return CsfSet([c.to(device) for c in self.csfs],
                      list(self.mode_csf), list(self.mode_depth))

    def storage_bytes(self) -> int:
        return sum(c.storage_bytes() for c in self.csfs)


def csf_alloc(t: SpTensor,
              policy: CsfAllocPolicy | str = CsfAllocPolicy.TWOMODE) -> CsfSet:
    policy = CsfAllocPolicy(policy)
    nm = t.nmodes
    if policy == CsfAllocPolicy.ONEMODE:
        perm = order_modes(t.dims, "smallfirst")
        c = build_csf(t, perm)
        return CsfSet([c], [0] * nm, [c.level_of_mode(m) for m in range(nm)])
    if policy == CsfAllocPolicy.TWOMODE:
        perm = order_modes(t.dims, "smallfirst")
        longest = perm[-1]
        c0 = build_csf(t, perm)
        c1 = build_csf(t, order_modes(t.dims, "root", longest))
        mode_csf, mode_depth = [], []
        for m in range(nm):
            if m == longest:
                mode_csf.append(1)
                mode_depth.append(0)
            else:
                mode_csf.append(0)
                mode_depth.append(c0.level_of_mode(m))
        return CsfSet([c0, c1], mode_csf, mode_depth)
    # ALLMODE
    csfs = [build_csf(t, order_modes(t.dims, "root", m)) for m in range(nm)]
    return CsfSet(csfs, list(range(nm)), [0] * nm)
