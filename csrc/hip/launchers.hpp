// The HIP launcher boundary: every host-callable entry point of
// csrc/hip/*.hip is declared here and nowhere else. The .hip file that owns a
// launcher includes this header and defines it (templates are explicitly
// instantiated there, one block per file); csrc/pybind.cpp and
// csrc/capi/capi_gpu.cpp include it and call. Plain C++17, no HIP header:
// `stream` is a hipStream_t passed as void *. C++ linkage, so a signature
// that drifts between the two sides fails to compile or link. Signatures use
// builtin types, pointers and the PODs below only.
//
// Return convention of every launcher that returns int:
//     0   launched (or nothing to do);
//   < 0   declined: the arguments do not qualify, nothing was launched;
//   > 0   a hipError_t — hipGetLastError() after the call's last launch, or
//         the error of a pre-launch query — error_string(rc) names it.
// All pointers are device pointers unless said otherwise; pointer TABLES
// (idx, mats, grams, ...) are host arrays of device pointers, read during
// the call only. Matrices are row-major and contiguous. Launches are
// asynchronous on `stream` and hipGraph-capturable.
#pragma once
#include <cstdint>

namespace splatt_store {
// bfloat16 factor storage: the upper 16 bits of an f32
struct bf16 { uint16_t v; };
}  // namespace splatt_store

namespace splatt {
namespace hip {

using splatt_store::bf16;

// ISA the kernels were compiled for (950 = gfx950)
int kernels_arch();
// hipGetErrorString of a positive launcher return value
const char * error_string(int rc);

// ------------------------------------------------ mttkrp_kernels.hip
// 3-mode CSF walk, V in {double, float}. which: 0 = root, 1 = internal,
// 2 = leaf output; Ma/Mb are the two non-output factors in level order
// ([rows, rank]). fptr0 has nslices + 1 entries, fptr1 nfibs + 1; fids0 may
// be null (dense root level). `out` ([rows, rank], pre-zeroed) accumulates
// with atomic adds. Any rank. Never declines.
template <typename V>
int mttkrp_csf3(int which, const int64_t * fptr0, const int32_t * fids0,
                const int64_t * fptr1, const int32_t * fids1,
                const int32_t * fids2, const V * vals, int64_t nslices,
                int64_t nfibs, int64_t nnz, const V * Ma, const V * Mb,
                V * out, int rank, void * stream);

// --------------------------------------------------- mttkrp_flat.hip
// Flat (expanded-CSF) MTTKRP: out[key[p], :] += vals[p] * prod_t
// mats[t][idx[t][p], :] over the launch's `nnz` nonzeros. V = compute and
// output type, S = factor storage type, VS = value-stream type;
// instantiated for <double>, <float>, <double, float>, <double, bf16>
// (reduced-precision factor storage) and <double, double, float> (f32 copy
// of f32-exact values). idx/mats: tables of 8, entries [0, nother) used,
// the rest null; nother in 2..7. `out` ([rows, rank], pre-zeroed)
// accumulates with atomic adds.
// Exactly one of key / rowptr is given:
//   key     int32 output row per nonzero (nnz entries); nrows/p0 unused.
//           With S == VS == V every rank and nother is served and the call
//           never declines; reduced storage needs a rank in {4,8,16,32,64}
//           and nother <= 4; an f32 value stream runs on the v7 kernel only.
//   rowptr  root output of a key-sorted stream: int64, nrows + 1 GLOBAL
//           stream positions; p0 is the global position of the launch's
//           first nonzero, i.e. idx/vals point at element p0. v7 only.
// v7 declines (-1) for a rank outside {8,16,32,64}, nother > 4,
// SPLATT_MTTKRP_U=1, streams that are not co-aligned to 128 B, and
// rank 8 / 3 modes with 8-byte values and factors.
template <typename V, typename S = V, typename VS = V>
int mttkrp_flat(const int32_t * key, const int64_t * rowptr, int64_t nrows,
                int64_t p0, const int32_t * const * idx,
                const S * const * mats, const VS * vals, int64_t nnz, V * out,
                int rank, int nother, void * stream);

// ---------------------------------------------------- mttkrp_lds.hip
// LDS-staged flat MTTKRP, root output of a bucketed build. One workgroup
// per block descriptor b in [0, nblocks): stream positions
// [blk_start[b], blk_end[b]) lie in one bucket of the staged level whose
// factor rows [blk_row0[b], blk_row0[b] + chunk) (clipped to dim0, the
// staged level's dimension) go to LDS: chunk * rank * sizeof(S) bytes must
// fit. rank in {4,8,16,32,64} (caller checked). `out` (pre-zeroed)
// accumulates with atomic adds. Never declines.
//
// flat5, V in {double, float}: separate streams; idx[0]/mats[0] are the
// staged level, then the remaining non-output levels. idx/mats: tables of
// at least 4, entries [0, nother) used, the rest null; nother in 2..4.
template <typename V>
int mttkrp_flat5(const int32_t * key, const int32_t * const * idx,
                 const V * const * mats, const V * vals,
                 const int64_t * blk_start, const int64_t * blk_end,
                 const int32_t * blk_row0, int64_t nblocks, int32_t chunk,
                 int32_t dim0, V * out, int rank, int nother, void * stream);
// flat6: packed stream, one int4 word per nonzero (x = output key,
// y = staged level, z/w = remaining levels). mats: table of at least 3 in
// that order, nother in 2..3. <V, S> as for mttkrp_flat: <double>, <float>,
// <double, float>, <double, bf16>.
template <typename V, typename S = V>
int mttkrp_flat6(const int32_t * pack, const S * const * mats,
                 const V * vals, const int64_t * blk_start,
                 const int64_t * blk_end, const int32_t * blk_row0,
                 int64_t nblocks, int32_t chunk, int32_t dim0, V * out,
                 int rank, int nother, void * stream);

// -------------------------------------------------- mttkrp_strip.hip
// Strip/window flat MTTKRP, root output of a strip-layout stream (f64
// compute, factors and output; VS in {double, float} as for mttkrp_flat).
// A strip s in [0, nstrips) is walked by one workgroup: output rows
// [s_row0[s], s_row0[s] + s_nrows[s]), s_nrows[s] <= tile_rows, accumulate
// in an LDS tile and are then written to `out`; s_flags[s] bit 0 / bit 1:
// the first / last row is shared with a neighbouring strip and is added
// atomically, so `out` must be pre-zeroed. s_bounds: nstrips x (ngroups + 1)
// stream positions, row s non-decreasing: group g of strip s is
// [s_bounds[s][g], s_bounds[s][g + 1]), inside [0, nnz), the length of key,
// idx and vals. key: int32 output row per nonzero;
// idx/mats: tables of at least 3, entries [0, nother) used, nother in 2..3,
// the window level first (the order only matters for speed). One launch of
// min(wgs, nstrips) workgroups, workgroup b taking strips b, b + grid, ...;
// `wgs` should not exceed strip_wgs(), or the grid is not co-resident.
// `pace` (96 words, device, or null): after each group the workgroups wait
// for each other on its arrival counter, each wait bounded by `pace_us`
// microseconds of wall clock; the launcher zeroes the words on `stream`
// first (a memset node under capture). After the launch word 0 holds the
// arrivals (grid x passes x ngroups), word 32 the workgroups whose wait ran
// out (they stop waiting, results do not change), word 64 the longest wait
// in ticks of strip_wall_khz(). Null: no waits. Two dispatches with one
// pace buffer running at once (two streams) would share the counter: they
// would pace wrongly, within the same bounds and with correct results; use
// one buffer per stream. Words 65 and 66 hold the sum of all workgroups'
// waits (ticks, modulo 2^32) and the number of calls that had to poll.
// `slots` (256 words, device, zeroed by the launcher like `pace`; or null)
// is a ring of 8 arrival counters, word 32 x i, which replaces word 0 as the
// thing waited on: call t of a workgroup arrives at slot t % 8 and waits for
// all arrivals of call t - ahead, so a workgroup may run `ahead` groups
// (0..7; 0 = the barrier) in front of the slowest; word 0 still ends at grid
// x passes x ngroups. Needs `pace`; ahead > 0 needs `slots`. Without
// `slots` the waits are on word 0 as before. `trace` (4 words per workgroup
// of the grid, device, or null; needs `pace`) receives per workgroup the XCC
// id, its wait sum, its polled calls and its longest wait.
// -1 = rank outside {16,32,64}, nother outside 2..3, a negative budget, a
// stream not aligned to 128 B, ahead outside 0..7 or slots / trace / ahead
// without what they need; -2 = the tile, tile_rows * (rank + 2) * 8 bytes,
// exceeds the device's LDS limit.
template <typename VS>
int mttkrp_strip(const int32_t * key, const int32_t * const * idx,
                 const double * const * mats, const VS * vals,
                 const int32_t * s_row0, const int32_t * s_nrows,
                 const int32_t * s_flags, const int64_t * s_bounds,
                 int ngroups, int64_t nstrips, int tile_rows, int wgs,
                 int64_t nnz, double * out, int rank, int nother,
                 void * stream, uint32_t * pace, int pace_us,
                 uint32_t * slots = nullptr, int ahead = 0,
                 uint32_t * trace = nullptr);
// Workgroups of that kernel instance resident at once on the current device
// (occupancy x compute units): the default `wgs`. 0 when the instance does
// not exist or the tile does not fit. Not for use during stream capture;
// calling it first also keeps mttkrp_strip free of attribute calls.
int strip_wgs(int rank, int nother, bool vals32, int tile_rows);
// Rate of the wall clock that bounds the waits, kHz (0: no device).
int strip_wall_khz();

// ---------------------------------------------------- mttkrp_det.hip
// Bitwise-deterministic MTTKRP, V in {double, float}. `out` ([rows, rank],
// pre-zeroed) is written with plain stores, no atomics. -1 = rank outside
// {4,8,16,32,64} or too many modes.
//
// det6: the packed, bucketed stream of flat6 (nother in 2..3, mats: table
// of at least 3) with per-bucket private outputs. blk_bucket_p0[b] is the
// stream position where block b's bucket starts. Workspaces, zeroed by the
// call: outb, nbuckets * nrows_out * rank elements; side,
// nblocks * 4 * (64 / rank) * 2 * rank elements.
template <typename V>
int mttkrp_det6(const int32_t * pack, const V * const * mats, const V * vals,
                const int64_t * blk_start, const int64_t * blk_end,
                const int32_t * blk_row0, const int64_t * blk_bucket_p0,
                int64_t nblocks, int32_t chunk, int32_t dim0,
                int64_t nrows_out, int64_t nbuckets, V * outb, V * side,
                V * out, int rank, int nother, void * stream);
// flat_det: key-sorted (depth-0) separate streams, nother in 2..4, idx/mats
// tables of 8. `side` is a workspace of side_elems elements, zeroed by the
// call; it needs flat_det_ws(nnz, rank) of them (-1 for a non-spec rank),
// else the call declines with -2.
int64_t flat_det_ws(int64_t nnz, int rank);
template <typename V>
int mttkrp_flat_det(const int32_t * key, const int32_t * const * idx,
                    const V * const * mats, const V * vals, int64_t nnz,
                    V * out, V * side, int64_t side_elems, int rank,
                    int nother, void * stream);

// -------------------------------------------------- dense_kernels.hip
// A is [n, F] with F <= 64; V in {double, float}.
// G (F x F, pre-zeroed) += A^T A, atomic adds. Never declines.
template <typename V>
int gram(const V * A, int64_t n, int F, V * G, void * stream);
// G = A^T A without atomics: Gpart (nparts * F * F elements, nparts >= 1)
// receives one partial per block, folded in block order. Never declines.
template <typename V>
int gram_det(const V * A, int64_t n, int F, V * Gpart, int64_t nparts, V * G,
             void * stream);
// C = A @ B, B is F x F. -1 unless F in {4,8,16,32,64}.
template <typename V>
int rowsolve(const V * A, const V * B, V * C, int64_t n, int F,
             void * stream);
// Ginv = G^-1 for SPD G (F x F), one workgroup. Never declines.
template <typename V>
int spd_inverse(const V * G, V * Ginv, int F, void * stream);
// which = 0: out[f] (pre-zeroed) += sum_i A[i,f]^2; which = 1:
// out[f] = max(out[f], max_i |A[i,f]|). f64, never decline.
int colacc(const double * A, int64_t n, int F, int which, double * out,
           void * stream);
// A[i,f] /= lam[f] in place
int colscale(double * A, int64_t n, int F, const double * lam, void * stream);
// out[f] (pre-zeroed) += sum_i X[i,f] * A[i,f]
int coldot(const double * X, const double * A, int64_t n, int F, double * out,
           void * stream);
// Front of the fused ALS tail, one launch: Ginv = inverse of
// (grams[0] .* ... .* grams[ngrams-1] + reg*I) — ngrams == 0 leaves Ginv
// alone — and the tail's accumulators reset: zero_gram (F x F) and
// zero_inner (F) to 0, lam_init (F) to 1; any of the three may be null.
// -1 for F outside 1..64 or more than 8 matrices.
int als_prep(const double * const * grams, int ngrams, double reg,
             double * Ginv, int F, double * zero_gram, double * lam_init,
             double * zero_inner, void * stream);

// ------------------------------------------------------ als_tail.hip
// The two passes of the fused tail: A = (K Ginv) / lam with
// lam = max(1, max_i |K Ginv|), gram += A^T A, inner[f] += sum_i K[i,f]
// A[i,f] (inner may be null). lam, gram and inner accumulate: they must
// have been reset by als_prep on this stream. K, A: [n, F], 16-B aligned,
// not aliased. -1 for F outside {16,32,64}, -2 for a misaligned pointer.
int als_tail(const double * K, const double * Ginv, int64_t n, int F,
             double * A, double * lam, double * gram, double * inner,
             void * stream);
// row count at which the tail's grid reaches its cap
int64_t als_tail_cap_rows();

// --------------------------------------------------- complete_als.hip
// Row-wise tensor-completion update of a root-sorted stream (f64), rank
// F in 1..64, nother in 2..7, idx/mats tables of 8.
// workspace doubles per segment slot at rank F
int64_t complete_slot_elems(int F);
// segments [seg0, seg0 + nseg) accumulate their normal equations; a
// single-segment row (seg_slot < 0) is solved into `out`, a multi-segment
// one leaves its partial in slot seg_slot - slot0 of `ws`.
int complete_segments(const int32_t * const * idx,
                      const double * const * mats, int nother,
                      const double * vals, const int64_t * seg_start,
                      const int32_t * seg_len, const int32_t * seg_row,
                      const int32_t * seg_slot, int64_t seg0, int64_t nseg,
                      int64_t slot0, int F, double reg, double * ws,
                      double * out, void * stream);
// multi-segment rows [m0, m0 + nm): fold slots mslot[m]..mslot[m+1] (minus
// slot0) and solve into out[mrow[m]]
int complete_reduce(const double * ws, const int32_t * mrow,
                    const int64_t * mslot, int64_t m0, int64_t nm,
                    int64_t slot0, int F, double reg, double * out,
                    void * stream);
// out[p] = sum_f lam[f] prod_t mats[t][inds[t][p], f], p in [0, n); lam may
// be null (all ones); nmodes in 1..8
int kruskal_predict(const int64_t * const * inds, const double * const * mats,
                    int nmodes, const double * lam, int64_t n, int F,
                    double * out, void * stream);

// ----------------------------------------------------------- ttmc.hip
// TTMc of a root-sorted stream (f64). idx/mats/ranks: the non-root levels
// in level order (tables of 8, nother in 2..7, each rank 1..32); a slot and
// an output row are prod(ranks) <= ttmc_max_cols() doubles.
int ttmc_max_cols();
// segments [seg0, seg0 + nseg): a single-segment row (seg_slot < 0) goes
// straight to `out`, a multi-segment one to slot seg_slot - slot0 of `ws`
int ttmc_segments(const int32_t * const * idx, const double * const * mats,
                  const int * ranks, int nother, const double * vals,
                  const int64_t * seg_start, const int32_t * seg_len,
                  const int32_t * seg_row, const int32_t * seg_slot,
                  int64_t seg0, int64_t nseg, int64_t slot0, double * ws,
                  double * out, void * stream);
// multi-segment rows [m0, m0 + nm): out[mrow[m]] = sum of slots
// mslot[m]..mslot[m+1] (minus slot0), P doubles each
int ttmc_reduce(const double * ws, const int32_t * mrow,
                const int64_t * mslot, int64_t m0, int64_t nm, int64_t slot0,
                int P, double * out, void * stream);

// ----------------------------------------------------------- admm.hip
// Fused block-ADMM update of one factor (f64, F in 1..64): H and U
// ([n, F]) are updated in place, iters receives one inner-iteration count
// per block of 64 rows. kind: constraint 0..3 with parameters w/lo/hi.
// variant: 0 = the default instance for this rank, 1 = VALU, 2 = MFMA
// (ranks 16/32/64 only).
int admm_update(const double * K, const double * Ginv, const double * rho,
                double * H, double * U, int32_t * iters, int64_t n, int F,
                int kind, double w, double lo, double hi, double inner_tol,
                int max_inner, int variant, void * stream);

// ------------------------------------------------------------ apr.hip
// Poisson CPD (CP-APR) multiplicative row update of a root-sorted stream
// (f64), rank F in 1..64, nother in 2..7, idx/mats tables of 8. B and Phi
// are [rows, F], iters / viol0 / done have one entry per row; a slot of `ws`
// is F doubles and slots are numbered from 0. Both return 0 or a positive
// hipError_t (hipErrorInvalidValue for arguments out of range) and never
// decline.
// segments [seg0, seg0 + nseg): a single-segment row (seg_slot < 0) runs up
// to max_inner inner iterations and stores B, Phi, iters, viol0; a segment
// of a multi-segment row whose done flag is clear leaves the partial Phi of
// ONE pass in slot seg_slot of `ws`.
int apr_segments(const int32_t * const * idx, const double * const * mats,
                 int nother, const double * vals, const int64_t * seg_start,
                 const int32_t * seg_len, const int32_t * seg_row,
                 const int32_t * seg_slot, int64_t seg0, int64_t nseg, int F,
                 double eps_div, double inner_tol, int max_inner,
                 const int32_t * done, double * ws, double * B, double * Phi,
                 int32_t * iters, double * viol0, void * stream);
// multi-segment rows [0, nm) that are not done: fold slots
// mslot[m]..mslot[m+1] into Phi[mrow[m]] and finish inner iteration `round`
// (1-based) of the row: iters = round, viol0 on round 1, then either set
// done (violation below inner_tol > 0) or B *= Phi; done is also set on
// round max_inner.
int apr_fold(const double * ws, const int32_t * mrow, const int64_t * mslot,
             int64_t nm, int F, int round, double inner_tol, int max_inner,
             int32_t * done, double * B, double * Phi, int32_t * iters,
             double * viol0, void * stream);

// -------------------------------------------------------- apr_pdnr.hip
// Poisson CPD damped-Newton row solver (PDNR) of a root-sorted stream (f64),
// rank F in 1..64, nother in 2..7, idx/mats tables of 8. One workgroup per
// entry of `rows` (rows that have nonzeros, any order; the caller issues the
// longest first) runs up to max_inner inner iterations of row rows[r], whose
// nonzeros are [rowptr[row], rowptr[row + 1]) of the stream: B ([all rows,
// F]) is updated in place, Phi receives the last pass's Phi, and iters,
// viol0, f0, f (objective at entry and exit), mu (final damping), nback
// (line-search evaluations) and nfail (rejected steps) one entry per row.
// Rows not listed are not written. Returns 0 or a positive hipError_t
// (hipErrorInvalidValue for arguments out of range or an LDS request over
// the device limit) and never declines.
int apr_pdnr(const int32_t * const * idx, const double * const * mats,
             int nother, const double * vals, const int64_t * rowptr,
             const int32_t * rows, int64_t nrows, int F, double eps_div,
             double inner_tol, int max_inner, double mu0, double * B,
             double * Phi, int32_t * iters, double * viol0, double * f0,
             double * f, double * mu, int32_t * nback, int32_t * nfail,
             void * stream);

// ------------------------------------------------------------ gcp.hip
// Generalized CPD loss-gradient pass of a root-sorted stream (f64), rank F
// in 1..64, nother in 2..7, idx/mats tables of 8. A (the output mode's
// factor) and G are [rows, F]. loss: 0 gaussian, 1 huber, 2 poisson,
// 3 poisson-log, 4 bernoulli-odds, 5 bernoulli-logit, 6 gamma, 7 rayleigh;
// `param` is huber's delta and unused otherwise. frow (one entry per row)
// may be null: the loss value is then not computed, and a slot of `ws` is F
// doubles; with frow it is F + 1. Slots are numbered from 0. Both return 0
// or a positive hipError_t (hipErrorInvalidValue for arguments out of range)
// and never decline. Rows without entries are not written: G and frow come
// in zeroed.
// segments [0, nseg): a single-segment row (seg_slot < 0) stores
// G[row] = sum dl/dm(val, mdl) pi and frow[row] = sum l(val, mdl); a segment
// of a multi-segment row leaves its partial sums in slot seg_slot of `ws`.
int gcp_segments(const int32_t * const * idx, const double * const * mats,
                 int nother, const double * vals, const int64_t * seg_start,
                 const int32_t * seg_len, const int32_t * seg_row,
                 const int32_t * seg_slot, int64_t nseg, int F, int loss,
                 double param, const double * A, double * ws, double * G,
                 double * frow, void * stream);
// multi-segment rows [0, nm): fold slots mslot[m]..mslot[m+1] in order into
// G[mrow[m]] (and frow[mrow[m]]); frow null or not as in gcp_segments.
int gcp_fold(const double * ws, const int32_t * mrow, const int64_t * mslot,
             int64_t nm, int F, double * G, double * frow, void * stream);

// ------------------------------------------------------------ sgcp.hip
// Stochastic GCP (f64). A sample is n = p + q coordinates, stored draws
// first: inds is [nmodes, n] int32 row-major, vals [n] (0 for the cell
// draws). mats/grads are host tables of nmodes device pointers, [dims[t], F]
// each, nmodes in 3..8, F in 1..64, loss and param as for gcp.hip. Adds the
// semi-stratified gradient estimate (weights wnz for stored draws, wz for
// cell draws) into grads with f64 atomics: grads come in zeroed, and the
// result is not bitwise reproducible. Every index must lie inside its
// factor: nothing is checked on the device. partials may be null; otherwise
// it has at least sgcp_nparts(n, nmodes, F) entries, every one of which is
// written, and their sum is the loss estimate. Returns 0 or a positive
// hipError_t (hipErrorInvalidValue for arguments out of range).
int64_t sgcp_nparts(int64_t n, int nmodes, int F);
int sgcp_grad(const int32_t * inds, const double * vals, int64_t n, int64_t p,
              const double * const * mats, double * const * grads, int nmodes,
              int F, int loss, double param, double wnz, double wz,
              double * partials, void * stream);
// One Adam step on flat buffers of n doubles, in place:
//   m = beta1 m + (1 - beta1) g;  v = beta2 v + ((1 - beta2) g) g
//   x = x - (lr (m c1)) / (sqrt(v c2) + eps);  x = max(x, lower) if bounded
//   g = 0
// c1, c2 are the bias corrections 1 / (1 - beta^step), computed by the
// caller. No contraction: every operation rounds once.
int adam_step(double * x, double * g, double * m, double * v, int64_t n,
              double lr, double beta1, double beta2, double eps, double c1,
              double c2, bool bounded, double lower, void * stream);

}  // namespace hip
}  // namespace splatt
