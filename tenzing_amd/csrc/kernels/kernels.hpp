// Host-side launch API of the hand-written gfx950 kernels (implemented in *.hip).
// All launches are asynchronous on the given hipStream_t (passed as void* so host-only
// translation units need no HIP headers) and never allocate or synchronize, so they can be
// captured into hipGraphs.
#pragma once

#include <cstdint>
#include <vector>
#include <string>

namespace tz {
namespace kern {

/// A 4-D box inside a pitched array, copied to/from a dense buffer.
/// The box is `n3 x n2 x n1` rows of `len` contiguous elements; row (i1,i2,i3) starts at
/// element `grid_off + i1*s1 + i2*s2 + i3*s3` of the array; the buffer is dense
/// ((i3*n2 + i2)*n1 + i1)*len + x. For the XYZQ halo layout rows are x-runs and
/// (i1,i2,i3) = (y,z,q); for QXYZ rows are (q,x)-runs and (i1,i2,i3) = (y,z,1).
struct BoxDesc {
  double *buf = nullptr;
  int64_t grid_off = 0;
  int64_t s1 = 0, s2 = 0, s3 = 0;
  int32_t len = 0, n1 = 0, n2 = 0, n3 = 0;
  /// unpack only: elements of row padding before / after each grid row that the writes may
  /// also cover (their values are undefined), so that short rows (x ghost runs of 9 doubles)
  /// become whole 16-B-aligned sectors written with 16-B stores; 0, 0: exactly the box
  int32_t lead = 0, trail = 0;
};

constexpr int kMaxBoxes = 32;

/// launch tuning of the box kernels (process-wide; measured defaults)
struct BoxTuning {
  // pack / unpack: items per lane the grid is sized for; 4 or 8 keep that many loads in flight,
  // 1-3 keep one in flight. 3 packs and unpacks 2 % faster than 4 in pipeline context
  // (scripts/ktune.py --unrolls, profiles/archive/r2_move_shape/ktune_unrolls*.jsonl); 8 is slower
  int unroll = 3;
  bool nt_pack = true;    // non-temporal grid loads in pack: -27 % pack time in pipeline context
  // non-temporal ghost stores in unpack: the ghosts are not read again within the exchange.
  // Round 1 measured +5 % on the one-rank pack -> copy -> unpack chain; the receive-buffer
  // unpack of the multi-rank exchange gains 7-8 % (2 loopback ranks, 0.228-0.239 -> 0.210-0.218
  // ms, scripts/nt_multi_ab.sh, profiles/archive/r2_nt/)
  bool nt_unpack = true;
  int max_blocks = 4096;  // cap per box (grid-stride beyond)
  // cap per box of the signalling put kernels, whose stores cross xGMI: one link moves ~77 GB/s per direction, which 64 blocks of posted 16-B
  // stores cover with a wide margin, while thousands of blocks stalled on a link would hold the
  // CU slots that the concurrent local moves, relay kernels and unpacks need
  int put_max_blocks = 64;
  // box_move (direct transfers): plain source loads and non-temporal ghost stores. The ghosts
  // are written once per exchange and nobody reads them inside it, so streaming them past the
  // caches leaves L2 / Infinity Cache to the interior slabs, which every exchange reads again:
  // 47.7 -> 44.4 us for the 26-direction move at 512^3 x 3 (scripts/move_ab.py; non-temporal
  // loads plus stores: 57.7 us).
  bool nt_move = false;
  bool nt_move_store = true;
  // box_move (direct transfers): items in flight per lane (1, 2 or 4) and
  // items per lane the grid is sized for (>= in flight; the lane loops over them). One in
  // flight, two per lane (twice the workgroups of 4 x 4) moves the 26 directions at 512^3 x 3
  // in 43.5 us against 44.1 us, the best of 10 shapes (scripts/move_ab.py --blocks,
  // profiles/archive/r2_move_shape/)
  int move_unroll = 1;
  int move_items = 2;
  int xcd_remap = 0; // box_move block order: 0 round-robin, 1 one contiguous range per XCD,
                     // 2 every box split into 8 contiguous per-XCD shares
  // moves of rows that start one element past a 16-B boundary peel that element and move the
  // rest with 16-B accesses (false: 8-B accesses throughout; XYZQ row-start layout, 26
  // directions: 92.0 -> 88.8 us, profiles/r5_roof/)
  bool peel_moves = true;
  // unpack boxes with lead / trail (BoxDesc) write their widened rows with 16-B stores (false:
  // exactly the box; the 26-direction unpack 66 -> 37 us, profiles/r5_unpack/)
  bool widen_unpack = true;
};
BoxTuning &box_tuning();
/// set BoxTuning::xcd_remap; throws std::invalid_argument unless mode is 0, 1 or 2
void set_xcd_remap(int mode);

/// A box-to-box move between two arrays of the SAME pitched layout: element (x,i1,i2,i3) of
/// the box at `src + src_off` goes to the same element of the box at `dst + dst_off`
/// (strides s1..s3, rows of `len`). This is the pack-free "direct" halo transfer: interior
/// slab -> ghost region of the neighbour's grid (own grid for self-neighbours, an IPC-mapped
/// peer grid over xGMI otherwise).
struct MoveDesc {
  const double *src = nullptr;
  double *dst = nullptr;
  int64_t src_off = 0, dst_off = 0;
  int64_t s1 = 0, s2 = 0, s3 = 0;
  int32_t len = 0, n1 = 0, n2 = 0, n3 = 0;
  /// row pair (self-wrap of the x axis in one array, src == dst): every row also moves its
  /// run [src - (dst_off - src_off) - ... ] back the other way. With delta = dst_off - src_off,
  /// row element e = src_off + row: [e, e + len) -> [e + delta, ...) AND
  /// [e + len + delta, e + 2 len + delta) -> [e + len, e + 2 len) -- the +x and -x boxes of one
  /// (dy, dz) moved by one lane per row, so that a row's ghost and source runs that share a
  /// cache line (x = 0 at the row start) are read and written while the line is in L2.
  /// At most kMaxPairLen elements per run.
  bool pair = false;
};
constexpr int kMaxPairLen = 8;
/// up to kMaxBoxes moves in ONE launch
void box_move_many(const MoveDesc *d, int n, void *stream);

/// Shape-matched roof probe of a move: whole 128-B lines of a pitched array, rows of `lines`
/// lines at `off` (elements, a multiple of 16) with strides s1..s3 (multiples of 16), read
/// (mode 0), written (mode 1) or read and written back by the same lane (mode 2), with full
/// 16-B accesses and the same flat indexing as the move. One launch for all boxes: the time of
/// touching exactly the lines a move touches, at the best access shape.
struct LineBox {
  double *base = nullptr;
  int64_t off = 0, s1 = 0, s2 = 0, s3 = 0;
  int32_t lines = 0, n1 = 0, n2 = 0, n3 = 0;
  /// 0 read, 1 write, 2 read + write back, 3 line-to-line copy to dst_base + dst_off (the
  /// move's own shape: each lane loads 16 B of a source line and stores them to its target line)
  int mode = 0;
  double *dst_base = nullptr;
  int64_t dst_off = 0;
};
/// variants: 0 one item in flight per lane + non-temporal stores, 1 four in flight + nt,
/// 2 one + plain stores, 3 four + plain
constexpr int kLineRoofVariants = 4;
void line_roof(const LineBox *boxes, int n, void *stream, int variant = 0);
/// the line boxes a batch of moves reads and writes (a move's rows at one intra-line alignment:
/// every row covers the same number of lines). `copies`: a move whose source and destination
/// rows cover the same number of lines becomes one mode-3 box (line-to-line copy, the move's
/// shape); otherwise reads and writes are separate boxes. Lines read and written by the same
/// rows become mode-2 boxes.
std::vector<LineBox> line_boxes(const MoveDesc *moves, int n, bool copies = true);
/// how box_move_many would move each box (no launch): "vec16", "vec8", "peeled", "pair" or
/// "empty"
std::vector<std::string> move_kinds(const MoveDesc *moves, int n);

/// Completion signal of a move whose destination is another rank's memory (IPC peer put):
/// when the last block of box i has stored its part, it makes every store of the box visible
/// at system scope and adds 1 to `flag[i]` (a counter in the receiver's uncached memory).
/// `done` holds one zero-initialized block counter per box (self-resetting).
struct MoveSignal {
  unsigned int *done = nullptr;
  unsigned long long *flag[kMaxBoxes] = {};
  /// store mode (flags in host memory, where a GPU read-modify-write would need PCIe
  /// AtomicOps): box k's flag has one writer, this one, so instead of adding 1 it stores
  /// ++count[k] (count: device memory, one counter per box, owned by the caller) with a
  /// system-scope release store. Boxes not in `store_mask` add 1 as usual.
  /// box_pack_many_signal only: no move puts into host memory, so box_move_many_signal throws
  /// when store_mask != 0 (and never reads count) instead of carrying an unused path.
  unsigned long long *count = nullptr;
  uint64_t store_mask = 0;
  /// workgroups per box at most (0: BoxTuning::put_max_blocks)
  int max_blocks = 0;
};
void box_move_many_signal(const MoveDesc *d, int n, const MoveSignal &sig, void *stream);
/// pack boxes of `grid` into their (possibly peer-mapped) dense buffers and signal each box's
/// completion like box_move_many_signal (IPC put into a neighbour's receive buffer)
void box_pack_many_signal(double *grid, const BoxDesc *d, int n, const MoveSignal &sig,
                          void *stream);

/// Device-side counter wait for IPC puts: for each of the `n` slots, spin (system-scope acquire
/// loads, s_sleep back-off) until `arrive[slot]` reaches expected[slot] + 1 - lag, then bump
/// expected[slot] and, if `signal` is given, add 1 to signal[k] (system scope, release).
/// lag 0: receiver waits for this round's arrival; lag 1: sender waits for the credit of its
/// previous put. A wait longer than `timeout_s` sets *err = 1 and gives up, so a lost peer
/// cannot hang the GPU.
void ipc_wait(const unsigned long long *arrive, unsigned long long *expected, const int *slots,
              int n, int *err, double timeout_s, void *stream, int lag = 0,
              unsigned long long *const *signal = nullptr);
/// add 1 to each of `n` (peer) counters, system scope, after the stream's prior work. With
/// `count` (device memory, n counters): store ++count[k] instead (single-writer counters in
/// host memory, no PCIe atomics; see MoveSignal::count)
void ipc_signal(unsigned long long *const *signal, int n, void *stream,
                unsigned long long *count = nullptr);

/// pack (grid -> buf) or unpack (buf -> grid) one box
void box_copy(double *grid, const BoxDesc &d, bool unpack, void *stream);
/// pack/unpack up to kMaxBoxes boxes in ONE launch (fused multi-face halo pack/unpack)
void box_copy_many(double *grid, const BoxDesc *d, int n, bool unpack, void *stream);

/// dst = src, `bytes` (16-B aligned pointers; the transport copy of self-neighbour exchanges)
void copy_bytes(void *dst, const void *src, size_t bytes, void *stream);
struct CopyDesc {
  void *dst = nullptr;
  const void *src = nullptr;
  size_t bytes = 0; // multiple of 16, 16-B aligned pointers
};
/// up to kMaxBoxes copies in one launch
void copy_many(const CopyDesc *d, int n, void *stream);

/// y[r] = sum_j A[r,j] x[j] for CSR A (f32 values, i32 indices). `lanesPerRow` in {1,2,4,8,16,32,64}
/// (0 = 8), or -1 for the CSR-stream kernel (block-contiguous nnz streaming + LDS segmented
/// reduction). When `accumulate`, y[r] += ... instead. lanesPerRow = kSpmvIlp + W (W = 1, 2, 4):
/// the ILP kernel (every lane issues 16 / W column loads, then the value loads and x gathers,
/// before using any).
constexpr int kSpmvIlp = 1000;
void csr_spmv(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val,
              const float *x, float *y, int lanesPerRow, bool accumulate, void *stream);
/// A CSR SpMV for box_move_spmv: y = A x (accumulate: y += A x) with the ILP kernel
/// (lanes = kSpmvIlp + W, W in {1, 2, 4})
struct SpmvJob {
  int nRows = 0;
  const int32_t *rowPtr = nullptr, *colInd = nullptr;
  const float *val = nullptr, *x = nullptr;
  float *y = nullptr;
  int lanes = kSpmvIlp + 4;
  bool accumulate = false;
};
/// Horizontal fusion: up to kMaxBoxes direct moves (as box_move_many, XCD remap 0) and one
/// SpMV in ONE launch. The SpMV's workgroups are spread evenly among the move's, so both run
/// at once from the first wave on, with no fork or join between two streams: the SpMV's L2
/// gathers fill the issue slots the move's HBM stream leaves idle (one GPU, 512^3 halo +
/// 150,000-row SpMV: 54.5 us one after the other, 49.2-49.8 us on two free-running streams,
/// scripts/coexec_probe.py)
void box_move_spmv(const MoveDesc *moves, int n, const SpmvJob &job, void *stream);
/// The grid of a box_move_spmv launch (host only, no launch): `move_blocks` move workgroups and
/// `spmv_blocks` = ceil(nRows * W / 256) SpMV workgroups in one grid of their sum. Workgroup b is
/// SpMV workgroup b / stride when stride divides b and that index is below spmv_blocks, else the
/// next move workgroup. stride = (move_blocks + spmv_blocks) / spmv_blocks, less one when even
/// (spmv_blocks = 0: the grid size + 1, so no workgroup is an SpMV one).
struct MoveSpmvShape {
  uint32_t move_blocks = 0, spmv_blocks = 0, stride = 1;
};
/// from the move workgroup count; this is the one copy of the arithmetic, the launcher calls it
MoveSpmvShape box_move_spmv_shape(uint32_t moveBlocks, int nRows, int lanes);
/// from the moves themselves, batched as box_move_spmv batches them (under the current BoxTuning)
MoveSpmvShape box_move_spmv_shape(const MoveDesc *moves, int n, int nRows, int lanes);
/// dst[i] = src[idx[i]]
void gather_f32(int n, const float *src, const int32_t *idx, float *dst, void *stream);
/// one peer's part of an IPC put of the SpMV x halo: dst[i] = src[idx[off + i]], i < n, then
/// *flag += 1 (system scope) once the whole segment is visible
struct PutSeg {
  float *dst = nullptr;
  int32_t off = 0, n = 0;
  unsigned long long *flag = nullptr;
};
constexpr int kMaxPutPeers = 64;
/// all peers' segments in one launch; `done` holds one zeroed completion counter per segment
void gather_put_signal(const float *src, const int32_t *idx, const PutSeg *segs, int nseg,
                       unsigned int *done, void *stream);
/// y = a + b (f32). The kernel reads and writes 16 bytes per access, so a, b and y must be
/// 16-byte aligned (as copy_bytes requires): throws std::runtime_error otherwise, before any launch
void vector_add_f32(int n, const float *a, const float *b, float *y, void *stream);
// ---- conjugate gradient (cg_kernels.hip): f32 vectors, f64 dot accumulation, every scalar an
// f64 in device memory. Results are deterministic (fixed partial count and summation order, no
// floating-point atomics) and no workgroup waits for another inside a launch: a dot product is
// one partial per block, and whoever needs the scalar sums the partials in its prologue.
/// partials per slab at most (a slab is kCgMaxPartials doubles, 2 KB)
constexpr int kCgMaxPartials = 256;
/// partials dot_partials_f32 / cg_fused_r write for vectors of n elements: ceil(n / 1024),
/// clamped to [1, kCgMaxPartials]
int dot_partial_count(int64_t n);
/// partials csr_spmv_dot writes: ceil(nRows * W / 1024), clamped likewise (`lanes`: W or kSpmvIlp + W)
int spmv_dot_partial_count(int nRows, int lanes);
/// partials[b] = block b's share of u . v, b < dot_partial_count(n); u may equal v. Vectors need
/// 4-byte alignment only (16-byte aligned ones are read with 16-byte loads, same results).
void dot_partials_f32(int64_t n, const float *u, const float *v, double *partials, void *stream);
/// *out = the sum of np partials, in the order every prologue uses: thread t of 256 holds
/// partial t (+0.0 from np on), xor butterfly over each wave64 (offsets 32, 16, .. 1), then the
/// four waves' sums in wave order. One block.
void sum_partials_f64(const double *partials, int np, double *out, void *stream);
/// alpha = pq != 0 ? rr / pq : 0 with pq the sum of the partials. One block.
void cg_alpha(const double *partials_pq, int np, const double *rr, double *alpha, void *stream);
/// rr_new = the sum of the partials; beta = rr != 0 ? rr_new / rr : 0; then rr = rr_new. One block.
void cg_beta(const double *partials_rr, int np, double *rr, double *beta, void *stream);
/// y[i] = fmaf(sign * float(*s), x[i], y[i]), sign = +1 or -1
void axpy_dev_f32(int64_t n, const double *s, int sign, const float *x, float *y, void *stream);
/// y[i] = fmaf(float(*s), y[i], x[i])
void xpay_dev_f32(int64_t n, const double *s, const float *x, float *y, void *stream);
/// q = A p as csr_spmv's ILP kernel computes it (lanes = kSpmvIlp + W, W = 1, 2, 4; same bits)
/// and partials_pq[b] = block b's share of p . q, b < spmv_dot_partial_count(nRows, lanes).
/// With partials_rr, block 0 also stores their sum to *rr (nothing in this launch reads rr).
void csr_spmv_dot(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *p,
                  float *q, int lanes, double *partials_pq, const double *partials_rr, int np_rr, double *rr,
                  void *stream);
/// x += alpha p with alpha formed as cg_alpha does (same bits as cg_alpha + axpy_dev_f32)
void cg_fused_x(int64_t n, const double *partials_pq, int np, const double *rr, const float *p, float *x,
                void *stream);
/// r -= alpha q (alpha likewise) and partials_rr = the partials of the new r . r (same bits as
/// cg_alpha + axpy_dev_f32 + dot_partials_f32)
void cg_fused_r(int64_t n, const double *partials_pq, int np, const double *rr, const float *q, float *r,
                double *partials_rr, void *stream);
/// p = r + beta p with beta = rr != 0 ? sum(partials_rr) / rr : 0 (rr is not written)
void cg_fused_p(int64_t n, const double *partials_rr, int np, const double *rr, const float *r, float *p,
                void *stream);
/// The single-reduction (Chronopoulos-Gear) recurrence, first launch: w = A r as csr_spmv's ILP
/// kernel computes it (lanes = kSpmvIlp + W, same bits), partials_gamma[b] = block b's share of
/// r . r and partials_delta[b] of r . w, b < spmv_dot_partial_count(nRows, lanes). With the four
/// scalar pointers (all or none), block 0 also copies *gamma_out to *gamma_prev and *alpha_out to
/// *alpha_prev: what the previous cg_sr_update published becomes what the next one reads.
void csr_spmv_dot2(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                   float *w, int lanes, double *partials_gamma, double *partials_delta, const double *gamma_out,
                   const double *alpha_out, double *gamma_prev, double *alpha_prev, void *stream);
/// Second launch. With gamma and delta the sums of the two slabs and gdiv(a, b) = b != 0 ? a / b : 0:
///   beta = gdiv(gamma, *gamma_prev), alpha = gdiv(gamma, delta - beta * gdiv(gamma, *alpha_prev))
/// (the product and the difference round separately), then with both rounded to f32
///   p = fmaf(beta, p, r), s = fmaf(beta, s, w), x = fmaf(alpha, p, x), r = fmaf(-alpha, s, r)
/// (same bits as xpay_dev_f32 twice and axpy_dev_f32 twice). Block 0 stores gamma, alpha and beta
/// to the three outputs, which must not alias gamma_prev / alpha_prev; those are not written.
void cg_sr_update(int64_t n, const double *partials_gamma, const double *partials_delta, int np,
                  const double *gamma_prev, const double *alpha_prev, const float *w, float *r, float *p, float *s,
                  float *x, double *gamma_out, double *alpha_out, double *beta_out, void *stream);
// ---- the same two launches for k = 2, 4 or 8 right-hand sides. A batched vector is n x k f32,
// row-major (element (i, j) at i * k + j: row i of all k vectors is 4 k <= 32 bytes inside one
// 128-byte line) and 16-byte aligned; batched slabs are k consecutive slabs of kCgMaxPartials
// doubles (column j's at + j * kCgMaxPartials); a batched scalar is an array of k doubles. Every
// column is computed exactly as the single kernels compute it alone: same bits.
/// Wout[:, j] = A R[:, j] and block b's shares of R[:, j] . R[:, j] and R[:, j] . Wout[:, j] in
/// slab j of partials_gamma / partials_delta; grid, row mapping, per-lane entry order and sums as
/// csr_spmv_dot2 (`lanes` likewise), so column j has the bits of csr_spmv_dot2 on column j alone.
/// With the four scalar arrays (all or none) block 0 copies k gammas and k alphas.
void csr_spmm_dot2(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *R,
                   float *Wout, int k, int lanes, double *partials_gamma, double *partials_delta,
                   const double *gamma_out, const double *alpha_out, double *gamma_prev, double *alpha_prev,
                   void *stream);
/// cg_sr_update for every column j with its own gamma_j, delta_j (slab j, np partials each),
/// gamma_prev[j], alpha_prev[j]: one pass over the n k elements. Block 0 stores k gammas, alphas
/// and betas to arrays that must not overlap gamma_prev / alpha_prev.
void cg_sr_update_batch(int64_t n, int k, const double *partials_gamma, const double *partials_delta, int np,
                        const double *gamma_prev, const double *alpha_prev, const float *W, float *R, float *P,
                        float *S, float *X, double *gamma_out, double *alpha_out, double *beta_out, void *stream);
// ---- the same four launches with a convergence test decided on the device. Every block of the
// update holds the same bits of gamma = r . r (sum of the gamma slab), so all blocks agree on
// stop = gamma <= *thresh without any hand-off; a NaN gamma never stops. "Stop" means "freeze":
// the stopped update writes no vector, the next SpMV returns at once, the update after it sums
// the same slab and stops again, however often the pair is replayed. thresh, done, iters (and
// all_done) must not share a byte with the iteration's scalars or with each other.
/// csr_spmv_dot2, unless *done is set: then every block returns before it writes anything (w,
/// both slabs and the previous scalars keep what the stopped update read)
void csr_spmv_dot2_stop(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                        float *w, int lanes, double *partials_gamma, double *partials_delta,
                        const double *gamma_out, const double *alpha_out, double *gamma_prev, double *alpha_prev,
                        const int *done, void *stream);
/// cg_sr_update with the test after its prologue. gamma <= *thresh: p, s, x, r, *alpha_out and
/// *beta_out are not written; block 0 stores *done = 1 and gamma. Otherwise cg_sr_update (same
/// bits), and block 0 also stores *done = 0 and adds 1 to *iters.
void cg_sr_update_stop(int64_t n, const double *partials_gamma, const double *partials_delta, int np,
                       const double *gamma_prev, const double *alpha_prev, const float *w, float *r, float *p,
                       float *s, float *x, double *gamma_out, double *alpha_out, double *beta_out,
                       const double *thresh, int *done, int64_t *iters, void *stream);
/// csr_spmm_dot2, unless *all_done is set (every column has stopped): then nothing is written.
/// While any column runs, a stopped one is computed again from its unchanged r: the same bits.
void csr_spmm_dot2_stop(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *R,
                        float *Wout, int k, int lanes, double *partials_gamma, double *partials_delta,
                        const double *gamma_out, const double *alpha_out, double *gamma_prev, double *alpha_prev,
                        const int *all_done, void *stream);
/// cg_sr_update_batch with one test per column: thresh[k], done[k], iters[k]. Column j with
/// gamma_j <= thresh[j] keeps its p, s, x, r, alpha_out[j] and beta_out[j] and gets done[j] = 1;
/// every other column is updated as cg_sr_update_stop updates it alone (same bits), done[j] = 0,
/// iters[j] += 1. *all_done = the AND of done; once it is 1 no block passes over the vectors.
void cg_sr_update_batch_stop(int64_t n, int k, const double *partials_gamma, const double *partials_delta, int np,
                             const double *gamma_prev, const double *alpha_prev, const float *W, float *R, float *P,
                             float *S, float *X, double *gamma_out, double *alpha_out, double *beta_out,
                             const double *thresh, int *done, int64_t *iters, int *all_done, void *stream);
// ---- the eight functions above as two: what an iteration of the family keeps in device memory,
// in one struct, and one launcher per launch. The eight fill an SrState and call these.
/// k = 1: single slabs and scalars; k = 2, 4, 8: k slabs per array, k doubles per scalar array.
/// The update publishes gamma, alpha and beta; the SpMV moves gamma and alpha to the prev pair.
/// The stop state (the last four) may be null where no launch tests; all_done serves the
/// batched form only.
struct SrState {
  int k = 1;
  double *partials_gamma = nullptr, *partials_delta = nullptr;
  double *gamma = nullptr, *alpha = nullptr, *beta = nullptr;
  double *gamma_prev = nullptr, *alpha_prev = nullptr;
  const double *thresh = nullptr;
  int *done = nullptr;
  int64_t *iters = nullptr;
  int *all_done = nullptr;
  double *partials_rho = nullptr; // the preconditioned pair's third slab (r . r); k = 1 only
};
/// csr_spmv_dot2 (batched: csr_spmm_dot2 on interleaved r and w), with `stop` its _stop form,
/// which reads st.done (batched: st.all_done). Every argument is checked here, and an error
/// carries the name of the function of the eight that (batched, stop) select.
void sr_spmv_dot2(bool batched, bool stop, int nRows, const int32_t *rowPtr, const int32_t *colInd,
                  const float *val, const float *r, float *w, int lanes, const SrState &st, void *stream);
/// cg_sr_update (batched: cg_sr_update_batch), with `stop` its _stop form; likewise
void sr_update(bool batched, bool stop, int64_t n, int np, const float *w, float *r, float *p, float *s, float *x,
               const SrState &st, void *stream);
// ---- the same recurrence preconditioned by M = diag(A) (Jacobi), one right-hand side, still two
// launches. dinv[i] = 1 / a_ii and u = dinv o r are two more f32 vectors; u is stored so that the
// SpMV gathers one vector, and always holds f32(dinv[i] * r[i]), a rounded product of its own.
// gamma = r . u and delta = u . (A u) take the places of r . r and r . (A r); beta and alpha are
// formed from them as cg_sr_update forms them. A third slab, rho = r . r, serves the stopping
// test, which stays the unpreconditioned form's: rho <= *thresh. No vector or slab of a launch
// may overlap another unless the launch only reads both; the scalar rules are the parents'.
/// w = A u as csr_spmv_dot2 computes w = A r (same grid, same mapping, same bits for the same
/// gathered vector), and block b's shares of r . u, u . w and r . r in the three slabs, b <
/// spmv_dot_partial_count(nRows, lanes). Block 0 moves the published scalars as csr_spmv_dot2 does.
void pcg_spmv_dot3(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                   const float *u, float *w, int lanes, double *partials_gamma, double *partials_delta,
                   double *partials_rho, const double *gamma_out, const double *alpha_out, double *gamma_prev,
                   double *alpha_prev, void *stream);
/// pcg_spmv_dot3, unless *done is set: then every block returns before it writes anything
void pcg_spmv_dot3_stop(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                        const float *u, float *w, int lanes, double *partials_gamma, double *partials_delta,
                        double *partials_rho, const double *gamma_out, const double *alpha_out, double *gamma_prev,
                        double *alpha_prev, const int *done, void *stream);
/// beta and alpha as cg_sr_update forms them from the two slabs, then with both rounded to f32 and
/// u_old = f32(dinv * r) (recomputed from the loaded values, not read from u):
///   p = fmaf(beta, p, u_old), s = fmaf(beta, s, w), x = fmaf(alpha, p, x), r = fmaf(-alpha, s, r),
///   u = f32(dinv * r)
/// (same bits as xpay_dev_f32 twice, axpy_dev_f32 twice and one f32 product). Block 0 publishes
/// gamma, alpha and beta.
void pcg_update(int64_t n, const double *partials_gamma, const double *partials_delta, int np,
                const double *gamma_prev, const double *alpha_prev, const float *w, const float *dinv, float *r,
                float *p, float *s, float *x, float *u, double *gamma_out, double *alpha_out, double *beta_out,
                void *stream);
/// pcg_update with the test after its prologue, on rho = the sum of np partials of partials_rho.
/// rho <= *thresh: no vector, *alpha_out or *beta_out is written; block 0 stores *done = 1 and
/// gamma. Otherwise pcg_update (same bits), *done = 0 and *iters += 1. A NaN rho never stops.
void pcg_update_stop(int64_t n, const double *partials_gamma, const double *partials_delta, int np,
                     const double *gamma_prev, const double *alpha_prev, const float *w, const float *dinv, float *r,
                     float *p, float *s, float *x, float *u, double *gamma_out, double *alpha_out, double *beta_out,
                     const double *partials_rho, const double *thresh, int *done, int64_t *iters, void *stream);
/// The four above as two launchers on an SrState with k = 1 and partials_rho set, as sr_spmv_dot2
/// and sr_update serve the unpreconditioned eight: every argument is checked here, once
void sr_pcg_spmv_dot3(bool stop, int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val,
                      const float *r, const float *u, float *w, int lanes, const SrState &st, void *stream);
void sr_pcg_update(bool stop, int64_t n, int np, const float *w, const float *dinv, float *r, float *p, float *s,
                   float *x, float *u, const SrState &st, void *stream);
// ---- mixed-precision iterative refinement around that f32 solve (cg_refine_kernels.hip): the
// solution is kept in f64, the residual b - A x64 is evaluated in f64 (A and b are f32 data, exact
// in f64), and the f32 recurrence solves A d = r64 to a modest tolerance again and again. One
// refinement step is the three launches below, in this order on one stream. The outer state
// (RefineOuter) must not share a byte with the iteration's scalars or the stop state, or with
// itself: the rule of thresh, done and iters above. Every launch returns before it writes
// anything once *outer.done is set, decided uniformly over its grid as *done is read above.
/// the outer threshold refine_tol^2 * b . b (the host's), the refined flag, the restarts of the
/// inner solve so far, and the last r64 . r64
struct RefineOuter {
  const double *thresh = nullptr;
  int *done = nullptr;
  int64_t *steps = nullptr;
  double *rr64 = nullptr;
};
/// x64[i] += double(x[i]) (one f64 add), then x[i] = s[i] = 0. f32 vectors 4-byte aligned.
void cg_refine_accumulate(int64_t n, float *x, float *s, double *x64, const int *outer_done, void *stream);
/// partials the next launch writes per slab: spmv_dot_partial_count(nRows, 4)
int cg_refine_partial_count(int nRows);
/// r64[i] = double(b[i]) - sum_j double(a_ij) * x64[col_j], products and sums in f64 (4 lanes per
/// row, a fixed order: the same bits on every call), and r[i] = p[i] = f32(r64[i]). With dinv and u
/// (both or neither): u[i] = f32(dinv[i] * r[i]), a rounded product of its own as pcg_update keeps
/// it, and p[i] = u[i]. partials64[b] = block b's share of r64 . r64, partials32[b] of r . r (the
/// new f32 vector), b < cg_refine_partial_count(nRows).
void cg_refine_residual(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *b,
                        const double *x64, const float *dinv, double *r64, float *r, float *p, float *u,
                        double *partials64, double *partials32, const int *outer_done, void *stream);
/// One block. With rr64 and rr32 the sums of np partials of the two slabs (sum_partials_f64's
/// order), *outer.rr64 = rr64. rr64 <= *outer.thresh (a NaN never passes): *outer.done = 1 and
/// nothing else is written. Otherwise the inner solve restarts: *thresh = tol2 * rr32, *done = 0,
/// the five scalars +0.0 (the next update then has beta = 0) and *outer.steps += 1. The inner
/// solve's iters is not an argument: it counts over the whole solve.
void cg_refine_decide(const double *partials64, const double *partials32, int np, double tol2, double *thresh,
                      int *done, double *gamma, double *alpha, double *beta, double *gamma_prev, double *alpha_prev,
                      const RefineOuter &outer, void *stream);

/// y += alpha * x (f64)
void axpy_f64(int64_t n, double alpha, const double *x, double *y, void *stream);
/// fill a[i] = base + scale * i (f64) — deterministic test patterns
void iota_f64(int64_t n, double base, double scale, double *a, void *stream);
/// empty kernel (launch-overhead probes, reference test/test_gpu_graph.cu:10)
void empty(void *stream);
/// spin for `ticks` of the constant-rate wall clock (synthetic device work for scheduling tests)
void busy_wait(int64_t ticks, int blocks, void *stream);

/// Process-wide device abort flag (host-coherent memory, allocated on first use). Every kernel
/// that spins (IPC arrival and credit waits, busy_wait) polls it and gives up once it is set,
/// so the runtime watchdog can drain a hung schedule's device work without killing the process.
/// The pointer is a kernel argument (hipGraph captures keep it valid: it is never freed).
const int *abort_flag();
/// host side: set or clear the flag (vector stores from the host; the kernels only load it)
void set_abort(bool on);
bool abort_set();

/// A box of the halo grid for the 7-point stencil (see stencil_kernels.hip). Element (i, y, z,
/// o) of the box is at base + o*so + z*sz + y*sy + i, for i < row (a contiguous run), y < ny,
/// z < nz, o < nouter; its x neighbours are +-xs away. The box must have a one-cell apron of
/// valid memory (ghosts) on every side.
struct StencilBox {
  const double *in = nullptr;
  double *out = nullptr;
  int64_t base = 0, sy = 0, sz = 0, so = 0;
  int32_t row = 0, ny = 0, nz = 0, nouter = 1, xs = 1;
  // elements at the start / end of every row that are not output cells: never stored, and read
  // only as neighbours of the output cells [m0, row - m1). A box can keep an aligned row (16-B
  // accesses) while excluding its first / last x cells (the ghost-free interior): masked by xs
  // or more, a side needs no x apron, and no result depends on the y / z aprons of masked
  // elements (tenzing_amd/utils/stencil_ref.py `needed` is this rule in numpy)
  int32_t m0 = 0, m1 = 0;
  double c0 = 0.4, c1 = 0.1;
};
/// stencil launch shape: rows per workgroup tile (4, 8, 16) and planes per z chunk (32, 64)
struct StencilTuning {
  int ty = 16; // 64 x 16 tiles (scripts/stencil_bench.py)
  // 64-plane chunks with the tiles in XCD-contiguous order (below): 512^3 x 3, interleaved
  // A/B in one process, QXYZ 1538 us / XYZQ 1483 us, against 1569-1573 / 1566 us for the best
  // hardware-order tiling (16-plane chunks, whose 4x the workgroups had beaten 64-plane ones in
  // the hardware order) and 1605 / 1589 us for torch's copy of the padded grid
  // (profiles/r6_stencil/)
  int zc = 64;
  int pf = 1;  // planes in flight beyond z + 1 (1 or 2)
  bool db = true; // double-buffered LDS tile (one barrier per plane instead of two)
  // tiles in XCD-contiguous order (each XCD a contiguous range of tiles, so a tile's row aprons
  // come from its own L2; FETCH_SIZE -8 %) instead of the hardware's round-robin over the 8 XCDs
  bool xcd_tiles = true;
};
StencilTuning &stencil_tuning();
/// out = c0 * in + c1 * (sum of the 6 face neighbours) over the box; `lds`: 2.5-D LDS-tiled
/// kernel, else neighbours straight from global memory (both march z with a register queue)
void stencil7(const StencilBox &b, bool lds, void *stream);
/// a box one or a few cells thick (the boundary shell) goes to a one-thread-per-element kernel
bool stencil_thin(const StencilBox &b);
/// several thin boxes in one launch
void stencil7_thin_many(const StencilBox *b, int n, void *stream);

/// Halo grid geometry for init / verification kernels.
struct HaloGeom {
  int32_t order = 0; // 0 = XYZQ (x fastest, q slowest, x-padded rows), 1 = QXYZ
  int64_t xoff = 0, sy = 0, sz = 0, sq = 0; // XYZQ strides (elements)
  int32_t nx = 0, ny = 0, nz = 0, nq = 0, g = 0;
  int32_t cx = 0, cy = 0, cz = 0, px = 1, py = 1, pz = 1;
  int32_t neighbors = 6; // which ghost regions an exchange fills (6 faces, 26 all)
  int32_t gen = 0;       // generation 0..3: shifts every value, so data left over from an
                         // earlier exchange of another generation fails the check
};
/// interior = encoded global coordinate, ghosts = -1
void halo_init(double *grid, const HaloGeom &g, void *stream);
/// count elements that differ from what a completed exchange must leave; result in *count
void halo_check(const double *grid, const HaloGeom &g, unsigned long long *count, void *stream);
/// stencil mode: count interior cells of `out` that differ from the 7-point stencil (default
/// coefficients) of the field halo_init writes (global coordinates, periodic) by more than
/// 2^-49 * want (derivation at stencil_check_k; a NaN counts)
void stencil_check(const double *out, const HaloGeom &g, unsigned long long *count, void *stream);

} // namespace kern
} // namespace tz
