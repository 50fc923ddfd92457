// Halo pack / unpack kernels for gfx950 (CDNA4).
//
// Reference kernels: src/halo_exchange/ops_halo_exchange.cu:519-664 (pack/unpack for QXYZ and
// XYZQ, one CUDA thread block of (32,4,4) per tile; their loops start at 0 without thread
// offsets, so every thread copies the same elements — SURVEY.md §7.4). Design here:
//  * one generic "box <-> dense buffer" copy: the box is rows of `len` contiguous elements
//    (x-runs for XYZQ, (q,x)-runs for QXYZ), so one kernel serves every face/edge/corner and
//    both storage orders;
//  * a flat 1-D work space (item = VEC consecutive doubles of one row, buffer offset =
//    item*VEC exactly) decoded with multiply-high "magic" division (no integer divides), so
//    consecutive lanes touch consecutive addresses of both the grid row and the buffer;
//  * 16-byte (double2) accesses whenever the row and all strides are even — the halo layout
//    (HaloExchange) pads x so interior rows start 64-B aligned, making every y/z face
//    dwordx4-vectorizable; 3-wide x faces fall back to 8-byte accesses (their 24-byte runs at a
//    4 KB pitch are sector-bound either way);
//  * 4 items in flight per lane (all loads issued before the stores) to cover HBM latency on a
//    wave64 machine without relying on occupancy alone;
//  * a multi-box variant packs every face/edge/corner of an exchange in ONE launch: blocks are
//    assigned to boxes through a prefix table in the kernel arguments (scalar loads, wave-
//    uniform), so small edge/corner boxes cost a handful of blocks instead of a launch each;
//  * a box-to-box "move" variant for the direct (pack-free) transfer: interior slab -> ghost
//    region of the same layout in one pass (2 bytes of HBM traffic per payload byte instead of
//    6 for pack -> copy -> unpack).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "spmv_device.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace tz {
namespace kern {

BoxTuning &box_tuning() {
  // process-wide launch tuning, changed only through its setters (bindings: kernels.set_*);
  // no environment overrides: every option can be flipped both ways inside one process
  static BoxTuning t;
  return t;
}

void set_xcd_remap(int mode) {
  if (mode < 0 || mode > 2)
    throw std::invalid_argument("xcd_remap must be 0 (round-robin), 1 (per-XCD range) or 2 (per-box)");
  box_tuning().xcd_remap = mode;
}

namespace {

// XCD block order of box_move_many_k only (the other batch kernels never read it, so it is a
// kernel argument of its own instead of part of every DevBatch copy)
struct DevRemap {
  uint32_t total;   // logical blocks (the launch may be padded up to a multiple of 8)
  uint32_t per_xcd; // 0: logical block = blockIdx.x; else blocks per XCD of the remap
  uint32_t box_xcd; // per-box remap: block_start padded to multiples of 8, nreal = real blocks
  uint16_t nreal[kMaxBoxes]; // (16 bits: max_blocks <= 65535)
};

// The dispatcher deals workgroups to the 8 XCDs round-robin (hardware block b runs on XCD
// b % 8). With the remap, XCD x runs logical blocks [x * per_xcd, (x + 1) * per_xcd): each
// pass of the grid-stride loop then covers one contiguous span of memory per XCD, so rows that
// cross a block boundary (72-B x-face runs) stay within one L2.
__device__ __forceinline__ uint32_t logical_block(const DevRemap &r) {
  if (r.per_xcd == 0) return blockIdx.x;
  return (blockIdx.x % 8u) * r.per_xcd + blockIdx.x / 8u;
}

// An unpack box whose rows may be widened over row padding (BoxDesc::lead / trail): grid rows of
// lead + len + trail elements written with 16-B stores when that makes them 16-B aligned, each
// element read from the dense buffer row (clamped into it for the padding elements, whose values
// nobody reads). Anything else: the plain box.
DevDesc make_dev_wide(const BoxDesc &b, bool unpack) {
  if (!unpack || !box_tuning().widen_unpack || (b.lead <= 0 && b.trail <= 0)) return make_dev(b);
  const int64_t wlen = int64_t(b.lead) + b.len + b.trail;
  const int64_t goff = b.grid_off - b.lead;
  if (b.lead < 0 || b.trail < 0 || b.len <= 0 || wlen % 2 != 0 || goff % 2 != 0 || goff < 0 ||
      b.s1 % 2 != 0 || b.s2 % 2 != 0 || b.s3 % 2 != 0)
    return make_dev(b);
  BoxDesc w = b;
  w.grid_off = goff;
  w.len = int32_t(wlen);
  DevDesc d = make_dev(w);
  // 16-B items on the grid side; the buffer is read one element at a time
  set_rows(d, RowKind::WideUnpack, uint32_t(wlen / 2), b);
  d.wide_len = b.len;
  d.wide_lead = b.lead;
  return d;
}

template <int VEC, bool UNPACK, int U, bool NT>
__device__ __forceinline__ void box_body(double *__restrict__ grid, const DevDesc &d, uint32_t tid,
                                         uint32_t nthreads) {
  using T = typename Vec<VEC>::T;
  T *__restrict__ buf = reinterpret_cast<T *>(d.buf);
  uint32_t it = tid;
  for (; it + (U - 1) * nthreads < d.items; it += U * nthreads) {
    T v[U];
    int64_t g[U];
#pragma unroll
    for (int k = 0; k < U; ++k) g[k] = grid_index<VEC>(d, it + k * nthreads);
    if (UNPACK) {
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = buf[it + k * nthreads];
#pragma unroll
      for (int k = 0; k < U; ++k) st<NT>(reinterpret_cast<T *>(grid + g[k]), v[k]);
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = ld<NT>(reinterpret_cast<const T *>(grid + g[k]));
#pragma unroll
      for (int k = 0; k < U; ++k) buf[it + k * nthreads] = v[k];
    }
  }
  for (; it < d.items; it += nthreads) {
    const int64_t g = grid_index<VEC>(d, it);
    if (UNPACK) st<NT>(reinterpret_cast<T *>(grid + g), buf[it]);
    else buf[it] = ld<NT>(reinterpret_cast<const T *>(grid + g));
  }
}

// widened unpack (make_dev_wide): whole 16-B pairs of the widened grid rows, each element from
// the dense buffer row, padding elements clamped to the row's ends
template <int U, bool NT>
__device__ __forceinline__ void unpack_wide_body(double *__restrict__ grid, const DevDesc &d, uint32_t tid,
                                                 uint32_t nthreads) {
  const double *__restrict__ buf = d.buf;
  const uint32_t blen = uint32_t(d.wide_len);
  const int32_t lead = d.wide_lead;
  const int32_t last = d.wide_len - 1;
  auto value = [&](uint32_t item) {
    const uint32_t row = d.dl.div(item);
    const int32_t x = int32_t(2 * (item - row * d.lvec)) - lead;
    const double *r = buf + int64_t(row) * blen;
    dbl2_t v;
    v.x = r[min(max(x, 0), last)];
    v.y = r[min(max(x + 1, 0), last)];
    return v;
  };
  uint32_t it = tid;
  for (; it + (U - 1) * nthreads < d.items; it += U * nthreads) {
    dbl2_t v[U];
    int64_t g[U];
#pragma unroll
    for (int k = 0; k < U; ++k) g[k] = grid_index<2>(d, it + k * nthreads);
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = value(it + k * nthreads);
#pragma unroll
    for (int k = 0; k < U; ++k) st<NT>(reinterpret_cast<dbl2_t *>(grid + g[k]), v[k]);
  }
  for (; it < d.items; it += nthreads)
    st<NT>(reinterpret_cast<dbl2_t *>(grid + grid_index<2>(d, it)), value(it));
}

// a pack or unpack of one box by threads `tid` of `nth` (make_dev / make_dev_wide kinds)
template <bool UNPACK, int U, bool NT>
__device__ __forceinline__ void copy_rows(double *__restrict__ grid, const DevDesc &d, uint32_t tid,
                                          uint32_t nth) {
  if (UNPACK && d.kind == RowKind::WideUnpack) unpack_wide_body<U, NT>(grid, d, tid, nth);
  else if (d.kind == RowKind::Vec16) box_body<2, UNPACK, U, NT>(grid, d, tid, nth);
  else box_body<1, UNPACK, U, NT>(grid, d, tid, nth);
}

template <bool UNPACK, int U, bool NT>
__global__ __launch_bounds__(kThreads) void box_copy_one_k(double *__restrict__ grid, DevDesc d) {
  copy_rows<UNPACK, U, NT>(grid, d, blockIdx.x * kThreads + threadIdx.x, gridDim.x * kThreads);
}

template <bool UNPACK, int U, bool NT>
__global__ __launch_bounds__(kThreads) void box_copy_many_k(double *__restrict__ grid, DevBatch b) {
  const BlockSlot s = find_block(b.block_start, b.n, blockIdx.x);
  copy_rows<UNPACK, U, NT>(grid, b.d[s.entry], s.tid, s.nth);
}

// direct move: src box -> dst box of the same layout (both rows addressed by one index)
template <int VEC, int U, bool NT, bool NTS>
__device__ __forceinline__ void move_body(const DevDesc &d, uint32_t tid, uint32_t nthreads) {
  using T = typename Vec<VEC>::T;
  const double *__restrict__ src = d.src;
  double *__restrict__ dst = d.dst + d.delta;
  uint32_t it = tid;
  for (; it + (U - 1) * nthreads < d.items; it += U * nthreads) {
    T v[U];
    int64_t g[U];
#pragma unroll
    for (int k = 0; k < U; ++k) g[k] = grid_index<VEC>(d, it + k * nthreads);
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = ld<NT>(reinterpret_cast<const T *>(src + g[k]));
#pragma unroll
    for (int k = 0; k < U; ++k) st<NTS>(reinterpret_cast<T *>(dst + g[k]), v[k]);
  }
  for (; it < d.items; it += nthreads) {
    const int64_t g = grid_index<VEC>(d, it);
    st<NTS>(reinterpret_cast<T *>(dst + g), ld<NT>(reinterpret_cast<const T *>(src + g)));
  }
}

// peeled rows (RowKind::Peeled, or PeeledTail with a tail): a row [x0, x0 + len) with x0 odd (the interior of
// an XYZQ grid with x = 0 at the row start begins at x = 3): element x0 alone, 16-B pairs from
// x0 + 1 (16-B aligned), and the last element alone when len - 1 is odd. Item xv of a row:
// xv < pairs a pair, then the head, then the tail; d.lvec = pairs + 1 + tail.
template <bool NT, bool NTS>
__device__ __forceinline__ void peel_body(const DevDesc &d, uint32_t tid, uint32_t nthreads) {
  const uint32_t tail = d.kind == RowKind::PeeledTail ? 1u : 0u;
  const uint32_t pairs = d.lvec - 1u - tail;
  const double *__restrict__ src = d.src;
  double *__restrict__ dst = d.dst + d.delta;
  for (uint32_t it = tid; it < d.items; it += nthreads) {
    const uint32_t row = d.dl.div(it);
    const uint32_t xv = it - row * d.lvec;
    const int64_t base = grid_index<1>(d, it) - int64_t(xv); // the row's x0
    if (xv < pairs) {
      const int64_t g = base + 1 + 2 * int64_t(xv);
      st<NTS>(reinterpret_cast<dbl2_t *>(dst + g), ld<NT>(reinterpret_cast<const dbl2_t *>(src + g)));
    } else {
      const int64_t g = xv == pairs ? base : base + 2 * int64_t(pairs) + 1;
      st<NTS>(dst + g, ld<NT>(src + g));
    }
  }
}

// row pair (MoveDesc::pair, d.run = len): item (row, k), k < 2 len: k < len moves element k of
// run A (row end -> row start), k >= len element k - len of run B (row start -> row end).
// Consecutive lanes cover consecutive k of a row, as the plain move covers a row's x: per row
// the same 2 line loads and 2 line stores as two separate boxes, but the lines a row's lanes
// load are the lines its lanes store into (x = 0 at the row start), within one wave.
template <int U, bool NTS>
__device__ __forceinline__ void pair_body(const DevDesc &d, uint32_t tid, uint32_t nthreads) {
  const int64_t len = d.run;
  const double *__restrict__ src = d.src;
  double *__restrict__ grid = d.dst;
  uint32_t it = tid;
  for (; it + (U - 1) * nthreads < d.items; it += U * nthreads) {
    double v[U];
    int64_t to[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t g = grid_index<1>(d, it + u * nthreads); // row base + k
      const uint32_t row = d.dl.div(it + u * nthreads);
      const int64_t k = int64_t(it + u * nthreads - row * d.lvec);
      const int64_t base = g - k;
      const int64_t from = k < len ? base + k : base + k + d.delta;          // A: end, B: start
      to[u] = k < len ? base + d.delta + k : base + k;                        // A: start, B: end
      v[u] = src[from];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st<NTS>(grid + to[u], v[u]);
  }
  for (; it < d.items; it += nthreads) {
    const int64_t g = grid_index<1>(d, it);
    const uint32_t row = d.dl.div(it);
    const int64_t k = int64_t(it - row * d.lvec);
    const int64_t base = g - k;
    const int64_t from = k < len ? base + k : base + k + d.delta;
    const int64_t to = k < len ? base + d.delta + k : base + k;
    st<NTS>(grid + to, src[from]);
  }
}

// the move of one box by threads `tid` of `nth` (make_move_batch kinds; PAIRS: the batch may
// hold row pairs)
template <int U, bool NT, bool NTS, bool PAIRS>
__device__ __forceinline__ void move_rows(const DevDesc &d, uint32_t tid, uint32_t nth) {
  // 16-B rows first, with one compare in front of them: the aligned layouts move nothing else,
  // and a workgroup lives for a few items only, so the tests before its body are part of its
  // time. The empty asm statement keeps the compiler from folding all four kinds into one
  // decision tree, which put two compares and two branches in front of every body.
  if (d.kind == RowKind::Vec16) return move_body<2, U, NT, NTS>(d, tid, nth);
  int32_t k = int32_t(d.kind);
  asm volatile("" : "+s"(k));
  const RowKind rest = RowKind(k);
  if (PAIRS && rest == RowKind::Pair) pair_body<U, NTS>(d, tid, nth);
  else if (rest == RowKind::Peeled || rest == RowKind::PeeledTail) peel_body<NT, NTS>(d, tid, nth);
  else move_body<1, U, NT, NTS>(d, tid, nth);
}

// one logical block `lb` of a batch of moves (box_move_many_k, box_move_spmv_k)
template <int U, bool NT, bool NTS>
__device__ __forceinline__ void move_block(const DevBatch &b, const DevRemap &r, uint32_t lb) {
  const BlockSlot s = find_block(b.block_start, b.n, lb);
  uint32_t nb = s.nb, j = s.blk;
  if (r.box_xcd) { // every box spread over all 8 XCDs, one contiguous share of it per XCD
    j = (j % 8u) * (nb / 8u) + j / 8u;
    nb = r.nreal[s.entry];
    if (j >= nb) return;
  }
  move_rows<U, NT, NTS, true>(b.d[s.entry], j * kThreads + threadIdx.x, nb * kThreads);
}

template <int U, bool NT, bool NTS>
__global__ __launch_bounds__(kThreads) void box_move_many_k(DevBatch b, DevRemap r) {
  const uint32_t lb = logical_block(r);
  if (lb >= r.total) return; // padding of the remapped launch (no barriers in this kernel)
  move_block<U, NT, NTS>(b, r, lb);
}

// the SpMV half of box_move_spmv_k (kernel arguments: device pointers and sizes)
struct SpmvDev {
  const int32_t *rowPtr, *colInd;
  const float *val, *x;
  float *y;
  int32_t nRows, accumulate;
  uint32_t nBlocks, stride; // SpMV workgroups; one every `stride` workgroups of the launch
};

// horizontal fusion: workgroup b is SpMV workgroup b / stride when b % stride == 0 (and that
// index < nBlocks), else move workgroup b - (SpMV workgroups at or before b). Both kinds are
// dispatched side by side from the first wave on. No barriers: a workgroup returns as soon as
// its part is done.
template <int U, bool NT, bool NTS, int W, int K>
__global__ __launch_bounds__(kThreads) void box_move_spmv_k(DevBatch b, SpmvDev sp) {
  const uint32_t bid = blockIdx.x;
  const uint32_t k = bid / sp.stride;
  if (bid % sp.stride == 0 && k < sp.nBlocks) {
    dev::csr_spmv_ilp_row<W, K>(int(k) * kThreads + int(threadIdx.x), sp.nRows, sp.rowPtr, sp.colInd,
                                sp.val, sp.x, sp.y, sp.accumulate);
    return;
  }
  const uint32_t before = min(sp.nBlocks, k + 1);
  DevRemap r{};
  move_block<U, NT, NTS>(b, r, bid - before);
}

struct DevSignal {
  unsigned int *done;
  unsigned long long *flag[kMaxBoxes];
  unsigned long long *count; // store mode (MoveSignal::count)
  uint64_t store_mask;
};

// explicit kernel arguments are limited to 4 KB; the largest signatures are checked here so a
// new field cannot push a launch over the limit
static_assert(sizeof(DevBatch) + sizeof(DevRemap) <= 4096, "box_move_many_k kernargs over 4 KB");
static_assert(sizeof(DevBatch) + sizeof(DevSignal) <= 4096, "box_move_signal_k kernargs over 4 KB");
static_assert(sizeof(double *) + sizeof(DevBatch) + sizeof(DevSignal) <= 4096,
              "box_pack_signal_k kernargs over 4 KB");
static_assert(sizeof(DevBatch) + sizeof(SpmvDev) <= 4096, "box_move_spmv_k kernargs over 4 KB");

// the box's last block publishes every block's (peer) stores with one system-scope signal
__device__ __forceinline__ void signal_box_done(const DevSignal &sig, int box, uint32_t nb) {
  signal_last_block(&sig.done[box], nb, [&] {
    if ((sig.store_mask >> box) & 1ull) {
      // single-writer flag (host memory): publish the new count with a plain release store
      const unsigned long long v = sig.count[box] + 1ull;
      sig.count[box] = v;
      __hip_atomic_store(sig.flag[box], v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      __hip_atomic_fetch_add(sig.flag[box], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  });
}

// peer put: the move, then the box's last block publishes it with one system-scope signal
template <int U, bool NT>
__global__ __launch_bounds__(kThreads) void box_move_signal_k(DevBatch b, DevSignal sig) {
  const BlockSlot s = find_block(b.block_start, b.n, blockIdx.x);
  move_rows<U, NT, false, false>(b.d[s.entry], s.tid, s.nth);
  signal_box_done(sig, s.entry, s.nb);
}

// IPC put into a neighbour's receive buffer: pack, then signal
template <int U, bool NT>
__global__ __launch_bounds__(kThreads) void box_pack_signal_k(double *__restrict__ grid, DevBatch b,
                                                              DevSignal sig) {
  const BlockSlot s = find_block(b.block_start, b.n, blockIdx.x);
  copy_rows<false, U, NT>(grid, b.d[s.entry], s.tid, s.nth);
  signal_box_done(sig, s.entry, s.nb);
}

constexpr int kMaxWaitSlots = 64;
struct WaitArgs {
  const unsigned long long *arrive;
  unsigned long long *expected;
  int *err;
  const int *abort; // process abort flag (kern::abort_flag): give up when set
  long long timeout_ticks;
  int n;
  int lag;  // wait for arrive[slot] >= expected[slot] + 1 - lag (then expected[slot] += 1)
  int wait; // 0: signal only
  int slot[kMaxWaitSlots];
  unsigned long long *signal[kMaxWaitSlots]; // after the wait: +1 (system scope), if non-null
  unsigned long long *count; // non-null: store ++count[i] into signal[i] instead (store mode)
};

// one wave: lane i waits for slot i, then (optionally) signals a peer's counter. Used for
// arrivals (receiver waits for the peers' puts, lag 0), credits (sender waits until the peer
// has consumed its previous put, lag 1) and releases (signal only).
__global__ __launch_bounds__(64) void ipc_wait_k(WaitArgs a) {
  const int i = threadIdx.x;
  if (i < a.n && a.wait) {
    const int s = a.slot[i];
    const unsigned long long want = a.expected[s] + 1 - (unsigned long long)a.lag;
    a.expected[s] += 1;
    const long long t0 = wall_clock64();
    for (uint32_t k = 1;
         __hip_atomic_load(&a.arrive[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < want; ++k) {
      __builtin_amdgcn_s_sleep(2);
      // the abort flag lives in host memory (a PCIe round trip): read it every 64 polls
      if (wall_clock64() - t0 > a.timeout_ticks ||
          ((k & 63u) == 0 && __hip_atomic_load(a.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))) {
        atomicOr(a.err, 1);
        break;
      }
    }
  }
  __threadfence_system();
  if (i < a.n && a.signal[i]) {
    if (a.count) {
      const unsigned long long v = a.count[i] + 1ull;
      a.count[i] = v;
      __hip_atomic_store(a.signal[i], v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      __hip_atomic_fetch_add(a.signal[i], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// the device batch of a move launch (shared by the plain and the signalling variant);
// `keep` maps batch entries back to input boxes
DevBatch make_move_batch(const MoveDesc *moves, int n, std::vector<int> &keep, int cap = 0, int unroll = 0) {
  DevBatch b{};
  for (int i = 0; i < n; ++i) {
    const MoveDesc &m = moves[i];
    if (!m.src || !m.dst) throw std::runtime_error("box_move_many: null array");
    const BoxDesc box = box_of(m, m.dst, m.src_off, m.len);
    DevDesc d = make_dev(box);
    if (d.items == 0) continue;
    d.src = m.src;
    d.delta = m.dst_off - m.src_off;
    if (m.pair) {
      if (m.src != m.dst || m.len < 1 || m.len > kMaxPairLen)
        throw std::runtime_error("box_move_many: a row pair needs src == dst and 1..8 elements per run");
      d.run = uint8_t(m.len);
      set_rows(d, RowKind::Pair, uint32_t(2 * m.len), box); // items (row, k < 2 len)
    } else {
      // 16-B accesses need both rows 16-B aligned: make_dev checked the source side (and the
      // destination base); the destination offset must be even as well
      if (d.kind == RowKind::Vec16 && (m.dst_off % 2 != 0 || reinterpret_cast<uintptr_t>(m.src) % 16 != 0))
        set_rows(d, RowKind::Vec8, uint32_t(m.len), box);
      // rows that start one element past a 16-B boundary on both sides (strides even): peel the
      // first element (and an odd last one), move the rest 16 B at a time
      if (d.kind == RowKind::Vec8 && box_tuning().peel_moves && m.len >= 3 && m.src_off % 2 != 0 &&
          m.dst_off % 2 != 0 && m.s1 % 2 == 0 && m.s2 % 2 == 0 && m.s3 % 2 == 0 &&
          reinterpret_cast<uintptr_t>(m.src) % 16 == 0 && reinterpret_cast<uintptr_t>(m.dst) % 16 == 0) {
        const uint32_t tail = uint32_t((m.len - 1) % 2), pairs = uint32_t((m.len - 1) / 2);
        set_rows(d, tail ? RowKind::PeeledTail : RowKind::Peeled, pairs + 1 + tail, box);
      }
    }
    append(b, d, blocks_for(d, cap, unroll));
    keep.push_back(i);
  }
  return b;
}

// workgroups per box of a signalling put: the launch's own cap, else the global one
int put_cap(const MoveSignal &sig) {
  return sig.max_blocks > 0 ? sig.max_blocks : box_tuning().put_max_blocks;
}

} // namespace

void box_copy(double *grid, const BoxDesc &b, bool unpack, void *stream) {
  if (!grid || !b.buf) throw std::runtime_error("box_copy: null grid or buffer");
  const DevDesc d = make_dev_wide(b, unpack);
  if (d.items == 0) return;
  const dim3 g(blocks_for(d));
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_copy(unpack, [&](auto un, auto u, auto nt) {
    hipLaunchKernelGGL((box_copy_one_k<decltype(un)::value, decltype(u)::value, decltype(nt)::value>), g,
                       dim3(kThreads), 0, s, grid, d);
  });
  TZ_HIP_LAUNCH_CHECK();
}

void box_copy_many(double *grid, const BoxDesc *boxes, int n, bool unpack, void *stream) {
  if (n <= 0) return;
  if (n > kMaxBoxes) throw std::runtime_error("box_copy_many: too many boxes");
  DevBatch b{};
  if (!grid) throw std::runtime_error("box_copy_many: null grid");
  for (int i = 0; i < n; ++i) {
    if (!boxes[i].buf) throw std::runtime_error("box_copy_many: null buffer");
    const DevDesc d = make_dev_wide(boxes[i], unpack);
    if (d.items == 0) continue;
    append(b, d, blocks_for(d));
  }
  if (b.n == 0) return;
  const dim3 g(total_blocks(b));
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_copy(unpack, [&](auto un, auto u, auto nt) {
    hipLaunchKernelGGL((box_copy_many_k<decltype(un)::value, decltype(u)::value, decltype(nt)::value>), g,
                       dim3(kThreads), 0, s, grid, b);
  });
  TZ_HIP_LAUNCH_CHECK();
}

void box_move_many(const MoveDesc *moves, int n, void *stream) {
  if (n <= 0) return;
  if (n > kMaxBoxes) throw std::runtime_error("box_move_many: too many boxes");
  std::vector<int> keep;
  const int U = box_tuning().move_unroll;
  if (U != 1 && U != 2 && U != 4) throw std::runtime_error("box_move_many: move_unroll must be 1, 2 or 4");
  const int items = std::max(U, box_tuning().move_items);
  DevBatch b = make_move_batch(moves, n, keep, 0, items);
  if (b.n == 0) return;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int mode = box_tuning().xcd_remap;
  DevRemap r{};
  if (mode == 2) { // pad every box to a multiple of 8 blocks, starting on a multiple of 8
    uint32_t t = 0;
    for (int i = 0; i < b.n; ++i) {
      const uint32_t nb = b.block_start[i + 1] - b.block_start[i];
      if (nb > 65535) throw std::runtime_error("box_move_many: too many blocks for the remap");
      r.nreal[i] = uint16_t(nb);
      b.block_start[i] = t;
      t += (nb + 7) / 8 * 8;
    }
    b.block_start[b.n] = t;
    r.box_xcd = 1;
  }
  r.total = total_blocks(b);
  r.per_xcd = mode == 1 ? (r.total + 7) / 8 : 0;
  const dim3 g(r.per_xcd ? r.per_xcd * 8 : r.total);
  const BoxTuning &t = box_tuning();
  dispatch_bools(t.nt_move, t.nt_move_store, [&](auto ntl, auto nts) {
    constexpr bool NT = decltype(ntl)::value, NTS = decltype(nts)::value;
    if (U == 1) hipLaunchKernelGGL((box_move_many_k<1, NT, NTS>), g, dim3(kThreads), 0, s, b, r);
    else if (U == 2) hipLaunchKernelGGL((box_move_many_k<2, NT, NTS>), g, dim3(kThreads), 0, s, b, r);
    else hipLaunchKernelGGL((box_move_many_k<4, NT, NTS>), g, dim3(kThreads), 0, s, b, r);
  });
  TZ_HIP_LAUNCH_CHECK();
}

namespace {
// one item in flight per lane, as the tuned move (BoxTuning::move_unroll 1)
template <int W, int K>
void launch_move_spmv(const dim3 &g, hipStream_t s, const DevBatch &b, const SpmvDev &sp) {
  const BoxTuning &t = box_tuning();
  dispatch_bools(t.nt_move, t.nt_move_store, [&](auto ntl, auto nts) {
    hipLaunchKernelGGL((box_move_spmv_k<1, decltype(ntl)::value, decltype(nts)::value, W, K>), g,
                       dim3(kThreads), 0, s, b, sp);
  });
}

// the moves' batch as box_move_spmv launches it (one item in flight, BoxTuning::move_items per lane)
DevBatch move_spmv_batch(const MoveDesc *moves, int n) {
  if (n > kMaxBoxes) throw std::runtime_error("box_move_spmv: too many boxes");
  std::vector<int> keep;
  const int items = std::max(1, box_tuning().move_items);
  return n > 0 ? make_move_batch(moves, n, keep, 0, items) : DevBatch{};
}

// lanes per row of the ILP kernel `lanes` names (throws unless kSpmvIlp + 1, 2 or 4)
int ilp_width(int lanes) {
  int W = 0;
  dispatch_ilp(lanes, "box_move_spmv: lanes must be kSpmvIlp + 1, 2 or 4",
               [&](auto w, auto) { W = decltype(w)::value; });
  return W;
}
} // namespace

MoveSpmvShape box_move_spmv_shape(uint32_t moveBlocks, int nRows, int lanes) {
  if (nRows < 0) throw std::runtime_error("box_move_spmv: bad SpMV job");
  MoveSpmvShape sh;
  sh.move_blocks = moveBlocks;
  sh.spmv_blocks = uint32_t((int64_t(nRows) * ilp_width(lanes) + kThreads - 1) / kThreads);
  const uint64_t all = uint64_t(sh.move_blocks) + sh.spmv_blocks;
  if (all >= (uint64_t(1) << 31)) throw std::runtime_error("box_move_spmv: grid too large");
  // an odd stride: the dispatcher deals workgroup b to XCD b % 8, so an even stride would put
  // every SpMV workgroup on the same XCD (a stride of 8: all on XCD 0, 61 instead of 50 us)
  sh.stride = sh.spmv_blocks ? uint32_t(all / sh.spmv_blocks) : uint32_t(all + 1);
  if (sh.spmv_blocks && sh.stride % 2 == 0) sh.stride -= 1;
  return sh;
}

MoveSpmvShape box_move_spmv_shape(const MoveDesc *moves, int n, int nRows, int lanes) {
  return box_move_spmv_shape(total_blocks(move_spmv_batch(moves, n)), nRows, lanes);
}

void box_move_spmv(const MoveDesc *moves, int n, const SpmvJob &job, void *stream) {
  if (job.nRows < 0 || (job.nRows > 0 && (!job.rowPtr || !job.y)))
    throw std::runtime_error("box_move_spmv: bad SpMV job");
  void (*launch)(const dim3 &, hipStream_t, const DevBatch &, const SpmvDev &) = nullptr;
  dispatch_ilp(job.lanes, "box_move_spmv: lanes must be kSpmvIlp + 1, 2 or 4", [&](auto w, auto k) {
    launch = &launch_move_spmv<decltype(w)::value, decltype(k)::value>;
  });
  const DevBatch b = move_spmv_batch(moves, n);
  const MoveSpmvShape sh = box_move_spmv_shape(total_blocks(b), job.nRows, job.lanes);
  SpmvDev sp{};
  sp.rowPtr = job.rowPtr;
  sp.colInd = job.colInd;
  sp.val = job.val;
  sp.x = job.x;
  sp.y = job.y;
  sp.nRows = job.nRows;
  sp.accumulate = job.accumulate ? 1 : 0;
  sp.nBlocks = sh.spmv_blocks;
  sp.stride = sh.stride;
  const uint32_t all = sh.move_blocks + sh.spmv_blocks;
  if (all == 0) return;
  launch(dim3{all}, static_cast<hipStream_t>(stream), b, sp);
  TZ_HIP_LAUNCH_CHECK();
}


void box_move_many_signal(const MoveDesc *moves, int n, const MoveSignal &sig, void *stream) {
  if (n <= 0) return;
  if (n > kMaxBoxes) throw std::runtime_error("box_move_many_signal: too many boxes");
  if (!sig.done) throw std::runtime_error("box_move_many_signal: null block counters");
  if (sig.store_mask) throw std::runtime_error("box_move_many_signal: store mode is for packs only");
  std::vector<int> keep;
  for (int i = 0; i < n; ++i)
    if (moves[i].pair) throw std::runtime_error("box_move_many_signal: row pairs are for self moves only");
  const DevBatch b = make_move_batch(moves, n, keep, put_cap(sig));
  if (b.n != n) throw std::runtime_error("box_move_many_signal: empty box (nothing to signal)");
  DevSignal ds{};
  ds.done = sig.done;
  for (int i = 0; i < n; ++i) {
    if (!sig.flag[keep[i]]) throw std::runtime_error("box_move_many_signal: null flag");
    ds.flag[i] = sig.flag[keep[i]];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 g(total_blocks(b));
  if (box_tuning().nt_move) hipLaunchKernelGGL((box_move_signal_k<4, true>), g, dim3(kThreads), 0, s, b, ds);
  else hipLaunchKernelGGL((box_move_signal_k<4, false>), g, dim3(kThreads), 0, s, b, ds);
  TZ_HIP_LAUNCH_CHECK();
}

void box_pack_many_signal(double *grid, const BoxDesc *boxes, int n, const MoveSignal &sig,
                          void *stream) {
  if (n <= 0) return;
  if (n > kMaxBoxes) throw std::runtime_error("box_pack_many_signal: too many boxes");
  if (!grid || !sig.done) throw std::runtime_error("box_pack_many_signal: null grid or counters");
  DevBatch b{};
  DevSignal ds{};
  ds.done = sig.done;
  ds.count = sig.count;
  ds.store_mask = sig.store_mask;
  if (sig.store_mask && !sig.count) throw std::runtime_error("box_pack_many_signal: store mode without counters");
  for (int i = 0; i < n; ++i) {
    if (!boxes[i].buf || !sig.flag[i]) throw std::runtime_error("box_pack_many_signal: null buffer/flag");
    const DevDesc d = make_dev(boxes[i]);
    if (d.items == 0) throw std::runtime_error("box_pack_many_signal: empty box (nothing to signal)");
    ds.flag[b.n] = sig.flag[i];
    append(b, d, blocks_for(d, put_cap(sig)));
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 g(total_blocks(b));
  if (box_tuning().nt_pack) hipLaunchKernelGGL((box_pack_signal_k<4, true>), g, dim3(kThreads), 0, s, grid, b, ds);
  else hipLaunchKernelGGL((box_pack_signal_k<4, false>), g, dim3(kThreads), 0, s, grid, b, ds);
  TZ_HIP_LAUNCH_CHECK();
}

void ipc_wait(const unsigned long long *arrive, unsigned long long *expected, const int *slots,
              int n, int *err, double timeout_s, void *stream, int lag,
              unsigned long long *const *signal) {
  if (n <= 0) return;
  if (n > kMaxWaitSlots) throw std::runtime_error("ipc_wait: too many slots");
  if (!arrive || !expected || !err) throw std::runtime_error("ipc_wait: null pointer");
  if (lag < 0 || lag > 1) throw std::runtime_error("ipc_wait: lag must be 0 or 1");
  WaitArgs a{};
  a.arrive = arrive;
  a.expected = expected;
  a.err = err;
  a.abort = abort_flag();
  a.timeout_ticks = (long long)(timeout_s * 1.0e8); // wall_clock64 runs at 100 MHz
  a.n = n;
  a.lag = lag;
  a.wait = 1;
  for (int i = 0; i < n; ++i) {
    a.slot[i] = slots[i];
    a.signal[i] = signal ? signal[i] : nullptr;
  }
  hipLaunchKernelGGL(ipc_wait_k, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  TZ_HIP_LAUNCH_CHECK();
}

void ipc_signal(unsigned long long *const *signal, int n, void *stream, unsigned long long *count) {
  if (n <= 0) return;
  if (n > kMaxWaitSlots) throw std::runtime_error("ipc_signal: too many counters");
  WaitArgs a{};
  a.n = n;
  a.wait = 0;
  a.count = count;
  for (int i = 0; i < n; ++i) {
    if (!signal[i]) throw std::runtime_error("ipc_signal: null counter");
    a.signal[i] = signal[i];
  }
  hipLaunchKernelGGL(ipc_wait_k, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  TZ_HIP_LAUNCH_CHECK();
}

std::vector<std::string> move_kinds(const MoveDesc *moves, int n) {
  if (n <= 0) return {};
  if (n > kMaxBoxes) throw std::runtime_error("move_kinds: too many boxes");
  std::vector<int> keep;
  const DevBatch b = make_move_batch(moves, n, keep);
  std::vector<std::string> out(size_t(n), "empty");
  for (int k = 0; k < b.n; ++k) {
    const char *name = "vec8";
    switch (b.d[k].kind) {
    case RowKind::Pair: name = "pair"; break;
    case RowKind::Peeled:
    case RowKind::PeeledTail: name = "peeled"; break;
    case RowKind::Vec16: name = "vec16"; break;
    default: break;
    }
    out[size_t(keep[size_t(k)])] = name;
  }
  return out;
}

} // namespace kern
} // namespace tz
