// Host side of the kernel launches, in three parts: the launch check; the runtime-value ->
// template-argument dispatchers and the prefix-table builder every batched launch uses; and the
// builders of the box batches of batch_device.hpp (halo and roof kernels only). Include from
// .hip translation units.
#pragma once

#include <hip/hip_runtime.h>

#include "batch_device.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

#define TZ_HIP_LAUNCH_CHECK()                                                                      \
  do {                                                                                             \
    hipError_t e_ = hipGetLastError();                                                             \
    if (e_ != hipSuccess)                                                                          \
      throw std::runtime_error(std::string("kernel launch failed: ") + hipGetErrorString(e_));     \
  } while (0)

namespace tz {
namespace kern {
namespace {

template <int N> using Int = std::integral_constant<int, N>;

// f(Int<W>, Int<K>) for the ILP SpMV with W = lanes - kSpmvIlp lanes per row (K = 16 / W loads
// in flight per lane); `what`: the message thrown for any other W
template <typename F> void dispatch_ilp(int lanes, const char *what, F &&f) {
  switch (lanes - kSpmvIlp) {
  case 1: f(Int<1>{}, Int<16>{}); break;
  case 2: f(Int<2>{}, Int<8>{}); break;
  case 4: f(Int<4>{}, Int<4>{}); break;
  default: throw std::runtime_error(what);
  }
}

// f(std::bool_constant<a>, std::bool_constant<b>): the (non-temporal loads, non-temporal stores)
// pair of the moves
template <typename F> void dispatch_bools(bool a, bool b, F &&f) {
  if (a && b) f(std::true_type{}, std::true_type{});
  else if (a) f(std::true_type{}, std::false_type{});
  else if (b) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

// f(std::bool_constant<unpack>, Int<U>, std::bool_constant<NT>) of a pack / unpack: U items in
// flight per lane from BoxTuning::unroll, NT from nt_pack / nt_unpack
template <typename F> void dispatch_copy(bool unpack, F &&f) {
  const BoxTuning &t = box_tuning();
  dispatch_bools(unpack, unpack ? t.nt_unpack : t.nt_pack, [&](auto un, auto nt) {
    if (t.unroll >= 8) f(un, Int<8>{}, nt);
    else if (t.unroll < 4) f(un, Int<1>{}, nt); // one item in flight, `unroll` items per lane
    else f(un, Int<4>{}, nt);
  });
}

// A prefix table under construction: block_start[0 .. n] with block_start[0] = 0 (a zero-
// initialized batch) and block_start[n] the workgroups of the launch so far. Adds an entry served
// by `blocks` workgroups and returns its index.
inline int append_blocks(uint32_t *block_start, int32_t &n, uint32_t blocks) {
  block_start[n + 1] = block_start[n] + blocks;
  return n++;
}
inline void append(DevBatch &b, const DevDesc &d, uint32_t blocks) {
  b.d[append_blocks(b.block_start, b.n, blocks)] = d;
}
inline uint32_t total_blocks(const DevBatch &b) { return b.block_start[b.n]; }

// ---- builders of DevDesc / DevBatch (batch_device.hpp), shared by halo_kernels.hip and
// roof_kernels.hip; blocks_for reads the process-wide BoxTuning

// the box of rows of `len` elements at `off` of `buf`, with the row counts and strides of `m`
// (a MoveDesc or a LineBox)
template <typename D> BoxDesc box_of(const D &m, double *buf, int64_t off, int32_t len) {
  BoxDesc b;
  b.buf = buf;
  b.grid_off = off;
  b.len = len;
  b.s1 = m.s1;
  b.s2 = m.s2;
  b.s3 = m.s3;
  b.n1 = m.n1;
  b.n2 = m.n2;
  b.n3 = m.n3;
  return b;
}

// `lvec` items per row of kind `kind`, over the rows of `b`
inline void set_rows(DevDesc &d, RowKind kind, uint32_t lvec, const BoxDesc &b) {
  const uint64_t items = uint64_t(lvec) * b.n1 * b.n2 * b.n3;
  if (items >= (uint64_t(1) << 31)) throw std::runtime_error("box too large for 32-bit indexing");
  d.kind = kind;
  d.lvec = lvec;
  d.items = uint32_t(items);
  d.dl = FastDiv(std::max<uint32_t>(lvec, 1));
}

inline DevDesc make_dev(const BoxDesc &b) {
  DevDesc d{};
  d.buf = b.buf;
  d.grid_off = b.grid_off;
  d.s1 = b.s1;
  d.s2 = b.s2;
  d.s3 = b.s3;
  const bool even = (b.len % 2 == 0) && (b.grid_off % 2 == 0) && (b.s1 % 2 == 0) &&
                    (b.s2 % 2 == 0) && (b.s3 % 2 == 0) &&
                    (reinterpret_cast<uintptr_t>(b.buf) % 16 == 0);
  d.n1 = uint32_t(b.n1);
  d.n2 = uint32_t(b.n2);
  set_rows(d, even ? RowKind::Vec16 : RowKind::Vec8, uint32_t(b.len / (even ? 2 : 1)), b);
  d.d1 = FastDiv(std::max<uint32_t>(d.n1, 1));
  d.d2 = FastDiv(std::max<uint32_t>(d.n2, 1));
  return d;
}

// `cap`: blocks per box at most (0: BoxTuning::max_blocks); `unroll`: items per lane (0:
// BoxTuning::unroll)
inline uint32_t blocks_for(const DevDesc &d, int cap = 0, int unroll = 0) {
  const BoxTuning &t = box_tuning();
  const uint64_t per = uint64_t(kThreads) * uint64_t(unroll > 0 ? unroll : t.unroll);
  uint64_t b = (uint64_t(d.items) + per - 1) / per;
  const uint64_t m = uint64_t(std::max(1, cap > 0 ? cap : t.max_blocks));
  return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(b, m)));
}

} // namespace
} // namespace kern
} // namespace tz
