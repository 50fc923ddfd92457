// Device side of the batched launches: the box descriptor and its flat indexing, the prefix-table
// lookup that tells a workgroup which entry of a batch it serves, and the last-block publish of
// the signalling puts. Device code only: include from .hip translation units.
//
// Everything here sits in the unnamed namespace, as it did when each .hip file kept its own copy:
// a kernel's symbol carries its argument types, and these are kernel argument types.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"

#include <cstdint>

namespace tz {
namespace kern {
namespace {

constexpr int kThreads = 256;

struct FastDiv {
  uint32_t m = 0, s = 0;
  FastDiv() = default;
  explicit FastDiv(uint32_t div) {
    while ((uint64_t(1) << s) < div) ++s;
    m = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << s) - div)) / div + 1);
  }
  __device__ __forceinline__ uint32_t div(uint32_t n) const {
    const uint32_t t = __umulhi(n, m);
    return uint32_t((uint64_t(t) + n) >> s);
  }
};

// how the items of a box cover its rows
enum class RowKind : int32_t {
  Vec8 = 1,   // one element per item
  Vec16,      // two elements (16 B) per item
  Peeled,     // move only (peel_body): head element, then 16-B pairs
  PeeledTail, // ... and a last element alone
  Pair,       // move only (pair_body): a row's two runs of `run` elements each
  WideUnpack, // unpack only (unpack_wide_body): 16-B items over the row and its padding
};

// The kernels read a descriptor with scalar loads straight from the kernel arguments, so the
// order of its fields decides how those loads pair up. Every field the move reads keeps the
// offset it had when each FastDiv still carried its divisor; the fields of one row kind or of the
// roof alone sit in the three words that freed.
struct DevDesc {
  union {
    double *buf; // pack / unpack: the dense buffer
    double *dst; // move, roof: the destination array
  };
  const double *src;  // move, roof: source array (grid_off indexes it)
  int64_t delta;      // move, roof: destination offset - source offset
  int64_t grid_off, s1, s2, s3;
  uint32_t lvec, n1, n2, items;
  int32_t wide_len; // WideUnpack: buffer row length
  FastDiv dl;
  int32_t wide_lead; // WideUnpack: elements of padding before each grid row
  FastDiv d1;
  uint8_t run;  // Pair: elements per run (MoveDesc::len)
  uint8_t roof; // line_roof_k only: LineBox::mode
  FastDiv d2;
  RowKind kind;
};
static_assert(sizeof(DevDesc) == 112, "DevDesc grew: see the kernarg limits in halo_kernels.hip");

struct DevBatch {
  DevDesc d[kMaxBoxes];
  uint32_t block_start[kMaxBoxes + 1];
  int32_t n;
};

typedef double dbl2_t __attribute__((ext_vector_type(2)));
template <int VEC> struct Vec;
template <> struct Vec<1> { using T = double; };
template <> struct Vec<2> { using T = dbl2_t; };

template <bool NT, typename T> __device__ __forceinline__ T ld(const T *p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, typename T> __device__ __forceinline__ void st(T *p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

template <int VEC>
__device__ __forceinline__ int64_t grid_index(const DevDesc &d, uint32_t it) {
  const uint32_t row = d.dl.div(it);
  const uint32_t xv = it - row * d.lvec;
  const uint32_t r1 = d.d1.div(row);
  const uint32_t i1 = row - r1 * d.n1;
  const uint32_t i3 = d.d2.div(r1);
  const uint32_t i2 = r1 - i3 * d.n2;
  return d.grid_off + int64_t(i1) * d.s1 + int64_t(i2) * d.s2 + int64_t(i3) * d.s3 +
         int64_t(xv) * VEC;
}

// Which entry (box, segment, copy) of a batch a workgroup serves. Entry k of a prefix table is
// served by the workgroups [block_start[k], block_start[k + 1]) of kThreads threads each; the
// table comes from the kernel arguments, so the search is scalar loads, uniform in the wave.
struct BlockSlot {
  int entry;
  uint32_t nb;  // workgroups that serve the entry
  uint32_t blk; // which of them this one is
  uint32_t tid; // this thread among their threads: blk * kThreads + threadIdx.x
  uint32_t nth; // nb * kThreads
};

__device__ __forceinline__ BlockSlot find_block(const uint32_t *block_start, int n, uint32_t block) {
  int e = 0;
  while (e + 1 < n && block >= block_start[e + 1]) ++e;
  const uint32_t nb = block_start[e + 1] - block_start[e];
  const uint32_t blk = block - block_start[e];
  return {e, nb, blk, blk * kThreads + threadIdx.x, nb * kThreads};
}

// The last of an entry's `nb` workgroups publishes every workgroup's (peer) stores: all
// workgroups call this after their stores, and `publish` (one system-scope release signal) runs
// in thread 0 of the last one. `done`: the entry's zero-initialized, self-resetting counter.
template <typename Publish>
__device__ __forceinline__ void signal_last_block(unsigned int *done, uint32_t nb, Publish publish) {
  __threadfence_system(); // this thread's peer stores are visible system-wide ...
  __syncthreads();        // ... for every thread of the block before it is counted
  if (threadIdx.x == 0) {
    const unsigned int prev = atomicAdd(done, 1u);
    if (prev == nb - 1) { // last block of this entry: every block's stores are fenced
      *done = 0;          // ready for the next iteration (kernel boundary orders it)
      __threadfence_system();
      publish();
    }
  }
}

} // namespace
} // namespace kern
} // namespace tz
