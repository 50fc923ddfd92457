// Shape-matched roof probe of the direct moves (gfx950): touches exactly the 128-B lines a batch
// of moves touches, at the best access shape (line_roof), and the host-side geometry that turns a
// batch of moves into those line boxes (line_boxes). A measurement tool, never on the timed path
// of an exchange.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"

#include <algorithm>
#include <stdexcept>
#include <vector>

namespace tz {
namespace kern {

namespace {

// shape-matched roof (line_roof): whole lines, 16-B accesses; d.roof carries the mode. U items
// per lane in flight (all loads issued before any is used); NTS: non-temporal stores (as the
// move's ghost stores)
template <int U, bool NTS>
__global__ __launch_bounds__(kThreads) void line_roof_k(DevBatch b, double zero, double *sink) {
  const BlockSlot s = find_block(b.block_start, b.n, blockIdx.x);
  const DevDesc &d = b.d[s.entry];
  const uint32_t nth = s.nth;
  // as a move: item g is read at src + g and written at dst + delta + g (modes 0-2: in place)
  const double *src = d.src;
  double *dst = d.dst + d.delta;
  const dbl2_t z = {zero, zero};
  dbl2_t acc = z;
  uint32_t it = s.tid;
  for (; it + (U - 1) * nth < d.items; it += U * nth) {
    int64_t g[U];
#pragma unroll
    for (int k = 0; k < U; ++k) g[k] = grid_index<2>(d, it + k * nth);
    if (d.roof == 1) {
#pragma unroll
      for (int k = 0; k < U; ++k) st<NTS>(reinterpret_cast<dbl2_t *>(dst + g[k]), z);
    } else if (d.roof == 3) { // line-to-line copy
      dbl2_t v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = *reinterpret_cast<const dbl2_t *>(src + g[k]);
#pragma unroll
      for (int k = 0; k < U; ++k) st<NTS>(reinterpret_cast<dbl2_t *>(dst + g[k]), v[k]);
    } else {
      dbl2_t v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = *reinterpret_cast<const dbl2_t *>(src + g[k]);
      if (d.roof == 0) {
#pragma unroll
        for (int k = 0; k < U; ++k) acc += v[k];
      } else {
#pragma unroll
        for (int k = 0; k < U; ++k) st<NTS>(reinterpret_cast<dbl2_t *>(dst + g[k]), v[k] + z); // read, written back by the same lane
      }
    }
  }
  for (; it < d.items; it += nth) {
    const int64_t g = grid_index<2>(d, it);
    const dbl2_t *from = reinterpret_cast<const dbl2_t *>(src + g);
    dbl2_t *to = reinterpret_cast<dbl2_t *>(dst + g);
    if (d.roof == 0) acc += *from;
    else if (d.roof == 1) st<NTS>(to, z);
    else if (d.roof == 3) st<NTS>(to, *from);
    else st<NTS>(to, *from + z);
  }
  if (acc.x + acc.y == 1.0e300) sink[0] = acc.x; // keeps the loads; never taken on a probe grid
}

} // namespace

std::vector<LineBox> line_boxes(const MoveDesc *moves, int n, bool copies) {
  std::vector<LineBox> reads, writes, moved;
  auto add = [](std::vector<LineBox> &v, const MoveDesc &m, double *base, int64_t off) {
    if (m.s1 % 16 || m.s2 % 16 || m.s3 % 16)
      throw std::runtime_error("line_boxes: row strides must be whole 128-B lines");
    LineBox b;
    b.base = base;
    b.off = off / 16 * 16;
    b.lines = int32_t((off + m.len - 1) / 16 - off / 16 + 1);
    b.s1 = m.s1;
    b.s2 = m.s2;
    b.s3 = m.s3;
    b.n1 = m.n1;
    b.n2 = m.n2;
    b.n3 = m.n3;
    v.push_back(b);
  };
  for (int i = 0; i < n; ++i) {
    const MoveDesc &m = moves[i];
    double *src = const_cast<double *>(m.src);
    if (m.pair) {
      const int64_t delta = m.dst_off - m.src_off;
      add(reads, m, src, m.src_off);
      add(reads, m, src, m.src_off + m.len + delta);
      add(writes, m, m.dst, m.dst_off);
      add(writes, m, m.dst, m.src_off + m.len);
    } else {
      add(reads, m, src, m.src_off);
      add(writes, m, m.dst, m.dst_off);
      const LineBox &r = reads.back(), &w = writes.back();
      if (copies && r.lines == w.lines && m.src_off % 16 == m.dst_off % 16) {
        LineBox c = r;
        c.mode = 3;
        c.dst_base = w.base;
        c.dst_off = w.off;
        moved.push_back(c);
        reads.pop_back();
        writes.pop_back();
      }
    }
  }
  auto same = [](const LineBox &a, const LineBox &b) {
    return a.base == b.base && a.off == b.off && a.lines == b.lines && a.s1 == b.s1 && a.s2 == b.s2 &&
           a.s3 == b.s3 && a.n1 == b.n1 && a.n2 == b.n2 && a.n3 == b.n3;
  };
  std::vector<LineBox> out;
  std::vector<bool> merged(writes.size(), false);
  for (LineBox r : reads) {
    r.mode = 0;
    for (size_t k = 0; k < writes.size(); ++k)
      if (!merged[k] && same(r, writes[k])) {
        r.mode = 2;
        merged[k] = true;
        break;
      }
    out.push_back(r);
  }
  for (size_t k = 0; k < writes.size(); ++k)
    if (!merged[k]) {
      LineBox w = writes[k];
      w.mode = 1;
      out.push_back(w);
    }
  out.insert(out.begin(), moved.begin(), moved.end());
  return out;
}

void line_roof(const LineBox *boxes, int n, void *stream, int variant) {
  if (variant < 0 || variant >= kLineRoofVariants) throw std::runtime_error("line_roof: bad variant");
  static double *sink = nullptr;
  if (!sink && hipMalloc(&sink, 64) != hipSuccess) throw std::runtime_error("line_roof: hipMalloc");
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int k0 = 0; k0 < n; k0 += kMaxBoxes) {
    DevBatch b{};
    for (int i = k0; i < std::min(n, k0 + kMaxBoxes); ++i) {
      const LineBox &l = boxes[i];
      DevDesc d = make_dev(box_of(l, l.base, l.off, l.lines * 16));
      if (d.items == 0) continue;
      if (d.kind != RowKind::Vec16) throw std::runtime_error("line_roof: boxes must be whole 128-B lines");
      d.src = l.base;
      d.roof = uint8_t(l.mode);
      if (l.mode == 3) { // source: base; target: dst_base + dst_off, same geometry
        if (!l.dst_base) throw std::runtime_error("line_roof: copy box without a target");
        d.dst = l.dst_base;
        d.delta = l.dst_off - l.off;
      }
      append(b, d, blocks_for(d, 0, std::max(1, box_tuning().move_items)));
    }
    if (b.n == 0) continue;
    const dim3 g(total_blocks(b)), t(kThreads);
    switch (variant) { // (items in flight per lane, non-temporal stores)
    case 0: hipLaunchKernelGGL((line_roof_k<1, true>), g, t, 0, s, b, 0.0, sink); break;
    case 1: hipLaunchKernelGGL((line_roof_k<4, true>), g, t, 0, s, b, 0.0, sink); break;
    case 2: hipLaunchKernelGGL((line_roof_k<1, false>), g, t, 0, s, b, 0.0, sink); break;
    default: hipLaunchKernelGGL((line_roof_k<4, false>), g, t, 0, s, b, 0.0, sink); break;
    }
    TZ_HIP_LAUNCH_CHECK();
  }
}

} // namespace kern
} // namespace tz
