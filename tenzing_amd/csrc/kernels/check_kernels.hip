// Grid initialization and verification kernels of the halo workloads (gfx950): the field a run
// starts from (halo_init), the check of a completed exchange (halo_check) and of the 7-point
// stencil of that field (stencil_check). Test support, never on the timed path.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"

#include <cstdint>

namespace tz {
namespace kern {

namespace {

__device__ __forceinline__ int64_t wrapi(int64_t a, int64_t n) {
  a %= n;
  return a < 0 ? a + n : a;
}

__device__ __forceinline__ double halo_value(int q, int64_t gx, int64_t gy, int64_t gz, int gen) {
  constexpr int64_t G = 65536;
  // exact in a double for nq <= 8 (below 2^53 with the generation in bits 51-52)
  return double(((int64_t(q) * G + gz) * G + gy) * G + gx + (int64_t(gen & 3) << 51));
}

// classify logical element (x,y,z,q); returns expected value after a complete exchange and
// writes the storage index
__device__ __forceinline__ double halo_expect(const HaloGeom &g, int64_t lin, int64_t &idx,
                                              bool afterExchange) {
  const int64_t X = g.nx + 2 * g.g, Y = g.ny + 2 * g.g, Z = g.nz + 2 * g.g;
  const int64_t x = lin % X;
  int64_t r = lin / X;
  const int64_t y = r % Y;
  r /= Y;
  const int64_t z = r % Z;
  const int q = int(r / Z);
  if (g.order == 0) idx = q * g.sq + z * g.sz + y * g.sy + x + g.xoff;
  else idx = q + int64_t(g.nq) * (x + g.xoff) + y * g.sy + z * g.sz;
  const int gx = (x < g.g || x >= g.nx + g.g), gy = (y < g.g || y >= g.ny + g.g),
            gz = (z < g.g || z >= g.nz + g.g);
  const int k = gx + gy + gz;
  if (k > 0) {
    const bool filled = afterExchange && (g.neighbors == 26 || k == 1);
    if (!filled) return -1.0;
  }
  const int64_t GX = int64_t(g.nx) * g.px, GY = int64_t(g.ny) * g.py, GZ = int64_t(g.nz) * g.pz;
  return halo_value(q, wrapi(int64_t(g.cx) * g.nx + x - g.g, GX),
                    wrapi(int64_t(g.cy) * g.ny + y - g.g, GY),
                    wrapi(int64_t(g.cz) * g.nz + z - g.g, GZ), g.gen);
}

__global__ __launch_bounds__(kThreads) void halo_init_k(double *__restrict__ grid, HaloGeom g) {
  const int64_t total = int64_t(g.nx + 2 * g.g) * (g.ny + 2 * g.g) * (g.nz + 2 * g.g) * g.nq;
  for (int64_t lin = int64_t(blockIdx.x) * kThreads + threadIdx.x; lin < total;
       lin += int64_t(gridDim.x) * kThreads) {
    int64_t idx;
    const double v = halo_expect(g, lin, idx, false);
    grid[idx] = v;
  }
}

__global__ __launch_bounds__(kThreads) void halo_check_k(const double *__restrict__ grid, HaloGeom g,
                                                         unsigned long long *count) {
  const int64_t total = int64_t(g.nx + 2 * g.g) * (g.ny + 2 * g.g) * (g.nz + 2 * g.g) * g.nq;
  unsigned long long bad = 0;
  for (int64_t lin = int64_t(blockIdx.x) * kThreads + threadIdx.x; lin < total;
       lin += int64_t(gridDim.x) * kThreads) {
    int64_t idx;
    const double v = halo_expect(g, lin, idx, true);
    bad += grid[idx] != v;
  }
  // wave64 reduction, one atomic per wave
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}

// stencil mode: out must hold c0 * v + c1 * (6 face neighbours of v) of the initialized field v
// (global coordinates, periodic), for every interior cell; counts the cells that do not.
// Tolerance: |out - want| <= 2^-49 * want. Every term of the stencil is non-negative (nothing
// cancels), so any evaluation order of its 7 terms (2 products, 5 sums, 1 product, 1 sum) is
// within about 5 * 2^-53 * want of the exact value; `want` here and `out` each carry that, and
// 16 * 2^-53 = 2^-49 bounds their difference (two honest orders in numpy differ by at most
// 2.5 * 2^-53 * want over 20^3 x 3 cells, generations 0-3). No absolute term: halo_value puts
// the generation in bits 51-52, so at generation 3 want reaches 7.3e15 and a relative 1e-12 let
// a stencil that read one y neighbour from the wrong row (off by c1 * 65536) pass. This bound
// sees a wrong y or z neighbour at every generation. A wrong x neighbour (off by c1 * 1) is
// below one ulp of `out` at generations 1-3 (ulp(2^51) = 0.5), so no tolerance can see it
// there; it is seen where want is small: generation 0, q = 0.
// Blind spot: the field is affine in (x, y, z) and c0 + 6 c1 = 1, so away from the periodic wrap
// the stencil of the field is the field, for ANY kernel that reads a symmetric pair of
// neighbours per axis (x twice instead of y, +-2 instead of +-1; and a ghost that the interior
// reads beside the exchange, a race, passes whenever it already held its final value). This
// check is the oracle for "every cell was computed after its ghosts arrived"; which neighbours
// the kernels read is checked on random data by tests/test_gpu_stencil_kernels.py.
__global__ __launch_bounds__(kThreads) void stencil_check_k(const double *__restrict__ out, HaloGeom g,
                                                            double c0, double c1,
                                                            unsigned long long *count) {
  const int64_t total = int64_t(g.nx) * g.ny * g.nz * g.nq;
  const int64_t GX = int64_t(g.nx) * g.px, GY = int64_t(g.ny) * g.py, GZ = int64_t(g.nz) * g.pz;
  unsigned long long bad = 0;
  for (int64_t lin = int64_t(blockIdx.x) * kThreads + threadIdx.x; lin < total;
       lin += int64_t(gridDim.x) * kThreads) {
    const int64_t x = lin % g.nx;
    int64_t r = lin / g.nx;
    const int64_t y = r % g.ny;
    r /= g.ny;
    const int64_t z = r % g.nz;
    const int q = int(r / g.nz);
    const int64_t X = x + g.g, Y = y + g.g, Z = z + g.g; // storage coordinates
    const int64_t idx = g.order == 0 ? q * g.sq + Z * g.sz + Y * g.sy + X + g.xoff
                                     : q + int64_t(g.nq) * (X + g.xoff) + Y * g.sy + Z * g.sz;
    const int64_t gx = int64_t(g.cx) * g.nx + x, gy = int64_t(g.cy) * g.ny + y,
                  gz = int64_t(g.cz) * g.nz + z;
    auto v = [&](int64_t dx, int64_t dy, int64_t dz) {
      return halo_value(q, wrapi(gx + dx, GX), wrapi(gy + dy, GY), wrapi(gz + dz, GZ), g.gen);
    };
    const double want = c0 * v(0, 0, 0) + c1 * (v(-1, 0, 0) + v(1, 0, 0) + v(0, -1, 0) +
                                                v(0, 1, 0) + v(0, 0, -1) + v(0, 0, 1));
    bad += !(fabs(out[idx] - want) <= 0x1p-49 * want); // (a NaN counts)
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}

} // namespace

void stencil_check(const double *out, const HaloGeom &g, unsigned long long *count, void *stream) {
  const StencilBox defaults;
  hipLaunchKernelGGL(stencil_check_k, dim3(4096), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     out, g, defaults.c0, defaults.c1, count);
  TZ_HIP_LAUNCH_CHECK();
}

void halo_init(double *grid, const HaloGeom &g, void *stream) {
  hipLaunchKernelGGL(halo_init_k, dim3(4096), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     grid, g);
  TZ_HIP_LAUNCH_CHECK();
}

void halo_check(const double *grid, const HaloGeom &g, unsigned long long *count, void *stream) {
  hipLaunchKernelGGL(halo_check_k, dim3(4096), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     grid, g, count);
  TZ_HIP_LAUNCH_CHECK();
}

} // namespace kern
} // namespace tz
