// Mixed-precision iterative refinement around the f32 single-reduction CG (cg_kernels.hip), for
// gfx950: the three launches of one refinement step. The solution is kept in f64 (x64); a step
// adds the f32 correction x to it, evaluates the residual r64 = b - A x64 in f64 (A and b are f32
// data, exact in f64) and restarts the f32 recurrence on f32(r64) with x = 0, or finds the f64
// residual below the outer threshold and declares the solve refined. Not in the reference.
//
// The two rules of cg_kernels.hip hold here too: deterministic results (fixed element -> thread
// -> partial mapping that depends on n alone, fixed summation orders, no floating-point atomics)
// and no hand-off between workgroups inside a launch (a dot product is one partial per block, and
// the one-block decide kernel sums the slabs in the order of sum_partials_f64).
//
// Every launch begins with `if (*outer_done) return;`, the same value in every thread of the
// grid, as the stopping kernels read *done: a refined state is written by nothing. outer_done is
// only ever set by the decide kernel, the last launch of a step.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"

#include <initializer_list>
#include <stdexcept>
#include <string>

namespace tz {
namespace kern {

namespace {

constexpr int kRefineThreads = 1024; // the residual pass: the grid of csr_spmv_dot2
constexpr int kRefineW = 4;          // lanes per row
constexpr int kRefineK = 4;          // entries in flight per lane

// block_sum and sum_partials of cg_kernels.hip (the same order, hence the same bits): xor
// butterfly inside each wave64, then the waves' sums in wave order
template <int NW> __device__ __forceinline__ double block_sum(double v, double *sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += sh[w];
  __syncthreads(); // sh may be reused
  return s;
}

template <int NW> __device__ __forceinline__ double sum_partials(const double *partials, int np, double *sh) {
  const double v = int(threadIdx.x) < np ? partials[threadIdx.x] : 0.0;
  return block_sum<NW>(v, sh);
}

// x64 += x (one f64 add per element: IEEE, so numpy's bits), then x = s = 0
__global__ __launch_bounds__(kThreads) void cg_refine_accumulate_k(int64_t n, float *__restrict__ x,
                                                                   float *__restrict__ s,
                                                                   double *__restrict__ x64,
                                                                   const int *__restrict__ outerDone) {
  if (*outerDone) return; // uniform over the grid
  const int64_t stride = int64_t(gridDim.x) * kThreads;
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    x64[i] += double(x[i]);
    x[i] = 0.f;
    s[i] = 0.f;
  }
}

// The row's sum of double(a_ij) * x64[col_j] in every one of its W lanes: the lane walks entries
// lane, lane + W, .. in order with one f64 chain (csr_spmv_ilp_sum's mapping, K loads in flight),
// then the W chains meet in an xor butterfly. A masked entry multiplies 0 by 0.
template <int W, int K>
__device__ __forceinline__ double csr_row_dot_f64(int row, int lane, const int32_t *__restrict__ rowPtr,
                                                  const int32_t *__restrict__ colInd,
                                                  const float *__restrict__ val,
                                                  const double *__restrict__ x) {
  const int b = rowPtr[row], e = rowPtr[row + 1];
  double sum = 0.0;
  for (int j0 = b + lane; j0 < e; j0 += W * K) {
    int c[K];
    double v[K], xv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = j0 + k * W;
      c[k] = j < e ? colInd[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = j0 + k * W;
      v[k] = j < e ? double(val[j]) : 0.0;
      xv[k] = c[k] >= 0 ? x[c[k]] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sum = fma(v[k], xv[k], sum);
  }
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, W);
  return sum;
}

// pcg_apply of cg_kernels.hip: u = f32(dinv * r), a rounded product of its own (this file too is
// built with -ffp-contract=fast; the empty asm keeps the product from any contraction)
__device__ __forceinline__ float pcg_apply(float dinv, float r) {
  float u = dinv * r;
  asm volatile("" : "+v"(u));
  return u;
}

// r64 = b - A x64 in f64, the restart of the f32 recurrence from it (r = p = f32(r64); PC: u =
// f32(dinv * r) and p = u, as reset() has it), and the block's partials of r64 . r64 and of r . r
// (the new f32 vector). Grid and row mapping of csr_spmv_dot2 with W lanes per row.
template <int W, int K, bool PC>
__global__ __launch_bounds__(kRefineThreads) void cg_refine_residual_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ b, const double *__restrict__ x64,
    const float *__restrict__ dinv, double *__restrict__ r64, float *__restrict__ r, float *__restrict__ p,
    float *__restrict__ u, double *__restrict__ partials64, double *__restrict__ partials32,
    const int *__restrict__ outerDone) {
  __shared__ double sh[kRefineThreads / 64];
  if (*outerDone) return; // uniform over the grid
  const int lane = threadIdx.x & (W - 1);
  const int rowsPerPass = int(gridDim.x) * (kRefineThreads / W);
  double acc64 = 0.0, acc32 = 0.0;
  // whole W-lane groups leave the loop together (W divides 64)
  for (int row = (blockIdx.x * kRefineThreads + threadIdx.x) / W; row < nRows; row += rowsPerPass) {
    const double sum = csr_row_dot_f64<W, K>(row, lane, rowPtr, colInd, val, x64);
    if (lane == 0) {
      const double rd = double(b[row]) - sum;
      const float rf = float(rd);
      r64[row] = rd;
      r[row] = rf;
      if constexpr (PC) {
        const float uf = pcg_apply(dinv[row], rf);
        u[row] = uf;
        p[row] = uf;
      } else {
        p[row] = rf;
      }
      acc64 += rd * rd;
      acc32 += double(rf) * double(rf);
    }
  }
  const double s64 = block_sum<kRefineThreads / 64>(acc64, sh);
  const double s32 = block_sum<kRefineThreads / 64>(acc32, sh);
  if (threadIdx.x == 0) {
    partials64[blockIdx.x] = s64;
    partials32[blockIdx.x] = s32;
  }
}

// One block. rr64 = the sum of the first slab, rr32 of the second. rr64 <= *outerThresh (a NaN
// compares false): the solve is refined, and nothing of the inner solve is touched. Otherwise the
// f32 recurrence restarts: its threshold becomes tol2 * rr32, its flag 0 and its five scalars 0,
// as reset() leaves them (the next iteration then has beta = 0; the SpMV's block 0 copies the
// published pair over the previous pair, so all five go). iters keeps counting over the whole solve.
__global__ __launch_bounds__(kThreads) void cg_refine_decide_k(
    const double *__restrict__ partials64, const double *__restrict__ partials32, int np, double tol2,
    double *__restrict__ thresh, int *__restrict__ done, double *__restrict__ gamma, double *__restrict__ alpha,
    double *__restrict__ beta, double *__restrict__ gammaPrev, double *__restrict__ alphaPrev,
    const double *__restrict__ outerThresh, int *__restrict__ outerDone, int64_t *__restrict__ outerSteps,
    double *__restrict__ rr64Out) {
  __shared__ double sh[kThreads / 64];
  if (*outerDone) return; // every thread reads it before the first barrier, thread 0 writes after the last
  const double rr64 = sum_partials<kThreads / 64>(partials64, np, sh);
  const double rr32 = sum_partials<kThreads / 64>(partials32, np, sh);
  if (threadIdx.x != 0) return;
  *rr64Out = rr64;
  if (rr64 <= *outerThresh) {
    *outerDone = 1;
    return;
  }
  *thresh = tol2 * rr32;
  *done = 0;
  *gamma = 0.0;
  *alpha = 0.0;
  *beta = 0.0;
  *gammaPrev = 0.0;
  *alphaPrev = 0.0;
  *outerSteps += 1;
}

struct Span {
  const void *p;
  size_t bytes;
  bool written;
};

template <typename T> Span span(const T *p, size_t count, bool written) { return {p, count * sizeof(T), written}; }

// no pointer null, every one aligned to `align` bytes
void check_ptrs(const std::string &pre, size_t align, const char *kind, std::initializer_list<const void *> ps) {
  for (const void *p : ps) {
    if (!p) throw std::runtime_error(pre + "null pointer");
    if (reinterpret_cast<uintptr_t>(p) % align)
      throw std::runtime_error(pre + kind + " must be " + std::to_string(align) + "-byte aligned");
  }
}

// nothing a launch writes may share a byte with anything else it touches (two it only reads may)
void check_disjoint(const std::string &pre, const char *what, std::initializer_list<Span> all) {
  for (const Span *a = all.begin(); a != all.end(); ++a)
    for (const Span *b = a + 1; b != all.end(); ++b) {
      const auto a0 = reinterpret_cast<uintptr_t>(a->p), b0 = reinterpret_cast<uintptr_t>(b->p);
      if ((a->written || b->written) && a->bytes && b->bytes && a0 < b0 + b->bytes && b0 < a0 + a->bytes)
        throw std::runtime_error(pre + what);
    }
}

} // namespace

int cg_refine_partial_count(int nRows) { return spmv_dot_partial_count(nRows, kRefineW); }

void cg_refine_accumulate(int64_t n, float *x, float *s, double *x64, const int *outerDone, void *stream) {
  const std::string pre = "cg_refine_accumulate: ";
  if (n <= 0) throw std::runtime_error(pre + "n must be positive");
  check_ptrs(pre, 4, "f32 vectors and outer_done", {x, s, outerDone});
  check_ptrs(pre, 8, "f64 vectors", {x64});
  const size_t m = size_t(n);
  check_disjoint(pre, "vectors and outer_done must not overlap",
                 {span(x, m, true), span(s, m, true), span(x64, m, true), span(outerDone, 1, false)});
  hipLaunchKernelGGL(cg_refine_accumulate_k, dim3(unsigned(dot_partial_count(n))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, x, s, x64, outerDone);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_refine_residual(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *b,
                        const double *x64, const float *dinv, double *r64, float *r, float *p, float *u,
                        double *partials64, double *partials32, const int *outerDone, void *stream) {
  const std::string pre = "cg_refine_residual: ";
  if (nRows <= 0) throw std::runtime_error(pre + "nRows must be positive");
  if ((dinv == nullptr) != (u == nullptr))
    throw std::runtime_error(pre + "null pointer (dinv and u come together or not at all)");
  check_ptrs(pre, 4, "f32 vectors, the matrix and outer_done", {rowPtr, colInd, val, b, r, p, outerDone});
  if (dinv) check_ptrs(pre, 4, "f32 vectors, the matrix and outer_done", {dinv, u});
  check_ptrs(pre, 8, "f64 vectors and slabs", {x64, r64, partials64, partials32});
  const size_t n = size_t(nRows), c = size_t(cg_refine_partial_count(nRows));
  check_disjoint(pre, "vectors, slabs and outer_done must not overlap",
                 {span(b, n, false), span(x64, n, false), span(dinv, dinv ? n : 0, false), span(r64, n, true),
                  span(r, n, true), span(p, n, true), span(u, u ? n : 0, true), span(partials64, c, true),
                  span(partials32, c, true), span(outerDone, 1, false)});
  const dim3 g{unsigned(c)}, blk(kRefineThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dinv)
    hipLaunchKernelGGL((cg_refine_residual_k<kRefineW, kRefineK, true>), g, blk, 0, s, nRows, rowPtr, colInd, val, b,
                       x64, dinv, r64, r, p, u, partials64, partials32, outerDone);
  else
    hipLaunchKernelGGL((cg_refine_residual_k<kRefineW, kRefineK, false>), g, blk, 0, s, nRows, rowPtr, colInd, val,
                       b, x64, dinv, r64, r, p, u, partials64, partials32, outerDone);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_refine_decide(const double *partials64, const double *partials32, int np, double tol2, double *thresh,
                      int *done, double *gamma, double *alpha, double *beta, double *gammaPrev, double *alphaPrev,
                      const RefineOuter &o, void *stream) {
  const std::string pre = "cg_refine_decide: ";
  if (np < 1 || np > kCgMaxPartials)
    throw std::runtime_error(pre + "1.." + std::to_string(kCgMaxPartials) + " partials");
  if (!(tol2 > 0)) throw std::runtime_error(pre + "tol2 must be positive");
  check_ptrs(pre, 8, "slabs and f64 / i64 scalars",
             {partials64, partials32, thresh, gamma, alpha, beta, gammaPrev, alphaPrev, o.thresh, o.steps, o.rr64});
  check_ptrs(pre, 4, "flags", {done, o.done});
  const size_t c = size_t(np);
  // the outer state shares no byte with the inner solve's scalars and stop state, nor anything
  // written with anything else
  check_disjoint(pre, "slabs, the inner scalars and stop state and the outer state must not overlap",
                 {span(partials64, c, false), span(partials32, c, false), span(thresh, 1, true), span(done, 1, true),
                  span(gamma, 1, true), span(alpha, 1, true), span(beta, 1, true), span(gammaPrev, 1, true),
                  span(alphaPrev, 1, true), span(o.thresh, 1, true), span(o.done, 1, true), span(o.steps, 1, true),
                  span(o.rr64, 1, true)});
  hipLaunchKernelGGL(cg_refine_decide_k, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), partials64,
                     partials32, np, tol2, thresh, done, gamma, alpha, beta, gammaPrev, alphaPrev, o.thresh, o.done,
                     o.steps, o.rr64);
  TZ_HIP_LAUNCH_CHECK();
}

} // namespace kern
} // namespace tz
