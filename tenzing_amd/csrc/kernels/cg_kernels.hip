// Conjugate-gradient kernels for gfx950: dot products, vector updates whose coefficient lives in
// device memory, the fused forms (SpMV + dot, update + dot) and the single-reduction form's two
// kernels (SpMV + two dots, one update of p, s, x and r), those two also for 2, 4 or 8 interleaved
// right-hand sides, and all four again with a convergence test decided on the device (*_stop):
// eight entry points over four bodies, a stopping one being its test in front of its parent's
// body; and the Jacobi-preconditioned pair of the single right-hand side (pcg_*), which shares
// those bodies' arithmetic. Not in the reference.
//
// Vectors are f32; dot products accumulate in f64 (the product of two f32 values is exact in
// f64); every scalar (rr, alpha, beta) is an f64 in device memory, so no launch argument carries
// a value computed on the GPU and a whole iteration captures into a hipGraph.
//
// Two rules hold for every kernel here:
//  1. Deterministic results. The element -> thread -> partial mapping depends only on n (never on
//     pointer alignment), every sum has a fixed order, and there are no floating-point atomics.
//  2. No hand-off between workgroups inside a launch (no tickets, no last-block reduce, no
//     spinning). A reduction ends at a launch boundary: a kernel writes one partial per block,
//     and the kernel that needs the scalar sums the partials itself in its prologue
//     (sum_partials: every block in the same order, hence the same bits in every block).
//
// Layout of a vector pass (dot_partials_f32 and every update): the vector is cut into quads of 4
// elements; quad k belongs to thread k % T of the pass k / T (T = blocks * 256), and the n % 4
// tail elements to threads 0.. of block 0. Aligned pointers move a quad with one 16-B access,
// others with four 4-B accesses; the arithmetic is the same.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "spmv_device.hpp"

#include <algorithm>
#include <initializer_list>
#include <stdexcept>
#include <string>

namespace tz {
namespace kern {

namespace {

// the vector and scalar kernels run kThreads (batch_device.hpp) threads per block
constexpr int kSpmvThreads = 1024; // csr_spmv_dot: at most 256 blocks must cover the chip

// Sum of one value per thread, returned to every thread: xor butterfly inside each wave64 (all
// lanes end with the same bits: a + b == b + a), then the waves' sums in wave order.
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

// The launch-boundary reduce: the sum of np <= 256 partials, the same bits in every thread of
// every block that calls it (thread t holds partial t, or +0.0 from np on)
template <int NW> __device__ __forceinline__ double sum_partials(const double *partials, int np, double *sh) {
  const double v = int(threadIdx.x) < np ? partials[threadIdx.x] : 0.0;
  return block_sum<NW>(v, sh);
}

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ float4 load_quad(const float *p, int64_t k, bool al) {
  if (al) return reinterpret_cast<const float4 *>(p)[k];
  const float *s = p + 4 * k;
  return make_float4(s[0], s[1], s[2], s[3]);
}

__device__ __forceinline__ void store_quad(float *p, int64_t k, bool al, float4 v) {
  if (al) {
    reinterpret_cast<float4 *>(p)[k] = v;
    return;
  }
  float *d = p + 4 * k;
  d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
}

__device__ __forceinline__ double dot_quad(double acc, float4 a, float4 b) {
  acc += double(a.x) * double(b.x);
  acc += double(a.y) * double(b.y);
  acc += double(a.z) * double(b.z);
  acc += double(a.w) * double(b.w);
  return acc;
}

// v = old in the lanes whose `keep` is set
__device__ __forceinline__ void keep_quad(float4 &v, float4 old, const bool (&keep)[4]) {
  v.x = keep[0] ? old.x : v.x, v.y = keep[1] ? old.y : v.y, v.z = keep[2] ? old.z : v.z, v.w = keep[3] ? old.w : v.w;
}

__global__ __launch_bounds__(kThreads) void dot_partials_k(int64_t n, const float *u, const float *v,
                                                           double *__restrict__ partials) {
  __shared__ double sh[kThreads / 64];
  const bool au = aligned16(u), av = aligned16(v);
  const int64_t nq = n / 4, stride = int64_t(gridDim.x) * kThreads;
  double acc = 0.0;
  for (int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x; k < nq; k += stride)
    acc = dot_quad(acc, load_quad(u, k, au), load_quad(v, k, av));
  const int64_t t = nq * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) acc += double(u[t]) * double(v[t]);
  const double s = block_sum<kThreads / 64>(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void sum_partials_k(const double *__restrict__ partials, int np,
                                                           double *__restrict__ out) {
  __shared__ double sh[kThreads / 64];
  const double s = sum_partials<kThreads / 64>(partials, np, sh);
  if (threadIdx.x == 0) *out = s;
}

__device__ __forceinline__ double guarded_div(double num, double den) { return den != 0.0 ? num / den : 0.0; }

__global__ __launch_bounds__(kThreads) void cg_alpha_k(const double *__restrict__ partialsPq, int np,
                                                       const double *__restrict__ rr,
                                                       double *__restrict__ alpha) {
  __shared__ double sh[kThreads / 64];
  const double pq = sum_partials<kThreads / 64>(partialsPq, np, sh);
  if (threadIdx.x == 0) *alpha = guarded_div(*rr, pq);
}

__global__ __launch_bounds__(kThreads) void cg_beta_k(const double *__restrict__ partialsRr, int np,
                                                      double *__restrict__ rr, double *__restrict__ beta) {
  __shared__ double sh[kThreads / 64];
  const double rrNew = sum_partials<kThreads / 64>(partialsRr, np, sh);
  if (threadIdx.x == 0) {
    *beta = guarded_div(rrNew, *rr);
    *rr = rrNew;
  }
}

// y = fmaf(a, x, y) over this thread's elements; with `sq`, the sum of the squares of what it
// stored (the partial of y . y, in dot_partials_k's order)
template <bool SQ>
__device__ __forceinline__ double axpy_pass(int64_t n, float a, const float *x, float *y) {
  const bool ax = aligned16(x), ay = aligned16(y);
  const int64_t nq = n / 4, stride = int64_t(gridDim.x) * kThreads;
  double acc = 0.0;
  for (int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x; k < nq; k += stride) {
    const float4 xv = load_quad(x, k, ax);
    float4 yv = load_quad(y, k, ay);
    yv.x = fmaf(a, xv.x, yv.x);
    yv.y = fmaf(a, xv.y, yv.y);
    yv.z = fmaf(a, xv.z, yv.z);
    yv.w = fmaf(a, xv.w, yv.w);
    store_quad(y, k, ay, yv);
    if (SQ) acc = dot_quad(acc, yv, yv);
  }
  const int64_t t = nq * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float yt = fmaf(a, x[t], y[t]);
    y[t] = yt;
    if (SQ) acc += double(yt) * double(yt);
  }
  return acc;
}

// y = fmaf(s, y, x)
__device__ __forceinline__ void xpay_pass(int64_t n, float s, const float *x, float *y) {
  const bool ax = aligned16(x), ay = aligned16(y);
  const int64_t nq = n / 4, stride = int64_t(gridDim.x) * kThreads;
  for (int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x; k < nq; k += stride) {
    const float4 xv = load_quad(x, k, ax);
    float4 yv = load_quad(y, k, ay);
    yv.x = fmaf(s, yv.x, xv.x);
    yv.y = fmaf(s, yv.y, xv.y);
    yv.z = fmaf(s, yv.z, xv.z);
    yv.w = fmaf(s, yv.w, xv.w);
    store_quad(y, k, ay, yv);
  }
  const int64_t t = nq * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) y[t] = fmaf(s, y[t], x[t]);
}

__global__ __launch_bounds__(kThreads) void axpy_dev_k(int64_t n, const double *__restrict__ s, float sign,
                                                       const float *x, float *y) {
  axpy_pass<false>(n, sign * float(*s), x, y);
}

__global__ __launch_bounds__(kThreads) void xpay_dev_k(int64_t n, const double *__restrict__ s,
                                                       const float *x, float *y) {
  xpay_pass(n, float(*s), x, y);
}

// x += alpha p, alpha = rr / (sum of the pq partials) formed in the prologue
__global__ __launch_bounds__(kThreads) void cg_fused_x_k(int64_t n, const double *__restrict__ partialsPq,
                                                         int np, const double *__restrict__ rr,
                                                         const float *p, float *x) {
  __shared__ double sh[kThreads / 64];
  const double alpha = guarded_div(*rr, sum_partials<kThreads / 64>(partialsPq, np, sh));
  axpy_pass<false>(n, float(alpha), p, x);
}

// r -= alpha q (the same prologue) and the partials of the new r . r
__global__ __launch_bounds__(kThreads) void cg_fused_r_k(int64_t n, const double *__restrict__ partialsPq,
                                                         int np, const double *__restrict__ rr,
                                                         const float *q, float *r,
                                                         double *__restrict__ partialsRr) {
  __shared__ double sh[kThreads / 64];
  const double alpha = guarded_div(*rr, sum_partials<kThreads / 64>(partialsPq, np, sh));
  const double acc = axpy_pass<true>(n, -float(alpha), q, r);
  const double s = block_sum<kThreads / 64>(acc, sh);
  if (threadIdx.x == 0) partialsRr[blockIdx.x] = s;
}

// p = r + beta p, beta = (sum of the new rr partials) / rr formed in the prologue
__global__ __launch_bounds__(kThreads) void cg_fused_p_k(int64_t n, const double *__restrict__ partialsRr,
                                                         int np, const double *__restrict__ rr,
                                                         const float *r, float *p) {
  __shared__ double sh[kThreads / 64];
  const double beta = guarded_div(sum_partials<kThreads / 64>(partialsRr, np, sh), *rr);
  xpay_pass(n, float(beta), r, p);
}

// q = A p with W lanes per row (dev::csr_spmv_ilp_sum, the arithmetic of csr_spmv's ILP kernel)
// in a grid-stride loop over the rows, and the block's partial of p . q. Block 0 also refreshes
// rr from the rr partials of the previous iteration's r update (partialsRr may be null).
template <int W, int K>
__global__ __launch_bounds__(kSpmvThreads) void csr_spmv_dot_k(int nRows, const int32_t *__restrict__ rowPtr,
                                                               const int32_t *__restrict__ colInd,
                                                               const float *__restrict__ val,
                                                               const float *__restrict__ p,
                                                               float *__restrict__ q,
                                                               double *__restrict__ partialsPq,
                                                               const double *__restrict__ partialsRr,
                                                               int npRr, double *__restrict__ rr) {
  __shared__ double sh[kSpmvThreads / 64];
  if (partialsRr && blockIdx.x == 0) { // uniform in the block
    const double s = sum_partials<kSpmvThreads / 64>(partialsRr, npRr, sh);
    if (threadIdx.x == 0) *rr = s;
  }
  const int lane = threadIdx.x & (W - 1);
  const int rowsPerPass = int(gridDim.x) * (kSpmvThreads / W);
  double acc = 0.0;
  // whole W-lane groups leave the loop together (W divides 64)
  for (int row = (blockIdx.x * kSpmvThreads + threadIdx.x) / W; row < nRows; row += rowsPerPass) {
    const float sum = dev::csr_spmv_ilp_sum<W, K>(row, lane, rowPtr, colInd, val, p);
    if (lane == 0) {
      q[row] = sum;
      acc += double(p[row]) * double(sum);
    }
  }
  const double s = block_sum<kSpmvThreads / 64>(acc, sh);
  if (threadIdx.x == 0) partialsPq[blockIdx.x] = s;
}

// ---- The single-reduction (Chronopoulos-Gear) recurrence: both dot products of an iteration
// come from the same vectors, gamma = r . r and delta = r . (A r), so both ride on the SpMV. Two
// launches per iteration, each for one right-hand side or for NR interleaved ones, and each of
// those four with or without a convergence test: eight entry points over four bodies. An entry
// point with the test (*_stop_k) is its test followed by the body its parent calls, so the two
// agree bit for bit by construction, not by copying.
//
// The test needs no hand-off inside a launch (rule 2). Every block of the update sums the same
// gamma slab in the same order, so gamma = r . r has the same bits in every block and `gamma <=
// *thresh` (thresh in device memory) sends the whole grid the same way: a stopped update writes no
// vector. Block 0 records the outcome in *done and the next launch reads it, as gammaOut and
// alphaOut travel. A set flag returns every block of the SpMV before it writes, so w, both slabs
// and the previous scalars keep what the stopped update saw; the next update forms the same gamma
// and stops again: a stopped iteration stays stopped under any number of replays. A NaN gamma
// compares false and never stops. tests/test_gpu_cg_tol_kernels.py holds each stopping kernel to
// its parent's bits all the same.

// w = A r as csr_spmv_dot_k computes q (same row body, same grid) and the block's partials of
// gamma and delta. Block 0 also moves the scalars the previous update published into the places
// the next update reads (gammaOut may be null): this launch lies between their writer and their
// next reader, and nothing in it reads either side.
//
// PC is the Jacobi-preconditioned form (u = dinv o r is a stored vector): w = A u, gamma = r . u,
// delta = u . w and a third slab, rho = r . r, which only the stopping test reads. Without PC, u
// and partialsRho are not read.
template <int W, int K, bool PC>
__device__ __forceinline__ void spmv_dot2_body(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, const float *__restrict__ u,
    float *__restrict__ w, double *__restrict__ partialsGamma, double *__restrict__ partialsDelta,
    double *__restrict__ partialsRho, const double *__restrict__ gammaOut, const double *__restrict__ alphaOut,
    double *__restrict__ gammaPrev, double *__restrict__ alphaPrev) {
  __shared__ double sh[kSpmvThreads / 64];
  if (gammaOut && blockIdx.x == 0 && threadIdx.x == 0) {
    *gammaPrev = *gammaOut;
    *alphaPrev = *alphaOut;
  }
  const int lane = threadIdx.x & (W - 1);
  const int rowsPerPass = int(gridDim.x) * (kSpmvThreads / W);
  double accG = 0.0, accD = 0.0, accR = 0.0;
  // whole W-lane groups leave the loop together (W divides 64)
  for (int row = (blockIdx.x * kSpmvThreads + threadIdx.x) / W; row < nRows; row += rowsPerPass) {
    const float sum = dev::csr_spmv_ilp_sum<W, K>(row, lane, rowPtr, colInd, val, PC ? u : r);
    if (lane == 0) {
      const double ri = double(r[row]);
      w[row] = sum;
      if constexpr (PC) {
        const double ui = double(u[row]);
        accG += ri * ui;
        accD += ui * double(sum);
        accR += ri * ri;
      } else {
        accG += ri * ri;
        accD += ri * double(sum);
      }
    }
  }
  const double g = block_sum<kSpmvThreads / 64>(accG, sh);
  const double d = block_sum<kSpmvThreads / 64>(accD, sh);
  if (threadIdx.x == 0) {
    partialsGamma[blockIdx.x] = g;
    partialsDelta[blockIdx.x] = d;
  }
  if constexpr (PC) {
    const double rho = block_sum<kSpmvThreads / 64>(accR, sh);
    if (threadIdx.x == 0) partialsRho[blockIdx.x] = rho;
  }
}

template <int W, int K>
__global__ __launch_bounds__(kSpmvThreads) void csr_spmv_dot2_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, float *__restrict__ w,
    double *__restrict__ partialsGamma, double *__restrict__ partialsDelta, const double *__restrict__ gammaOut,
    const double *__restrict__ alphaOut, double *__restrict__ gammaPrev, double *__restrict__ alphaPrev) {
  spmv_dot2_body<W, K, false>(nRows, rowPtr, colInd, val, r, nullptr, w, partialsGamma, partialsDelta, nullptr,
                              gammaOut, alphaOut, gammaPrev, alphaPrev);
}

template <int W, int K>
__global__ __launch_bounds__(kSpmvThreads) void csr_spmv_dot2_stop_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, float *__restrict__ w,
    double *__restrict__ partialsGamma, double *__restrict__ partialsDelta, const double *__restrict__ gammaOut,
    const double *__restrict__ alphaOut, double *__restrict__ gammaPrev, double *__restrict__ alphaPrev,
    const int *__restrict__ done) {
  if (*done) return; // uniform over the grid
  spmv_dot2_body<W, K, false>(nRows, rowPtr, colInd, val, r, nullptr, w, partialsGamma, partialsDelta, nullptr,
                              gammaOut, alphaOut, gammaPrev, alphaPrev);
}

template <int W, int K>
__global__ __launch_bounds__(kSpmvThreads) void pcg_spmv_dot3_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, const float *__restrict__ u,
    float *__restrict__ w, double *__restrict__ partialsGamma, double *__restrict__ partialsDelta,
    double *__restrict__ partialsRho, const double *__restrict__ gammaOut, const double *__restrict__ alphaOut,
    double *__restrict__ gammaPrev, double *__restrict__ alphaPrev) {
  spmv_dot2_body<W, K, true>(nRows, rowPtr, colInd, val, r, u, w, partialsGamma, partialsDelta, partialsRho,
                             gammaOut, alphaOut, gammaPrev, alphaPrev);
}

template <int W, int K>
__global__ __launch_bounds__(kSpmvThreads) void pcg_spmv_dot3_stop_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, const float *__restrict__ u,
    float *__restrict__ w, double *__restrict__ partialsGamma, double *__restrict__ partialsDelta,
    double *__restrict__ partialsRho, const double *__restrict__ gammaOut, const double *__restrict__ alphaOut,
    double *__restrict__ gammaPrev, double *__restrict__ alphaPrev, const int *__restrict__ done) {
  if (*done) return; // uniform over the grid
  spmv_dot2_body<W, K, true>(nRows, rowPtr, colInd, val, r, u, w, partialsGamma, partialsDelta, partialsRho,
                             gammaOut, alphaOut, gammaPrev, alphaPrev);
}

// N block_sums behind one barrier, in two steps. wave_sums: the same butterfly per value, then
// the NW wave sums of value i in sh[i * NW ..] (N * NW doubles) and the barrier. wave_total: the
// wave sums of value i added in wave order, block_sum<NW>(v[i])'s bits in whichever thread asks.
template <int NW, int N> __device__ __forceinline__ void wave_sums(double (&v)[N], double *sh) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) sh[i * NW + (threadIdx.x >> 6)] = v[i];
  }
  __syncthreads();
}

template <int NW> __device__ __forceinline__ double wave_total(const double *sh, int i) {
  double s = sh[i * NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += sh[i * NW + w];
  return s;
}

// For a block whose result only leaves through one store per value: thread i < N returns the
// sum of value i (other threads: unspecified)
template <int NW, int N> __device__ __forceinline__ double block_sum_n(double (&v)[N], double *sh) {
  wave_sums<NW>(v, sh);
  return wave_total<NW>(sh, int(threadIdx.x) < N ? int(threadIdx.x) : 0);
}

// spmv_dot2_body for NR right-hand sides, interleaved (element (i, j) of R and Wout at i * NR +
// j): the same grid and the same row -> lane group -> block mapping, and per column the same
// entry order, fmaf chain, xor reduction and block_sum (dev::csr_spmm_ilp_sum, block_sum_n). So
// column j of Wout and slab j of both partial arrays (slab j starts at j * kCgMaxPartials) have
// the bits csr_spmv_dot2_k writes for column j alone, while the matrix is streamed once and an
// entry's NR x values come from one line. Block 0 moves the NR published gammas and alphas.
template <int W, int K, int NR>
__device__ __forceinline__ void spmm_dot2_body(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, float *__restrict__ w,
    double *__restrict__ partialsGamma, double *__restrict__ partialsDelta, const double *__restrict__ gammaOut,
    const double *__restrict__ alphaOut, double *__restrict__ gammaPrev, double *__restrict__ alphaPrev) {
  __shared__ double sh[2 * NR * (kSpmvThreads / 64)];
  if (gammaOut && blockIdx.x == 0 && int(threadIdx.x) < NR) {
    gammaPrev[threadIdx.x] = gammaOut[threadIdx.x];
    alphaPrev[threadIdx.x] = alphaOut[threadIdx.x];
  }
  const int lane = threadIdx.x & (W - 1);
  const int rowsPerPass = int(gridDim.x) * (kSpmvThreads / W);
  double acc[2 * NR]; // gamma of column j at j, delta at NR + j
#pragma unroll
  for (int j = 0; j < 2 * NR; ++j) acc[j] = 0.0;
  // whole W-lane groups leave the loop together (W divides 64)
  for (int row = (blockIdx.x * kSpmvThreads + threadIdx.x) / W; row < nRows; row += rowsPerPass) {
    float sum[NR];
    dev::csr_spmm_ilp_sum<W, K, NR>(row, lane, rowPtr, colInd, val, r, sum);
    if (lane == 0) {
      float ri[NR];
      dev::load_row<NR>(r + int64_t(row) * NR, ri);
      dev::store_row<NR>(w + int64_t(row) * NR, sum);
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        acc[j] += double(ri[j]) * double(ri[j]);
        acc[NR + j] += double(ri[j]) * double(sum[j]);
      }
    }
  }
  const double sum = block_sum_n<kSpmvThreads / 64, 2 * NR>(acc, sh);
  const int t = threadIdx.x; // thread j writes gamma's slab j, thread NR + j delta's
  if (t < NR) partialsGamma[t * kCgMaxPartials + blockIdx.x] = sum;
  else if (t < 2 * NR) partialsDelta[(t - NR) * kCgMaxPartials + blockIdx.x] = sum;
}

template <int W, int K, int NR>
__global__ __launch_bounds__(kSpmvThreads) void csr_spmm_dot2_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, float *__restrict__ w,
    double *__restrict__ partialsGamma, double *__restrict__ partialsDelta, const double *__restrict__ gammaOut,
    const double *__restrict__ alphaOut, double *__restrict__ gammaPrev, double *__restrict__ alphaPrev) {
  spmm_dot2_body<W, K, NR>(nRows, rowPtr, colInd, val, r, w, partialsGamma, partialsDelta, gammaOut, alphaOut,
                           gammaPrev, alphaPrev);
}

// returns early only once every column has stopped (*allDone, which block 0 of the batched update
// writes). Until then a stopped column is computed again from its unchanged r: the same w, the
// same gamma, so the update stops it again without remembering that it had.
template <int W, int K, int NR>
__global__ __launch_bounds__(kSpmvThreads) void csr_spmm_dot2_stop_k(
    int nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colInd,
    const float *__restrict__ val, const float *__restrict__ r, float *__restrict__ w,
    double *__restrict__ partialsGamma, double *__restrict__ partialsDelta, const double *__restrict__ gammaOut,
    const double *__restrict__ alphaOut, double *__restrict__ gammaPrev, double *__restrict__ alphaPrev,
    const int *__restrict__ allDone) {
  if (*allDone) return; // uniform over the grid
  spmm_dot2_body<W, K, NR>(nRows, rowPtr, colInd, val, r, w, partialsGamma, partialsDelta, gammaOut, alphaOut,
                           gammaPrev, alphaPrev);
}

// alpha = gamma / (delta - beta * (gamma / alphaPrev)), every division guarded. The product and
// the difference round separately (no fma), so the bits are those of the same expression in any
// IEEE f64 arithmetic. This file is built with -ffp-contract=fast, which disregards `#pragma
// clang fp contract(off)` (the difference still compiled to one v_fma_f64), so the product
// passes through an empty asm statement that the compiler cannot fuse across.
__device__ __forceinline__ double sr_alpha(double gamma, double delta, double beta, double alphaPrev) {
  double t = beta * guarded_div(gamma, alphaPrev);
  asm volatile("" : "+v"(t));
  return guarded_div(gamma, delta - t);
}

// The recurrence on one element, the only place it is written (xpay_pass, xpay_pass,
// axpy_pass(+a), axpy_pass(-a) in one sweep) ...
// z is what p is built from: r itself, or the preconditioned residual u = dinv o r.
__device__ __forceinline__ void sr_elem(float b, float a, float w, float z, float &r, float &p, float &s,
                                        float &x) {
  p = fmaf(b, p, z);
  s = fmaf(b, s, w);
  x = fmaf(a, p, x);
  r = fmaf(-a, s, r);
}

// ... on a quad whose lanes each have their own beta and alpha ...
__device__ __forceinline__ void sr_quad(const float (&b)[4], const float (&a)[4], float4 w, float4 &r, float4 &p,
                                        float4 &s, float4 &x) {
  sr_elem(b[0], a[0], w.x, r.x, r.x, p.x, s.x, x.x);
  sr_elem(b[1], a[1], w.y, r.y, r.y, p.y, s.y, x.y);
  sr_elem(b[2], a[2], w.z, r.z, r.z, p.z, s.z, x.z);
  sr_elem(b[3], a[3], w.w, r.w, r.w, p.w, s.w, x.w);
}

// ... and on element t of the five vectors (the tails)
__device__ __forceinline__ void sr_elem_at(int64_t t, float b, float a, const float *w, float *r, float *p,
                                           float *s, float *x) {
  float rt = r[t], pt = p[t], st = s[t], xt = x[t];
  sr_elem(b, a, w[t], rt, rt, pt, st, xt);
  p[t] = pt, s[t] = st, x[t] = xt, r[t] = rt;
}

// The update's prologue: gamma and delta from the two slabs, then beta and alpha from them and
// the previous iteration's gamma and alpha; the same bits in every thread of every block
struct SrScalars {
  double gamma, alpha, beta;
};
__device__ __forceinline__ SrScalars sr_scalars(const double *__restrict__ partialsGamma,
                                                const double *__restrict__ partialsDelta, int np,
                                                const double *__restrict__ gammaPrev,
                                                const double *__restrict__ alphaPrev) {
  __shared__ double sh[kThreads / 64];
  const double gamma = sum_partials<kThreads / 64>(partialsGamma, np, sh);
  const double delta = sum_partials<kThreads / 64>(partialsDelta, np, sh);
  const double beta = guarded_div(gamma, *gammaPrev);
  return {gamma, sr_alpha(gamma, delta, beta, *alphaPrev), beta};
}

// One pass over the five vectors with beta and alpha rounded to f32
__device__ __forceinline__ void sr_pass(int64_t n, float b, float a, const float *w, float *r, float *p, float *s,
                                        float *x) {
  const float b4[4] = {b, b, b, b}, a4[4] = {a, a, a, a};
  const bool aw = aligned16(w), ar = aligned16(r), ap = aligned16(p), as = aligned16(s), ax = aligned16(x);
  const int64_t nq = n / 4, stride = int64_t(gridDim.x) * kThreads;
  for (int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x; k < nq; k += stride) {
    const float4 wv = load_quad(w, k, aw);
    float4 rv = load_quad(r, k, ar), pv = load_quad(p, k, ap), sv = load_quad(s, k, as), xv = load_quad(x, k, ax);
    sr_quad(b4, a4, wv, rv, pv, sv, xv);
    store_quad(p, k, ap, pv);
    store_quad(s, k, as, sv);
    store_quad(x, k, ax, xv);
    store_quad(r, k, ar, rv);
  }
  const int64_t t = nq * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) sr_elem_at(t, b, a, w, r, p, s, x);
}

// The second launch: prologue, then the pass. Block 0 publishes gamma, alpha and beta to places
// no block of this launch reads.
__global__ __launch_bounds__(kThreads) void cg_sr_update_k(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, float *r,
    float *p, float *s, float *x, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut) {
  const SrScalars c = sr_scalars(partialsGamma, partialsDelta, np, gammaPrev, alphaPrev);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *gammaOut = c.gamma;
    *alphaOut = c.alpha;
    *betaOut = c.beta;
  }
  sr_pass(n, float(c.beta), float(c.alpha), w, r, p, s, x);
}

// The test between the same prologue and the same pass. gamma <= *thresh ends every block before
// it touches a vector, and block 0 stores only gamma and *done = 1. Otherwise block 0 also stores
// *done = 0 and counts the iteration in *iters; no block's path depends on done or iters.
__global__ __launch_bounds__(kThreads) void cg_sr_update_stop_k(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, float *r,
    float *p, float *s, float *x, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut, const double *__restrict__ thresh, int *__restrict__ done,
    int64_t *__restrict__ iters) {
  const SrScalars c = sr_scalars(partialsGamma, partialsDelta, np, gammaPrev, alphaPrev);
  if (c.gamma <= *thresh) { // the same bits, hence the same branch, in every block
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      *gammaOut = c.gamma;
      *done = 1;
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *gammaOut = c.gamma;
    *alphaOut = c.alpha;
    *betaOut = c.beta;
    *done = 0;
    *iters += 1;
  }
  sr_pass(n, float(c.beta), float(c.alpha), w, r, p, s, x);
}

// ---- The Jacobi-preconditioned update. u = dinv o r is a stored vector that this launch keeps
// equal to f32(dinv[i] * r[i]) bit for bit: a rounded product of its own, kept from contraction
// into the fmaf that follows it as sr_alpha keeps its product. The old u is recomputed from the
// dinv and r the pass loads anyway (the same bits as the stored one) and not read back: 44 bytes
// per row instead of 48.
__device__ __forceinline__ float pcg_apply(float dinv, float r) {
  float u = dinv * r;
  asm volatile("" : "+v"(u));
  return u;
}

__device__ __forceinline__ void pcg_elem(float b, float a, float w, float dinv, float &r, float &p, float &s,
                                         float &x, float &u) {
  sr_elem(b, a, w, pcg_apply(dinv, r), r, p, s, x);
  u = pcg_apply(dinv, r);
}

// sr_pass with the preconditioner: one pass over w, dinv, r, p, s, x and u in the same layout
__device__ __forceinline__ void pcg_pass(int64_t n, float b, float a, const float *w, const float *dinv, float *r,
                                         float *p, float *s, float *x, float *u) {
  const bool aw = aligned16(w), ad = aligned16(dinv), ar = aligned16(r), ap = aligned16(p), as = aligned16(s),
             ax = aligned16(x), au = aligned16(u);
  const int64_t nq = n / 4, stride = int64_t(gridDim.x) * kThreads;
  for (int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x; k < nq; k += stride) {
    const float4 wv = load_quad(w, k, aw), dv = load_quad(dinv, k, ad);
    float4 rv = load_quad(r, k, ar), pv = load_quad(p, k, ap), sv = load_quad(s, k, as), xv = load_quad(x, k, ax);
    float4 uv;
    pcg_elem(b, a, wv.x, dv.x, rv.x, pv.x, sv.x, xv.x, uv.x);
    pcg_elem(b, a, wv.y, dv.y, rv.y, pv.y, sv.y, xv.y, uv.y);
    pcg_elem(b, a, wv.z, dv.z, rv.z, pv.z, sv.z, xv.z, uv.z);
    pcg_elem(b, a, wv.w, dv.w, rv.w, pv.w, sv.w, xv.w, uv.w);
    store_quad(p, k, ap, pv);
    store_quad(s, k, as, sv);
    store_quad(x, k, ax, xv);
    store_quad(r, k, ar, rv);
    store_quad(u, k, au, uv);
  }
  const int64_t t = nq * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float rt = r[t], pt = p[t], st = s[t], xt = x[t], ut;
    pcg_elem(b, a, w[t], dinv[t], rt, pt, st, xt, ut);
    p[t] = pt, s[t] = st, x[t] = xt, r[t] = rt, u[t] = ut;
  }
}

// cg_sr_update_k with gamma = r . u and delta = u . (A u) in the two slabs
__global__ __launch_bounds__(kThreads) void pcg_update_k(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, const float *dinv,
    float *r, float *p, float *s, float *x, float *u, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut) {
  const SrScalars c = sr_scalars(partialsGamma, partialsDelta, np, gammaPrev, alphaPrev);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *gammaOut = c.gamma;
    *alphaOut = c.alpha;
    *betaOut = c.beta;
  }
  pcg_pass(n, float(c.beta), float(c.alpha), w, dinv, r, p, s, x, u);
}

// cg_sr_update_stop_k's test on rho = r . r, the sum of the third slab: the criterion of the
// unpreconditioned form (gamma = r . u is no norm of r). The same bits in every block.
__global__ __launch_bounds__(kThreads) void pcg_update_stop_k(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, const float *dinv,
    float *r, float *p, float *s, float *x, float *u, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut, const double *__restrict__ partialsRho, const double *__restrict__ thresh,
    int *__restrict__ done, int64_t *__restrict__ iters) {
  __shared__ double sh[kThreads / 64];
  const SrScalars c = sr_scalars(partialsGamma, partialsDelta, np, gammaPrev, alphaPrev);
  const double rho = sum_partials<kThreads / 64>(partialsRho, np, sh);
  if (rho <= *thresh) { // a NaN rho compares false
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      *gammaOut = c.gamma;
      *done = 1;
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *gammaOut = c.gamma;
    *alphaOut = c.alpha;
    *betaOut = c.beta;
    *done = 0;
    *iters += 1;
  }
  pcg_pass(n, float(c.beta), float(c.alpha), w, dinv, r, p, s, x, u);
}

// The update for NR right-hand sides, interleaved: one pass over the n * NR elements in the quad
// layout, every column with its own beta and alpha. A thread's quads always hold the same columns
// (the pass stride, blocks * 256 quads, is a multiple of NR elements), so it keeps four (beta,
// alpha) pairs in registers. The prologue sums the 2 NR slabs together (wave_sums: thread t holds
// partial t of each, one butterfly per slab, one barrier), then thread j < NR adds the four wave
// sums of gamma_j and of delta_j in wave order (the bits of sum_partials), forms beta_j and
// alpha_j as sr_scalars does and leaves them, rounded to f32, in LDS for the block.
//
// STOP adds one test per column: thread j < NR also forms stop_j = gamma_j <= thresh[j], the same
// in every block. A stopped column is frozen by a per-lane select that stores back the p, s, x
// and r it loaded (a thread's lanes always hold the same columns); its alpha and beta are not
// published and its iters not counted. Once every column has stopped no block passes over the
// vectors. Block 0 stores done[j] = stop_j and *allDone = their AND. Without STOP the last four
// arguments are not read and shStop, never referenced, takes no LDS.
template <int NR, bool STOP>
__device__ __forceinline__ void sr_update_batch_body(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, float *r,
    float *p, float *s, float *x, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut, const double *__restrict__ thresh, int *__restrict__ done,
    int64_t *__restrict__ iters, int *__restrict__ allDone) {
  constexpr int NW = kThreads / 64;
  __shared__ double sh[2 * NR * NW];
  __shared__ float shB[NR], shA[NR];
  __shared__ int shStop[NR];
  const int tid = threadIdx.x;
  double v[2 * NR]; // gamma of column j at j, delta at NR + j
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    v[j] = tid < np ? partialsGamma[j * kCgMaxPartials + tid] : 0.0;
    v[NR + j] = tid < np ? partialsDelta[j * kCgMaxPartials + tid] : 0.0;
  }
  wave_sums<NW>(v, sh);
  if (tid < NR) {
    const double gamma = wave_total<NW>(sh, tid), delta = wave_total<NW>(sh, NR + tid);
    const double beta = guarded_div(gamma, gammaPrev[tid]);
    const double alpha = sr_alpha(gamma, delta, beta, alphaPrev[tid]);
    bool stop = false;
    if constexpr (STOP) stop = gamma <= thresh[tid];
    if (blockIdx.x == 0) {
      gammaOut[tid] = gamma;
      if constexpr (STOP) done[tid] = stop;
      if (!stop) {
        alphaOut[tid] = alpha;
        betaOut[tid] = beta;
        if constexpr (STOP) iters[tid] += 1;
      }
    }
    shB[tid] = float(beta);
    shA[tid] = float(alpha);
    if constexpr (STOP) shStop[tid] = stop;
  }
  __syncthreads();
  if constexpr (STOP) {
    bool all = true;
#pragma unroll
    for (int j = 0; j < NR; ++j) all = all && shStop[j] != 0;
    if (blockIdx.x == 0 && tid == 0) *allDone = all;
    if (all) return; // uniform over the grid
  }
  const int col0 = (4 * tid) & (NR - 1);
  float b[4], a[4];
  bool keep[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b[i] = shB[(col0 + i) & (NR - 1)];
    a[i] = shA[(col0 + i) & (NR - 1)];
    if constexpr (STOP) keep[i] = shStop[(col0 + i) & (NR - 1)] != 0;
  }
  const int64_t total = n * NR, nq = total / 4, stride = int64_t(gridDim.x) * kThreads;
  for (int64_t k = int64_t(blockIdx.x) * kThreads + tid; k < nq; k += stride) {
    const float4 wv = load_quad(w, k, true);
    float4 rv = load_quad(r, k, true), pv = load_quad(p, k, true), sv = load_quad(s, k, true),
           xv = load_quad(x, k, true);
    const float4 r0 = rv, p0 = pv, s0 = sv, x0 = xv;
    sr_quad(b, a, wv, rv, pv, sv, xv);
    if constexpr (STOP) {
      keep_quad(pv, p0, keep);
      keep_quad(sv, s0, keep);
      keep_quad(xv, x0, keep);
      keep_quad(rv, r0, keep);
    }
    store_quad(p, k, true, pv);
    store_quad(s, k, true, sv);
    store_quad(x, k, true, xv);
    store_quad(r, k, true, rv);
  }
  // the total % 4 tail elements (NR = 2 with an odd n only)
  const int64_t t = nq * 4 + tid;
  bool live = blockIdx.x == 0 && t < total;
  if constexpr (STOP) live = live && !shStop[t & (NR - 1)];
  if (live) sr_elem_at(t, shB[t & (NR - 1)], shA[t & (NR - 1)], w, r, p, s, x);
}

template <int NR>
__global__ __launch_bounds__(kThreads) void cg_sr_update_batch_k(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, float *r,
    float *p, float *s, float *x, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut) {
  sr_update_batch_body<NR, false>(n, partialsGamma, partialsDelta, np, gammaPrev, alphaPrev, w, r, p, s, x,
                                  gammaOut, alphaOut, betaOut, nullptr, nullptr, nullptr, nullptr);
}

template <int NR>
__global__ __launch_bounds__(kThreads) void cg_sr_update_batch_stop_k(
    int64_t n, const double *__restrict__ partialsGamma, const double *__restrict__ partialsDelta, int np,
    const double *__restrict__ gammaPrev, const double *__restrict__ alphaPrev, const float *w, float *r,
    float *p, float *s, float *x, double *__restrict__ gammaOut, double *__restrict__ alphaOut,
    double *__restrict__ betaOut, const double *__restrict__ thresh, int *__restrict__ done,
    int64_t *__restrict__ iters, int *__restrict__ allDone) {
  sr_update_batch_body<NR, true>(n, partialsGamma, partialsDelta, np, gammaPrev, alphaPrev, w, r, p, s, x,
                                 gammaOut, alphaOut, betaOut, thresh, done, iters, allDone);
}

void check_vec(const char *what, int64_t n, const void *a, const void *b) {
  if (n <= 0) throw std::runtime_error(std::string(what) + ": n must be positive");
  if (!a || !b) throw std::runtime_error(std::string(what) + ": null pointer");
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 4)
    throw std::runtime_error(std::string(what) + ": vectors must be 4-byte aligned");
}

void check_np(const char *what, const void *partials, int np) {
  if (!partials || np < 1 || np > kCgMaxPartials)
    throw std::runtime_error(std::string(what) + ": 1.." + std::to_string(kCgMaxPartials) + " partials");
}

} // namespace

int dot_partial_count(int64_t n) {
  return int(std::min<int64_t>(kCgMaxPartials, std::max<int64_t>(1, (n + 4 * kThreads - 1) / (4 * kThreads))));
}

int spmv_dot_partial_count(int nRows, int lanes) {
  const int64_t threads = int64_t(nRows) * (lanes > kSpmvIlp ? lanes - kSpmvIlp : lanes);
  return int(std::min<int64_t>(kCgMaxPartials, std::max<int64_t>(1, (threads + kSpmvThreads - 1) / kSpmvThreads)));
}

void dot_partials_f32(int64_t n, const float *u, const float *v, double *partials, void *stream) {
  check_vec("dot_partials_f32", n, u, v);
  if (!partials) throw std::runtime_error("dot_partials_f32: null pointer");
  hipLaunchKernelGGL(dot_partials_k, dim3(dot_partial_count(n)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, u, v, partials);
  TZ_HIP_LAUNCH_CHECK();
}

void sum_partials_f64(const double *partials, int np, double *out, void *stream) {
  check_np("sum_partials_f64", partials, np);
  if (!out) throw std::runtime_error("sum_partials_f64: null pointer");
  hipLaunchKernelGGL(sum_partials_k, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), partials,
                     np, out);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_alpha(const double *partialsPq, int np, const double *rr, double *alpha, void *stream) {
  check_np("cg_alpha", partialsPq, np);
  if (!rr || !alpha) throw std::runtime_error("cg_alpha: null pointer");
  hipLaunchKernelGGL(cg_alpha_k, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), partialsPq, np,
                     rr, alpha);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_beta(const double *partialsRr, int np, double *rr, double *beta, void *stream) {
  check_np("cg_beta", partialsRr, np);
  if (!rr || !beta) throw std::runtime_error("cg_beta: null pointer");
  hipLaunchKernelGGL(cg_beta_k, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), partialsRr, np,
                     rr, beta);
  TZ_HIP_LAUNCH_CHECK();
}

void axpy_dev_f32(int64_t n, const double *s, int sign, const float *x, float *y, void *stream) {
  check_vec("axpy_dev_f32", n, x, y);
  if (!s || (sign != 1 && sign != -1)) throw std::runtime_error("axpy_dev_f32: scalar pointer and sign +-1");
  hipLaunchKernelGGL(axpy_dev_k, dim3(dot_partial_count(n)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, s, float(sign), x, y);
  TZ_HIP_LAUNCH_CHECK();
}

void xpay_dev_f32(int64_t n, const double *s, const float *x, float *y, void *stream) {
  check_vec("xpay_dev_f32", n, x, y);
  if (!s) throw std::runtime_error("xpay_dev_f32: null pointer");
  hipLaunchKernelGGL(xpay_dev_k, dim3(dot_partial_count(n)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, s, x, y);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_fused_x(int64_t n, const double *partialsPq, int np, const double *rr, const float *p, float *x,
                void *stream) {
  check_vec("cg_fused_x", n, p, x);
  check_np("cg_fused_x", partialsPq, np);
  if (!rr) throw std::runtime_error("cg_fused_x: null pointer");
  hipLaunchKernelGGL(cg_fused_x_k, dim3(dot_partial_count(n)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, partialsPq, np, rr, p, x);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_fused_r(int64_t n, const double *partialsPq, int np, const double *rr, const float *q, float *r,
                double *partialsRr, void *stream) {
  check_vec("cg_fused_r", n, q, r);
  check_np("cg_fused_r", partialsPq, np);
  if (!rr || !partialsRr) throw std::runtime_error("cg_fused_r: null pointer");
  hipLaunchKernelGGL(cg_fused_r_k, dim3(dot_partial_count(n)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, partialsPq, np, rr, q, r, partialsRr);
  TZ_HIP_LAUNCH_CHECK();
}

void cg_fused_p(int64_t n, const double *partialsRr, int np, const double *rr, const float *r, float *p,
                void *stream) {
  check_vec("cg_fused_p", n, r, p);
  check_np("cg_fused_p", partialsRr, np);
  if (!rr) throw std::runtime_error("cg_fused_p: null pointer");
  hipLaunchKernelGGL(cg_fused_p_k, dim3(dot_partial_count(n)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), n, partialsRr, np, rr, r, p);
  TZ_HIP_LAUNCH_CHECK();
}

void csr_spmv_dot(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *p,
                  float *q, int lanes, double *partialsPq, const double *partialsRr, int npRr, double *rr,
                  void *stream) {
  if (nRows <= 0) throw std::runtime_error("csr_spmv_dot: nRows must be positive");
  if (!rowPtr || !colInd || !val || !p || !q || !partialsPq)
    throw std::runtime_error("csr_spmv_dot: null pointer");
  if (partialsRr) {
    check_np("csr_spmv_dot", partialsRr, npRr);
    if (!rr) throw std::runtime_error("csr_spmv_dot: null pointer");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_ilp(lanes, "csr_spmv_dot: lanes must be kSpmvIlp + 1, 2 or 4", [&](auto w, auto k) {
    constexpr int W = decltype(w)::value, K = decltype(k)::value;
    const dim3 g(unsigned(spmv_dot_partial_count(nRows, W))), b(kSpmvThreads);
    hipLaunchKernelGGL((csr_spmv_dot_k<W, K>), g, b, 0, s, nRows, rowPtr, colInd, val, p, q, partialsPq,
                       partialsRr, npRr, rr);
  });
  TZ_HIP_LAUNCH_CHECK();
}

// ---- the single-reduction family: every argument check once, in the two launchers

namespace {

// f(Int<NR>) for k right-hand sides, Int<1> for the single kernels: the one place k is validated
template <typename F> void dispatch_nrhs(const char *what, bool batched, int k, F &&f) {
  if (!batched && k == 1) f(Int<1>{});
  else if (batched && k == 2) f(Int<2>{});
  else if (batched && k == 4) f(Int<4>{});
  else if (batched && k == 8) f(Int<8>{});
  else throw std::runtime_error(std::string(what) + ": k must be 2, 4 or 8 right-hand sides");
}

const char *sr_name(bool batched, bool stop, const char *single, const char *singleStop, const char *batch,
                    const char *batchStop) {
  return batched ? (stop ? batchStop : batch) : (stop ? singleStop : single);
}

struct Span {
  const void *p;
  size_t bytes;
};

// `count` elements at p (none at a null p)
template <typename T> Span span(const T *p, size_t count) { return {p, p ? count * sizeof(T) : 0}; }

// the two share a byte
bool overlap(Span a, Span b) {
  const auto a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
  return a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// single vectors are read in 4-byte accesses when they must be, batched ones never
void check_sr_vecs(const char *what, bool batched, std::initializer_list<const void *> vecs) {
  for (const void *v : vecs) {
    if (!v) throw std::runtime_error(std::string(what) + ": null pointer");
    if (reinterpret_cast<uintptr_t>(v) % (batched ? 16 : 4))
      throw std::runtime_error(std::string(what) + (batched ? ": batched vectors must be 16-byte aligned"
                                                            : ": vectors must be 4-byte aligned"));
  }
}

void check_sr_spmv(const char *what, bool batched, bool stop, int nRows, const int32_t *rowPtr,
                   const int32_t *colInd, const float *val, const float *r, const float *w, const SrState &st) {
  const std::string pre = std::string(what) + ": ";
  const size_t k = size_t(st.k);
  const int *flag = batched ? st.all_done : st.done;
  if (nRows <= 0) throw std::runtime_error(pre + "nRows must be positive");
  if (!rowPtr || !colInd || !val || !r || !w || !st.partials_gamma || !st.partials_delta || (stop && !flag))
    throw std::runtime_error(pre + "null pointer");
  if (batched) {
    check_sr_vecs(what, true, {r, w});
    if (r == w) throw std::runtime_error(pre + "R and Wout must differ");
  }
  // a batched slab array is k whole slabs; how much of a single slab is in use only the caller
  // knows (its partial count), so there the same pointer is refused
  const size_t slab = batched ? k * kCgMaxPartials : 1;
  if (overlap(span(st.partials_gamma, slab), span(st.partials_delta, slab)))
    throw std::runtime_error(pre + "the two slab arrays must not overlap");
  if (st.gamma || st.alpha || st.gamma_prev || st.alpha_prev) {
    if (!st.gamma || !st.alpha || !st.gamma_prev || !st.alpha_prev)
      throw std::runtime_error(pre + "null pointer (the four scalar arrays come together or not at all)");
    // every block reads the flag while block 0 may already have moved the scalars
    if (stop && (overlap(span(flag, 1), span(st.gamma_prev, k)) || overlap(span(flag, 1), span(st.alpha_prev, k))))
      throw std::runtime_error(pre + (batched ? "all_done" : "done") + " must not alias the previous scalars");
  }
}

void check_sr_update(const char *what, bool batched, bool stop, int64_t n, int np, const float *w, const float *r,
                     const float *p, const float *s, const float *x, const SrState &st) {
  const std::string pre = std::string(what) + ": ";
  const size_t k = size_t(st.k);
  if (n <= 0) throw std::runtime_error(pre + "n must be positive");
  check_sr_vecs(what, batched, {w, r, p, s, x});
  check_np(what, st.partials_gamma, np);
  check_np(what, st.partials_delta, np);
  if (!st.gamma_prev || !st.alpha_prev || !st.gamma || !st.alpha || !st.beta)
    throw std::runtime_error(pre + "null pointer");
  const Span prev[2] = {span(st.gamma_prev, k), span(st.alpha_prev, k)};
  const Span out[3] = {span(st.gamma, k), span(st.alpha, k), span(st.beta, k)};
  // a block reads gamma_prev / alpha_prev while block 0 may already have published
  for (const Span &o : out)
    if (overlap(o, prev[0]) || overlap(o, prev[1]))
      throw std::runtime_error(pre + "the published scalars must not alias the previous ones");
  if (overlap(out[0], out[1]) || overlap(out[0], out[2]) || overlap(out[1], out[2]))
    throw std::runtime_error(pre + "the three published arrays must not alias each other");
  if (!stop) return;
  // thresh is read by every block while block 0 publishes, and done / iters / all_done are stores
  // of block 0: none may share a byte with a scalar the launch reads or publishes, or with each other
  if (!st.thresh || !st.done || !st.iters || (batched && !st.all_done)) throw std::runtime_error(pre + "null pointer");
  const Span own[4] = {span(st.thresh, k), span(st.done, k), span(st.iters, k),
                       span(st.all_done, batched ? 1 : 0)};
  for (const Span &o : own)
    for (const Span &sc : {prev[0], prev[1], out[0], out[1], out[2]})
      if (overlap(o, sc))
        throw std::runtime_error(pre + "thresh, done, iters and all_done must not alias the iteration's scalars");
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (overlap(own[i], own[j]))
        throw std::runtime_error(pre + "thresh, done, iters and all_done must not alias each other");
}

// The preconditioned pair's own ground: a launch's vectors and slabs, each read only or written.
// Nothing a launch writes may share a byte with anything else it touches (two it only reads may)
struct Access {
  Span s;
  bool written;
};

void check_disjoint(const std::string &pre, std::initializer_list<Access> all) {
  for (const Access *a = all.begin(); a != all.end(); ++a)
    for (const Access *b = a + 1; b != all.end(); ++b)
      if ((a->written || b->written) && overlap(a->s, b->s))
        throw std::runtime_error(pre + "vectors and slabs must not overlap");
}

// check_sr_spmv on r and w, then u, the rho slab and the overlaps (`cnt` partials per slab)
void check_pcg_spmv(const char *what, bool stop, int nRows, int cnt, const int32_t *rowPtr, const int32_t *colInd,
                    const float *val, const float *r, const float *u, const float *w, const SrState &st) {
  const std::string pre = std::string(what) + ": ";
  if (st.k != 1) throw std::runtime_error(pre + "one right-hand side only");
  check_sr_spmv(what, false, stop, nRows, rowPtr, colInd, val, r, w, st);
  if (!u || !st.partials_rho) throw std::runtime_error(pre + "null pointer");
  check_sr_vecs(what, false, {r, u, w});
  const size_t n = size_t(nRows), c = size_t(cnt);
  check_disjoint(pre, {{span(r, n), false}, {span(u, n), false}, {span(w, n), true},
                       {span(st.partials_gamma, c), true}, {span(st.partials_delta, c), true},
                       {span(st.partials_rho, c), true}});
}

// check_sr_update on the five vectors, then dinv, u, the rho slab (read with `stop` only) and the overlaps
void check_pcg_update(const char *what, bool stop, int64_t n, int np, const float *w, const float *dinv,
                      const float *r, const float *p, const float *s, const float *x, const float *u,
                      const SrState &st) {
  const std::string pre = std::string(what) + ": ";
  if (st.k != 1) throw std::runtime_error(pre + "one right-hand side only");
  check_sr_update(what, false, stop, n, np, w, r, p, s, x, st);
  check_sr_vecs(what, false, {dinv, u});
  if (stop) check_np(what, st.partials_rho, np);
  const size_t m = size_t(n), c = size_t(np);
  check_disjoint(pre, {{span(w, m), false}, {span(dinv, m), false}, {span(r, m), true}, {span(p, m), true},
                       {span(s, m), true}, {span(x, m), true}, {span(u, m), true},
                       {span(st.partials_gamma, c), false}, {span(st.partials_delta, c), false},
                       {span(stop ? st.partials_rho : nullptr, c), false}});
}

// The public signatures say which side of an iteration a launch only reads; SrState serves both
// launches, so it holds every pointer writable
SrState sr_state(int k, const double *partialsGamma, const double *partialsDelta, const double *gamma,
                 const double *alpha, const double *beta, const double *gammaPrev, const double *alphaPrev) {
  const auto m = [](const double *p) { return const_cast<double *>(p); };
  return {k, m(partialsGamma), m(partialsDelta), m(gamma), m(alpha), m(beta), m(gammaPrev), m(alphaPrev)};
}

} // namespace

void sr_spmv_dot2(bool batched, bool stop, int nRows, const int32_t *rowPtr, const int32_t *colInd,
                  const float *val, const float *r, float *w, int lanes, const SrState &st, void *stream) {
  const char *what =
      sr_name(batched, stop, "csr_spmv_dot2", "csr_spmv_dot2_stop", "csr_spmm_dot2", "csr_spmm_dot2_stop");
  const std::string badLanes = std::string(what) + ": lanes must be kSpmvIlp + 1, 2 or 4";
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_nrhs(what, batched, st.k, [&](auto nr) {
    check_sr_spmv(what, batched, stop, nRows, rowPtr, colInd, val, r, w, st);
    dispatch_ilp(lanes, badLanes.c_str(), [&](auto lanesPerRow, auto depth) {
      constexpr int NR = decltype(nr)::value, W = decltype(lanesPerRow)::value, K = decltype(depth)::value;
      const dim3 g(unsigned(spmv_dot_partial_count(nRows, W))), b(kSpmvThreads);
      auto launch = [&](auto kernel, auto... flag) {
        hipLaunchKernelGGL(kernel, g, b, 0, s, nRows, rowPtr, colInd, val, r, w, st.partials_gamma,
                           st.partials_delta, st.gamma, st.alpha, st.gamma_prev, st.alpha_prev, flag...);
      };
      if constexpr (NR == 1) {
        if (stop) launch(csr_spmv_dot2_stop_k<W, K>, st.done);
        else launch(csr_spmv_dot2_k<W, K>);
      } else {
        if (stop) launch(csr_spmm_dot2_stop_k<W, K, NR>, st.all_done);
        else launch(csr_spmm_dot2_k<W, K, NR>);
      }
    });
  });
  TZ_HIP_LAUNCH_CHECK();
}

void sr_update(bool batched, bool stop, int64_t n, int np, const float *w, float *r, float *p, float *s, float *x,
               const SrState &st, void *stream) {
  const char *what =
      sr_name(batched, stop, "cg_sr_update", "cg_sr_update_stop", "cg_sr_update_batch", "cg_sr_update_batch_stop");
  hipStream_t stm = static_cast<hipStream_t>(stream);
  dispatch_nrhs(what, batched, st.k, [&](auto nr) {
    constexpr int NR = decltype(nr)::value;
    check_sr_update(what, batched, stop, n, np, w, r, p, s, x, st);
    const dim3 g(unsigned(dot_partial_count(n * NR))), b(kThreads);
    auto launch = [&](auto kernel, auto... stopState) {
      hipLaunchKernelGGL(kernel, g, b, 0, stm, n, st.partials_gamma, st.partials_delta, np, st.gamma_prev,
                         st.alpha_prev, w, r, p, s, x, st.gamma, st.alpha, st.beta, stopState...);
    };
    if constexpr (NR == 1) {
      if (stop) launch(cg_sr_update_stop_k, st.thresh, st.done, st.iters);
      else launch(cg_sr_update_k);
    } else {
      if (stop) launch(cg_sr_update_batch_stop_k<NR>, st.thresh, st.done, st.iters, st.all_done);
      else launch(cg_sr_update_batch_k<NR>);
    }
  });
  TZ_HIP_LAUNCH_CHECK();
}

void sr_pcg_spmv_dot3(bool stop, int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val,
                      const float *r, const float *u, float *w, int lanes, const SrState &st, void *stream) {
  const char *what = stop ? "pcg_spmv_dot3_stop" : "pcg_spmv_dot3";
  const std::string badLanes = std::string(what) + ": lanes must be kSpmvIlp + 1, 2 or 4";
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_ilp(lanes, badLanes.c_str(), [&](auto lanesPerRow, auto depth) {
    constexpr int W = decltype(lanesPerRow)::value, K = decltype(depth)::value;
    const int cnt = nRows > 0 ? spmv_dot_partial_count(nRows, W) : 1;
    check_pcg_spmv(what, stop, nRows, cnt, rowPtr, colInd, val, r, u, w, st);
    const dim3 g{unsigned(cnt)}, b(kSpmvThreads);
    auto launch = [&](auto kernel, auto... flag) {
      hipLaunchKernelGGL(kernel, g, b, 0, s, nRows, rowPtr, colInd, val, r, u, w, st.partials_gamma,
                         st.partials_delta, st.partials_rho, st.gamma, st.alpha, st.gamma_prev, st.alpha_prev,
                         flag...);
    };
    if (stop) launch(pcg_spmv_dot3_stop_k<W, K>, st.done);
    else launch(pcg_spmv_dot3_k<W, K>);
  });
  TZ_HIP_LAUNCH_CHECK();
}

void sr_pcg_update(bool stop, int64_t n, int np, const float *w, const float *dinv, float *r, float *p, float *s,
                   float *x, float *u, const SrState &st, void *stream) {
  const char *what = stop ? "pcg_update_stop" : "pcg_update";
  hipStream_t stm = static_cast<hipStream_t>(stream);
  check_pcg_update(what, stop, n, np, w, dinv, r, p, s, x, u, st);
  const dim3 g(unsigned(dot_partial_count(n))), b(kThreads);
  auto launch = [&](auto kernel, auto... stopState) {
    hipLaunchKernelGGL(kernel, g, b, 0, stm, n, st.partials_gamma, st.partials_delta, np, st.gamma_prev,
                       st.alpha_prev, w, dinv, r, p, s, x, u, st.gamma, st.alpha, st.beta, stopState...);
  };
  if (stop) launch(pcg_update_stop_k, static_cast<const double *>(st.partials_rho), st.thresh, st.done, st.iters);
  else launch(pcg_update_k);
  TZ_HIP_LAUNCH_CHECK();
}

// ---- the entry points: fill the state, call the launcher

void csr_spmv_dot2(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                   float *w, int lanes, double *partialsGamma, double *partialsDelta, const double *gammaOut,
                   const double *alphaOut, double *gammaPrev, double *alphaPrev, void *stream) {
  const SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, nullptr, gammaPrev, alphaPrev);
  sr_spmv_dot2(false, false, nRows, rowPtr, colInd, val, r, w, lanes, st, stream);
}

void csr_spmv_dot2_stop(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                        float *w, int lanes, double *partialsGamma, double *partialsDelta, const double *gammaOut,
                        const double *alphaOut, double *gammaPrev, double *alphaPrev, const int *done,
                        void *stream) {
  SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, nullptr, gammaPrev, alphaPrev);
  st.done = const_cast<int *>(done);
  sr_spmv_dot2(false, true, nRows, rowPtr, colInd, val, r, w, lanes, st, stream);
}

void csr_spmm_dot2(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *R,
                   float *Wout, int k, int lanes, double *partialsGamma, double *partialsDelta,
                   const double *gammaOut, const double *alphaOut, double *gammaPrev, double *alphaPrev,
                   void *stream) {
  const SrState st = sr_state(k, partialsGamma, partialsDelta, gammaOut, alphaOut, nullptr, gammaPrev, alphaPrev);
  sr_spmv_dot2(true, false, nRows, rowPtr, colInd, val, R, Wout, lanes, st, stream);
}

void csr_spmm_dot2_stop(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *R,
                        float *Wout, int k, int lanes, double *partialsGamma, double *partialsDelta,
                        const double *gammaOut, const double *alphaOut, double *gammaPrev, double *alphaPrev,
                        const int *allDone, void *stream) {
  SrState st = sr_state(k, partialsGamma, partialsDelta, gammaOut, alphaOut, nullptr, gammaPrev, alphaPrev);
  st.all_done = const_cast<int *>(allDone);
  sr_spmv_dot2(true, true, nRows, rowPtr, colInd, val, R, Wout, lanes, st, stream);
}

void cg_sr_update(int64_t n, const double *partialsGamma, const double *partialsDelta, int np,
                  const double *gammaPrev, const double *alphaPrev, const float *w, float *r, float *p, float *s,
                  float *x, double *gammaOut, double *alphaOut, double *betaOut, void *stream) {
  const SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, betaOut, gammaPrev, alphaPrev);
  sr_update(false, false, n, np, w, r, p, s, x, st, stream);
}

void cg_sr_update_stop(int64_t n, const double *partialsGamma, const double *partialsDelta, int np,
                       const double *gammaPrev, const double *alphaPrev, const float *w, float *r, float *p,
                       float *s, float *x, double *gammaOut, double *alphaOut, double *betaOut,
                       const double *thresh, int *done, int64_t *iters, void *stream) {
  SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, betaOut, gammaPrev, alphaPrev);
  st.thresh = thresh, st.done = done, st.iters = iters;
  sr_update(false, true, n, np, w, r, p, s, x, st, stream);
}

void cg_sr_update_batch(int64_t n, int k, const double *partialsGamma, const double *partialsDelta, int np,
                        const double *gammaPrev, const double *alphaPrev, const float *W, float *R, float *P,
                        float *S, float *X, double *gammaOut, double *alphaOut, double *betaOut, void *stream) {
  const SrState st = sr_state(k, partialsGamma, partialsDelta, gammaOut, alphaOut, betaOut, gammaPrev, alphaPrev);
  sr_update(true, false, n, np, W, R, P, S, X, st, stream);
}

void cg_sr_update_batch_stop(int64_t n, int k, const double *partialsGamma, const double *partialsDelta, int np,
                             const double *gammaPrev, const double *alphaPrev, const float *W, float *R, float *P,
                             float *S, float *X, double *gammaOut, double *alphaOut, double *betaOut,
                             const double *thresh, int *done, int64_t *iters, int *allDone, void *stream) {
  SrState st = sr_state(k, partialsGamma, partialsDelta, gammaOut, alphaOut, betaOut, gammaPrev, alphaPrev);
  st.thresh = thresh, st.done = done, st.iters = iters, st.all_done = allDone;
  sr_update(true, true, n, np, W, R, P, S, X, st, stream);
}

void pcg_spmv_dot3(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                   const float *u, float *w, int lanes, double *partialsGamma, double *partialsDelta,
                   double *partialsRho, const double *gammaOut, const double *alphaOut, double *gammaPrev,
                   double *alphaPrev, void *stream) {
  SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, nullptr, gammaPrev, alphaPrev);
  st.partials_rho = partialsRho;
  sr_pcg_spmv_dot3(false, nRows, rowPtr, colInd, val, r, u, w, lanes, st, stream);
}

void pcg_spmv_dot3_stop(int nRows, const int32_t *rowPtr, const int32_t *colInd, const float *val, const float *r,
                        const float *u, float *w, int lanes, double *partialsGamma, double *partialsDelta,
                        double *partialsRho, const double *gammaOut, const double *alphaOut, double *gammaPrev,
                        double *alphaPrev, const int *done, void *stream) {
  SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, nullptr, gammaPrev, alphaPrev);
  st.partials_rho = partialsRho, st.done = const_cast<int *>(done);
  sr_pcg_spmv_dot3(true, nRows, rowPtr, colInd, val, r, u, w, lanes, st, stream);
}

void pcg_update(int64_t n, const double *partialsGamma, const double *partialsDelta, int np,
                const double *gammaPrev, const double *alphaPrev, const float *w, const float *dinv, float *r,
                float *p, float *s, float *x, float *u, double *gammaOut, double *alphaOut, double *betaOut,
                void *stream) {
  const SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, betaOut, gammaPrev, alphaPrev);
  sr_pcg_update(false, n, np, w, dinv, r, p, s, x, u, st, stream);
}

void pcg_update_stop(int64_t n, const double *partialsGamma, const double *partialsDelta, int np,
                     const double *gammaPrev, const double *alphaPrev, const float *w, const float *dinv, float *r,
                     float *p, float *s, float *x, float *u, double *gammaOut, double *alphaOut, double *betaOut,
                     const double *partialsRho, const double *thresh, int *done, int64_t *iters, void *stream) {
  SrState st = sr_state(1, partialsGamma, partialsDelta, gammaOut, alphaOut, betaOut, gammaPrev, alphaPrev);
  st.partials_rho = const_cast<double *>(partialsRho), st.thresh = thresh, st.done = done, st.iters = iters;
  sr_pcg_update(true, n, np, w, dinv, r, p, s, x, u, st, stream);
}

} // namespace kern
} // namespace tz
