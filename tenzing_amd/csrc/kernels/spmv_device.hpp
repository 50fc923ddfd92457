// Device bodies shared by the SpMV kernels (spmv_kernels.hip) and the fused move + SpMV kernel
// (halo_kernels.hip). Device code only: include from .hip translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tz {
namespace kern {
namespace dev {

// CSR with instruction-level parallelism, for global thread `gtid`: W lanes per row, and every
// lane issues all K of its column loads, then all K value loads and x gathers, before it uses
// any (one pass covers W*K entries of the row). Short rows (10 entries on average here) then cost
// one latency chain per row (row pointers -> columns -> x) with few, loaded waves, instead of one
// chain per W entries on 4-8x as many waves. Whole W-lane groups exit together (W divides 64).
// the row's sum, in every one of its W lanes (all W lanes of a row call this together)
template <int W, int K>
__device__ __forceinline__ float csr_spmv_ilp_sum(int row, int lane, const int32_t *__restrict__ rowPtr,
                                                  const int32_t *__restrict__ colInd,
                                                  const float *__restrict__ val,
                                                  const float *__restrict__ x) {
  const int b = rowPtr[row], e = rowPtr[row + 1];
  float sum = 0.f;
  for (int j0 = b + lane; j0 < e; j0 += W * K) {
    int c[K];
    float v[K], xv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = j0 + k * W;
      c[k] = j < e ? colInd[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = j0 + k * W;
      v[k] = j < e ? val[j] : 0.f;
      xv[k] = c[k] >= 0 ? x[c[k]] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sum = fmaf(v[k], xv[k], sum);
  }
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, W);
  return sum;
}

// NR floats at p (NR * 4-byte aligned; NR = 2, 4 or 8): one 8-byte, one 16-byte or two 16-byte loads
template <int NR> __device__ __forceinline__ void load_row(const float *p, float (&o)[NR]) {
  if constexpr (NR == 2) {
    const float2 a = *reinterpret_cast<const float2 *>(p);
    o[0] = a.x, o[1] = a.y;
  } else {
#pragma unroll
    for (int q = 0; q < NR / 4; ++q) {
      const float4 a = reinterpret_cast<const float4 *>(p)[q];
      o[4 * q] = a.x, o[4 * q + 1] = a.y, o[4 * q + 2] = a.z, o[4 * q + 3] = a.w;
    }
  }
}

template <int NR> __device__ __forceinline__ void store_row(float *p, const float (&v)[NR]) {
  if constexpr (NR == 2) {
    *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int q = 0; q < NR / 4; ++q)
      reinterpret_cast<float4 *>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
}

// csr_spmv_ilp_sum for NR interleaved vectors (element (i, j) at x[i * NR + j]): sum[j] = the
// row's product with column j, in every one of the row's W lanes. A lane walks the same entries
// in the same order (lane, lane + W, ..) and every column has its own fmaf chain and its own xor
// reduction, so sum[j] has the bits csr_spmv_ilp_sum<W, any K> gives on column j alone. The
// column index and the value of an entry are loaded once and its NR x values with one access of
// 4 NR bytes (inside one 128-byte line). A pass holds KP = min(K, 32 / NR) entries per lane, all
// of its loads issued before any is used: 32 gathered floats in flight per lane at every NR keep
// a 1024-thread block below 128 VGPRs. Masked entries multiply 0 by 0, as in the single body.
template <int W, int K, int NR>
__device__ __forceinline__ void csr_spmm_ilp_sum(int row, int lane, const int32_t *__restrict__ rowPtr,
                                                 const int32_t *__restrict__ colInd,
                                                 const float *__restrict__ val, const float *__restrict__ x,
                                                 float (&sum)[NR]) {
  constexpr int KP = K * NR <= 32 ? K : 32 / NR;
  const int b = rowPtr[row], e = rowPtr[row + 1];
#pragma unroll
  for (int j = 0; j < NR; ++j) sum[j] = 0.f;
  for (int j0 = b + lane; j0 < e; j0 += W * KP) {
    int c[KP];
    float v[KP], xv[KP][NR];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int j = j0 + k * W;
      c[k] = j < e ? colInd[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int j = j0 + k * W;
      v[k] = j < e ? val[j] : 0.f;
      if (c[k] >= 0) {
        load_row<NR>(x + int64_t(c[k]) * NR, xv[k]);
      } else {
#pragma unroll
        for (int q = 0; q < NR; ++q) xv[k][q] = 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
#pragma unroll
      for (int q = 0; q < NR; ++q) sum[q] = fmaf(v[k], xv[k][q], sum[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < NR; ++q) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) sum[q] += __shfl_xor(sum[q], off, W);
  }
}

template <int W, int K>
__device__ __forceinline__ void csr_spmv_ilp_row(int gtid, int nRows, const int32_t *__restrict__ rowPtr,
                                                 const int32_t *__restrict__ colInd,
                                                 const float *__restrict__ val,
                                                 const float *__restrict__ x, float *__restrict__ y,
                                                 int accumulate) {
  const int row = gtid / W;
  const int lane = gtid & (W - 1);
  if (row >= nRows) return;
  const float sum = csr_spmv_ilp_sum<W, K>(row, lane, rowPtr, colInd, val, x);
  if (lane == 0) y[row] = accumulate ? y[row] + sum : sum;
}

} // namespace dev
} // namespace kern
} // namespace tz
