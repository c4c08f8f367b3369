// table_moments.h — batch statistics of a point-major feature table [N, C] by 256-thread workgroups (sp_bn.hip, sp_inorm.hip;
// DESIGN.md 6.4.3).  Device only.
//
// Thread layout (RowLanes): C = 4 C4 floats per row; thread tid owns the four channels c4 = tid % C4 and walks the rows
// rs, rs + rpi, ... of its workgroup's range with rs = tid / C4, rpi = 256 / C4.  The 256 % C4 leftover threads (rs >= rpi,
// !live()) take part in barriers and in nothing else: they load nothing, and what they leave in LDS is never read.
//
// Barrier contract of rows_to_moments, rows_to_grad_sums and partials_sum2: EVERY thread of a workgroup of exactly 256 threads
// calls (uniform control flow, idle threads included); the LDS array is the caller's, needs no barrier on entry, and must not be
// touched again before a barrier of the caller's: the functions do NOT end in one (their last step reads LDS in the rs == 0
// threads / in thread 0).  moments_add and the other helpers are per-thread and have no barrier.
// Every sum is taken in a fixed order: two runs give the same bits.
#pragma once
#include "attn_common.h"

namespace vdetr {

struct RowLanes {
  int C4, c4, rs, rpi;
  __device__ __forceinline__ bool live() const { return rs < rpi; }
};
__device__ __forceinline__ RowLanes row_lanes(int C) {
  const int C4 = C >> 2, tid = threadIdx.x;
  return RowLanes{C4, tid % C4, tid / C4, 256 / C4};
}

// (count, mean, M2 about the mean) of four channels, and Chan et al.'s merge of two such aggregates
struct Moments {
  float n;
  f32x4 mu, m2;
};
__device__ __forceinline__ void moments_add(Moments& a, float nb, const f32x4& mb, const f32x4& sb) {
  if (nb <= 0.f) return;
  const float nn = a.n + nb;
  const f32x4 d = mb - a.mu;
  a.mu += d * (nb / nn);
  a.m2 += sb + d * d * (a.n * nb / nn);
  a.n = nn;
}
// ... with partial b of a [np][3][C] array / with an aggregate kept as 9 floats in LDS
__device__ __forceinline__ void moments_add_partial(Moments& a, const float* part, int b, int C, int c4) {
  const float* p = part + (size_t)b * 3 * C;
  moments_add(a, p[c4 * 4], reinterpret_cast<const f32x4*>(p + C)[c4], reinterpret_cast<const f32x4*>(p + 2 * C)[c4]);
}
__device__ __forceinline__ void moments_add_lds(Moments& a, const float* o) {
  moments_add(a, o[0], f32x4{o[1], o[2], o[3], o[4]}, f32x4{o[5], o[6], o[7], o[8]});
}
__device__ __forceinline__ void moments_store_lds(float* o, const Moments& a) {
  o[0] = a.n;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[1 + e] = a.mu[e]; o[5 + e] = a.m2[e]; }
}

// rows r0 .. r1 of x -> partial blockIdx.x of part [np][3][C]: count, mean, M2 about ITS mean (two sweeps over rows that stay in cache)
__device__ __forceinline__ void rows_to_moments(RowLanes L, const float* __restrict__ x, int C, int r0, int r1, float* __restrict__ part,
                                                f32x4 (&red)[256]) {
  const int tid = threadIdx.x;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (L.live())
    for (int r = r0 + L.rs; r < r1; r += L.rpi) s += reinterpret_cast<const f32x4*>(x)[(size_t)r * L.C4 + L.c4];
  red[tid] = s;
  __syncthreads();
  f32x4 tot = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < L.rpi; ++j) tot += red[j * L.C4 + L.c4];  // fixed order (idle threads read in bounds and drop the result)
  const float cnt = (float)(r1 - r0);
  const f32x4 mean = tot / cnt;
  __syncthreads();
  f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
  if (L.live())
    for (int r = r0 + L.rs; r < r1; r += L.rpi) {
      const f32x4 d = reinterpret_cast<const f32x4*>(x)[(size_t)r * L.C4 + L.c4] - mean;
      m2 += d * d;
    }
  red[tid] = m2;
  __syncthreads();
  if (L.rs == 0) {
    f32x4 t2 = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L.rpi; ++j) t2 += red[j * L.C4 + L.c4];
    float* p = part + (size_t)blockIdx.x * 3 * C;
    reinterpret_cast<f32x4*>(p)[L.c4] = f32x4{cnt, cnt, cnt, cnt};
    reinterpret_cast<f32x4*>(p + C)[L.c4] = mean;
    reinterpret_cast<f32x4*>(p + 2 * C)[L.c4] = t2;
  }
}

// rows r0 .. r1 -> partial blockIdx.x of part [np][2][C]: sum g, sum g xhat with g = grad(i) of element i = r C4 + c4 and
// xhat = (x - mean) invstd of the statistics rows given
template <typename Grad>
__device__ __forceinline__ void rows_to_grad_sums(RowLanes L, const float* x, int C, int r0, int r1, const float* mean_row,
                                                  const float* invstd_row, Grad grad, float* part, f32x4 (&red)[2][256]) {
  const int tid = threadIdx.x;
  f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = {0.f, 0.f, 0.f, 0.f};
  if (L.live()) {
    const f32x4 mean = reinterpret_cast<const f32x4*>(mean_row)[L.c4], invstd = reinterpret_cast<const f32x4*>(invstd_row)[L.c4];
    for (int r = r0 + L.rs; r < r1; r += L.rpi) {
      const size_t i = (size_t)r * L.C4 + L.c4;
      const f32x4 g = grad(i);
      const f32x4 xh = (reinterpret_cast<const f32x4*>(x)[i] - mean) * invstd;
      sg += g;
      sgx += g * xh;
    }
  }
  red[0][tid] = sg;
  red[1][tid] = sgx;
  __syncthreads();
  if (L.rs == 0) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L.rpi; ++j) { a += red[0][j * L.C4 + L.c4]; b += red[1][j * L.C4 + L.c4]; }
    float* p = part + (size_t)blockIdx.x * 2 * C;
    reinterpret_cast<f32x4*>(p)[L.c4] = a;
    reinterpret_cast<f32x4*>(p + C)[L.c4] = b;
  }
}

// channels 4 c4 .. 4 c4 + 3 of the sum of the np partials [2][C] by ONE workgroup: thread t adds the partials t, t + 256, ...,
// then a fixed tree: lane shuffles inside a wave, the 4 wave sums through LDS (one barrier instead of 16).  Thread 0, which
// alone holds the sums, passes them to done(sg, sgx).
template <typename Done>
__device__ __forceinline__ void partials_sum2(const float* part, int np, int C, int c4, f32x4 (&red)[2][4], Done done) {
  const int tid = threadIdx.x;
  f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = {0.f, 0.f, 0.f, 0.f};
  for (int b = tid; b < np; b += 256) {
    const float* p = part + (size_t)b * 2 * C;
    sg += reinterpret_cast<const f32x4*>(p)[c4];
    sgx += reinterpret_cast<const f32x4*>(p + C)[c4];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = __shfl_down(sg[e], off), b = __shfl_down(sgx[e], off);
      if ((tid & 63) < off) { sg[e] += a; sgx[e] += b; }
    }
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = sg; red[1][tid >> 6] = sgx; }
  __syncthreads();
  if (tid == 0) {
    for (int w2 = 1; w2 < 4; ++w2) { sg += red[0][w2]; sgx += red[1][w2]; }
    done(sg, sgx);
  }
}

}  // namespace vdetr
