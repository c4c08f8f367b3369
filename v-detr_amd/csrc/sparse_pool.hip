// sparse_pool.hip — sum / average / max pooling of a sparse tensor over a kernel map, gfx950.
//
// Reference: ME.MinkowskiSumPooling / MinkowskiAvgPooling / MinkowskiMaxPooling / MinkowskiPoolingTranspose behind
// models/modules/common.py:192-259 (avg_pool, avg_unpool, sum_pool).  MinkowskiEngine is un-vendored; what is restated is the
// published definition over the occupied neighbours N(u) = {k : nbr[k][u] >= 0} of an output site u:
//   sum: y[u] = sum_{k in N(u)} x[nbr[k][u]]   (ascending k)
//   avg: that sum times 1 / |N(u)|  (the neighbours that exist, not K); |N(u)| = 0 gives 0
//   max: per channel the maximum over N(u), arg[u][c] = the LOWEST k that attains it; an empty N(u) gives 0 and arg = -1
// The backward is a GATHER through the inverse map inv[k][i] (the output row that reads input row i through offset k, unique on a
// lattice: vdetr_sp_inverse_map_i32):  dx[i] = sum_k dy[inv[k][i]] * inv_count[inv[k][i]]  (max: where arg[inv[k][i]][c] == k),
// ascending k.  No float atomics, no memset: fixed summation order, two runs agree bit for bit.
//
// Shape: whole-row gathers.  A thread owns one row's channel quad (16 bytes); the threads of a workgroup walk consecutive quads of
// consecutive rows, so a wave's map entries are one or a few words and its row reads are contiguous 256 B - 2 KB pieces.  Map
// entries are fetched eight offsets at a time and their rows requested together (the index -> row chain per offset left
// sp_gather_kernel latency-bound).  At most 127 rows per destination, evenly loaded: one thread per destination quad is enough.
#include "common.h"

namespace vdetr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SpPoolParams {
  int K, nout, nin, C4, mode;
  const float* x;
  const int* nbr;
  float* y;
  float* inv_count;
  signed char* arg;
};

constexpr int kPoolGroup = 8;

__global__ __launch_bounds__(256) void sp_pool_fwd_kernel(SpPoolParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.nout * P.C4) return;
  const int c4 = (int)(t % P.C4);
  const int u = (int)(t / P.C4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc = zero;
  int cnt = 0;
  int a0 = -1, a1 = -1, a2 = -1, a3 = -1;
  for (int k0 = 0; k0 < P.K; k0 += kPoolGroup) {
    int i[kPoolGroup];
#pragma unroll
    for (int j = 0; j < kPoolGroup; ++j) i[j] = k0 + j < P.K ? P.nbr[(size_t)(k0 + j) * P.nout + u] : -1;
    f32x4 v[kPoolGroup];
#pragma unroll
    for (int j = 0; j < kPoolGroup; ++j) {
      v[j] = zero;
      if (i[j] >= 0 && i[j] < P.nin) v[j] = reinterpret_cast<const f32x4*>(P.x)[(size_t)i[j] * P.C4 + c4];
    }
#pragma unroll
    for (int j = 0; j < kPoolGroup; ++j) {
      if (i[j] < 0 || i[j] >= P.nin) continue;
      if (P.mode == 2) {
        const int k = k0 + j;
        if (cnt == 0 || v[j][0] > acc[0]) { acc[0] = v[j][0]; a0 = k; }
        if (cnt == 0 || v[j][1] > acc[1]) { acc[1] = v[j][1]; a1 = k; }
        if (cnt == 0 || v[j][2] > acc[2]) { acc[2] = v[j][2]; a2 = k; }
        if (cnt == 0 || v[j][3] > acc[3]) { acc[3] = v[j][3]; a3 = k; }
      } else {
        acc += v[j];
      }
      ++cnt;
    }
  }
  if (P.mode == 1) {
    const float ic = cnt > 0 ? 1.f / (float)cnt : 0.f;
    acc = acc * ic;
    if (c4 == 0) P.inv_count[u] = ic;
  } else if (P.mode == 2) {
    const unsigned packed = (unsigned)(a0 & 0xff) | ((unsigned)(a1 & 0xff) << 8) | ((unsigned)(a2 & 0xff) << 16) | ((unsigned)(a3 & 0xff) << 24);
    reinterpret_cast<unsigned*>(P.arg)[t] = packed;  // [nout][C] int8: four channels = one word
  }
  reinterpret_cast<f32x4*>(P.y)[t] = acc;
}

struct SpPoolGrads {
  const int* inv;
  const float* dy;
  float* dx;
};

__global__ __launch_bounds__(256) void sp_pool_bwd_kernel(SpPoolParams P, SpPoolGrads G) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.nin * P.C4) return;
  const int c4 = (int)(t % P.C4);
  const int i = (int)(t / P.C4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc = zero;
  for (int k0 = 0; k0 < P.K; k0 += kPoolGroup) {
    int u[kPoolGroup];
#pragma unroll
    for (int j = 0; j < kPoolGroup; ++j) {
      u[j] = k0 + j < P.K ? G.inv[(size_t)(k0 + j) * P.nin + i] : -1;
      if (u[j] >= P.nout) u[j] = -1;
    }
    f32x4 g[kPoolGroup];
    float s[kPoolGroup];
    unsigned a[kPoolGroup];
#pragma unroll
    for (int j = 0; j < kPoolGroup; ++j) {
      g[j] = zero;
      s[j] = 1.f;
      a[j] = 0u;
      if (u[j] >= 0) {
        g[j] = reinterpret_cast<const f32x4*>(G.dy)[(size_t)u[j] * P.C4 + c4];
        if (P.mode == 1) s[j] = P.inv_count[u[j]];
        if (P.mode == 2) a[j] = reinterpret_cast<const unsigned*>(P.arg)[(size_t)u[j] * P.C4 + c4];
      }
    }
#pragma unroll
    for (int j = 0; j < kPoolGroup; ++j) {
      if (u[j] < 0) continue;
      if (P.mode == 2) {
        const unsigned k = (unsigned)(k0 + j);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (((a[j] >> (8 * e)) & 0xffu) == k) acc[e] += g[j][e];
      } else if (P.mode == 1) {
        acc += g[j] * s[j];
      } else {
        acc += g[j];
      }
    }
  }
  reinterpret_cast<f32x4*>(G.dx)[t] = acc;
}

static int pool_fill(const vdetr_sp_pool_desc* d, SpPoolParams* P, const char* op) {
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  VDETR_REQUIRE(d->C > 0 && d->C % 4 == 0, "%s: C=%d must be a positive multiple of 4 (float4 rows)", op, d->C);
  VDETR_REQUIRE(d->K >= 1 && d->K <= 127, "%s: K=%d must be in 1 .. 127 (the int8 argmax)", op, d->K);
  VDETR_REQUIRE(d->mode >= 0 && d->mode <= 2, "%s: mode=%d (0 sum, 1 avg, 2 max)", op, d->mode);
  VDETR_REQUIRE(d->nout >= 0, "%s: nout=%d is negative", op, d->nout);
  VDETR_REQUIRE(d->nin >= 0, "%s: nin=%d is negative", op, d->nin);
  P->K = d->K; P->nout = d->nout; P->nin = d->nin; P->C4 = d->C / 4; P->mode = d->mode;
  P->x = d->x; P->nbr = d->nbr; P->y = d->y; P->inv_count = d->inv_count; P->arg = d->arg;
  return VDETR_OK;
}

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_sp_pool_fwd_f32(const vdetr_sp_pool_desc* d, vdetr_stream_t stream) {
  SpPoolParams P;
  if (int e = pool_fill(d, &P, "sp_pool_fwd")) return e;
  if (d->nout == 0) return VDETR_OK;
  VDETR_REQUIRE(d->nbr, "sp_pool_fwd: nbr is NULL with nout=%d", d->nout);
  VDETR_REQUIRE(d->y, "sp_pool_fwd: y is NULL with nout=%d", d->nout);
  VDETR_REQUIRE(d->x || d->nin == 0, "sp_pool_fwd: x is NULL with nin=%d", d->nin);
  VDETR_REQUIRE(d->mode != 1 || d->inv_count, "sp_pool_fwd: inv_count is NULL with mode=%d (avg stores 1/|N|)", d->mode);
  VDETR_REQUIRE(d->mode != 2 || d->arg, "sp_pool_fwd: arg is NULL with mode=%d (max stores its argmax)", d->mode);
  const long long blocks = ((long long)d->nout * P.C4 + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_pool_fwd: nout=%d x C=%d is more than one launch covers", d->nout, d->C);
  hipLaunchKernelGGL(sp_pool_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_pool_fwd");
}

extern "C" int vdetr_sp_pool_bwd_f32(const vdetr_sp_pool_desc* d, const int32_t* inv, const float* dy, float* dx,
                                     vdetr_stream_t stream) {
  SpPoolParams P;
  if (int e = pool_fill(d, &P, "sp_pool_bwd")) return e;
  if (d->nin == 0) return VDETR_OK;
  VDETR_REQUIRE(inv, "sp_pool_bwd: inv is NULL with nin=%d", d->nin);
  VDETR_REQUIRE(dx, "sp_pool_bwd: dx is NULL with nin=%d", d->nin);
  VDETR_REQUIRE(dy || d->nout == 0, "sp_pool_bwd: dy is NULL with nout=%d", d->nout);
  VDETR_REQUIRE(d->mode != 1 || d->inv_count || d->nout == 0, "sp_pool_bwd: inv_count is NULL with mode=%d (avg reads the forward's 1/|N|)", d->mode);
  VDETR_REQUIRE(d->mode != 2 || d->arg || d->nout == 0, "sp_pool_bwd: arg is NULL with mode=%d (max reads the forward's argmax)", d->mode);
  const long long blocks = ((long long)d->nin * P.C4 + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_pool_bwd: nin=%d x C=%d is more than one launch covers", d->nin, d->C);
  if (d->nout == 0) P.nout = 0;  // every inverse entry then counts as empty: dx is written as zeros
  SpPoolGrads G{inv, dy, dx};
  hipLaunchKernelGGL(sp_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, G);
  return check_launch("sp_pool_bwd");
}
