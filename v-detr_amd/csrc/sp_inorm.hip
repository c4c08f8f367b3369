// sp_inorm.hip — InstanceNorm over the point-major feature table [N, C] of a sparse tensor, gfx950.
//
// Reference: ME.MinkowskiInstanceNorm (models/mink_resnet.py with stem_bn = False; models/modules/common.py:24-30): per scene and
// channel, y = (x - mean) * rsqrt(var + eps) * gamma + beta with the biased variance over the scene's sites.  Key order keeps a
// scene's rows contiguous: scene s is the rows seg[s] .. seg[s+1] (seg on the device; nothing here is read back by the host).
//
// The structure is sp_bn.hip's with the partials cut at scene boundaries; the thread layout, the partials of a row range, Chan's
// merge and the sum of all partials are the functions of table_moments.h that sp_bn.hip calls:
//   forward : stats (a workgroup per chunk of one scene: count, mean, M2 about ITS mean, two sweeps over rows that stay in cache)
//             -> apply (every workgroup merges the partials of ITS scene with Chan's formula in index order — deterministic — and
//             writes y; the first workgroup of a scene stores mean / invstd)
//   backward: partials of sum(g), sum(g xhat) per chunk -> dx = gamma invstd (g - mean_s(g) - xhat mean_s(g xhat))
//             -> dgamma / dbeta = the sums of ALL partials in index order.
// Chunks: a scene of n rows has ceil(n / rows) of them, so a launch needs at most ceil(N / rows) + nseg workgroups, a number the
// host knows without the scene sizes; workgroup b finds its scene by walking seg (nseg is a batch size: tens).  The stats chunks
// are large (about 64 per table: a workgroup of the second launch re-reads its scene's partials from L2, and 64 x C x 3 floats is
// what keeps that below the rows it streams), the apply chunks small (HBM streams over the whole chip).
#include "table_moments.h"

namespace vdetr {

static inline int inorm_round16(int r) { return (r + 15) / 16 * 16; }
static inline int inorm_stat_rows(int N) { const int r = (N + 63) / 64; return inorm_round16(r < 16 ? 16 : r); }
// an upper bound of ceil(N / inorm_stat_rows(N)) that grows with N (the count itself drops where the rows step up: 64 chunks at
// N = 1024, 33 at 1025): the rows are at least 16 and at least N / 64
static inline size_t inorm_chunk_bound(int N) {
  const long by16 = ((long)N + 15) / 16;
  return (size_t)(by16 < 64 ? by16 : 64);
}
static inline int inorm_apply_rows(int N) { int r = N / 1024; r = r < 16 ? 16 : r > 128 ? 128 : r; return inorm_round16(r); }

struct SpInParams {
  int N, C, nseg, rows_s, rows_a;
  float eps;
  const float* x;
  const int* seg;
  const float *gamma, *beta;
  float *y, *save_mean, *save_invstd;
  float* part;
};

struct SpInGrads {
  const float* dy;
  float *dx, *dgamma, *dbeta;
};

__device__ __forceinline__ int in_clamp(int v, int N) { return v < 0 ? 0 : v > N ? N : v; }

// workgroup b of a launch whose chunks hold `rows` rows: its scene and row range; false: b is past the last chunk
__device__ __forceinline__ bool in_locate(const SpInParams& P, int rows, int b, int& s, int& r0, int& r1) {
  int acc = 0;
  for (int q = 0; q < P.nseg; ++q) {
    const int a = in_clamp(P.seg[q], P.N), e = in_clamp(P.seg[q + 1], P.N);
    const int nb = e > a ? (e - a + rows - 1) / rows : 0;
    if (b < acc + nb) {
      s = q;
      r0 = a + (b - acc) * rows;
      r1 = min(e, r0 + rows);
      return true;
    }
    acc += nb;
  }
  return false;
}

// the stats chunks (partials) of scene s: first index and count; s = nseg: the total
__device__ __forceinline__ void in_parts(const SpInParams& P, int s, int& p0, int& np) {
  int acc = 0;
  np = 0;
  for (int q = 0; q < P.nseg && q <= s; ++q) {
    const int a = in_clamp(P.seg[q], P.N), e = in_clamp(P.seg[q + 1], P.N);
    const int nb = e > a ? (e - a + P.rows_s - 1) / P.rows_s : 0;
    if (q == s) { np = nb; break; }
    acc += nb;
  }
  p0 = acc;
}

// partial [chunk][3][C]: count, mean, M2
__global__ __launch_bounds__(256) void sp_in_stats_kernel(SpInParams P) {
  __shared__ f32x4 red[256];
  int s, r0, r1;
  if (!in_locate(P, P.rows_s, blockIdx.x, s, r0, r1)) return;  // (uniform)
  rows_to_moments(row_lanes(P.C), P.x, P.C, r0, r1, P.part, red);
}

__global__ __launch_bounds__(256) void sp_in_apply_kernel(SpInParams P) {
  __shared__ float agg[256][9];
  __shared__ f32x4 fin[2][256];
  int s, r0, r1;
  if (!in_locate(P, P.rows_a, blockIdx.x, s, r0, r1)) return;  // (uniform)
  int p0, np;
  in_parts(P, s, p0, np);
  const int tid = threadIdx.x;
  const auto [C4, c4, rs, rpi] = row_lanes(P.C);
  const bool act = rs < rpi;
  // thread (c4, rs) merges the partials rs, rs + rpi, ... of the scene; thread (c4, 0) then merges the rpi aggregates in order
  Moments a{0.f, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (act)
    for (int j = rs; j < np; j += rpi) moments_add_partial(a, P.part, p0 + j, P.C, c4);
  moments_store_lds(agg[tid], a);
  __syncthreads();
  if (rs == 0) {
    const int lim = min(rpi, np);
    for (int j = 1; j < lim; ++j) moments_add_lds(a, agg[j * C4 + c4]);
    const f32x4 var = a.m2 / a.n;
    f32x4 invstd;
#pragma unroll
    for (int e = 0; e < 4; ++e) invstd[e] = rsqrtf(var[e] + P.eps);
    fin[0][c4] = a.mu;
    fin[1][c4] = invstd;
    if (r0 == in_clamp(P.seg[s], P.N)) {  // the scene's first workgroup keeps the statistics for the backward
      reinterpret_cast<f32x4*>(P.save_mean + (size_t)s * P.C)[c4] = a.mu;
      reinterpret_cast<f32x4*>(P.save_invstd + (size_t)s * P.C)[c4] = invstd;
    }
  }
  __syncthreads();
  if (!act) return;
  const f32x4 mean = fin[0][c4], invstd = fin[1][c4];
  const f32x4 g = P.gamma ? reinterpret_cast<const f32x4*>(P.gamma)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 b = P.beta ? reinterpret_cast<const f32x4*>(P.beta)[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + rs; r < r1; r += rpi) {
    const size_t i = (size_t)r * C4 + c4;
    reinterpret_cast<f32x4*>(P.y)[i] = (reinterpret_cast<const f32x4*>(P.x)[i] - mean) * invstd * g + b;
  }
}

// partial [chunk][2][C]: sum g, sum g * xhat
__global__ __launch_bounds__(256) void sp_in_bwd_stats_kernel(SpInParams P, SpInGrads G) {
  __shared__ f32x4 red[2][256];
  int s, r0, r1;
  if (!in_locate(P, P.rows_s, blockIdx.x, s, r0, r1)) return;  // (uniform)
  const auto grad = [&](size_t i) { return reinterpret_cast<const f32x4*>(G.dy)[i]; };
  rows_to_grad_sums(row_lanes(P.C), P.x, P.C, r0, r1, P.save_mean + (size_t)s * P.C, P.save_invstd + (size_t)s * P.C, grad, P.part, red);
}

__global__ __launch_bounds__(256) void sp_in_bwd_apply_kernel(SpInParams P, SpInGrads G) {
  __shared__ f32x4 red[2][256];
  int s, r0, r1;
  if (!in_locate(P, P.rows_a, blockIdx.x, s, r0, r1)) return;  // (uniform)
  int p0, np;
  in_parts(P, s, p0, np);
  const int tid = threadIdx.x;
  const auto [C4, c4, rs, rpi] = row_lanes(P.C);
  const bool act = rs < rpi;
  f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = {0.f, 0.f, 0.f, 0.f};
  if (act)
    for (int j = rs; j < np; j += rpi) {
      const float* p = P.part + (size_t)(p0 + j) * 2 * P.C;
      sg += reinterpret_cast<const f32x4*>(p)[c4];
      sgx += reinterpret_cast<const f32x4*>(p + P.C)[c4];
    }
  red[0][tid] = sg;
  red[1][tid] = sgx;
  __syncthreads();
  if (!act) return;
  const int lim = min(rpi, np);
  f32x4 tg = {0.f, 0.f, 0.f, 0.f}, tgx = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < lim; ++j) { tg += red[0][j * C4 + c4]; tgx += red[1][j * C4 + c4]; }  // fixed order, every thread alike
  const f32x4 mean = reinterpret_cast<const f32x4*>(P.save_mean + (size_t)s * P.C)[c4];
  const f32x4 invstd = reinterpret_cast<const f32x4*>(P.save_invstd + (size_t)s * P.C)[c4];
  const f32x4 gam = P.gamma ? reinterpret_cast<const f32x4*>(P.gamma)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
  const float invn = 1.f / (float)(in_clamp(P.seg[s + 1], P.N) - in_clamp(P.seg[s], P.N));
  const f32x4 mg = tg * invn, mgx = tgx * invn, k = gam * invstd;
  for (int r = r0 + rs; r < r1; r += rpi) {
    const size_t i = (size_t)r * C4 + c4;
    const f32x4 g = reinterpret_cast<const f32x4*>(G.dy)[i];
    const f32x4 xh = (reinterpret_cast<const f32x4*>(P.x)[i] - mean) * invstd;
    reinterpret_cast<f32x4*>(G.dx)[i] = k * (g - mg - xh * mgx);
  }
}

// one workgroup per 4 channels: the sums of ALL partials (thread t: partials t, t + 256, ...; fixed tree) -> dgamma, dbeta
__global__ __launch_bounds__(256) void sp_in_bwd_params_kernel(SpInParams P, SpInGrads G) {
  __shared__ f32x4 red[2][4];
  int p0, np;
  in_parts(P, P.nseg, p0, np);  // p0 = the number of partials of all scenes
  const int c4 = blockIdx.x;
  partials_sum2(P.part, p0, P.C, c4, red, [&](const f32x4& sg, const f32x4& sgx) {
    if (G.dgamma) reinterpret_cast<f32x4*>(G.dgamma)[c4] = sgx;
    if (G.dbeta) reinterpret_cast<f32x4*>(G.dbeta)[c4] = sg;
  });
}

static int in_fill(const vdetr_sp_inorm_desc* d, SpInParams* P, const char* op) {
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  VDETR_REQUIRE(d->C > 0 && d->C % 4 == 0 && d->C <= 1024, "%s: C=%d must be a positive multiple of 4 and <= 1024", op, d->C);
  VDETR_REQUIRE(d->N >= 0, "%s: N=%d is negative", op, d->N);
  VDETR_REQUIRE(d->nseg >= 0, "%s: nseg=%d is negative", op, d->nseg);
  VDETR_REQUIRE_WORKSPACE_ALIGNED(op, "workspace", d->workspace, 16);
  P->N = d->N; P->C = d->C; P->nseg = d->nseg; P->eps = d->eps;
  P->rows_s = inorm_stat_rows(d->N); P->rows_a = inorm_apply_rows(d->N);
  P->x = d->x; P->seg = d->seg; P->gamma = d->gamma; P->beta = d->beta;
  P->y = d->y; P->save_mean = d->save_mean; P->save_invstd = d->save_invstd; P->part = (float*)d->workspace;
  return VDETR_OK;
}

}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_sp_inorm_workspace_bytes(int N, int C, int nseg) {
  if (N < 0) N = 0;
  if (nseg < 0) nseg = 0;
  if (C < 0) C = 0;
  return (inorm_chunk_bound(N) + (size_t)nseg + 1) * 3 * (size_t)C * sizeof(float);
}

extern "C" int vdetr_sp_inorm_fwd_f32(const vdetr_sp_inorm_desc* d, vdetr_stream_t stream) {
  SpInParams P;
  if (int e = in_fill(d, &P, "sp_inorm_fwd")) return e;
  if (d->N == 0 || d->nseg == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x, "sp_inorm_fwd: x is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->y, "sp_inorm_fwd: y is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->seg, "sp_inorm_fwd: seg is NULL with nseg=%d", d->nseg);
  VDETR_REQUIRE(d->save_mean && d->save_invstd, "sp_inorm_fwd: %s is NULL", d->save_mean ? "save_invstd" : "save_mean");
  VDETR_REQUIRE(d->workspace, "sp_inorm_fwd: workspace is NULL (vdetr_sp_inorm_workspace_bytes)");
  const int grid_s = ceil_div(d->N, P.rows_s) + d->nseg, grid_a = ceil_div(d->N, P.rows_a) + d->nseg;
  hipLaunchKernelGGL(sp_in_stats_kernel, dim3(grid_s), dim3(256), 0, (hipStream_t)stream, P);
  if (int e = check_launch("sp_inorm_stats")) return e;
  hipLaunchKernelGGL(sp_in_apply_kernel, dim3(grid_a), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_inorm_apply");
}

extern "C" int vdetr_sp_inorm_bwd_f32(const vdetr_sp_inorm_desc* d, const float* dy, float* dx, float* dgamma, float* dbeta,
                                      vdetr_stream_t stream) {
  SpInParams P;
  if (int e = in_fill(d, &P, "sp_inorm_bwd")) return e;
  if (d->N == 0 || d->nseg == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x, "sp_inorm_bwd: x is NULL with N=%d", d->N);
  VDETR_REQUIRE(dy, "sp_inorm_bwd: dy is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->seg, "sp_inorm_bwd: seg is NULL with nseg=%d", d->nseg);
  VDETR_REQUIRE(d->save_mean && d->save_invstd, "sp_inorm_bwd: %s is NULL", d->save_mean ? "save_invstd" : "save_mean");
  VDETR_REQUIRE(d->workspace, "sp_inorm_bwd: workspace is NULL (vdetr_sp_inorm_workspace_bytes)");
  SpInGrads G{dy, dx, dgamma, dbeta};
  const int grid_s = ceil_div(d->N, P.rows_s) + d->nseg, grid_a = ceil_div(d->N, P.rows_a) + d->nseg;
  hipLaunchKernelGGL(sp_in_bwd_stats_kernel, dim3(grid_s), dim3(256), 0, (hipStream_t)stream, P, G);
  if (int e = check_launch("sp_inorm_bwd_stats")) return e;
  if (dx) {
    hipLaunchKernelGGL(sp_in_bwd_apply_kernel, dim3(grid_a), dim3(256), 0, (hipStream_t)stream, P, G);
    if (int e = check_launch("sp_inorm_bwd_apply")) return e;
  }
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(sp_in_bwd_params_kernel, dim3(d->C / 4), dim3(256), 0, (hipStream_t)stream, P, G);
    if (int e = check_launch("sp_inorm_bwd_params")) return e;
  }
  return VDETR_OK;
}
