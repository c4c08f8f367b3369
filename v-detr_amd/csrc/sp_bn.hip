// sp_bn.hip — BatchNorm (+ residual) (+ ReLU / ELU) over the point-major feature table [N, C] of a sparse tensor, gfx950.
//
// Reference: ME.MinkowskiBatchNorm = nn.BatchNorm1d over all sites of the batch, followed by MinkowskiReLU / MinkowskiELU,
// and in the residual blocks by `out += residual; relu` (models/mink_resnet.py:38-84 via MinkowskiEngine's BasicBlock;
// models/model_vdetr.py:141-176).  ATen's channels-last statistics kernels take ~41 us per call on a [36k, 64] table (9 MB:
// 2 us of HBM time) and the block needs 4-6 launches; here
//   forward : stats partials (a workgroup per bn_rows(N) rows, 16 to 128: mean and sum of squared deviations from ITS mean, two
//             sweeps over rows that stay in cache) -> apply (every workgroup merges the partials with Chan's formula in a fixed order —
//             deterministic — and writes y = act(xhat * gamma + beta + residual); workgroup 0 also stores mean / invstd
//             and updates the running statistics)
//   backward: partials of sum(g), sum(g * xhat) with g = dy * act'(y) -> apply dx = gamma * invstd * (g - mean(g) -
//             xhat * mean(g xhat)), dresidual = g; workgroup 0 stores dgamma / dbeta.
// Pure HBM streams: x (and residual) read twice / once, y written once.
#include "bn_common.h"
#include "table_moments.h"

namespace vdetr {

constexpr int kBnRowsMin = 16, kBnRowsMax = 128;  // rows per workgroup: chosen so that a table gives >= ~1000 workgroups
static inline int bn_rows(int N) { int r = N / 1024; r = r < kBnRowsMin ? kBnRowsMin : r > kBnRowsMax ? kBnRowsMax : r; return (r + 15) / 16 * 16; }
// an upper bound of ceil(N / bn_rows(N)) that grows with N (the count itself drops where the rows step up: 1088 workgroups at
// N = 17407, 544 at 17408).  Rows of 16: ceil(N / 16) <= 1088; rows of 32 .. 112: N < (rows + 1) * 1024, so at most
// 1024 + ceil(1023 / rows) <= 1056 workgroups; rows of 128: ceil(N / 128).
static inline size_t bn_block_bound(int N) {
  const long by16 = ((long)N + 15) / 16, by128 = ((long)N + 127) / 128;
  const long low = by16 < 1088 ? by16 : 1088;
  return (size_t)(low > by128 ? low : by128);
}

// d act / d pre-activation from the OUTPUT y
__device__ __forceinline__ f32x4 bn_act_grad(f32x4 dy, f32x4 y, int act) {
  if (act == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dy[e] = y[e] > 0.f ? dy[e] : 0.f;
  } else if (act == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dy[e] = y[e] > 0.f ? dy[e] : dy[e] * (y[e] + 1.f);
  }
  return dy;
}

// thread layout and partials: table_moments.h.  A workgroup takes bn_rows(N) rows, 16 to 128.
// partial [nblk][3][C]: count, mean, M2   (forward)   /   [nblk][2][C]: sum g, sum g xhat   (backward)
__global__ __launch_bounds__(256) void sp_bn_stats_kernel(const float* __restrict__ x, int N, int C, int kBnRows, float* __restrict__ part) {
  __shared__ f32x4 red[256];
  const RowLanes L = row_lanes(C);
  const int r0 = blockIdx.x * kBnRows, r1 = min(N, r0 + kBnRows);
  rows_to_moments(L, x, C, r0, r1, part, red);
}

struct SpBnParams {
  int N, C, act, training, nblk, rows;
  float eps, momentum;
  const float *x, *gamma, *beta, *residual;
  float *running_mean, *running_var, *y, *save_mean, *save_invstd;
  float* part;
  float* sums;  // backward: [2][C] = sum g, sum g xhat (behind the partials in the workspace)
  long long* num_batches_tracked;
};

// one workgroup per 4 channels: thread t merges the partials t, t + 256, ... ; the 256 aggregates are merged in index order by
// a fixed tree through LDS (deterministic); thread 0 stores mean / invstd and updates the running statistics
__global__ __launch_bounds__(256) void sp_bn_finalize_kernel(SpBnParams P) {
  __shared__ float lds[4][9];
  const int c4 = blockIdx.x, tid = threadIdx.x;
  Moments a{0.f, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int b = tid; b < P.nblk; b += 256) moments_add_partial(a, P.part, b, P.C, c4);
  // fixed merge tree (deterministic): inside a wave through lane shuffles (no barrier), then the 4 wave aggregates through LDS.
  // (The first version merged all 256 aggregates through LDS: 8 levels, 16 barriers, 7.8 us for a few KB.)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float on = __shfl_down(a.n, off);
    f32x4 omu, om2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { omu[e] = __shfl_down(a.mu[e], off); om2[e] = __shfl_down(a.m2[e], off); }
    if ((tid & 63) < off) moments_add(a, on, omu, om2);
  }
  if ((tid & 63) == 0) moments_store_lds(lds[tid >> 6], a);
  __syncthreads();
  if (tid == 0) {
    for (int w2 = 1; w2 < 4; ++w2) moments_add_lds(a, lds[w2]);
  }
  if (tid == 0) {
    const f32x4 mean = a.mu, var = a.m2 / a.n;
    f32x4 invstd;
#pragma unroll
    for (int e = 0; e < 4; ++e) invstd[e] = rsqrtf(var[e] + P.eps);
    reinterpret_cast<f32x4*>(P.save_mean)[c4] = mean;
    reinterpret_cast<f32x4*>(P.save_invstd)[c4] = invstd;
    if (P.running_mean) {  // nn.BatchNorm1d: running = (1 - m) running + m stat, unbiased variance
      const float unb = a.n > 1.f ? a.n / (a.n - 1.f) : 1.f;
      f32x4* rm = reinterpret_cast<f32x4*>(P.running_mean) + c4;
      f32x4* rv = reinterpret_cast<f32x4*>(P.running_var) + c4;
      *rm = *rm * (1.f - P.momentum) + mean * P.momentum;
      *rv = *rv * (1.f - P.momentum) + var * (unb * P.momentum);
      if (c4 == 0 && P.num_batches_tracked) *P.num_batches_tracked += 1;
    }
  }
}

__global__ __launch_bounds__(256) void sp_bn_apply_kernel(SpBnParams P) {
  const auto [C4, c4, rs, rpi] = row_lanes(P.C);
  if (rs >= rpi) return;
  f32x4 mean, invstd;
  if (P.training) {  // left by sp_bn_finalize_kernel
    mean = reinterpret_cast<const f32x4*>(P.save_mean)[c4];
    invstd = reinterpret_cast<const f32x4*>(P.save_invstd)[c4];
  } else {
    mean = reinterpret_cast<const f32x4*>(P.running_mean)[c4];
    const f32x4 var = reinterpret_cast<const f32x4*>(P.running_var)[c4];
#pragma unroll
    for (int e = 0; e < 4; ++e) invstd[e] = rsqrtf(var[e] + P.eps);
    if (blockIdx.x == 0 && rs == 0 && P.save_mean) {  // what a backward pass in eval mode normalises with
      reinterpret_cast<f32x4*>(P.save_mean)[c4] = mean;
      reinterpret_cast<f32x4*>(P.save_invstd)[c4] = invstd;
    }
  }
  const f32x4 g = P.gamma ? reinterpret_cast<const f32x4*>(P.gamma)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 b = P.beta ? reinterpret_cast<const f32x4*>(P.beta)[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 scale = invstd * g, shift = b - mean * scale;
  const int r0 = blockIdx.x * P.rows, r1 = min(P.N, r0 + P.rows);
  for (int r = r0 + rs; r < r1; r += rpi) {
    const size_t i = (size_t)r * C4 + c4;
    f32x4 v = reinterpret_cast<const f32x4*>(P.x)[i] * scale + shift;
    if (P.residual) v += reinterpret_cast<const f32x4*>(P.residual)[i];
    reinterpret_cast<f32x4*>(P.y)[i] = bn_act(v, P.act);
  }
}

struct SpBnGrads {
  const float* dy;
  float *dx, *dres, *dgamma, *dbeta;
};

// partial [nblk][2][C]: sum g, sum g * xhat
__global__ __launch_bounds__(256) void sp_bn_bwd_stats_kernel(SpBnParams P, SpBnGrads G) {
  __shared__ f32x4 red[2][256];
  const RowLanes L = row_lanes(P.C);
  const int r0 = blockIdx.x * P.rows, r1 = min(P.N, r0 + P.rows);
  const auto grad = [&](size_t i) { return bn_act_grad(reinterpret_cast<const f32x4*>(G.dy)[i], reinterpret_cast<const f32x4*>(P.y)[i], P.act); };
  rows_to_grad_sums(L, P.x, P.C, r0, r1, P.save_mean, P.save_invstd, grad, P.part, red);
}

// one workgroup per 4 channels: sums of the partials (thread t: partials t, t + 256, ...; fixed tree) -> sums, dgamma, dbeta
__global__ __launch_bounds__(256) void sp_bn_bwd_finalize_kernel(SpBnParams P, SpBnGrads G) {
  __shared__ f32x4 red[2][4];
  const int c4 = blockIdx.x;
  partials_sum2(P.part, P.nblk, P.C, c4, red, [&](const f32x4& sg, const f32x4& sgx) {
    reinterpret_cast<f32x4*>(P.sums)[c4] = sg;
    reinterpret_cast<f32x4*>(P.sums + P.C)[c4] = sgx;
    if (G.dgamma) reinterpret_cast<f32x4*>(G.dgamma)[c4] = sgx;
    if (G.dbeta) reinterpret_cast<f32x4*>(G.dbeta)[c4] = sg;
  });
}

__global__ __launch_bounds__(256) void sp_bn_bwd_apply_kernel(SpBnParams P, SpBnGrads G) {
  const auto [C4, c4, rs, rpi] = row_lanes(P.C);
  if (rs >= rpi) return;
  const f32x4 sg = reinterpret_cast<const f32x4*>(P.sums)[c4], sgx = reinterpret_cast<const f32x4*>(P.sums + P.C)[c4];
  const f32x4 mean = reinterpret_cast<const f32x4*>(P.save_mean)[c4], invstd = reinterpret_cast<const f32x4*>(P.save_invstd)[c4];
  const f32x4 gam = P.gamma ? reinterpret_cast<const f32x4*>(P.gamma)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
  const float invn = 1.f / (float)P.N;
  const f32x4 mg = sg * invn, mgx = sgx * invn, k = gam * invstd;
  const int r0 = blockIdx.x * P.rows, r1 = min(P.N, r0 + P.rows);
  for (int r = r0 + rs; r < r1; r += rpi) {
    const size_t i = (size_t)r * C4 + c4;
    const f32x4 g = bn_act_grad(reinterpret_cast<const f32x4*>(G.dy)[i], reinterpret_cast<const f32x4*>(P.y)[i], P.act);
    if (G.dres) reinterpret_cast<f32x4*>(G.dres)[i] = g;
    if (G.dx) {
      const f32x4 xh = (reinterpret_cast<const f32x4*>(P.x)[i] - mean) * invstd;
      reinterpret_cast<f32x4*>(G.dx)[i] = P.training ? k * (g - mg - xh * mgx) : k * g;
    }
  }
}

static int fill(const vdetr_spbn_desc* d, SpBnParams* P, const char* op) {
  VDETR_REQUIRE(d && d->N >= 0 && d->C > 0, "%s: bad descriptor", op);
  VDETR_REQUIRE(d->C % 4 == 0 && d->C <= 1024, "%s: C=%d must be a multiple of 4 and <= 1024", op, d->C);
  VDETR_REQUIRE(d->act >= 0 && d->act <= 2, "%s: act %d", op, d->act);
  VDETR_REQUIRE_WORKSPACE_ALIGNED(op, "workspace", d->workspace, 16);
  P->N = d->N; P->C = d->C; P->act = d->act; P->training = d->training; P->rows = bn_rows(d->N); P->nblk = ceil_div(d->N, P->rows);
  P->eps = d->eps; P->momentum = d->momentum;
  P->x = d->x; P->gamma = d->gamma; P->beta = d->beta; P->residual = d->residual;
  P->running_mean = d->running_mean; P->running_var = d->running_var; P->y = d->y;
  P->save_mean = d->save_mean; P->save_invstd = d->save_invstd; P->part = (float*)d->workspace;
  P->sums = P->part ? P->part + (size_t)P->nblk * 3 * d->C : nullptr;
  P->num_batches_tracked = (long long*)d->num_batches_tracked;
  return VDETR_OK;
}

}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_sp_bn_workspace_bytes(int N, int C) {
  if (C <= 0) return 0;
  return (bn_block_bound(N > 0 ? N : 1) * 3 + 2) * (size_t)C * sizeof(float);  // partials + the backward's two sums
}

extern "C" int vdetr_sp_bn_act_fwd_f32(const vdetr_spbn_desc* d, vdetr_stream_t stream) {
  SpBnParams P;
  if (int e = fill(d, &P, "sp_bn_act_fwd")) return e;
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x && d->y, "sp_bn_act_fwd: null pointer");
  VDETR_REQUIRE(d->training ? (d->workspace && d->save_mean && d->save_invstd) : (d->running_mean && d->running_var),
                "sp_bn_act_fwd: %s", d->training ? "training needs workspace, save_mean, save_invstd" : "eval needs running statistics");
  if (d->training) {
    hipLaunchKernelGGL(sp_bn_stats_kernel, dim3(P.nblk), dim3(256), 0, (hipStream_t)stream, d->x, d->N, d->C, P.rows, P.part);
    if (int e = check_launch("sp_bn_stats")) return e;
    hipLaunchKernelGGL(sp_bn_finalize_kernel, dim3(d->C / 4), dim3(256), 0, (hipStream_t)stream, P);
    if (int e = check_launch("sp_bn_finalize")) return e;
  }
  hipLaunchKernelGGL(sp_bn_apply_kernel, dim3(P.nblk), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_bn_apply");
}

extern "C" int vdetr_sp_bn_act_bwd_f32(const vdetr_spbn_desc* d, const float* dy, float* dx, float* dresidual, float* dgamma,
                                       float* dbeta, vdetr_stream_t stream) {
  SpBnParams P;
  if (int e = fill(d, &P, "sp_bn_act_bwd")) return e;
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x && d->y && dy && d->workspace && d->save_mean && d->save_invstd, "sp_bn_act_bwd: null pointer");
  SpBnGrads G{dy, dx, dresidual, dgamma, dbeta};
  hipLaunchKernelGGL(sp_bn_bwd_stats_kernel, dim3(P.nblk), dim3(256), 0, (hipStream_t)stream, P, G);
  if (int e = check_launch("sp_bn_bwd_stats")) return e;
  hipLaunchKernelGGL(sp_bn_bwd_finalize_kernel, dim3(d->C / 4), dim3(256), 0, (hipStream_t)stream, P, G);
  if (int e = check_launch("sp_bn_bwd_finalize")) return e;
  hipLaunchKernelGGL(sp_bn_bwd_apply_kernel, dim3(P.nblk), dim3(256), 0, (hipStream_t)stream, P, G);
  return check_launch("sp_bn_bwd_apply");
}
