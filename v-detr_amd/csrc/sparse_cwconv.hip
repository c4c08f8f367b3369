// sparse_cwconv.hip — channelwise (depthwise) convolution of a sparse tensor over a kernel map, gfx950.
//
// Reference: ME.MinkowskiChannelwiseConvolution, the depthwise layer of the module library around the backbone.  MinkowskiEngine
// is un-vendored; what is restated is the definition over the occupied neighbours N(u) = {k : 0 <= nbr[k][u] < nin} of an output
// site u, with ONE weight per (offset, channel), W [K, C], and no mixing across channels:
//   forward  y[u][c]  = (sum_{k in N(u)} W[k][c] * x[nbr[k][u]][c]) + b[c]     the sum starts at +0, one fmaf per term in ascending
//                                                                             k; the bias (optional) is added last
//   dgrad    dx[i][c] = sum_k W[k][c] * dy[inv[k][i]][c]                       the same body through the inverse map, ascending k
//   wgrad    dW[k][c] = sum_{u : k in N(u)} x[nbr[k][u]][c] * dy[u][c]         db[c] = sum_u dy[u][c]
// An empty N(u) gives b[c] (exact +0 without a bias); an input row nobody reads gets dx = +0; an offset without a pair gets a dW
// row of +0.  No float atomics, no memset, no host read: every sum has a fixed order and two runs agree bit for bit.
//
// Forward and dgrad are ONE kernel (sp_cwconv_gather_kernel) with the map and the row counts swapped, shaped as
// sp_pool_fwd_kernel: a thread owns one destination row's channel quad, map entries are fetched eight offsets at a time and
// their rows requested together.  The weight quad W[k][c4] comes through the cache, not LDS: its address does not depend on the
// map, so it is requested beside the map entries and is off the index -> row chain; and a workgroup's 256 threads cover
// 256 / C4 rows, so a staged copy would be read 4 (C = 256) to 16 (C = 64) times per element after costing the same global read
// plus a barrier, and K * C * 4 bytes (508 KB at 127 x 1024) does not fit LDS in general.
//
// wgrad is two launches.  sp_cwconv_wgrad_part_kernel: grid (chunks, channel slabs).  A workgroup owns vdetr_sp_cwconv_chunk_rows
// output rows and a slab of S <= 16 channel quads; its threads are S quads x R = 256 / S row lanes.  Offsets go four at a time
// (offset K is the bias row: x == 1, so the sweep that reads dy leaves db too): a thread walks the rows u0 + r, u0 + r + R, ...
// of its lane in ascending order with four f32x4 accumulators, the R lanes are joined left to right pairwise in LDS (16 KB), and
// lane 0 writes the chunk's partial [K + 1, C].  dy of the chunk is re-read once per offset group from the cache (80 rows x 64
// channels = 20 KB).  Registers: 4 accumulators + 4 rows + dy = 36 VGPRs of payload; no array indexed by a runtime k.
// sp_cwconv_wgrad_fold_kernel: 16 quads x 16 runs per workgroup; a run adds its contiguous chunks in ascending order, the runs
// are joined left to right pairwise.  The order depends on (nout, K, C) alone.
#include "common.h"

namespace vdetr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCwGroup = 8;      // offsets per round of the gather kernel
constexpr int kCwOffsets = 4;    // offsets per round of the weight-gradient sweep
constexpr int kCwMinRows = 64;   // rows of a chunk, at least
constexpr int kCwMaxChunks = 512;
constexpr int kCwFoldRuns = 16;

static inline int cw_chunk_rows(int nout) {
  const long r = ((long)nout + kCwMaxChunks - 1) / kCwMaxChunks;
  const long r16 = (r + 15) / 16 * 16;
  return (int)(r16 < kCwMinRows ? kCwMinRows : r16);
}
// an upper bound of ceil(nout / cw_chunk_rows(nout)) that grows with nout (the count itself drops where the rows step up)
static inline size_t cw_chunk_bound(int nout) {
  const long by_row = ((long)nout + kCwMinRows - 1) / kCwMinRows;
  return (size_t)(by_row < kCwMaxChunks ? by_row : kCwMaxChunks);
}

__device__ inline f32x4 cw_fma(f32x4 a, f32x4 b, f32x4 c) {
  f32x4 r;
  r[0] = fmaf(a[0], b[0], c[0]); r[1] = fmaf(a[1], b[1], c[1]); r[2] = fmaf(a[2], b[2], c[2]); r[3] = fmaf(a[3], b[3], c[3]);
  return r;
}

// dst[u] = (sum over the present k of w[k] * src[map[k][u]]) + bias: the forward (map = nbr, dst = y) and, with the inverse map
// and the row counts swapped, the input gradient (map = inv, src = dy, dst = dx, no bias)
struct SpCwGather {
  int K, ndst, nsrc, C4;
  const float* src;
  const int* map;
  const float* w;
  const float* bias;
  float* dst;
};

__global__ __launch_bounds__(256) void sp_cwconv_gather_kernel(SpCwGather P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.ndst * P.C4) return;
  const int c4 = (int)(t % P.C4);
  const int u = (int)(t / P.C4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc = zero;
  for (int k0 = 0; k0 < P.K; k0 += kCwGroup) {
    int i[kCwGroup];
    f32x4 w[kCwGroup];
#pragma unroll
    for (int j = 0; j < kCwGroup; ++j) {
      i[j] = -1;
      w[j] = zero;
      if (k0 + j < P.K) {
        i[j] = P.map[(size_t)(k0 + j) * P.ndst + u];
        w[j] = reinterpret_cast<const f32x4*>(P.w)[(size_t)(k0 + j) * P.C4 + c4];
      }
      if (i[j] >= P.nsrc) i[j] = -1;
    }
    f32x4 v[kCwGroup];
#pragma unroll
    for (int j = 0; j < kCwGroup; ++j) {
      v[j] = zero;
      if (i[j] >= 0) v[j] = reinterpret_cast<const f32x4*>(P.src)[(size_t)i[j] * P.C4 + c4];
    }
#pragma unroll
    for (int j = 0; j < kCwGroup; ++j)
      if (i[j] >= 0) acc = cw_fma(w[j], v[j], acc);
  }
  if (P.bias) acc += reinterpret_cast<const f32x4*>(P.bias)[c4];
  reinterpret_cast<f32x4*>(P.dst)[t] = acc;
}

struct SpCwWgrad {
  int K, nout, nin, C4, rows, S, k_begin;  // k_begin: 0, or K when only db is wanted (the bias row alone)
  const float* x;
  const int* nbr;
  const float* dy;
  float* part;  // [chunks][K + 1][C]: row K is the bias partial
};

// joins the R = 256 / S row lanes of red[.][lane * S + q] left to right pairwise: (0 + 1) + (2 + 3), ...; the result is in lane 0
template <int N>
__device__ inline void cw_join_lanes(f32x4 (*red)[256], int S, int lanes, int r) {
  for (int stride = 1; stride < lanes; stride *= 2) {
    if (r % (2 * stride) == 0 && r + stride < lanes) {
#pragma unroll
      for (int j = 0; j < N; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + stride * S];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void sp_cwconv_wgrad_part_kernel(SpCwWgrad P) {
  __shared__ f32x4 red[kCwOffsets][256];
  const int S = P.S, R = 256 / S;
  const int q = threadIdx.x % S, r = threadIdx.x / S;
  const int c4 = blockIdx.y * S + q;
  const bool live = c4 < P.C4;
  const int u0 = blockIdx.x * P.rows;
  const int u1 = u0 + P.rows < P.nout ? u0 + P.rows : P.nout;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 one = {1.f, 1.f, 1.f, 1.f};
  for (int k0 = P.k_begin; k0 <= P.K; k0 += kCwOffsets) {
    f32x4 acc[kCwOffsets];
#pragma unroll
    for (int j = 0; j < kCwOffsets; ++j) acc[j] = zero;
    if (live) {
      for (int u = u0 + r; u < u1; u += R) {
        const f32x4 g = reinterpret_cast<const f32x4*>(P.dy)[(size_t)u * P.C4 + c4];
        int i[kCwOffsets];
#pragma unroll
        for (int j = 0; j < kCwOffsets; ++j) {
          i[j] = k0 + j < P.K ? P.nbr[(size_t)(k0 + j) * P.nout + u] : -1;
          if (i[j] >= P.nin) i[j] = -1;
        }
        f32x4 v[kCwOffsets];
        bool has[kCwOffsets];
#pragma unroll
        for (int j = 0; j < kCwOffsets; ++j) {
          has[j] = i[j] >= 0 || k0 + j == P.K;
          v[j] = one;  // (the bias row)
          if (i[j] >= 0) v[j] = reinterpret_cast<const f32x4*>(P.x)[(size_t)i[j] * P.C4 + c4];
        }
#pragma unroll
        for (int j = 0; j < kCwOffsets; ++j)
          if (has[j]) acc[j] = cw_fma(v[j], g, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kCwOffsets; ++j) red[j][threadIdx.x] = acc[j];
    __syncthreads();
    cw_join_lanes<kCwOffsets>(red, S, R, r);
    if (r == 0 && live) {
#pragma unroll
      for (int j = 0; j < kCwOffsets; ++j)
        if (k0 + j <= P.K)
          reinterpret_cast<f32x4*>(P.part)[((size_t)blockIdx.x * (P.K + 1) + (k0 + j)) * P.C4 + c4] = red[j][q];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void sp_cwconv_wgrad_fold_kernel(int K, int C4, int chunks, const float* part, float* dw, float* db) {
  __shared__ f32x4 red[1][256];
  constexpr int Q = 256 / kCwFoldRuns;
  const int q = threadIdx.x % Q, s = threadIdx.x / Q;
  const int total = (K + 1) * C4;
  const int e = blockIdx.x * Q + q;  // the quad e of a partial [K + 1, C]
  const bool live = e < total && (dw || e >= K * C4);  // (without dw only the bias rows of the partials were written)
  const int per = (chunks + kCwFoldRuns - 1) / kCwFoldRuns;
  const int c0 = s * per;
  const int c1 = c0 + per < chunks ? c0 + per : chunks;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (live)
    for (int c = c0; c < c1; ++c) acc += reinterpret_cast<const f32x4*>(part)[(size_t)c * total + e];
  red[0][threadIdx.x] = acc;
  __syncthreads();
  cw_join_lanes<1>(red, Q, kCwFoldRuns, s);
  if (s == 0 && live) {
    if (e < K * C4) reinterpret_cast<f32x4*>(dw)[e] = red[0][q];
    else if (db) reinterpret_cast<f32x4*>(db)[e - K * C4] = red[0][q];
  }
}

static int cw_check(const vdetr_sp_cwconv_desc* d, const char* op) {
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  VDETR_REQUIRE(d->C >= 4 && d->C <= 1024 && d->C % 4 == 0, "%s: C=%d must be a multiple of 4 in 4 .. 1024 (float4 rows)", op, d->C);
  VDETR_REQUIRE(d->K >= 1 && d->K <= 127, "%s: K=%d must be in 1 .. 127 (the kernel maps' range)", op, d->K);
  VDETR_REQUIRE(d->nout >= 0, "%s: nout=%d is negative", op, d->nout);
  VDETR_REQUIRE(d->nin >= 0, "%s: nin=%d is negative", op, d->nin);
  return VDETR_OK;
}

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_sp_cwconv_chunk_rows(int nout) { return cw_chunk_rows(nout < 0 ? 0 : nout); }

extern "C" size_t vdetr_sp_cwconv_workspace_bytes(int K, int nout, int C) {
  if (K < 1 || K > 127 || C < 4 || C > 1024 || C % 4 || nout < 0) return 0;
  return cw_chunk_bound(nout) * (size_t)(K + 1) * (size_t)C * sizeof(float);
}

extern "C" int vdetr_sp_cwconv_fwd_f32(const vdetr_sp_cwconv_desc* d, vdetr_stream_t stream) {
  const char* op = "sp_cwconv_fwd";
  if (int e = cw_check(d, op)) return e;
  if (d->nout == 0) return VDETR_OK;
  VDETR_REQUIRE(d->nbr, "%s: nbr is NULL with nout=%d", op, d->nout);
  VDETR_REQUIRE(d->w, "%s: w is NULL with K=%d", op, d->K);
  VDETR_REQUIRE(d->y, "%s: y is NULL with nout=%d", op, d->nout);
  VDETR_REQUIRE(d->x || d->nin == 0, "%s: x is NULL with nin=%d", op, d->nin);
  const long long blocks = ((long long)d->nout * (d->C / 4) + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "%s: nout=%d x C=%d is more than one launch covers", op, d->nout, d->C);
  SpCwGather P{d->K, d->nout, d->nin, d->C / 4, d->x, d->nbr, d->w, d->bias, d->y};
  hipLaunchKernelGGL(sp_cwconv_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch(op);
}

extern "C" int vdetr_sp_cwconv_dgrad_f32(const vdetr_sp_cwconv_desc* d, const int32_t* inv, const float* dy, float* dx,
                                         vdetr_stream_t stream) {
  const char* op = "sp_cwconv_dgrad";
  if (int e = cw_check(d, op)) return e;
  if (d->nin == 0) return VDETR_OK;
  VDETR_REQUIRE(inv, "%s: inv is NULL with nin=%d", op, d->nin);
  VDETR_REQUIRE(d->w, "%s: w is NULL with K=%d", op, d->K);
  VDETR_REQUIRE(dx, "%s: dx is NULL with nin=%d", op, d->nin);
  VDETR_REQUIRE(dy || d->nout == 0, "%s: dy is NULL with nout=%d", op, d->nout);
  const long long blocks = ((long long)d->nin * (d->C / 4) + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "%s: nin=%d x C=%d is more than one launch covers", op, d->nin, d->C);
  // (nout == 0: every inverse entry counts as absent and dx is written as zeros)
  SpCwGather P{d->K, d->nin, d->nout, d->C / 4, dy, inv, d->w, nullptr, dx};
  hipLaunchKernelGGL(sp_cwconv_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch(op);
}

extern "C" int vdetr_sp_cwconv_wgrad_f32(const vdetr_sp_cwconv_desc* d, const float* dy, float* dw, float* db, vdetr_stream_t stream) {
  const char* op = "sp_cwconv_wgrad";
  if (int e = cw_check(d, op)) return e;
  VDETR_REQUIRE(dw || db, "%s: dw is NULL and db is NULL (one of them is wanted)", op);
  VDETR_REQUIRE_WORKSPACE_ALIGNED(op, "workspace", d->workspace, 16);
  const int C4 = d->C / 4;
  const int rows = cw_chunk_rows(d->nout);
  const int chunks = ceil_div(d->nout, rows);
  if (d->nout > 0) {
    VDETR_REQUIRE(dy, "%s: dy is NULL with nout=%d", op, d->nout);
    VDETR_REQUIRE(d->nbr, "%s: nbr is NULL with nout=%d", op, d->nout);
    VDETR_REQUIRE(d->x || d->nin == 0, "%s: x is NULL with nin=%d", op, d->nin);
    VDETR_REQUIRE(d->workspace, "%s: workspace is NULL (vdetr_sp_cwconv_workspace_bytes)", op);
    int S = 1;
    while (S < C4 && S < 16) S *= 2;
    SpCwWgrad P{d->K, d->nout, d->nin, C4, rows, S, dw ? 0 : d->K, d->x, d->nbr, dy, (float*)d->workspace};
    hipLaunchKernelGGL(sp_cwconv_wgrad_part_kernel, dim3(chunks, ceil_div(C4, S)), dim3(256), 0, (hipStream_t)stream, P);
    if (int e = check_launch("sp_cwconv_wgrad_part")) return e;
  }
  // (nout == 0: no chunk, and the fold writes zeros)
  hipLaunchKernelGGL(sp_cwconv_wgrad_fold_kernel, dim3(ceil_div((long)(d->K + 1) * C4, 256 / kCwFoldRuns)), dim3(256), 0,
                     (hipStream_t)stream, d->K, C4, chunks, (const float*)d->workspace, dw, db);
  return check_launch("sp_cwconv_wgrad_fold");
}
