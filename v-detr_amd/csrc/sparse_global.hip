// sparse_global.hip — a sparse tensor's table [N, C] against one row per scene, gfx950: global pooling (sum / avg / max),
// broadcast (add / mul / cat) and the squeeze-excite gate of the inference form.
//
// Key order keeps a scene's rows contiguous: scene s is the rows seg[s] .. seg[s+1], seg [nseg + 1] i32 on the device (values
// clamped to [0, N]); nothing here is read back by the host, nothing uses a float atomic, every sum has a fixed order.
// The structure is sp_inorm.hip's: chunks are cut at scene boundaries, a scene of n rows has ceil(n / rows) of them, so a launch
// needs at most ceil(N / rows) + nseg workgroups, a number the host knows without the scene sizes; workgroup b finds its scene by
// walking seg (nseg is a batch size: tens).
//   pooling forward  : partials per chunk (large chunks, about 64 per table) -> a workgroup per scene folds its scene's partials
//                      in ascending chunk order (a second launch, not a "last workgroup" ticket: README round 6)
//   pooling backward : one streaming launch (small chunks); every element of dx is written
//   broadcast forward: one streaming launch; a workgroup's rows belong to one scene, its g row is read once per lane
//   broadcast backward: the sweep that writes dx also leaves the chunk partials of dg (dy is read once) -> the fold above
//   SE gate          : the pooling partials, then the fold of an average pooling that goes on, in the scene's workgroup, to
//                      gate = sigmoid(W2 relu(W1 p + b1) + b2)
// Thread layout: a lane owns four channels (a float4) and walks rows; table_moments.h's RowLanes where C <= 1024, and the same
// layout with a loop over column groups where a concatenated row is wider than 256 float4.
#include <limits.h>

#include "table_moments.h"

namespace vdetr {

static inline int sg_round16(int r) { return (r + 15) / 16 * 16; }
// the partial chunks: about 64 per table (a scene's fold re-reads 64 x C floats from L2), never below 16 rows
static inline int sg_chunk_rows(int N) { const int r = (int)(((long)N + 63) / 64); return sg_round16(r < 16 ? 16 : r); }
// the streaming chunks: about 1024 per table, 16 .. 128 rows
static inline int sg_stream_rows(int N) { int r = N / 1024; r = r < 16 ? 16 : r > 128 ? 128 : r; return sg_round16(r); }
// an upper bound of ceil(N / sg_chunk_rows(N)) that grows with N (the chunk count itself does not: it drops where the rows step up)
static inline size_t sg_chunk_bound(int N, int nseg) {
  const long byrow = ((long)N + 15) / 16;
  return (size_t)(byrow < 64 ? byrow : 64) + (size_t)nseg;
}

struct SgSeg {
  int N, nseg;
  const int* seg;
};

__device__ __forceinline__ int sg_clamp(int v, int N) { return v < 0 ? 0 : v > N ? N : v; }

// workgroup b of a launch whose chunks hold `rows` rows: its scene and row range; false: b is past the last chunk
__device__ __forceinline__ bool sg_locate(const SgSeg& S, int rows, int b, int& s, int& r0, int& r1) {
  int acc = 0;
  for (int q = 0; q < S.nseg; ++q) {
    const int a = sg_clamp(S.seg[q], S.N), e = sg_clamp(S.seg[q + 1], S.N);
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

// the chunks of `rows` rows of scene s: first index and count, and the scene's row count
__device__ __forceinline__ void sg_parts(const SgSeg& S, int rows, int s, int& p0, int& np, int& n) {
  int acc = 0;
  np = 0;
  n = 0;
  for (int q = 0; q <= s; ++q) {
    const int a = sg_clamp(S.seg[q], S.N), e = sg_clamp(S.seg[q + 1], S.N);
    const int nb = e > a ? (e - a + rows - 1) / rows : 0;
    if (q == s) { np = nb; n = e > a ? e - a : 0; break; }
    acc += nb;
  }
  p0 = acc;
}

// np.max / np.argmax of a column, as a merge of (value, row) pairs in any order: a NaN beats every number, among NaNs and among
// equal numbers the lower row wins.  From (-inf, INT_MAX): a column of -inf ends at its first row.
__device__ __forceinline__ void sg_max_merge(float& v, int& r, float u, int q) {
  const bool nu = u != u, nv = v != v;
  if (nu ? (!nv || q < r) : (!nv && (u > v || (u == v && q < r)))) { v = u; r = q; }
}

struct SgPoolParams {
  SgSeg S;
  int C, mode, rows_p, rows_s;
  const float* x;
  float* y;
  int* arg;
  float* part;  // [chunks][C] sums or maxima
  int* parg;    // [chunks][C] rows of the maxima
};

// rows r0 .. r1 of x, the live lanes' own sums in `a` -> the workgroup's sum in the rs == 0 lanes (fixed order); ends without a barrier
__device__ __forceinline__ f32x4 sg_rows_sum(const RowLanes& L, f32x4 a, f32x4 (&red)[256]) {
  red[threadIdx.x] = a;
  __syncthreads();
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
  if (L.rs == 0)
    for (int j = 0; j < L.rpi; ++j) t += red[j * L.C4 + L.c4];
  return t;
}

__global__ __launch_bounds__(256) void sg_pool_sum_part_kernel(SgPoolParams P) {
  __shared__ f32x4 red[256];
  int s, r0, r1;
  if (!sg_locate(P.S, P.rows_p, blockIdx.x, s, r0, r1)) return;  // (uniform)
  const RowLanes L = row_lanes(P.C);
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (L.live())
    for (int r = r0 + L.rs; r < r1; r += L.rpi) a += reinterpret_cast<const f32x4*>(P.x)[(size_t)r * L.C4 + L.c4];
  const f32x4 t = sg_rows_sum(L, a, red);
  if (L.rs == 0) reinterpret_cast<f32x4*>(P.part + (size_t)blockIdx.x * P.C)[L.c4] = t;
}

__global__ __launch_bounds__(256) void sg_pool_max_part_kernel(SgPoolParams P) {
  __shared__ f32x4 redv[256];
  __shared__ int redr[256][4];
  int s, r0, r1;
  if (!sg_locate(P.S, P.rows_p, blockIdx.x, s, r0, r1)) return;  // (uniform)
  const RowLanes L = row_lanes(P.C);
  const int tid = threadIdx.x;
  float v[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int w[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  if (L.live())
    for (int r = r0 + L.rs; r < r1; r += L.rpi) {
      const f32x4 u = reinterpret_cast<const f32x4*>(P.x)[(size_t)r * L.C4 + L.c4];
#pragma unroll
      for (int e = 0; e < 4; ++e) sg_max_merge(v[e], w[e], u[e], r);
    }
  redv[tid] = f32x4{v[0], v[1], v[2], v[3]};
#pragma unroll
  for (int e = 0; e < 4; ++e) redr[tid][e] = w[e];
  __syncthreads();
  if (L.rs != 0) return;
  for (int j = 1; j < L.rpi; ++j) {
    const f32x4 u = redv[j * L.C4 + L.c4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sg_max_merge(v[e], w[e], u[e], redr[j * L.C4 + L.c4][e]);
  }
  reinterpret_cast<f32x4*>(P.part + (size_t)blockIdx.x * P.C)[L.c4] = f32x4{v[0], v[1], v[2], v[3]};
  reinterpret_cast<int4*>(P.parg + (size_t)blockIdx.x * P.C)[L.c4] = make_int4(w[0], w[1], w[2], w[3]);
}

// the sum of scene s's partials [np][C] in ascending chunk order: lane (c4, rs) adds the partials rs, rs + rpi, ..., the rs == 0
// lanes then add the rpi lane sums in order.  Every thread of the workgroup calls; the result is in the rs == 0 lanes.
__device__ __forceinline__ f32x4 sg_fold_sum(const RowLanes& L, const float* part, int C, int p0, int np, f32x4 (&red)[256]) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (L.live())
    for (int j = L.rs; j < np; j += L.rpi) a += reinterpret_cast<const f32x4*>(part + (size_t)(p0 + j) * C)[L.c4];
  return sg_rows_sum(L, a, red);
}

// one workgroup per scene: y[s] = the fold of the scene's partials (sum; avg: times 1 / n; a scene without rows: 0)
__global__ __launch_bounds__(256) void sg_fold_sum_kernel(SgSeg S, int C, int rows, int avg, const float* part, float* y) {
  __shared__ f32x4 red[256];
  const int s = blockIdx.x;
  int p0, np, n;
  sg_parts(S, rows, s, p0, np, n);
  const RowLanes L = row_lanes(C);
  f32x4 t = sg_fold_sum(L, part, C, p0, np, red);
  if (L.rs != 0) return;
  if (avg && n > 0) t = t * (1.0f / (float)n);
  reinterpret_cast<f32x4*>(y + (size_t)s * C)[L.c4] = t;
}

__global__ __launch_bounds__(256) void sg_fold_max_kernel(SgPoolParams P) {
  __shared__ f32x4 redv[256];
  __shared__ int redr[256][4];
  const int s = blockIdx.x, tid = threadIdx.x;
  int p0, np, n;
  sg_parts(P.S, P.rows_p, s, p0, np, n);
  const RowLanes L = row_lanes(P.C);
  float v[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int w[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  if (L.live())
    for (int j = L.rs; j < np; j += L.rpi) {
      const f32x4 u = reinterpret_cast<const f32x4*>(P.part + (size_t)(p0 + j) * P.C)[L.c4];
      const int4 q = reinterpret_cast<const int4*>(P.parg + (size_t)(p0 + j) * P.C)[L.c4];
      sg_max_merge(v[0], w[0], u[0], q.x);
      sg_max_merge(v[1], w[1], u[1], q.y);
      sg_max_merge(v[2], w[2], u[2], q.z);
      sg_max_merge(v[3], w[3], u[3], q.w);
    }
  redv[tid] = f32x4{v[0], v[1], v[2], v[3]};
#pragma unroll
  for (int e = 0; e < 4; ++e) redr[tid][e] = w[e];
  __syncthreads();
  if (L.rs != 0) return;
  const int lim = min(L.rpi, np);
  for (int j = 1; j < lim; ++j) {
    const f32x4 u = redv[j * L.C4 + L.c4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sg_max_merge(v[e], w[e], u[e], redr[j * L.C4 + L.c4][e]);
  }
  if (n == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = 0.f; w[e] = -1; }
  }
  reinterpret_cast<f32x4*>(P.y + (size_t)s * P.C)[L.c4] = f32x4{v[0], v[1], v[2], v[3]};
  reinterpret_cast<int4*>(P.arg + (size_t)s * P.C)[L.c4] = make_int4(w[0], w[1], w[2], w[3]);
}

// dx [N, C] from dy [nseg, C]: sum: dy[s]; avg: dy[s] * (1 / n); max: dy[s, c] where arg[s, c] is this row, else +0
__global__ __launch_bounds__(256) void sg_pool_bwd_kernel(SgPoolParams P, const float* dy, float* dx) {
  int s, r0, r1;
  if (!sg_locate(P.S, P.rows_s, blockIdx.x, s, r0, r1)) return;  // (uniform)
  const RowLanes L = row_lanes(P.C);
  if (!L.live()) return;
  f32x4 g = reinterpret_cast<const f32x4*>(dy + (size_t)s * P.C)[L.c4];
  if (P.mode == VDETR_POOL_AVG) {
    const int n = sg_clamp(P.S.seg[s + 1], P.S.N) - sg_clamp(P.S.seg[s], P.S.N);
    g = g * (1.0f / (float)n);
  }
  if (P.mode != VDETR_POOL_MAX) {
    for (int r = r0 + L.rs; r < r1; r += L.rpi) reinterpret_cast<f32x4*>(dx)[(size_t)r * L.C4 + L.c4] = g;
    return;
  }
  const int4 a = reinterpret_cast<const int4*>(P.arg + (size_t)s * P.C)[L.c4];
  for (int r = r0 + L.rs; r < r1; r += L.rpi)
    reinterpret_cast<f32x4*>(dx)[(size_t)r * L.C4 + L.c4] =
        f32x4{a.x == r ? g[0] : 0.f, a.y == r ? g[1] : 0.f, a.z == r ? g[2] : 0.f, a.w == r ? g[3] : 0.f};
}

// ---- broadcast -------------------------------------------------------------------------------------------------------------------
struct SgBcastParams {
  SgSeg S;
  int Cx, Cg, mode, relu, rows;
  const float *x, *g, *residual;
  float* y;
  float* part;  // backward: [chunks][Cg]
};

// the lanes of a row of W4 float4 that may be wider than the workgroup: column groups of `w` lanes, rows rs, rs + rpi, ...
struct WideLanes {
  int w, c, rs, rpi;
  __device__ __forceinline__ bool live() const { return rs < rpi; }
};
__device__ __forceinline__ WideLanes wide_lanes(int W4) {
  const int w = W4 < 256 ? W4 : 256, tid = threadIdx.x;
  return WideLanes{w, tid % w, tid / w, 256 / w};
}

__device__ __forceinline__ f32x4 sg_relu4(const f32x4& v) {
  return f32x4{v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f, v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f};
}

__global__ __launch_bounds__(256) void sg_bcast_fwd_kernel(SgBcastParams P) {
  int s, r0, r1;
  if (!sg_locate(P.S, P.rows, blockIdx.x, s, r0, r1)) return;  // (uniform)
  const int X4 = P.Cx >> 2, G4 = P.Cg >> 2;
  const int Y4 = P.mode == VDETR_BCAST_CAT ? X4 + G4 : X4;
  const WideLanes L = wide_lanes(Y4);
  if (!L.live()) return;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(P.x);
  const f32x4* res4 = reinterpret_cast<const f32x4*>(P.residual);
  f32x4* y4 = reinterpret_cast<f32x4*>(P.y);
  for (int q = L.c; q < Y4; q += L.w) {
    const bool from_g = P.mode != VDETR_BCAST_CAT || q >= X4;
    const f32x4 g = from_g ? reinterpret_cast<const f32x4*>(P.g + (size_t)s * P.Cg)[P.mode == VDETR_BCAST_CAT ? q - X4 : q]
                           : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = r0 + L.rs; r < r1; r += L.rpi) {
      f32x4 v;
      if (P.mode == VDETR_BCAST_CAT) {
        v = q < X4 ? x4[(size_t)r * X4 + q] : g;
      } else {
        const f32x4 xv = x4[(size_t)r * X4 + q];
        v = P.mode == VDETR_BCAST_ADD ? xv + g : xv * g;
        if (res4) v += res4[(size_t)r * X4 + q];
      }
      if (P.relu) v = sg_relu4(v);
      y4[(size_t)r * Y4 + q] = v;
    }
  }
}

// dx (or NULL) and, with dg wanted, partial blockIdx.x of part [chunks][Cg]: add: sum dy; mul: sum dy * x; cat: sum of the last Cg columns
__global__ __launch_bounds__(256) void sg_bcast_bwd_kernel(SgBcastParams P, const float* dy, float* dx, int want_dg) {
  __shared__ f32x4 red[256];
  int s, r0, r1;
  if (!sg_locate(P.S, P.rows, blockIdx.x, s, r0, r1)) return;  // (uniform)
  const int X4 = P.Cx >> 2, G4 = P.Cg >> 2;
  const bool cat = P.mode == VDETR_BCAST_CAT, mul = P.mode == VDETR_BCAST_MUL;
  const int D4 = cat ? X4 + G4 : X4;
  const WideLanes L = wide_lanes(D4);
  const int tid = threadIdx.x;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(P.x);
  const f32x4* dy4 = reinterpret_cast<const f32x4*>(dy);
  f32x4* dx4 = reinterpret_cast<f32x4*>(dx);
  for (int q0 = 0; q0 < D4; q0 += L.w) {  // (uniform trip count: the barriers below are reached by every thread)
    const int q = q0 + L.c;
    const bool on = L.live() && q < D4;
    const bool to_x = !cat || q < X4, to_g = !cat || q >= X4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      const f32x4 g = mul && dx ? reinterpret_cast<const f32x4*>(P.g + (size_t)s * P.Cg)[q] : f32x4{1.f, 1.f, 1.f, 1.f};
      for (int r = r0 + L.rs; r < r1; r += L.rpi) {
        const f32x4 d = dy4[(size_t)r * D4 + q];
        if (dx && to_x) dx4[(size_t)r * X4 + q] = mul ? d * g : d;
        if (want_dg && to_g) a += mul ? d * x4[(size_t)r * X4 + q] : d;
      }
    }
    if (!want_dg) continue;  // (uniform)
    red[tid] = a;
    __syncthreads();
    if (on && L.rs == 0 && to_g) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < L.rpi; ++j) t += red[j * L.w + L.c];
      reinterpret_cast<f32x4*>(P.part + (size_t)blockIdx.x * P.Cg)[cat ? q - X4 : q] = t;
    }
    __syncthreads();
  }
}

// ---- the squeeze-excite gate of the inference form -------------------------------------------------------------------------------------
struct SgGateParams {
  SgSeg S;
  int C, H, rows_p;
  const float *part, *w1, *b1, *w2, *b2;
  float* gate;
};

// sum over the 64 lanes of a wave, the same value in every lane (a fixed butterfly)
__device__ __forceinline__ float sg_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// one workgroup per scene: p = the scene's average (the fold of sg_fold_sum_kernel), h = relu(W1 p + b1), gate = sigmoid(W2 h + b2).
// A wave per output row, its lanes over the row's inputs (coalesced weight reads), fmaf in ascending order per lane.
__global__ __launch_bounds__(256) void sg_gate_kernel(SgGateParams P) {
  __shared__ f32x4 red[256];
  __shared__ __attribute__((aligned(16))) float p[1024];
  __shared__ float h[256];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int p0, np, n;
  sg_parts(P.S, P.rows_p, s, p0, np, n);
  const RowLanes L = row_lanes(P.C);
  f32x4 t = sg_fold_sum(L, P.part, P.C, p0, np, red);
  if (L.rs == 0) {
    if (n > 0) t = t * (1.0f / (float)n);
    reinterpret_cast<f32x4*>(p)[L.c4] = t;
  }
  __syncthreads();
  for (int j = wave; j < P.H; j += 4) {
    const float* w = P.w1 + (size_t)j * P.C;
    float a = 0.f;
    for (int c = lane; c < P.C; c += 64) a = fmaf(w[c], p[c], a);
    a = sg_wave_sum(a);
    if (lane == 0) {
      a += P.b1 ? P.b1[j] : 0.f;
      h[j] = a > 0.f ? a : 0.f;
    }
  }
  __syncthreads();
  for (int c = wave; c < P.C; c += 4) {
    const float* w = P.w2 + (size_t)c * P.H;
    float a = 0.f;
    for (int j = lane; j < P.H; j += 64) a = fmaf(w[j], h[j], a);
    a = sg_wave_sum(a);
    if (lane == 0) {
      a += P.b2 ? P.b2[c] : 0.f;
      P.gate[(size_t)s * P.C + c] = 1.0f / (1.0f + expf(-a));
    }
  }
}

// ---- descriptor checks -----------------------------------------------------------------------------------------------------------------
static int sg_check_table(const char* op, const char* name, int C) {
  VDETR_REQUIRE(C > 0 && C % 4 == 0 && C <= 1024, "%s: %s=%d must be a positive multiple of 4 and <= 1024", op, name, C);
  return VDETR_OK;
}

static int sg_check_sizes(const char* op, int N, int nseg) {
  VDETR_REQUIRE(N >= 0, "%s: N=%d is negative", op, N);
  VDETR_REQUIRE(nseg >= 0, "%s: nseg=%d is negative", op, nseg);
  return VDETR_OK;
}

static int sg_pool_fill(const vdetr_sp_global_pool_desc* d, SgPoolParams* P, const char* op) {
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  if (int e = sg_check_table(op, "C", d->C)) return e;
  if (int e = sg_check_sizes(op, d->N, d->nseg)) return e;
  VDETR_REQUIRE(d->mode == VDETR_POOL_SUM || d->mode == VDETR_POOL_AVG || d->mode == VDETR_POOL_MAX,
                "%s: mode=%d is none of VDETR_POOL_SUM, VDETR_POOL_AVG, VDETR_POOL_MAX", op, d->mode);
  P->S = SgSeg{d->N, d->nseg, d->seg};
  P->C = d->C; P->mode = d->mode;
  P->rows_p = sg_chunk_rows(d->N); P->rows_s = sg_stream_rows(d->N);
  P->x = d->x; P->y = d->y; P->arg = d->arg;
  const size_t chunks = sg_chunk_bound(d->N, d->nseg);
  P->part = (float*)d->workspace;
  P->parg = d->workspace ? (int*)((float*)d->workspace + chunks * (size_t)d->C) : nullptr;
  return VDETR_OK;
}

static int sg_bcast_fill(const vdetr_sp_broadcast_desc* d, SgBcastParams* P, const char* op) {
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  if (int e = sg_check_table(op, "Cx", d->Cx)) return e;
  if (int e = sg_check_table(op, "Cg", d->Cg)) return e;
  if (int e = sg_check_sizes(op, d->N, d->nseg)) return e;
  VDETR_REQUIRE(d->mode == VDETR_BCAST_ADD || d->mode == VDETR_BCAST_MUL || d->mode == VDETR_BCAST_CAT,
                "%s: mode=%d is none of VDETR_BCAST_ADD, VDETR_BCAST_MUL, VDETR_BCAST_CAT", op, d->mode);
  VDETR_REQUIRE(d->mode == VDETR_BCAST_CAT || d->Cg == d->Cx, "%s: Cg=%d differs from Cx=%d (add and mul need equal widths)", op,
                d->Cg, d->Cx);
  VDETR_REQUIRE(d->mode != VDETR_BCAST_CAT || !d->residual, "%s: residual with mode=%d (add and mul only)", op, d->mode);
  P->S = SgSeg{d->N, d->nseg, d->seg};
  P->Cx = d->Cx; P->Cg = d->Cg; P->mode = d->mode; P->relu = d->relu != 0;
  P->rows = sg_stream_rows(d->N);
  P->x = d->x; P->g = d->g; P->residual = d->residual; P->y = d->y; P->part = (float*)d->workspace;
  return VDETR_OK;
}

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_sp_global_chunk_rows(int N) { return sg_chunk_rows(N < 0 ? 0 : N); }

extern "C" size_t vdetr_sp_global_pool_workspace_bytes(int N, int C, int nseg) {
  if (N < 0) N = 0;
  if (nseg < 0) nseg = 0;
  if (C < 0) C = 0;
  return sg_chunk_bound(N, nseg) * (size_t)C * (sizeof(float) + sizeof(int));
}

extern "C" size_t vdetr_sp_broadcast_workspace_bytes(int N, int Cg, int nseg) {
  if (N < 0) N = 0;
  if (nseg < 0) nseg = 0;
  if (Cg < 0) Cg = 0;
  return sg_chunk_bound(N, nseg) * (size_t)Cg * sizeof(float);
}

extern "C" int vdetr_sp_global_pool_fwd_f32(const vdetr_sp_global_pool_desc* d, vdetr_stream_t stream) {
  SgPoolParams P;
  const char* op = "sp_global_pool_fwd";
  if (int e = sg_pool_fill(d, &P, op)) return e;
  if (d->N == 0 || d->nseg == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x, "%s: x is NULL with N=%d", op, d->N);
  VDETR_REQUIRE(d->seg, "%s: seg is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->y, "%s: y is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->mode != VDETR_POOL_MAX || d->arg, "%s: arg is NULL with mode=VDETR_POOL_MAX", op);
  VDETR_REQUIRE(d->workspace, "%s: workspace is NULL (vdetr_sp_global_pool_workspace_bytes)", op);
  VDETR_REQUIRE_WORKSPACE_ALIGNED(op, "workspace", d->workspace, 16);
  const int grid = ceil_div(d->N, P.rows_p) + d->nseg;
  if (d->mode == VDETR_POOL_MAX) {
    hipLaunchKernelGGL(sg_pool_max_part_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
    if (int e = check_launch("sp_global_pool_max_part")) return e;
    hipLaunchKernelGGL(sg_fold_max_kernel, dim3(d->nseg), dim3(256), 0, (hipStream_t)stream, P);
    return check_launch("sp_global_pool_max_fold");
  }
  hipLaunchKernelGGL(sg_pool_sum_part_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
  if (int e = check_launch("sp_global_pool_sum_part")) return e;
  hipLaunchKernelGGL(sg_fold_sum_kernel, dim3(d->nseg), dim3(256), 0, (hipStream_t)stream, P.S, P.C, P.rows_p,
                     d->mode == VDETR_POOL_AVG ? 1 : 0, (const float*)P.part, P.y);
  return check_launch("sp_global_pool_sum_fold");
}

extern "C" int vdetr_sp_global_pool_bwd_f32(const vdetr_sp_global_pool_desc* d, const float* dy, float* dx, vdetr_stream_t stream) {
  SgPoolParams P;
  const char* op = "sp_global_pool_bwd";
  if (int e = sg_pool_fill(d, &P, op)) return e;
  if (d->N == 0 || d->nseg == 0) return VDETR_OK;
  VDETR_REQUIRE(d->seg, "%s: seg is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(dy, "%s: dy is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(dx, "%s: dx is NULL with N=%d", op, d->N);
  VDETR_REQUIRE(d->mode != VDETR_POOL_MAX || d->arg, "%s: arg is NULL with mode=VDETR_POOL_MAX", op);
  const int grid = ceil_div(d->N, P.rows_s) + d->nseg;
  hipLaunchKernelGGL(sg_pool_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, dy, dx);
  return check_launch("sp_global_pool_bwd");
}

extern "C" int vdetr_sp_broadcast_fwd_f32(const vdetr_sp_broadcast_desc* d, vdetr_stream_t stream) {
  SgBcastParams P;
  const char* op = "sp_broadcast_fwd";
  if (int e = sg_bcast_fill(d, &P, op)) return e;
  if (d->N == 0 || d->nseg == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x, "%s: x is NULL with N=%d", op, d->N);
  VDETR_REQUIRE(d->g, "%s: g is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->seg, "%s: seg is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->y, "%s: y is NULL with N=%d", op, d->N);
  const int grid = ceil_div(d->N, P.rows) + d->nseg;
  hipLaunchKernelGGL(sg_bcast_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_broadcast_fwd");
}

extern "C" int vdetr_sp_broadcast_bwd_f32(const vdetr_sp_broadcast_desc* d, const float* dy, float* dx, float* dg,
                                          vdetr_stream_t stream) {
  SgBcastParams P;
  const char* op = "sp_broadcast_bwd";
  if (int e = sg_bcast_fill(d, &P, op)) return e;
  if (d->N == 0 || d->nseg == 0 || (!dx && !dg)) return VDETR_OK;
  VDETR_REQUIRE(dy, "%s: dy is NULL with N=%d", op, d->N);
  VDETR_REQUIRE(d->seg, "%s: seg is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->mode != VDETR_BCAST_MUL || !dx || d->g, "%s: g is NULL (dx of mode=VDETR_BCAST_MUL reads it)", op);
  VDETR_REQUIRE(d->mode != VDETR_BCAST_MUL || !dg || d->x, "%s: x is NULL (dg of mode=VDETR_BCAST_MUL reads it)", op);
  VDETR_REQUIRE(!dg || d->workspace, "%s: workspace is NULL (vdetr_sp_broadcast_workspace_bytes)", op);
  if (dg) VDETR_REQUIRE_WORKSPACE_ALIGNED(op, "workspace", d->workspace, 16);
  if (dg) P.rows = sg_chunk_rows(d->N);  // the sweep leaves partials: the large chunks of the fold
  const int grid = ceil_div(d->N, P.rows) + d->nseg;
  hipLaunchKernelGGL(sg_bcast_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, dy, dx, dg ? 1 : 0);
  if (int e = check_launch("sp_broadcast_bwd")) return e;
  if (dg) {
    hipLaunchKernelGGL(sg_fold_sum_kernel, dim3(d->nseg), dim3(256), 0, (hipStream_t)stream, P.S, P.Cg, P.rows, 0,
                       (const float*)P.part, dg);
    return check_launch("sp_broadcast_bwd_fold");
  }
  return VDETR_OK;
}

extern "C" int vdetr_sp_se_gate_f32(const vdetr_sp_se_gate_desc* d, vdetr_stream_t stream) {
  const char* op = "sp_se_gate";
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  if (int e = sg_check_table(op, "C", d->C)) return e;
  if (int e = sg_check_sizes(op, d->N, d->nseg)) return e;
  VDETR_REQUIRE(d->H >= 1 && d->H <= 256, "%s: H=%d must be in 1 .. 256", op, d->H);
  if (d->N == 0 || d->nseg == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x, "%s: x is NULL with N=%d", op, d->N);
  VDETR_REQUIRE(d->seg, "%s: seg is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->w1 && d->w2, "%s: %s is NULL", op, d->w1 ? "w2" : "w1");
  VDETR_REQUIRE(d->gate, "%s: gate is NULL with nseg=%d", op, d->nseg);
  VDETR_REQUIRE(d->workspace, "%s: workspace is NULL (vdetr_sp_global_pool_workspace_bytes)", op);
  VDETR_REQUIRE_WORKSPACE_ALIGNED(op, "workspace", d->workspace, 16);
  SgPoolParams P{};
  P.S = SgSeg{d->N, d->nseg, d->seg};
  P.C = d->C; P.mode = VDETR_POOL_AVG; P.rows_p = sg_chunk_rows(d->N); P.rows_s = sg_stream_rows(d->N);
  P.x = d->x; P.part = (float*)d->workspace;
  const int grid = ceil_div(d->N, P.rows_p) + d->nseg;
  hipLaunchKernelGGL(sg_pool_sum_part_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
  if (int e = check_launch("sp_se_gate_part")) return e;
  SgGateParams G{P.S, d->C, d->H, P.rows_p, P.part, d->w1, d->b1, d->w2, d->b2, d->gate};
  hipLaunchKernelGGL(sg_gate_kernel, dim3(d->nseg), dim3(256), 0, (hipStream_t)stream, G);
  return check_launch("sp_se_gate");
}
