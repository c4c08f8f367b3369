// group_mlp.hip — PointNet++ set abstraction and feature propagation in inference form, ONE launch each.
//
// Reference: PointnetSAModuleVotes / PointnetFPModule (third_party/pointnet2/pointnet2_modules.py): ball query -> grouping ->
// SharedMLP (Conv2d 1x1 -> BatchNorm2d -> ReLU, 1 to 3 times) -> max over the neighbours, and three_nn -> three_interpolate ->
// concatenation -> SharedMLP.  As a composition of ops the grouped tensor [B, 3 + C, M, S] and every activation of the MLP are
// written and read back before the pooling throws them away.  In eval mode BatchNorm is a per-channel affine and nothing crosses
// a centre, so a workgroup can own a tile of grouped rows from the gather to the pooled result:
//
//   prologue   SA: row (b, m, s) = ((xyz[idx] - new_xyz) * inv_radius, features[:, idx]);  FP: (sum_k w_k known[:, idx_k], unknow)
//              -> LDS tile xs[rows][stride], zero-padded to a multiple of 16 columns
//   layer l    acc = xs[:, :K] * Wt_l  (v_mfma_f32_16x16x4_f32: exact fp32 products, f32 accumulation), barrier,
//              xs[:, :out_l] = relu(scale_l * acc + shift_l), barrier       (the output replaces the input)
//   epilogue   SA: max over the S rows of each centre -> out[b][c][m];  FP: out[b][c][i] = xs[i][c]
//
// Tiles: 64 rows for the set abstraction (S in {16, 32, 64} divides it: a centre never straddles two workgroups), 32 rows for the
// feature propagation (few rows in all: more workgroups).  256 threads; a wave owns 64-column blocks of the layer's output and as
// many 16-row tiles as keeps all four waves busy (gm_layer).  MFMA rows = tile rows, MFMA column j of tile u = column
// 64 block + 4 j + u (heads.hip's interleave): the four B operands of one contraction index are one float4 of an image row, and a
// lane's four accumulators of a row are four adjacent columns, one float4 of the LDS tile.
// LDS rows are (widest layer rounded up to 64) + 4 floats: 16 consecutive rows land on 16 different 16-byte slots.
//
// pw_mlp_kernel is the point-wise sibling (PointnetLFPModuleMSG's shared post MLP): no gather, rows = (scale, scene, point).
#include "attn_common.h"

namespace vdetr {

constexpr int kGmThreads = 256;
constexpr int kGmMaxIn = 512;   // longest first contraction
constexpr int kGmMaxW = 256;    // widest layer

__device__ __forceinline__ f32x4 gm_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void gm_st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

struct GmArgs {
  vdetr_group_mlp_desc mlp;
  const float* pts;      // SA: xyz [B, N, 3]
  const float* feats;    // SA: features [B, C, N] or null; FP: known_feats [B, C2, m]
  const float* other;    // SA: new_xyz [B, M, 3];          FP: unknow_feats [B, C1, n] or null
  const int32_t* idx;    // SA: [B, M, S];                  FP: [B, n, 3]
  const float* weight;   //                                 FP: [B, n, 3]
  float* out;
  int N, M, S, C, use_xyz;  // SA: points, centres, neighbours, feature channels; FP: N = n, M = m, C = C2
  float inv_radius;
  int stride;            // floats per LDS row
  long rows;             // SA: B M S; FP: B n
};

// One step of 16 contraction indices: lane (kg = lane >> 4, c = lane & 15) holds, for e = 0 .. 3, index 16 m + 4 kg + e of both operands.
template <int RT>
__device__ __forceinline__ void gm_load(const float* __restrict__ wp, const float* ap, int cpad, int stride, int m, f32x4 (&b)[4], f32x4 (&a)[RT]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) b[e] = gm_ld4(wp + (size_t)(16 * m + e) * cpad);
#pragma unroll
  for (int t = 0; t < RT; ++t) a[t] = gm_ld4(ap + 16 * t * stride + 16 * m);
}
template <int RT>
__device__ __forceinline__ void gm_mma(const f32x4 (&b)[4], const f32x4 (&a)[RT], f32x4 (&acc)[RT][4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][e], b[e][u], acc[t][u], 0, 0, 0);
}
// acc[t][u][r] += sum_{k < 16 k16} xs[16 t + 4 kg + r][k] Wt[k][col0 + 4 c + u]     (xs: the wave's first row; Wt rows of cpad floats)
template <int RT>
__device__ __forceinline__ void gm_run(const float* xs, int stride, const float* __restrict__ Wt, int cpad, int k16, int col0, int lane,
                                       f32x4 (&acc)[RT][4]) {
  const int c = lane & 15, kg = lane >> 4;
  const float* wp = Wt + (size_t)(4 * kg) * cpad + col0 + 4 * c;
  const float* ap = xs + c * stride + 4 * kg;
  f32x4 b0[4], b1[4], a0[RT], a1[RT];
  gm_load<RT>(wp, ap, cpad, stride, 0, b0, a0);
  int m = 0;
  for (; m + 2 <= k16; m += 2) {  // the next step's operands are requested before this step's products
    gm_load<RT>(wp, ap, cpad, stride, m + 1, b1, a1);
    gm_mma<RT>(b0, a0, acc);
    if (m + 2 < k16) gm_load<RT>(wp, ap, cpad, stride, m + 2, b0, a0);
    gm_mma<RT>(b1, a1, acc);
  }
  if (m < k16) gm_mma<RT>(b0, a0, acc);
}

// A wave's share of a layer: NR column blocks (block0, block0 + 1, ..) of the RT row tiles from rt0 on.  Every wave passes both
// barriers; `active` (wave-uniform) says whether it has a share.
template <int RT, int NR>
__device__ __forceinline__ void gm_share(float* xs, int stride, const float* __restrict__ Wt, const float* __restrict__ sc,
                                         const float* __restrict__ sh, int k16, int cpad, int block0, int rt0, bool active, int lane) {
  f32x4 acc[NR][RT][4];
#pragma unroll
  for (int n = 0; n < NR; ++n)
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[n][t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (active) {
#pragma unroll
    for (int n = 0; n < NR; ++n) gm_run<RT>(xs + 16 * rt0 * stride, stride, Wt, cpad, k16, 64 * (block0 + n), lane, acc[n]);
  }
  __syncthreads();  // every wave has read the layer's input: the tile becomes its output
  if (active) {
    const int c = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int col = 64 * (block0 + n) + 4 * c;
      const f32x4 s4 = gm_ld4(sc + col), h4 = gm_ld4(sh + col);
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f32x4 h;
#pragma unroll
          for (int u = 0; u < 4; ++u) h[u] = fmaxf(acc[n][t][u][r] * s4[u] + h4[u], 0.f);
          gm_st4(xs + (16 * (rt0 + t) + 4 * kg + r) * stride + col, h);
        }
    }
  }
  __syncthreads();
}

// NT row tiles x (cpad / 64) column blocks over four waves
template <int NT>
__device__ __forceinline__ void gm_layer(float* xs, int stride, const float* __restrict__ Wt, const float* __restrict__ sc,
                                         const float* __restrict__ sh, int k16, int cpad, int w, int lane) {
  const int blocks = cpad >> 6;  // 1 .. 4, the same in every wave
  if (NT == 4) {
    if (blocks == 4) gm_share<4, 1>(xs, stride, Wt, sc, sh, k16, cpad, w, 0, true, lane);
    else if (blocks == 3) gm_share<1, 3>(xs, stride, Wt, sc, sh, k16, cpad, 0, w, true, lane);
    else if (blocks == 2) gm_share<2, 1>(xs, stride, Wt, sc, sh, k16, cpad, w & 1, 2 * (w >> 1), true, lane);
    else gm_share<1, 1>(xs, stride, Wt, sc, sh, k16, cpad, 0, w, true, lane);
  } else {  // NT == 2
    if (blocks >= 3) gm_share<2, 1>(xs, stride, Wt, sc, sh, k16, cpad, w, 0, w < blocks, lane);
    else if (blocks == 2) gm_share<1, 1>(xs, stride, Wt, sc, sh, k16, cpad, w & 1, w >> 1, true, lane);
    else gm_share<1, 1>(xs, stride, Wt, sc, sh, k16, cpad, 0, w, w < 2, lane);
  }
}

template <int NT, bool SA>
__global__ __launch_bounds__(kGmThreads) void group_mlp_kernel(GmArgs A) {
  extern __shared__ __attribute__((aligned(16))) float gm_xs[];
  float* xs = gm_xs;
  constexpr int kRows = 16 * NT, kGroups = kGmThreads / kRows;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int stride = A.stride, cin = A.mlp.cin, k0pad = (cin + 15) & ~15;
  const long row0 = (long)blockIdx.x * kRows;
  {  // ---- prologue: thread = (row r, every kGroups-th column from cq on) ----
    const int r = tid % kRows, cq = tid / kRows;
    const long g = row0 + r;
    const bool live = g < A.rows;
    float* xr = xs + r * stride;
    if (SA) {
      long b = 0, cg = 0;
      int j = 0;
      if (live) {
        cg = g / A.S;
        b = cg / A.M;
        j = min(max(A.idx[g], 0), A.N - 1);
      }
      const int x3 = A.use_xyz ? 3 : 0;
      for (int k = cq; k < k0pad; k += kGroups) {
        float v = 0.f;
        if (live) {
          if (k < x3) v = (A.pts[(b * A.N + j) * 3 + k] - A.other[cg * 3 + k]) * A.inv_radius;
          else if (k < cin) v = A.feats[(b * A.C + (k - x3)) * A.N + j];
        }
        xr[k] = v;
      }
    } else {
      long b = 0, i = 0;
      int j0 = 0, j1 = 0, j2 = 0;
      float w0 = 0.f, w1 = 0.f, w2 = 0.f;
      if (live) {
        b = g / A.N;
        i = g - b * A.N;
        j0 = min(max(A.idx[g * 3], 0), A.M - 1); j1 = min(max(A.idx[g * 3 + 1], 0), A.M - 1); j2 = min(max(A.idx[g * 3 + 2], 0), A.M - 1);
        w0 = A.weight[g * 3]; w1 = A.weight[g * 3 + 1]; w2 = A.weight[g * 3 + 2];
      }
      for (int k = cq; k < k0pad; k += kGroups) {
        float v = 0.f;
        if (live) {
          if (k < A.C) {  // three_interpolate's order: t = p2 w2; t = fma(p1, w1, t); t = fma(p3, w3, t)
            const float* p = A.feats + (b * A.C + k) * A.M;
            v = __fmaf_rn(p[j2], w2, __fmaf_rn(p[j0], w0, __fmul_rn(p[j1], w1)));
          } else if (k < cin) {
            v = A.other[(b * (cin - A.C) + (k - A.C)) * A.N + i];
          }
        }
        xr[k] = v;
      }
    }
  }
  __syncthreads();
  // ---- the layers ----
  int kin = k0pad, cout = 0;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    if (l < A.mlp.nlayers) {
      cout = A.mlp.width[l];
      gm_layer<NT>(xs, stride, A.mlp.wt[l], A.mlp.scale[l], A.mlp.shift[l], kin >> 4, (cout + 63) & ~63, w, lane);
      kin = cout;
    }
  }
  // ---- epilogue (gm_share ended on a barrier) ----
  if (SA) {
    const int S = A.S, cpt = kRows / S;  // centres of this tile
    for (int o = tid; o < cpt * cout; o += kGmThreads) {
      const int jc = o / cout, ch = o - jc * cout;
      const long cg = (long)blockIdx.x * cpt + jc;
      if (cg * S >= A.rows) continue;
      const float* p = xs + jc * S * stride + ch;
      float mx = p[0];
      for (int s = 1; s < S; ++s) mx = fmaxf(mx, p[s * stride]);
      const long b = cg / A.M, m = cg - b * A.M;
      A.out[(b * cout + ch) * A.M + m] = mx;
    }
  } else {
    for (int o = tid; o < kRows * cout; o += kGmThreads) {
      const int r = o % kRows, ch = o / kRows;
      const long g = row0 + r;
      if (g >= A.rows) continue;
      const long b = g / A.N, i = g - b * A.N;
      A.out[(b * cout + ch) * A.N + i] = xs[r * stride + ch];
    }
  }
}

// The shared post MLP of PointnetLFPModuleMSG on every scale's pooled features, ONE launch for up to four scales: row g = (scale k,
// scene b, point i) = concat(pooled[k][b][:, i], features2[b][:, i]); the result goes to the scale's channel slice of `out`, so
// neither the per-scale concatenation nor the one over the scales exists.  32-row tiles like the feature propagation; a row is
// decomposed on its own, so a tile may straddle a scene and a scale boundary.
struct PwArgs {
  vdetr_group_mlp_desc mlp;
  const float* p0; const float* p1; const float* p2; const float* p3;  // pooled [B, Ck, n] per scale (named, not an array: the scale is per thread)
  const float* feats2;   // [B, C2, n] or null
  float* out;            // [B, out_channels, n]
  int n, Ck, C2, out_channels, out_channel0;
  int stride;            // floats per LDS row
  long bn;               // B n
  long rows;             // K B n
};

__global__ __launch_bounds__(kGmThreads) void pw_mlp_kernel(PwArgs A) {
  extern __shared__ __attribute__((aligned(16))) float gm_xs[];
  float* xs = gm_xs;
  constexpr int kRows = 32, kGroups = kGmThreads / kRows;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int stride = A.stride, cin = A.mlp.cin, k0pad = (cin + 15) & ~15;
  // thread = (row r, every kGroups-th column from cq on), in the prologue and in the epilogue: the row is decomposed once
  const int r = tid % kRows, cq = tid / kRows;
  const long g = (long)blockIdx.x * kRows + r;
  const bool live = g < A.rows;
  long k = 0, b = 0, i = 0;
  if (live) {
    k = g / A.bn;
    const long rem = g - k * A.bn;
    b = rem / A.n;
    i = rem - b * A.n;
  }
  {  // ---- prologue ----
    const float* pk = k == 0 ? A.p0 : k == 1 ? A.p1 : k == 2 ? A.p2 : A.p3;
    const float* pr = pk + b * A.Ck * A.n + i;                          // channel c of the row: pr[c n]
    const float* fr = A.feats2 ? A.feats2 + b * A.C2 * A.n + i : pk;    // (never read when C2 == 0: cin == Ck)
    float* xr = xs + r * stride;
    for (int c = cq; c < k0pad; c += kGroups) {
      float v = 0.f;
      if (live) {
        if (c < A.Ck) v = pr[(long)c * A.n];
        else if (c < cin) v = fr[(long)(c - A.Ck) * A.n];
      }
      xr[c] = v;
    }
  }
  __syncthreads();
  // ---- the layers ----
  int kin = k0pad, cout = 0;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    if (l < A.mlp.nlayers) {
      cout = A.mlp.width[l];
      gm_layer<2>(xs, stride, A.mlp.wt[l], A.mlp.scale[l], A.mlp.shift[l], kin >> 4, (cout + 63) & ~63, w, lane);
      kin = cout;
    }
  }
  // ---- epilogue (gm_share ended on a barrier): consecutive threads store consecutive i ----
  if (live) {
    float* orow = A.out + (b * A.out_channels + A.out_channel0 + k * cout) * A.n + i;
    const float* xr = xs + r * stride;
    for (int ch = cq; ch < cout; ch += kGroups) orow[(long)ch * A.n] = xr[ch];
  }
}

// One layer's transposed, zero-padded image and its folded vectors (vdetr_group_mlp_pack_f32)
__global__ __launch_bounds__(kGmThreads) void group_mlp_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                                     int cin, int cout, int kpad, int cpad, float* __restrict__ wt,
                                                                     float* __restrict__ scale, float* __restrict__ shift) {
  const int o = blockIdx.x * kGmThreads + threadIdx.x;
  if (o < kpad * cpad) {
    const int k = o / cpad, c = o - k * cpad;
    wt[o] = (k < cin && c < cout) ? w[(size_t)c * cin + k] : 0.f;
  }
  if (o < cpad) {
    float s = 0.f, h = 0.f;
    if (o < cout) {
      const float bv = bias ? bias[o] : 0.f;
      if (gamma) {
        s = gamma[o] * (1.f / sqrtf(var[o] + eps));
        h = beta[o] + (bv - mean[o]) * s;
      } else {
        s = 1.f;
        h = bv;
      }
    }
    scale[o] = s;
    shift[o] = h;
  }
}

}  // namespace vdetr

using namespace vdetr;

#define GM_ALIGNED(p) ((((uintptr_t)(p)) & 15) == 0)

// checks the MLP part of a descriptor; *maxw: the widest LDS row it needs (floats, a multiple of 64)
static int gm_check_mlp(const vdetr_group_mlp_desc* m, const char* op, int* maxw) {
  VDETR_REQUIRE(m->nlayers >= 1 && m->nlayers <= 3, "%s: nlayers=%d outside [1, 3]", op, m->nlayers);
  VDETR_REQUIRE(m->cin >= 1 && m->cin <= kGmMaxIn, "%s: cin=%d outside [1, %d]", op, m->cin, kGmMaxIn);
  int wmax = (m->cin + 63) & ~63;
  for (int l = 0; l < m->nlayers; ++l) {
    const int c = m->width[l];
    VDETR_REQUIRE(c >= 16 && c <= kGmMaxW && c % 16 == 0, "%s: width[%d]=%d is not a multiple of 16 in [16, %d]", op, l, c, kGmMaxW);
    VDETR_REQUIRE(m->wt[l] && m->scale[l] && m->shift[l], "%s: null image or vector of layer %d", op, l);
    VDETR_REQUIRE(GM_ALIGNED(m->wt[l]) && GM_ALIGNED(m->scale[l]) && GM_ALIGNED(m->shift[l]), "%s: images and vectors must be 16-B aligned", op);
    const int cp = (c + 63) & ~63;
    if (cp > wmax) wmax = cp;
  }
  *maxw = wmax;
  return VDETR_OK;
}

template <int NT, bool SA>
static int gm_launch(const GmArgs& A, vdetr_stream_t stream, const char* op) {
  const size_t lds = (size_t)16 * NT * A.stride * sizeof(float);
  if (int e = set_lds(group_mlp_kernel<NT, SA>, lds, op)) return e;
  hipLaunchKernelGGL((group_mlp_kernel<NT, SA>), dim3(ceil_div(A.rows, 16 * NT)), dim3(kGmThreads), lds, (hipStream_t)stream, A);
  return check_launch(op);
}

extern "C" int vdetr_group_mlp_pack_f32(const float* w, const float* bias, const float* gamma, const float* beta, const float* mean,
                                        const float* var, float eps, int cin, int cout, float* wt, float* scale, float* shift,
                                        vdetr_stream_t stream) {
  VDETR_REQUIRE(w && wt && scale && shift, "group_mlp_pack: null pointer");
  VDETR_REQUIRE(cin >= 1 && cin <= kGmMaxIn && cout >= 1 && cout <= kGmMaxW, "group_mlp_pack: cin=%d outside [1, %d] or cout=%d outside [1, %d]",
                cin, kGmMaxIn, cout, kGmMaxW);
  VDETR_REQUIRE((gamma != nullptr) == (beta != nullptr) && (gamma != nullptr) == (mean != nullptr) && (gamma != nullptr) == (var != nullptr),
                "group_mlp_pack: gamma, beta, mean and var go together");
  const int kpad = (cin + 15) & ~15, cpad = (cout + 63) & ~63;
  hipLaunchKernelGGL(group_mlp_pack_kernel, dim3(ceil_div((long)kpad * cpad, kGmThreads)), dim3(kGmThreads), 0, (hipStream_t)stream, w, bias,
                     gamma, beta, mean, var, eps, cin, cout, kpad, cpad, wt, scale, shift);
  return check_launch("group_mlp_pack");
}

extern "C" int vdetr_sa_mlp_max_infer_f32(const vdetr_sa_mlp_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d != nullptr, "sa_mlp_max_infer: null descriptor");
  VDETR_REQUIRE(d->B > 0 && d->N > 0 && d->M > 0, "sa_mlp_max_infer: B=%d, N=%d, M=%d must be positive", d->B, d->N, d->M);
  VDETR_REQUIRE(d->S == 16 || d->S == 32 || d->S == 64, "sa_mlp_max_infer: S=%d is not 16, 32 or 64", d->S);
  VDETR_REQUIRE(d->C >= 0 && (d->C > 0) == (d->features != nullptr), "sa_mlp_max_infer: C=%d and features do not go together", d->C);
  VDETR_REQUIRE(d->mlp.cin == (d->use_xyz ? 3 : 0) + d->C, "sa_mlp_max_infer: cin=%d is not %d + C=%d", d->mlp.cin, d->use_xyz ? 3 : 0, d->C);
  int maxw = 0;
  if (int e = gm_check_mlp(&d->mlp, "sa_mlp_max_infer", &maxw)) return e;
  const long lim = 2147483647L, cout = d->mlp.width[d->mlp.nlayers - 1];
  VDETR_REQUIRE((long)d->B * d->M * d->S <= lim && (long)d->B * (d->C > 3 ? d->C : 3) * d->N <= lim && (long)d->B * cout * d->M <= lim,
                "sa_mlp_max_infer: a tensor of 2^31 elements or more");
  VDETR_REQUIRE(d->xyz && d->new_xyz && d->idx && d->out, "sa_mlp_max_infer: null operand");
  GmArgs A;
  A.mlp = d->mlp;
  A.pts = d->xyz; A.feats = d->features; A.other = d->new_xyz; A.idx = d->idx; A.weight = nullptr; A.out = d->out;
  A.N = d->N; A.M = d->M; A.S = d->S; A.C = d->C; A.use_xyz = d->use_xyz ? 1 : 0;
  A.inv_radius = d->inv_radius;
  A.stride = maxw + 4;
  A.rows = (long)d->B * d->M * d->S;
  return gm_launch<4, true>(A, stream, "sa_mlp_max_infer");
}

extern "C" int vdetr_fp_mlp_infer_f32(const vdetr_fp_mlp_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d != nullptr, "fp_mlp_infer: null descriptor");
  VDETR_REQUIRE(d->B > 0 && d->n > 0 && d->m > 0, "fp_mlp_infer: B=%d, n=%d, m=%d must be positive", d->B, d->n, d->m);
  VDETR_REQUIRE(d->C2 > 0 && d->C1 >= 0 && (d->C1 > 0) == (d->unknow_feats != nullptr), "fp_mlp_infer: C1=%d, C2=%d and the feature tensors do not go together",
                d->C1, d->C2);
  VDETR_REQUIRE(d->mlp.cin == d->C1 + d->C2, "fp_mlp_infer: cin=%d is not C1=%d + C2=%d", d->mlp.cin, d->C1, d->C2);
  int maxw = 0;
  if (int e = gm_check_mlp(&d->mlp, "fp_mlp_infer", &maxw)) return e;
  const long lim = 2147483647L, cout = d->mlp.width[d->mlp.nlayers - 1];
  VDETR_REQUIRE((long)d->B * d->n * 3 <= lim && (long)d->B * d->C2 * d->m <= lim && (long)d->B * d->C1 * d->n <= lim && (long)d->B * cout * d->n <= lim,
                "fp_mlp_infer: a tensor of 2^31 elements or more");
  VDETR_REQUIRE(d->known_feats && d->idx && d->weight && d->out, "fp_mlp_infer: null operand");
  GmArgs A;
  A.mlp = d->mlp;
  A.pts = nullptr; A.feats = d->known_feats; A.other = d->unknow_feats; A.idx = d->idx; A.weight = d->weight; A.out = d->out;
  A.N = d->n; A.M = d->m; A.S = 1; A.C = d->C2; A.use_xyz = 0;
  A.inv_radius = 1.f;
  A.stride = maxw + 4;
  A.rows = (long)d->B * d->n;
  return gm_launch<2, false>(A, stream, "fp_mlp_infer");
}

extern "C" int vdetr_pw_mlp_infer_f32(const vdetr_pw_mlp_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d != nullptr, "pw_mlp_infer: null descriptor");
  VDETR_REQUIRE(d->K >= 1 && d->K <= 4, "pw_mlp_infer: K=%d outside [1, 4]", d->K);
  VDETR_REQUIRE(d->B > 0 && d->n > 0, "pw_mlp_infer: B=%d, n=%d must be positive", d->B, d->n);
  VDETR_REQUIRE(d->Ck >= 1 && d->C2 >= 0 && (d->C2 > 0) == (d->features2 != nullptr), "pw_mlp_infer: Ck=%d, C2=%d and features2 do not go together",
                d->Ck, d->C2);
  VDETR_REQUIRE(d->mlp.cin == d->Ck + d->C2, "pw_mlp_infer: cin=%d is not Ck=%d + C2=%d", d->mlp.cin, d->Ck, d->C2);
  int maxw = 0;
  if (int e = gm_check_mlp(&d->mlp, "pw_mlp_infer", &maxw)) return e;
  const long lim = 2147483647L, cout = d->mlp.width[d->mlp.nlayers - 1];
  VDETR_REQUIRE(d->out_channel0 >= 0 && d->out_channels >= 1 && (long)d->out_channel0 + d->K * cout <= d->out_channels,
                "pw_mlp_infer: out_channel0=%d + K=%d x %ld channels do not fit out_channels=%d", d->out_channel0, d->K, cout, d->out_channels);
  VDETR_REQUIRE((long)d->K * d->B * d->n <= lim && (long)d->B * d->Ck * d->n <= lim && (long)d->B * d->C2 * d->n <= lim &&
                    (long)d->B * d->out_channels * d->n <= lim,
                "pw_mlp_infer: a tensor of 2^31 elements or more");
  bool operands = d->out != nullptr;
  for (int k = 0; k < d->K; ++k) operands = operands && d->pooled[k] != nullptr;
  VDETR_REQUIRE(operands, "pw_mlp_infer: null operand");
  PwArgs A;
  A.mlp = d->mlp;
  A.p0 = d->pooled[0]; A.p1 = d->pooled[1]; A.p2 = d->pooled[2]; A.p3 = d->pooled[3];
  A.feats2 = d->features2; A.out = d->out;
  A.n = d->n; A.Ck = d->Ck; A.C2 = d->C2; A.out_channels = d->out_channels; A.out_channel0 = d->out_channel0;
  A.stride = maxw + 4;
  A.bn = (long)d->B * d->n;
  A.rows = A.bn * d->K;
  const size_t lds = (size_t)32 * A.stride * sizeof(float);
  if (int e = set_lds(pw_mlp_kernel, lds, "pw_mlp_infer")) return e;
  hipLaunchKernelGGL(pw_mlp_kernel, dim3(ceil_div(A.rows, 32)), dim3(kGmThreads), lds, (hipStream_t)stream, A);
  return check_launch("pw_mlp_infer");
}
