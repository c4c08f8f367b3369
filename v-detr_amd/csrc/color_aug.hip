// color_aug.hip — the per-point arithmetic a training scan goes through before the cuboid crop, and the colour step after
// the scale (reference datasets/scannet.py:202-295, 436-451, 461-464, 544-560).  The host draws every number
// from the legacy random stream (scene_prep.draw_color_augment / draw_sunrgbd_color); nothing is drawn here.
//   vdetr_color_augment_f32   three launches:
//     color_bounds_kernel   one workgroup per scene-aligned tile of 256 rows: float32 min / max of the DROPPED colours, a NaN
//                           handed on as np.min / np.max do -> one partial per tile
//     color_scale_kernel    one wave per scene: merges the partials -> lo, hi, 255 / (hi - lo)
//     color_apply_kernel    one lane per row: drop, contrast, jitter, hue / saturation, each skipped where its gate did not fire
//   vdetr_append_height_f32   nine launches: four passes of (height_hist_kernel, height_pick_kernel), a radix select, 8 bits
//                           a pass, of THREE order statistics of the z column at once (k, its neighbour, and the last one, which
//                           is a NaN exactly if the column holds one: numpy's own test), then height_write_kernel
//   vdetr_sunrgbd_color_f32   one launch, in place
// Partials go out with ordinary stores: no global atomics, no ticket (README "Two findings about the chip"); the LDS
// histograms count integers, so two runs give the same bits.  -ffp-contract=off as everywhere: every product and sum below
// is one IEEE operation, in the dtype numpy uses for it (include/vdetr_hip.h).
#include "scene_tiles.h"

namespace vdetr {
namespace {

constexpr int kTile = VDETR_COLOR_AUG_TILE;
constexpr int kSelTile = VDETR_HEIGHT_TILE;
constexpr int kSelRows = kSelTile / 256;     // rows per lane of the histogram kernel
constexpr int kSel = 3;                      // order statistics selected at once
constexpr int kBins = 256;
constexpr int kBound = 9;                    // floats per tile / scene: min rgb, max rgb, then "holds a NaN" rgb or the scale rgb

__device__ __forceinline__ bool drops(const vdetr_color_aug_desc& d, int b) {
  return d.keep != nullptr && d.params[(size_t)b * VDETR_COLOR_AUG_PARAMS + 7] != 0.0;
}

// ---- the four colour augmentations ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTile) void color_bounds_kernel(vdetr_color_aug_desc d, int total_rows, float* bounds) {
  __shared__ float red[kTile / kWave][kBound];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  const bool found = locate_tile(d.offsets, d.B, kTile, t, b, local_tile);
  const float inf = __builtin_huge_valf();
  float v[kBound] = {inf, inf, inf, -inf, -inf, -inf, 0.f, 0.f, 0.f};
  if (found) {
    const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
    const int j = local_tile * kTile + tid;
    if (j < rows && begin + j < total_rows) {
      const float* src = d.points + (size_t)(begin + j) * d.W + 3;
      const bool drop = drops(d, b);
      const float keep = drop && !d.keep[begin + j] ? 0.0f : 1.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float x = drop ? src[k] * keep : src[k];
        if (x != x) v[6 + k] = 1.f;                                    // np.min / np.max hand a NaN on
        else v[k] = v[3 + k] = x;
      }
    }
  }
  store_tile_partial(v, red, bounds, t);
}

__global__ __launch_bounds__(kWave) void color_scale_kernel(vdetr_color_aug_desc d, int num_tiles, const float* bounds, float* scene) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int first = first_tile(d.offsets, b, kTile), nt = tiles_of(d.offsets[b + 1] - d.offsets[b], kTile);
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, bad[3] = {0.f, 0.f, 0.f};
  for (int i = lane; i < nt && first + i < num_tiles; i += kWave) {
    const float* q = bounds + (size_t)(first + i) * kBound;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], q[k]); hi[k] = fmaxf(hi[k], q[3 + k]); bad[k] = fmaxf(bad[k], q[6 + k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = wave_allmin_f32(lo[k]); hi[k] = wave_allmax_f32(hi[k]); bad[k] = wave_allmax_f32(bad[k]);
    if (bad[k] != 0.f) lo[k] = hi[k] = __builtin_nanf("");
  }
  if (lane < 3) {
    const float l = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lo[2], h = lane == 0 ? hi[0] : lane == 1 ? hi[1] : hi[2];
    float* o = scene + (size_t)b * kBound;
    o[lane] = l;
    o[3 + lane] = h;
    o[6 + lane] = __fdiv_rn(255.0f, h - l);                            // scale = 255 / (hi - lo) in float32; a constant channel: inf
  }
}

__device__ __forceinline__ double clip_f64(double v, double lo, double hi) {   // np.clip: a NaN stays
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}

__device__ __forceinline__ double remainder_one(double a) {            // np.remainder(a, 1.0): fmod, the sign of the divisor
  double m = a - trunc(a);                                             // fmod(a, 1.0), exact
  if (m != 0.0) {
    if (m < 0.0) m = m + 1.0;                                          // may round to 1.0, as it does in numpy
  } else {
    m = 0.0;                                                           // copysign(0, 1)
  }
  return m;
}

__device__ __forceinline__ float to_uint8(double v) {                  // astype('uint8'): truncation; a NaN gives 0
  return v != v ? 0.0f : (float)(unsigned char)(int)v;
}

__device__ __forceinline__ double max_nan(double a, double b) { return a != a ? a : b != b ? b : (a > b ? a : b); }
__device__ __forceinline__ double min_nan(double a, double b) { return a != a ? a : b != b ? b : (a < b ? a : b); }

__device__ __forceinline__ void hue_saturation(float* x, double hue_val, double sat_ratio) {
  // rgb_to_hsv (scannet.py:237-260) in float64
  const double r = (double)x[0], g = (double)x[1], b = (double)x[2];
  const double maxc = max_nan(max_nan(r, g), b), minc = min_nan(min_nan(r, g), b);
  const double v = maxc;
  const bool mask = maxc != minc;
  double s = 0.0, rc = 0.0, gc = 0.0, bc = 0.0;
  if (mask) {
    const double span = maxc - minc;
    s = span / maxc;
    rc = (maxc - r) / span;
    gc = (maxc - g) / span;
    bc = (maxc - b) / span;
  }
  double h = r == maxc ? bc - gc : g == maxc ? (2.0 + rc) - bc : (4.0 + gc) - rc;
  h = remainder_one(h / 6.0);
  // HueSaturationTranslation.__call__ (:290-293)
  h = remainder_one((hue_val + h) + 1.0);
  s = clip_f64(sat_ratio * s, 0.0, 1.0);
  // hsv_to_rgb (:263-281)
  const double h6 = h * 6.0;
  int i = h6 != h6 ? 0 : (int)(unsigned char)(int)h6;
  const double f = h6 - (double)i;
  const double p = v * (1.0 - s);
  const double q = v * (1.0 - s * f);
  const double t = v * (1.0 - s * (1.0 - f));
  i = i % 6;
  double o0, o1, o2;
  if (s == 0.0) { o0 = v; o1 = v; o2 = v; }
  else if (i == 1) { o0 = q; o1 = v; o2 = p; }
  else if (i == 2) { o0 = p; o1 = v; o2 = t; }
  else if (i == 3) { o0 = p; o1 = q; o2 = v; }
  else if (i == 4) { o0 = t; o1 = p; o2 = v; }
  else if (i == 5) { o0 = v; o1 = p; o2 = q; }
  else { o0 = v; o1 = t; o2 = p; }
  x[0] = to_uint8(o0); x[1] = to_uint8(o1); x[2] = to_uint8(o2);
}

__global__ __launch_bounds__(kTile) void color_apply_kernel(vdetr_color_aug_desc d, int total_rows, const float* scene) {
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, kTile, t, b, local_tile)) return;   // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int j = local_tile * kTile + tid;
  const long row = (long)begin + j;
  if (j >= rows || row >= total_rows) return;
  const double* q = d.params + (size_t)b * VDETR_COLOR_AUG_PARAMS;
  const float* src = d.points + (size_t)row * d.W;
  float* out = d.out + (size_t)row * d.W;
  float x[3] = {src[3], src[4], src[5]};
  if (drops(d, b)) {                                                   // point_cloud[:, 3:] *= colors_drop[:, None]
    const float keep = d.keep[row] ? 1.0f : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = x[k] * keep;
  }
  if (q[0] != 0.0) {                                                   // ChromaticAutoContrast: float32 throughout
    const float* s = scene + (size_t)b * kBound;
    const float keep_part = (float)q[1], blend = (float)q[2];         // Python floats there: rounded to float32, then multiplied
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float contrast = (x[k] - s[k]) * s[6 + k];
      const float left = keep_part * x[k], right = blend * contrast;
      x[k] = left + right;
    }
  }
  if (d.noise != nullptr && q[3] >= 0.0 && (long)q[3] + j < (long)d.noise_rows) {   // ChromaticJitter: float64, rounded once
    const double* noise = d.noise + ((size_t)q[3] + (size_t)j) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (float)clip_f64(noise[k] + (double)x[k], 0.0, 255.0);
  }
  if (q[4] != 0.0) hue_saturation(x, q[5], q[6]);
  out[0] = src[0]; out[1] = src[1]; out[2] = src[2];
  out[3] = x[0]; out[4] = x[1]; out[5] = x[2];
  for (int k = 6; k < d.W; ++k) out[k] = src[k];
}

// ---- the height channel: np.percentile(z, 0.99) by radix select ------------------------------------------------------------------
// order-preserving image of a float32; every NaN becomes the largest key (numpy sorts them to the end)
__device__ __forceinline__ unsigned key_of(float z) {
  if (z != z) return 0xffffffffu;
  const unsigned u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// state [B, kSel, 2]: the key bits fixed so far, the rank that is left among the keys that share them
__global__ __launch_bounds__(256) void height_hist_kernel(vdetr_color_aug_desc d, int total_rows, int shift, const unsigned* state,
                                                          unsigned* partial) {
  __shared__ unsigned hist[kSel][kBins];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  const bool found = locate_tile(d.offsets, d.B, kSelTile, t, b, local_tile);   // uniform
#pragma unroll
  for (int s = 0; s < kSel; ++s) hist[s][tid] = 0u;
  __syncthreads();
  if (found) {
    const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
    unsigned prefix[kSel];
#pragma unroll
    for (int s = 0; s < kSel; ++s) prefix[s] = shift == 24 ? 0u : state[((size_t)b * kSel + s) * 2];
    const unsigned high = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
#pragma unroll
    for (int r = 0; r < kSelRows; ++r) {
      const int j = local_tile * kSelTile + r * 256 + tid;
      if (j < rows && begin + j < total_rows) {
        const unsigned key = key_of(d.points[(size_t)(begin + j) * d.W + 2]);
        const unsigned digit = (key >> shift) & 0xffu;
#pragma unroll
        for (int s = 0; s < kSel; ++s)
          if ((key & high) == prefix[s]) atomicAdd(&hist[s][digit], 1u);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kSel; ++s) partial[((size_t)t * kSel + s) * kBins + tid] = hist[s][tid];
}

__global__ __launch_bounds__(256) void height_pick_kernel(vdetr_color_aug_desc d, int num_tiles, int shift, const unsigned* partial,
                                                          unsigned* state) {
  __shared__ unsigned count[kSel][kBins];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int rows = d.offsets[b + 1] - d.offsets[b];
  const int first = first_tile(d.offsets, b, kSelTile), nt = tiles_of(rows, kSelTile);
  unsigned sum[kSel] = {0u, 0u, 0u};
  for (int i = 0; i < nt && first + i < num_tiles; ++i) {
#pragma unroll
    for (int s = 0; s < kSel; ++s) sum[s] += partial[((size_t)(first + i) * kSel + s) * kBins + tid];
  }
#pragma unroll
  for (int s = 0; s < kSel; ++s) count[s][tid] = sum[s];
  __syncthreads();
  if (tid < kSel) {
    unsigned* st = state + ((size_t)b * kSel + tid) * 2;
    unsigned prefix = 0u, rank;
    if (shift == 24) {
      const int k = tid == 2 ? rows - 1 : d.select[b * VDETR_HEIGHT_SELECT + tid];
      rank = (unsigned)(k < 0 ? 0 : k >= rows ? rows - 1 : k);
    } else {
      prefix = st[0];
      rank = st[1];
    }
    int digit = kBins - 1;                                              // the counts add up to more than the rank: a guard
    for (int i = 0; i < kBins; ++i) {
      const unsigned c = count[tid][i];
      if (rank < c) { digit = i; break; }
      rank -= c;
    }
    st[0] = prefix | ((unsigned)digit << shift);
    st[1] = rank;
  }
}

__global__ __launch_bounds__(256) void height_write_kernel(vdetr_color_aug_desc d, int total_rows, const unsigned* state) {
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, 256, t, b, local_tile)) return;     // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int j = local_tile * 256 + tid;
  const long row = (long)begin + j;
  if (j >= rows || row >= total_rows) return;
  const unsigned* st = state + (size_t)b * kSel * 2;
  // numpy's _lerp on the two float32 order statistics with the float32 weight the host took from the row count
  const float lower = value_of(st[0]), upper = value_of(st[2]);
  const float gamma = __uint_as_float((unsigned)d.select[b * VDETR_HEIGHT_SELECT + 2]);
  const float diff = upper - lower;
  float floor_height;
  if (gamma >= 0.5f) {
    const float rest = 1.0f - gamma, back = diff * rest;
    floor_height = upper - back;
  } else {
    const float step = diff * gamma;
    floor_height = lower + step;
  }
  if (st[4] == 0xffffffffu) floor_height = __builtin_nanf("");         // the last of the sorted column is a NaN: so is the percentile
  const float* src = d.points + (size_t)row * d.W;
  float* out = d.out + (size_t)row * (d.W + 1);
  for (int k = 0; k < d.W; ++k) out[k] = src[k];
  out[d.W] = src[2] - floor_height;
}

// ---- --coloraug_sunrgbd, in place on the normalised colours -------------------------------------------------------------------------
__global__ __launch_bounds__(kTile) void sunrgbd_color_kernel(vdetr_color_aug_desc d, int total_rows) {
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, kTile, t, b, local_tile)) return;   // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int j = local_tile * kTile + tid;
  const long row = (long)begin + j;
  if (j >= rows || row >= total_rows) return;
  const double* q = d.params + (size_t)b * VDETR_COLOR_AUG_PARAMS;
  const float* src = d.points + (size_t)row * d.W + 3;
  float* out = d.out + (size_t)row * d.W + 3;
  const double jitter = d.noise[row];
  const float keep = d.keep[row] ? 1.0f : 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float x = src[k] + 0.5f;
    x = (float)((double)x * q[k]);                                     // a float64 operand: float64, rounded into the float32 cloud
    x = (float)((double)x + q[3 + k]);
    x = (float)((double)x + jitter);
    x = x < 0.0f ? 0.0f : x;                                           // np.clip: a NaN stays
    x = x > 1.0f ? 1.0f : x;
    x = x * keep;
    out[k] = x - 0.5f;
  }
}

// the two workspaces
struct ColorWork {
  float* bounds;      // [tiles, kBound]
  float* scene;       // [B, kBound] lo, hi, scale
};

ColorWork lay_out_color(Carver& c, long tiles, int B) {
  ColorWork w;
  w.bounds = c.take<float>((size_t)tiles * kBound);
  w.scene = c.take<float>((size_t)B * kBound);
  return w;
}

struct HeightWork {
  unsigned* partial;  // [tiles, kSel, kBins] a pass's histograms
  unsigned* state;    // [B, kSel, 2]
};

HeightWork lay_out_height(Carver& c, long tiles, int B) {
  HeightWork w;
  w.partial = c.take<unsigned>((size_t)tiles * kSel * kBins);
  w.state = c.take<unsigned>((size_t)B * kSel * 2);
  return w;
}

int check_desc(const vdetr_color_aug_desc* d, const int32_t* offsets_host, const char* op) {
  VDETR_REQUIRE(d && offsets_host, "%s: null descriptor or offsets", op);
  VDETR_REQUIRE(d->B >= 0 && d->B <= kMaxScenes, "%s: %d scenes (0 .. %d)", op, d->B, kMaxScenes);
  return VDETR_OK;
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_color_aug_workspace_bytes(const int32_t* offsets_host, int B) {
  if (!offsets_host || B <= 0) return 0;
  const long tiles = count_tiles(offsets_host, B, kTile, nullptr);
  if (tiles <= 0) return 0;
  Carver c(nullptr);
  lay_out_color(c, tiles, B);
  return c.bytes() + 256;
}

extern "C" size_t vdetr_append_height_workspace_bytes(const int32_t* offsets_host, int B) {
  if (!offsets_host || B <= 0) return 0;
  const long tiles = count_tiles(offsets_host, B, kSelTile, nullptr);
  if (tiles <= 0) return 0;
  Carver c(nullptr);
  lay_out_height(c, tiles, B);
  return c.bytes() + 256;
}

extern "C" int vdetr_color_augment_f32(const vdetr_color_aug_desc* desc, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
                                       vdetr_stream_t stream) {
  if (int e = check_desc(desc, offsets_host, "color_augment")) return e;
  if (desc->B == 0) return VDETR_OK;
  const vdetr_color_aug_desc& d = *desc;
  VDETR_REQUIRE(d.W >= 6, "color_augment: %d floats per row, rgb sits in columns 3:6", d.W);
  const long tiles = count_tiles(offsets_host, d.B, kTile, "color_augment");
  if (tiles < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(tiles <= 0x7fffffffL / kBound, "color_augment: %ld tiles", tiles);
  VDETR_REQUIRE(d.points && d.offsets && d.out && d.params, "color_augment: null pointer");
  VDETR_REQUIRE(d.points != d.out, "color_augment: out is the input");
  VDETR_REQUIRE(d.noise_rows >= 0 && (d.noise_rows == 0 || d.noise), "color_augment: %d noise rows without noise", d.noise_rows);
  if (int e = require_workspace("color_augment", workspace, workspace_bytes, vdetr_color_aug_workspace_bytes(offsets_host, d.B))) return e;
  Carver c(workspace);
  const ColorWork w = lay_out_color(c, tiles, d.B);
  const int total = (int)offsets_host[d.B];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(color_bounds_kernel, dim3((unsigned)tiles), dim3(kTile), 0, s, d, total, w.bounds);
  hipLaunchKernelGGL(color_scale_kernel, dim3(d.B), dim3(kWave), 0, s, d, (int)tiles, (const float*)w.bounds, w.scene);
  hipLaunchKernelGGL(color_apply_kernel, dim3((unsigned)tiles), dim3(kTile), 0, s, d, total, (const float*)w.scene);
  return check_launch("color_augment");
}

extern "C" int vdetr_append_height_f32(const vdetr_color_aug_desc* desc, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
                                       vdetr_stream_t stream) {
  if (int e = check_desc(desc, offsets_host, "append_height")) return e;
  if (desc->B == 0) return VDETR_OK;
  const vdetr_color_aug_desc& d = *desc;
  VDETR_REQUIRE(d.W >= 3, "append_height: %d floats per row, z sits in column 2", d.W);
  const long tiles = count_tiles(offsets_host, d.B, kSelTile, "append_height");
  if (tiles < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(tiles <= 0x7fffffffL / (kSel * kBins), "append_height: %ld tiles", tiles);
  VDETR_REQUIRE(d.points && d.offsets && d.out && d.select, "append_height: null pointer");
  VDETR_REQUIRE(d.points != d.out, "append_height: out is the input");
  if (int e = require_workspace("append_height", workspace, workspace_bytes, vdetr_append_height_workspace_bytes(offsets_host, d.B))) return e;
  Carver c(workspace);
  const HeightWork w = lay_out_height(c, tiles, d.B);
  const int total = (int)offsets_host[d.B];
  const long write_tiles = count_tiles(offsets_host, d.B, 256, nullptr);
  hipStream_t s = (hipStream_t)stream;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(height_hist_kernel, dim3((unsigned)tiles), dim3(256), 0, s, d, total, shift, (const unsigned*)w.state, w.partial);
    hipLaunchKernelGGL(height_pick_kernel, dim3(d.B), dim3(256), 0, s, d, (int)tiles, shift, (const unsigned*)w.partial, w.state);
  }
  hipLaunchKernelGGL(height_write_kernel, dim3((unsigned)write_tiles), dim3(256), 0, s, d, total, (const unsigned*)w.state);
  return check_launch("append_height");
}

extern "C" int vdetr_sunrgbd_color_f32(const vdetr_color_aug_desc* desc, const int32_t* offsets_host, vdetr_stream_t stream) {
  if (int e = check_desc(desc, offsets_host, "sunrgbd_color")) return e;
  if (desc->B == 0) return VDETR_OK;
  const vdetr_color_aug_desc& d = *desc;
  VDETR_REQUIRE(d.W >= 6, "sunrgbd_color: %d floats per row, rgb sits in columns 3:6", d.W);
  const long tiles = count_tiles(offsets_host, d.B, kTile, "sunrgbd_color");
  if (tiles < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(tiles <= 0x7fffffffL, "sunrgbd_color: %ld tiles", tiles);
  VDETR_REQUIRE(d.points && d.offsets && d.out && d.params && d.noise && d.keep, "sunrgbd_color: null pointer");
  VDETR_REQUIRE(d.noise_rows >= offsets_host[d.B], "sunrgbd_color: %d jitter values for %d rows", d.noise_rows, offsets_host[d.B]);
  hipLaunchKernelGGL(sunrgbd_color_kernel, dim3((unsigned)tiles), dim3(kTile), 0, (hipStream_t)stream, d, (int)offsets_host[d.B]);
  return check_launch("sunrgbd_color");
}
