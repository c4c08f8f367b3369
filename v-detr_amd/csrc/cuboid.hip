// cuboid.hip — the cuboid crop of a training scene (reference utils/random_cuboid.py:38-98 as called from
// datasets/scannet.py:476-498).  The host draws every scene's attempts (crop ranges, centre rows: scene_prep.draw_cuboid_trials)
// and uploads one table; every attempt is then decided here at once.  vdetr_cuboid_crop_f32 is five launches:
//   cuboid_bounds_kernel   one workgroup per scene-aligned tile of 256 raw rows: float32 min / max of xyz -> one partial per tile
//   cuboid_boxes_kernel    one wave per scene: merges the partials into range_xyz, one lane per attempt forms the crop box
//   cuboid_count_kernel    one workgroup per tile: the tile's rows sit in LDS, one lane per ATTEMPT walks them and keeps the
//                          count and the float32 min / max of the rows inside -> one partial per (tile, attempt)
//   cuboid_select_kernel   one workgroup per scene: one lane per attempt sums the partials in tile order and applies the three
//                          conditions; the first accepted attempt wins; the box list is compacted in order; the winning
//                          attempt's counts become the tiles' output offsets
//   cuboid_compact_kernel  one workgroup per tile: a ballot scan of the winning attempt's rows -> kept_rows, ascending
// and vdetr_cuboid_compose_i32 one: choices[b, j] = kept_rows[b][drawn[b, j]].  Partials go out with ordinary stores: no
// atomics, no ticket, nothing that depends on scheduling (README "Two findings about the chip"), so two runs give the same
// bits.  Every decision is a comparison of exactly defined values (include/vdetr_hip.h), -ffp-contract=off as everywhere.
#include "block_scan.h"
#include "scene_tiles.h"

namespace vdetr {
namespace {

constexpr int kTile = VDETR_CUBOID_TILE;
constexpr int kStat = 7;          // words per (tile, attempt): count, min xyz, max xyz
constexpr int kBound = 9;         // floats per tile of the raw bounds: min xyz, max xyz, "holds a NaN" xyz

// the workspace
struct Work {
  float* bounds;      // [tiles, kBound]
  double* crop;       // [B, T, 6] max xyz, min xyz of every attempt (NaN: the attempt is not valid)
  int32_t* stats;     // [tiles, T, kStat]
  int32_t* tile_base; // [tiles] rows the winning attempt keeps in the scene's earlier tiles
};

Work lay_out(Carver& c, long tiles, int B, int T) {
  Work w;
  w.bounds = c.take<float>((size_t)tiles * kBound);
  w.crop = c.take<double>((size_t)B * T * 6);
  w.stats = c.take<int32_t>((size_t)tiles * T * kStat);
  w.tile_base = c.take<int32_t>((size_t)tiles);
  return w;
}

__global__ __launch_bounds__(kTile) void cuboid_bounds_kernel(vdetr_cuboid_desc d, int total_rows, float* bounds) {
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
      const float* src = d.points + (size_t)(begin + j) * d.W;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float x = src[k];
        if (x != x) v[6 + k] = 1.f;                                    // np.max / np.min hand a NaN on: so does the range
        else v[k] = v[3 + k] = x;
      }
    }
  }
  store_tile_partial(v, red, bounds, t);
}

__global__ __launch_bounds__(kWave) void cuboid_boxes_kernel(vdetr_cuboid_desc d, int num_tiles, int total_rows, const float* bounds,
                                                             double* crop) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int first = first_tile(d.offsets, b, kTile), nt = tiles_of(rows, kTile);
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, bad[3] = {0.f, 0.f, 0.f};
  for (int i = lane; i < nt && first + i < num_tiles; i += kWave) {
    const float* q = bounds + (size_t)(first + i) * kBound;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], q[k]); hi[k] = fmaxf(hi[k], q[3 + k]); bad[k] = fmaxf(bad[k], q[6 + k]); }
  }
  float range[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = wave_allmin_f32(lo[k]); hi[k] = wave_allmax_f32(hi[k]); bad[k] = wave_allmax_f32(bad[k]);
    range[k] = bad[k] != 0.f ? __builtin_nanf("") : hi[k] - lo[k];     // float32 max minus float32 min, in float32
  }
  for (int a = lane; a < d.T; a += kWave) {
    const double* q = d.trials + ((size_t)b * (d.T + 1) + a) * VDETR_CUBOID_TRIAL;
    double* o = crop + ((size_t)b * d.T + a) * 6;
    const double centre = q[3];
    const long row = (long)centre;
    const bool valid = centre >= 0.0 && row < rows && begin + row < total_rows;
    const float* c = d.points + (size_t)(begin + (valid ? row : 0)) * d.W;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double half = ((double)range[k] * q[k]) / 2.0;             // new_range = range_xyz * crop_range / 2.0 in float64
      o[k] = valid ? (double)c[k] + half : __builtin_nan("");          // a NaN bound: no row is inside
      o[3 + k] = valid ? (double)c[k] - half : __builtin_nan("");
    }
  }
}

// one lane per attempt over the tile's rows in LDS (every lane reads the same address: a broadcast).  Both comparisons are
// false for a NaN coordinate and for a NaN bound.
__global__ __launch_bounds__(VDETR_CUBOID_ATTEMPT_LANES) void cuboid_count_kernel(vdetr_cuboid_desc d, int total_rows, const double* crop,
                                                                                  int32_t* stats) {
  __shared__ float xyz[kTile][3];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, kTile, t, b, local_tile)) return;          // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int base = local_tile * kTile;
  int here = rows - base;
  here = here > kTile ? kTile : here;
  for (int j = tid; j < here; j += VDETR_CUBOID_ATTEMPT_LANES) {
    const long row = (long)begin + base + j;
    const float* src = d.points + (size_t)(row < total_rows ? row : 0) * d.W;
    const bool ok = row < total_rows;
    xyz[j][0] = ok ? src[0] : __builtin_nanf("");
    xyz[j][1] = ok ? src[1] : __builtin_nanf("");
    xyz[j][2] = ok ? src[2] : __builtin_nanf("");
  }
  __syncthreads();
  const float inf = __builtin_huge_valf();
  for (int a = tid; a < d.T; a += VDETR_CUBOID_ATTEMPT_LANES) {
    const double* q = crop + ((size_t)b * d.T + a) * 6;
    const double hx = q[0], hy = q[1], hz = q[2], lx = q[3], ly = q[4], lz = q[5];
    int count = 0;
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (int j = 0; j < here; ++j) {
      const float x = xyz[j][0], y = xyz[j][1], z = xyz[j][2];
      const bool in = (double)x <= hx && (double)y <= hy && (double)z <= hz && (double)x >= lx && (double)y >= ly && (double)z >= lz;
      if (in) {
        ++count;
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
      }
    }
    int32_t* o = stats + ((size_t)t * d.T + a) * kStat;
    o[0] = count;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[1 + k] = (int32_t)__float_as_uint(mn[k]); o[4 + k] = (int32_t)__float_as_uint(mx[k]); }
  }
}

template <typename T>
__device__ __forceinline__ bool centre_inside(const T* box, const float* mn, const float* mx) {
  // the centres in their own dtype against the float32 bounds of the kept rows, both ends inclusive
  return (double)box[0] >= (double)mn[0] && (double)box[1] >= (double)mn[1] && (double)box[2] >= (double)mn[2] &&
         (double)box[0] <= (double)mx[0] && (double)box[1] <= (double)mx[1] && (double)box[2] <= (double)mx[2];
}

__device__ __forceinline__ bool box_inside(const vdetr_cuboid_desc& d, int b, int g, const float* mn, const float* mx) {
  const size_t at = ((size_t)b * d.G + g) * 6;
  return d.boxes_f64 ? centre_inside((const double*)d.boxes + at, mn, mx) : centre_inside((const float*)d.boxes + at, mn, mx);
}

__global__ __launch_bounds__(VDETR_CUBOID_ATTEMPT_LANES) void cuboid_select_kernel(vdetr_cuboid_desc d, int num_tiles, const int32_t* stats,
                                                                                   int32_t* tile_base) {
  __shared__ int win[VDETR_CUBOID_ATTEMPT_LANES / kWave];
  __shared__ float win_box[6];
  __shared__ int win_count;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int rows = d.offsets[b + 1] - d.offsets[b];
  const int first = first_tile(d.offsets, b, kTile), nt = tiles_of(rows, kTile);
  long nbox = d.box_counts[b];
  nbox = nbox < 0 ? 0 : nbox > d.G ? d.G : nbox;
  const bool filter = d.trials[((size_t)b * (d.T + 1) + d.T) * VDETR_CUBOID_TRIAL] != 0.0;
  const float inf = __builtin_huge_valf();

  // the first accepted attempt of each lane's own (a, a + lanes, ...), then the smallest over the workgroup
  int mine = 0x7fffffff, mine_count = 0;
  float mine_box[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (int a = tid; a < d.T && mine == 0x7fffffff; a += VDETR_CUBOID_ATTEMPT_LANES) {
    const bool valid = d.trials[((size_t)b * (d.T + 1) + a) * VDETR_CUBOID_TRIAL + 3] >= 0.0;
    int count = 0;
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (int i = 0; i < nt && first + i < num_tiles; ++i) {
      const int32_t* q = stats + ((size_t)(first + i) * d.T + a) * kStat;
      count += q[0];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        mn[k] = fminf(mn[k], __uint_as_float((unsigned)q[1 + k]));
        mx[k] = fmaxf(mx[k], __uint_as_float((unsigned)q[4 + k]));
      }
    }
    bool ok = valid && count >= d.min_points && count > 0;
    if (ok && filter) {
      bool any = false;
      for (int g = 0; g < nbox && !any; ++g) any = box_inside(d, b, g, mn, mx);
      ok = any;
    }
    if (ok) {
      mine = a;
      mine_count = count;
#pragma unroll
      for (int k = 0; k < 3; ++k) { mine_box[k] = mn[k]; mine_box[3 + k] = mx[k]; }
    }
  }
  const unsigned best_in_wave = wave_allmin_u32((unsigned)mine);
  if ((tid & (kWave - 1)) == 0) win[tid / kWave] = (int)best_in_wave;
  __syncthreads();
  int trial = win[0];
#pragma unroll
  for (int w = 1; w < VDETR_CUBOID_ATTEMPT_LANES / kWave; ++w) trial = min(trial, win[w]);
  if (mine == trial && trial != 0x7fffffff) {                          // exactly one lane owns the winning attempt
    win_count = mine_count;
#pragma unroll
    for (int k = 0; k < 6; ++k) win_box[k] = mine_box[k];
  }
  __syncthreads();
  const bool accepted = trial != 0x7fffffff;
  if (!accepted) trial = -1;

  // the tiles' output offsets: the winning attempt's counts in tile order; every row on the fallback
  if (tid == 0) {
    int acc = 0;
    for (int i = 0; i < nt && first + i < num_tiles; ++i) {
      tile_base[first + i] = acc;
      int here = rows - i * kTile;
      here = here > kTile ? kTile : here;
      acc += accepted ? stats[((size_t)(first + i) * d.T + trial) * kStat] : here;
    }
  }

  // the box list, compacted in its order by the first wave; rows past the kept ones are zero
  if (tid < kWave) {
    const bool sift = accepted && filter;
    int kept = 0;
    for (int g0 = 0; g0 < d.G; g0 += kWave) {
      const int g = g0 + tid;
      const bool keep = g < nbox && (!sift || box_inside(d, b, g, win_box, win_box + 3));
      const unsigned long long mask = __ballot(keep);
      if (keep) {
        const int to = kept + __popcll(mask & ((1ull << tid) - 1ull));
        const size_t src = ((size_t)b * d.G + g) * 6, dst = ((size_t)b * d.G + to) * 6;
        for (int k = 0; k < 6; ++k) {
          if (d.boxes_f64) ((double*)d.out_boxes)[dst + k] = ((const double*)d.boxes)[src + k];
          else ((float*)d.out_boxes)[dst + k] = ((const float*)d.boxes)[src + k];
        }
        d.out_classes[(size_t)b * d.G + to] = d.box_classes[(size_t)b * d.G + g];
      }
      kept += __popcll(mask);
    }
    for (int g = kept + tid; g < d.G; g += kWave) {
      const size_t dst = ((size_t)b * d.G + g) * 6;
      for (int k = 0; k < 6; ++k) {
        if (d.boxes_f64) ((double*)d.out_boxes)[dst + k] = 0.0;
        else ((float*)d.out_boxes)[dst + k] = 0.f;
      }
      d.out_classes[(size_t)b * d.G + g] = 0;
    }
    if (tid == 0) {
      d.out_counts[b] = kept;
      d.result[b * VDETR_CUBOID_RESULT + 0] = trial;
      d.result[b * VDETR_CUBOID_RESULT + 1] = accepted ? win_count : rows;
      d.result[b * VDETR_CUBOID_RESULT + 2] = kept;
      d.result[b * VDETR_CUBOID_RESULT + 3] = 0;
    }
  }
}

__global__ __launch_bounds__(kTile) void cuboid_compact_kernel(vdetr_cuboid_desc d, int total_rows, const double* crop,
                                                               const int32_t* tile_base) {
  __shared__ int wave_count[kTile / kWave];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, kTile, t, b, local_tile)) return;          // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int trial = d.result[b * VDETR_CUBOID_RESULT], kept_rows = d.result[b * VDETR_CUBOID_RESULT + 1];
  const int j = local_tile * kTile + tid;
  bool in = j < rows && begin + j < total_rows;
  if (in && trial >= 0) {
    const double* q = crop + ((size_t)b * d.T + trial) * 6;
    const float* src = d.points + (size_t)(begin + j) * d.W;
    const float x = src[0], y = src[1], z = src[2];
    in = (double)x <= q[0] && (double)y <= q[1] && (double)z <= q[2] && (double)x >= q[3] && (double)y >= q[4] && (double)z >= q[5];
  }
  int in_tile;
  const int to = tile_base[t] + block_rank<kTile>(in, wave_count, in_tile);
  if (in && to < kept_rows && to < rows) d.kept_rows[begin + to] = j;   // the counts and this test agree: the bound is a guard
}

__global__ __launch_bounds__(256) void cuboid_compose_kernel(vdetr_cuboid_desc d, int total_rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)d.B * d.num_points) return;
  const int b = (int)(i / d.num_points);
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int kept = d.result[b * VDETR_CUBOID_RESULT + 1];
  const int pick = d.drawn[i];
  const bool ok = pick >= 0 && pick < kept && pick < rows && begin + pick < total_rows;
  d.choices[i] = ok ? d.kept_rows[begin + pick] : -1;                  // prepare_scenes turns a row outside its scene into NaN
}

int check_desc(const vdetr_cuboid_desc* d, const int32_t* offsets_host, const char* op) {
  VDETR_REQUIRE(d && offsets_host, "%s: null descriptor or offsets", op);
  VDETR_REQUIRE(d->B >= 0 && d->W >= 3 && d->G >= 0 && d->num_points >= 0, "%s: bad dimension (B %d, W %d, G %d, num_points %d)", op,
                d->B, d->W, d->G, d->num_points);
  VDETR_REQUIRE(d->B <= kMaxScenes, "%s: %d scenes > %d", op, d->B, kMaxScenes);
  VDETR_REQUIRE(d->T >= 1 && d->T <= VDETR_CUBOID_MAX_TRIALS, "%s: %d attempts (1 .. %d)", op, d->T, VDETR_CUBOID_MAX_TRIALS);
  VDETR_REQUIRE(d->min_points >= 1, "%s: min_points %d < 1", op, d->min_points);
  return VDETR_OK;
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_cuboid_workspace_bytes(const int32_t* offsets_host, int B, int T) {
  if (!offsets_host || B <= 0 || T <= 0) return 0;
  const long tiles = count_tiles(offsets_host, B, kTile, nullptr);
  if (tiles <= 0) return 0;
  Carver c(nullptr);
  lay_out(c, tiles, B, T);
  return c.bytes() + 256;
}

extern "C" int vdetr_cuboid_crop_f32(const vdetr_cuboid_desc* desc, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
                                     vdetr_stream_t stream) {
  if (int e = check_desc(desc, offsets_host, "cuboid_crop")) return e;
  if (desc->B == 0) return VDETR_OK;
  const vdetr_cuboid_desc& d = *desc;
  const long tiles = count_tiles(offsets_host, d.B, kTile, "cuboid");
  if (tiles < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(tiles <= 0x7fffffffL / (d.T * kStat), "cuboid_crop: %ld tiles x %d attempts", tiles, d.T);
  VDETR_REQUIRE(d.points && d.offsets && d.trials && d.box_counts && d.out_counts && d.result && d.kept_rows, "cuboid_crop: null pointer");
  VDETR_REQUIRE(d.G == 0 || (d.boxes && d.box_classes && d.out_boxes && d.out_classes), "cuboid_crop: %d box slots without boxes or classes",
                d.G);
  if (int e = require_workspace("cuboid_crop", workspace, workspace_bytes, vdetr_cuboid_workspace_bytes(offsets_host, d.B, d.T))) return e;
  Carver carver(workspace);
  const Work c = lay_out(carver, tiles, d.B, d.T);
  const int total = (int)offsets_host[d.B];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cuboid_bounds_kernel, dim3((unsigned)tiles), dim3(kTile), 0, s, d, total, c.bounds);
  hipLaunchKernelGGL(cuboid_boxes_kernel, dim3(d.B), dim3(kWave), 0, s, d, (int)tiles, total, (const float*)c.bounds, c.crop);
  hipLaunchKernelGGL(cuboid_count_kernel, dim3((unsigned)tiles), dim3(VDETR_CUBOID_ATTEMPT_LANES), 0, s, d, total, (const double*)c.crop,
                     c.stats);
  hipLaunchKernelGGL(cuboid_select_kernel, dim3(d.B), dim3(VDETR_CUBOID_ATTEMPT_LANES), 0, s, d, (int)tiles, (const int32_t*)c.stats,
                     c.tile_base);
  hipLaunchKernelGGL(cuboid_compact_kernel, dim3((unsigned)tiles), dim3(kTile), 0, s, d, total, (const double*)c.crop,
                     (const int32_t*)c.tile_base);
  return check_launch("cuboid_crop");
}

extern "C" int vdetr_cuboid_compose_i32(const vdetr_cuboid_desc* desc, const int32_t* offsets_host, vdetr_stream_t stream) {
  if (int e = check_desc(desc, offsets_host, "cuboid_compose")) return e;
  if (desc->B == 0) return VDETR_OK;
  const vdetr_cuboid_desc& d = *desc;
  if (count_tiles(offsets_host, d.B, kTile, "cuboid") < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(d.num_points >= 1, "cuboid_compose: num_points %d < 1", d.num_points);
  VDETR_REQUIRE(d.offsets && d.result && d.kept_rows && d.drawn && d.choices, "cuboid_compose: null pointer");
  const long n = (long)d.B * d.num_points;
  VDETR_REQUIRE(n <= 0x7fffffffL, "cuboid_compose: %ld choices", n);
  hipLaunchKernelGGL(cuboid_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d,
                     (int)offsets_host[d.B]);
  return check_launch("cuboid_compose");
}
