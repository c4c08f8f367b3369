// scene_prep.hip — a loaded scan -> the model's inputs and the criterion's targets (reference
// datasets/scannet.py:510-626).  Two launches:
//   scene_prep_points_kernel   one workgroup per scene-aligned tile of 256 kept rows: gather through `choices`, flip,
//                              rotate, translate, scale, colour affine, packed store; min / max of the float32 xyz -> one
//                              partial per tile (ordinary stores, no atomics, no ticket: README "Two findings about the chip")
//   scene_prep_targets_kernel  one wave per scene: merges the scene's partials (min / max: any order gives the same bits),
//                              carries the boxes through the same augmentation in fp64 and writes every gt_* tensor.
// The arithmetic follows numpy on the reference's dtypes step by step (include/vdetr_hip.h): the build's -ffp-contract=off
// keeps every product and sum a separate IEEE operation.
#include "scene_tiles.h"

namespace vdetr {
namespace {

constexpr int kTile = VDETR_SCENE_PREP_TILE;

struct ScenePose {
  bool flip_x, flip_y;
  double c, s, tx, ty, tz, scale;
};

__device__ __forceinline__ ScenePose load_pose(const double* params, int b) {
  const double* q = params + (size_t)b * VDETR_SCENE_PREP_PARAMS;
  ScenePose p;
  p.flip_x = q[0] != 0.0;
  p.flip_y = q[1] != 0.0;
  p.c = q[2]; p.s = q[3]; p.tx = q[4]; p.ty = q[5]; p.tz = q[6]; p.scale = q[7];
  return p;
}

// row . rotz(angle)^T as np.dot forms it: every output is the 3-term sum over the row, zeros of the matrix included
__device__ __forceinline__ void rotate_z(const ScenePose& p, double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = (x * p.c + y * (-p.s)) + z * 0.0;
  oy = (x * p.s + y * p.c) + z * 0.0;
  oz = (x * 0.0 + y * 0.0) + z * 1.0;
}

// locate_tile for the kept rows: with num_points every scene keeps that many, the same number of tiles each.  The ragged case
// is locate_tile's / first_tile's loop written out, here and in scene_prep_targets_kernel: called as functions they leave both
// kernels with other instructions
__device__ __forceinline__ bool locate_kept_tile(const vdetr_scene_prep_desc& d, int t, int& b, int& local_tile) {
  if (d.num_points > 0) {
    const int per = tiles_of(d.num_points, kTile);
    b = t / per;
    local_tile = t - b * per;
    return b < d.B;
  }
  int acc = 0;
  for (b = 0; b < d.B; ++b) {
    const int nt = tiles_of(d.offsets[b + 1] - d.offsets[b], kTile);
    if (t < acc + nt) break;
    acc += nt;
  }
  local_tile = t - acc;
  return b < d.B;
}

__global__ __launch_bounds__(kTile) void scene_prep_points_kernel(vdetr_scene_prep_desc d, int total_rows, float* partials) {
  __shared__ float red[kTile / kWave][6];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  const bool found = locate_kept_tile(d, t, b, local_tile);  // uniform over the workgroup
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  if (found) {
    const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
    const int keep = d.num_points > 0 ? d.num_points : rows;
    const int j = local_tile * kTile + tid;
    const long out_row = (d.num_points > 0 ? (long)b * d.num_points : (long)begin) + j;
    const int W = 3 + d.C;
    if (j < keep && (d.num_points > 0 || out_row < total_rows)) {
      long pick = j;
      if (d.num_points > 0) {
        const size_t ci = (size_t)b * d.num_points + j;
        pick = d.choices_i64 ? (long)((const int64_t*)d.choices)[ci] : (long)((const int32_t*)d.choices)[ci];
      }
      float* out = d.out_points + (size_t)out_row * W;
      const long src_row = begin + pick;
      if (pick < 0 || pick >= rows || src_row >= total_rows) {
        for (int k = 0; k < W; ++k) out[k] = __builtin_nanf("");   // the bounds skip the row: fminf / fmaxf drop a NaN
      } else {
        const float* src = d.points + (size_t)src_row * W;
        const ScenePose p = load_pose(d.params, b);
        float x = src[0], y = src[1], z = src[2];
        if (p.flip_x) x = -1.0f * x;
        if (p.flip_y) y = -1.0f * y;
        double rx, ry, rz;
        rotate_z(p, (double)x, (double)y, (double)z, rx, ry, rz);
        x = (float)rx; y = (float)ry; z = (float)rz;                   // each step lands in the float32 cloud
        x = (float)((double)x + p.tx); y = (float)((double)y + p.ty); z = (float)((double)z + p.tz);
        const float sc = (float)p.scale;                               // a Python float there: numpy multiplies in float32
        x = x * sc; y = y * sc; z = z * sc;
        out[0] = x; out[1] = y; out[2] = z;
        lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
        int k = 3;
        if (d.color_mode == VDETR_COLOR_MEAN) {
          const double mean[3] = {109.8, 97.2, 83.8};
          for (; k < 6; ++k) out[k] = (float)(((double)src[k] - mean[k - 3]) / 256.0);
        } else if (d.color_mode == VDETR_COLOR_UNIT) {
          for (; k < 6; ++k) out[k] = src[k] / 255.0f - 0.5f;
        }
        for (; k < W; ++k) out[k] = src[k];
      }
    }
  }
  // every lane is active here (idle ones carry +-inf).  store_tile_partial's body, kept in this form: through the template
  // the compiler orders this kernel's instructions differently
  const int wave = tid / kWave;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mn = wave_allmin_f32(lo[k]), mx = wave_allmax_f32(hi[k]);
    if ((tid & (kWave - 1)) == 0) { red[wave][k] = mn; red[wave][3 + k] = mx; }
  }
  __syncthreads();
  if (tid < 6) {
    float v = red[0][tid];
    for (int w = 1; w < kTile / kWave; ++w) v = tid < 3 ? fminf(v, red[w][tid]) : fmaxf(v, red[w][tid]);
    partials[(size_t)t * 6 + tid] = v;
  }
}

__global__ __launch_bounds__(kWave) void scene_prep_targets_kernel(vdetr_scene_prep_desc d, int num_tiles, const float* partials) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int first = 0, nt;
  if (d.num_points > 0) {
    nt = tiles_of(d.num_points, kTile);
    first = b * nt;
  } else {
    for (int i = 0; i < b; ++i) first += tiles_of(d.offsets[i + 1] - d.offsets[i], kTile);
    nt = tiles_of(d.offsets[b + 1] - d.offsets[b], kTile);
  }
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int i = lane; i < nt && first + i < num_tiles; i += kWave) {
    const float* q = partials + (size_t)(first + i) * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], q[k]); hi[k] = fmaxf(hi[k], q[3 + k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = wave_allmin_f32(lo[k]); hi[k] = wave_allmax_f32(hi[k]); }
  if (lane < 3) {
    d.dims_min[b * 3 + lane] = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lo[2];
    d.dims_max[b * 3 + lane] = lane == 0 ? hi[0] : lane == 1 ? hi[1] : hi[2];
  }

  const ScenePose p = load_pose(d.params, b);
  long count = d.box_counts[b];
  count = count < 0 ? 0 : count > d.G ? d.G : count;
  for (int g = lane; g < d.max_obj; g += kWave) {
    const bool here = g < count;
    float in[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                    // padding rows are zero boxes and take every step too
    long cls = 0;
    if (here) {
      const float* q = d.boxes + ((size_t)b * d.G + g) * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) in[k] = q[k];
      cls = d.box_classes[(size_t)b * d.G + g];
    }
    if (p.flip_x) in[0] = -1.0f * in[0];
    if (p.flip_y) in[1] = -1.0f * in[1];
    // rotate_aligned_boxes (scannet.py:179-199): from here on the box is fp64
    double box[6];
    rotate_z(p, (double)in[0], (double)in[1], (double)in[2], box[0], box[1], box[2]);
    const float hx = in[3] / 2.0f, hy = in[4] / 2.0f;
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float sx = (k == 1 || k == 2) ? 1.0f : -1.0f, sy = k >= 2 ? 1.0f : -1.0f;
      double ex, ey, ez;
      rotate_z(p, (double)(sx * hx), (double)(sy * hy), 0.0, ex, ey, ez);
      mx = k == 0 ? ex : fmax(mx, ex);
      my = k == 0 ? ey : fmax(my, ey);
    }
    box[3] = 2.0 * mx; box[4] = 2.0 * my; box[5] = (double)in[5];
    box[0] = box[0] + p.tx; box[1] = box[1] + p.ty; box[2] = box[2] + p.tz;
#pragma unroll
    for (int k = 0; k < 6; ++k) box[k] = box[k] * p.scale;

    const size_t r = (size_t)b * d.max_obj + g;
    float cen[3], siz[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cen[k] = (float)box[k];
      siz[k] = (float)box[3 + k];
      d.centers[r * 3 + k] = cen[k];
      d.sizes[r * 3 + k] = siz[k];
      // shift_scale_points to [0, 1] and scale_points by 1 / extent, in float32 (pc_util.py:38-73)
      const float ext = hi[k] - lo[k];
      const float nrm = ((cen[k] - lo[k]) * 1.0f) / ext + 0.0f;
      d.centers_norm[r * 3 + k] = nrm * (here ? 1.0f : 0.0f);
      d.sizes_norm[r * 3 + k] = siz[k] * (1.0f / ext);
      float res = 0.f;
      if (here) res = (cls >= 0 && cls < d.num_classes) ? (float)(box[3 + k] - d.mean_size[cls * 3 + k]) : __builtin_nanf("");
      d.size_residual[r * 3 + k] = res;
    }
    // box_parametrization_to_corners_np at angle 0: camera frame (x, -z, y), sizes (l, w, h) on (x, z, y); fp64 sums
    const float ccx = cen[0], ccy = -1.0f * cen[2], ccz = cen[1];
    const float l2 = siz[0] / 2.0f, w2 = siz[1] / 2.0f, h2 = siz[2] / 2.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float vx = ((k >> 1) & 1) ? -l2 : l2;
      const float vy = k >= 4 ? -h2 : h2;
      const float vz = (k == 0 || k == 3 || k == 4 || k == 7) ? w2 : -w2;
      float* o = d.corners + (r * 8 + k) * 3;
      o[0] = (float)((double)vx + (double)ccx);
      o[1] = (float)((double)vy + (double)ccy);
      o[2] = (float)((double)vz + (double)ccz);
    }
    d.sem_cls[r] = here ? cls : 0;
    d.present[r] = here ? 1.0f : 0.0f;
    d.angle_class[r] = 0;
    d.angle_residual[r] = 0.f;
    d.angles[r] = 0.f;
  }
}

// count_tiles for the kept rows: num_points per scene where it is given; the offsets are checked either way
long count_kept_tiles(const int32_t* offsets_host, int B, int num_points, const char* op) {
  const long tiles = count_tiles(offsets_host, B, kTile, op);
  return tiles < 0 || num_points <= 0 ? tiles : (long)B * ((num_points + kTile - 1) / kTile);
}

// the workspace: 6 floats per tile
float* lay_out(Carver& c, long tiles) { return c.take_unpadded<float>((size_t)tiles * 6); }

int check_desc(const vdetr_scene_prep_desc* d, const int32_t* offsets_host, const void* workspace, size_t workspace_bytes,
               long* tiles) {
  VDETR_REQUIRE(d && offsets_host, "scene_prep: null descriptor or offsets");
  VDETR_REQUIRE(d->B >= 0 && d->C >= 0 && d->G >= 0 && d->max_obj >= 0 && d->num_points >= 0, "scene_prep: negative dimension");
  VDETR_REQUIRE(d->B <= kMaxScenes, "scene_prep: %d scenes > %d", d->B, kMaxScenes);
  VDETR_REQUIRE(d->G <= d->max_obj, "scene_prep: %d box slots > max_obj %d", d->G, d->max_obj);
  VDETR_REQUIRE(d->color_mode == VDETR_COLOR_KEEP || ((d->color_mode == VDETR_COLOR_MEAN || d->color_mode == VDETR_COLOR_UNIT) && d->C >= 3),
                "scene_prep: color_mode %d with %d feature columns", d->color_mode, d->C);
  *tiles = count_kept_tiles(offsets_host, d->B, d->num_points, "scene_prep");
  if (*tiles < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(*tiles <= 0x7fffffffL, "scene_prep: %ld tiles", *tiles);
  const size_t need = vdetr_scene_prep_workspace_bytes(offsets_host, d->B, d->num_points);
  return d->B > 0 ? require_workspace("scene_prep", workspace, workspace_bytes, need) : VDETR_OK;
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_scene_prep_workspace_bytes(const int32_t* offsets_host, int B, int num_points) {
  if (!offsets_host || B <= 0 || num_points < 0) return 0;
  const long tiles = count_kept_tiles(offsets_host, B, num_points, nullptr);
  if (tiles <= 0) return 0;
  Carver c(nullptr);
  lay_out(c, tiles);
  return c.bytes() + 256;
}

extern "C" int vdetr_scene_prep_points_f32(const vdetr_scene_prep_desc* desc, const int32_t* offsets_host, void* workspace,
                                           size_t workspace_bytes, vdetr_stream_t stream) {
  long tiles = 0;
  if (int e = check_desc(desc, offsets_host, workspace, workspace_bytes, &tiles)) return e;
  if (desc->B == 0) return VDETR_OK;
  VDETR_REQUIRE(desc->points && desc->offsets && desc->params && desc->out_points, "scene_prep_points: null pointer");
  VDETR_REQUIRE(desc->num_points == 0 || desc->choices, "scene_prep_points: num_points %d without choices", desc->num_points);
  Carver c(workspace);
  hipLaunchKernelGGL(scene_prep_points_kernel, dim3((unsigned)tiles), dim3(kTile), 0, (hipStream_t)stream, *desc,
                     (int)offsets_host[desc->B], lay_out(c, tiles));
  return check_launch("scene_prep_points");
}

extern "C" int vdetr_scene_prep_targets_f32(const vdetr_scene_prep_desc* desc, const int32_t* offsets_host, const void* workspace,
                                            size_t workspace_bytes, vdetr_stream_t stream) {
  long tiles = 0;
  if (int e = check_desc(desc, offsets_host, workspace, workspace_bytes, &tiles)) return e;
  if (desc->B == 0) return VDETR_OK;
  const vdetr_scene_prep_desc& d = *desc;
  VDETR_REQUIRE(d.offsets && d.params && d.box_counts && d.mean_size && d.dims_min && d.dims_max && d.corners && d.centers &&
                    d.centers_norm && d.sizes && d.sizes_norm && d.size_residual && d.angle_class && d.sem_cls &&
                    d.angle_residual && d.angles && d.present,
                "scene_prep_targets: null pointer");
  VDETR_REQUIRE(d.G == 0 || (d.boxes && d.box_classes), "scene_prep_targets: %d box slots without boxes or classes", d.G);
  Carver c(workspace);
  hipLaunchKernelGGL(scene_prep_targets_kernel, dim3(d.B), dim3(kWave), 0, (hipStream_t)stream, d, (int)tiles,
                     (const float*)lay_out(c, tiles));
  return check_launch("scene_prep_targets");
}
