// scene_tiles.h — what the loader chain's files share (scene_prep.hip, cuboid.hip, color_aug.hip, normals.hip, scan_export.hip; DESIGN.md
// 6.4 "Scene-aligned tiles, partials and the workspace carver").  A packed batch is cut into tiles of `tile` rows that never
// straddle scenes; a workgroup finds its scene by adding up the tile counts of the device offsets (B <= kMaxScenes).  A
// per-scene min / max goes through ONE partial per tile, written with ordinary stores, which one wave per scene merges in a
// second launch: no atomics, no ticket, and float min / max give the same bits in any order.  The host half sizes the grid
// from the host offsets; the workspace carver these files began with now serves the whole library from workspace.h.
#pragma once
#include "wave.h"
#include "workspace.h"

namespace vdetr {

constexpr int kMaxScenes = 4096;

// ---- device: tiles ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tiles_of(int rows, int tile) { return (rows + tile - 1) / tile; }

// scene and tile within it of tile t; uniform over the workgroup.  false: t lies past the last scene's tiles
__device__ __forceinline__ bool locate_tile(const int32_t* offsets, int B, int tile, int t, int& b, int& local_tile) {
  int acc = 0;
  for (b = 0; b < B; ++b) {
    const int nt = tiles_of(offsets[b + 1] - offsets[b], tile);
    if (t < acc + nt) break;
    acc += nt;
  }
  local_tile = t - acc;
  return b < B;
}

__device__ __forceinline__ int first_tile(const int32_t* offsets, int b, int tile) {
  int first = 0;
  for (int i = 0; i < b; ++i) first += tiles_of(offsets[i + 1] - offsets[i], tile);
  return first;
}

// ---- device: partials ---------------------------------------------------------------------------------------------------------
// K values per lane -> partials[t * K + k]: the first three reduced by min over the workgroup, the rest by max (DPP within
// the wave, one LDS row per wave across them).  Every lane of the workgroup calls it; idle ones carry the identities.
// (scene_prep_points_kernel keeps its own K = 6 copy for the same reason as below.)
template <int K, int WAVES>
__device__ __forceinline__ void store_tile_partial(const float (&v)[K], float (&red)[WAVES][K], float* partials, int t) {
  const int tid = threadIdx.x, wave = tid / kWave;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float r = k < 3 ? wave_allmin_f32(v[k]) : wave_allmax_f32(v[k]);
    if ((tid & (kWave - 1)) == 0) red[wave][k] = r;
  }
  __syncthreads();
  if (tid < K) {
    float r = red[0][tid];
    for (int w = 1; w < WAVES; ++w) r = tid < 3 ? fminf(r, red[w][tid]) : fmaxf(r, red[w][tid]);
    partials[(size_t)t * K + tid] = r;
  }
}

// The second half of the pattern, one wave per scene folding its tiles' partials (fminf / fmaxf per lane, then wave_allmin /
// wave_allmax), is written out in cuboid_boxes_kernel, color_scale_kernel and scene_prep_targets_kernel: as a template the
// compiler simplifies the loop before it inlines it and each of the three kernels comes out with other instructions.

// ---- host: the grid ----------------------------------------------------------------------------------------------------------
// number of tiles, or -1 if the host offsets are unusable (with the error set if `op` is given)
inline long count_tiles(const int32_t* offsets_host, int B, int tile, const char* op) {
  long tiles = 0;
  for (int b = 0; b < B; ++b) {
    const long n = (long)offsets_host[b + 1] - offsets_host[b];
    if (n <= 0 || offsets_host[b] < 0) {
      if (op) set_error("%s: scene %d has no points (offsets %d .. %d)", op, b, offsets_host[b], offsets_host[b + 1]);
      return -1;
    }
    tiles += (n + tile - 1) / tile;
  }
  return tiles;
}

}  // namespace vdetr
