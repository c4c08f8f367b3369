// sparse_voxel.hip — from a raw cloud to the sites of tensor stride 1: voxel keys, the site / inverse / first / segment maps behind
// a stable key sort, the quantisation modes (sum, average, max, first) with their gradients, and the label rule.  gfx950.
//
// Reference: ME.SparseTensor(features, coordinates=ME.utils.batch_sparse_collate([(p[:, :3] / voxel_size, ...)])) of
// models/model_vdetr.py:248-259, ME.SparseTensorQuantizationMode, ME.utils.sparse_quantize and TensorField.  MinkowskiEngine is
// un-vendored: what is this package's own definition (site order, fold order, winners) is DESIGN 6.15.
//
// Keys.  One thread per point: the scene of a row is a binary search of the device offsets (B + 1 words, no per-scene launch and
// no host loop), the voxel index is floorf(p * inv) with inv = (float)(1.0 / voxel_size), taken in double and rounded ONCE on the
// host — the arithmetic of ATen's `tensor / python_float` on the device, which multiplies by a reciprocal instead of dividing, as
// measured against the device expression itself.  A
// point that no key can hold (sparse_key.h; a non-finite coordinate as well) gets the key -1, which sorts first: after the sort
// ONE comparison of the first sorted key is the range flag.  No memset, no atomics, every thread writes only its own key.
//
// Sites.  The two-launch compaction of block_scan.h over tiles of kVoxelTile SORTED keys and the sort's permutation.  What is
// counted are the run heads (key[i] != key[i - 1]).  Launch 2 writes, per sorted position i of site row r: inverse[order[i]] = r,
// order32[i]; per head: sites[r], first[r] = order[i] (the stable sort makes the head the lowest input row of the run),
// seg[r] = i.  The workgroup of the last tile writes seg[M], M and the flag (or, in its place, the highest batch index + 1: the
// last key holds it).
// A run may cross tiles or be longer than one: the site row is a global prefix of the heads, nothing is per tile but the count.
//
// Features.  One lane per (site, channel) folds the run in ascending input-row order in float32: two runs agree bit for bit and
// np.add.at / np.maximum.at restate it.  Adjacent lanes read adjacent channels of one row.  A run of L points costs L dependent
// loads on its lanes while the other lanes of the wave idle: L = N (every point in one voxel) is one workgroup's serial walk of
// the whole table.  Real clouds at 1-5 cm voxels have runs of 1-8.  The gradients are gathers through `inverse`.
#include "block_scan.h"
#include "sparse_key.h"
#include "workspace.h"

namespace vdetr {

constexpr int kVoxelThreads = 256;
constexpr int kVoxelItems = 4;                             // consecutive sorted keys per thread
constexpr int kVoxelTile = kVoxelThreads * kVoxelItems;    // sorted keys per workgroup (vdetr_sp_voxel_tile)

// ---- keys --------------------------------------------------------------------------------------------------------------------------
// the voxel index of one coordinate, or an index no key holds (1 << 20) where the coordinate or its product has none
__device__ __forceinline__ int voxel_index(float p, float inv) {
  const float f = floorf(p * inv);
  return (f >= -32768.f && f <= 32767.f) ? (int)f : (1 << 20);  // (a NaN fails both comparisons)
}

struct VoxelKeysParams {
  int N, B, stride;
  float inv;
  const float* points;
  const int32_t* offsets;
  int64_t* keys;
};

__global__ __launch_bounds__(256) void voxel_keys_kernel(VoxelKeysParams P) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= P.N) return;
  // the scene b with offsets[b] <= i < offsets[b + 1]: the last b whose offset is <= i (empty scenes share an offset: the last wins)
  int lo = 0, hi = P.B;  // invariant: offsets[lo] <= i, and offsets[hi] > i or hi == B
  while (hi - lo > 1) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (P.offsets[mid] <= i) lo = mid; else hi = mid;
  }
  const bool inside = P.offsets[lo] <= i && i < P.offsets[lo + 1];
  const float* p = P.points + (size_t)i * P.stride;
  const int x = voxel_index(p[0], P.inv), y = voxel_index(p[1], P.inv), z = voxel_index(p[2], P.inv);
  P.keys[i] = key_pack(inside ? lo : -1, x, y, z);
}

struct CoordKeysParams {
  int N;
  const int32_t* coords;  // [N, 4]
  int64_t* keys;
};

__global__ __launch_bounds__(256) void coord_keys_kernel(CoordKeysParams P) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= P.N) return;
  const int4 c = reinterpret_cast<const int4*>(P.coords)[i];
  P.keys[i] = key_pack(c.x, c.y, c.z, c.w);
}

// The candidate keys of a region (expand_coordinates): one thread per (offset k, site i) writes cand[k * N + i], the key
// of site i moved by offsets[k] (key_shift) — offset-major, so that adjacent lanes read adjacent keys and write adjacent
// candidates.  A coordinate that leaves its field makes the whole candidate -1, the range flag of the keys above.
struct RegionKeysParams {
  int N;
  long long total;         // K * N < 2^31
  const int64_t* keys;     // [N]
  const int32_t* offsets;  // [K, 3]
  int64_t* cand;           // [K * N]
};

__global__ __launch_bounds__(256) void region_keys_kernel(RegionKeysParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= P.total) return;
  const int k = (int)(t / P.N);
  const int i = (int)(t - (long long)k * P.N);
  const int32_t* o = P.offsets + (size_t)k * 3;
  P.cand[t] = key_shift(P.keys[i], o[0], o[1], o[2]);
}

// ---- sites -------------------------------------------------------------------------------------------------------------------------
struct VoxelSitesParams {
  int N, tiles;
  const int64_t* sorted;   // [N] ascending
  const int64_t* order;    // [N] the stable sort's permutation
  int64_t* sites;          // [N], M written
  int64_t* first;          // [N], M written
  int32_t* inverse;        // [N]
  int32_t* order32;        // [N]
  int32_t* seg;            // [N + 1], M + 1 written
  int32_t* count;          // [2]: M; -1 (range flag) or the highest batch index + 1
  int* tile_counts;        // [tiles]
};

__device__ __forceinline__ bool run_head(const int64_t* sorted, int i) { return i == 0 || sorted[i] != sorted[i - 1]; }

__global__ __launch_bounds__(kVoxelThreads) void voxel_heads_kernel(VoxelSitesParams P) {
  __shared__ int wave_sums[kVoxelThreads / kWave];
  const int first = (int)blockIdx.x * kVoxelTile + (int)threadIdx.x * kVoxelItems;
  int heads = 0;
#pragma unroll
  for (int e = 0; e < kVoxelItems; ++e)
    if (first + e < P.N) heads += run_head(P.sorted, first + e) ? 1 : 0;
  int total;
  block_exclusive_sum<kVoxelThreads>(heads, wave_sums, total);
  if (threadIdx.x == 0) P.tile_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_fill_kernel(VoxelSitesParams P) {
  __shared__ int wave_sums[kVoxelThreads / kWave];
  // heads in the earlier tiles
  const int before = block_sum<kVoxelThreads>((int)blockIdx.x, [&](int t) { return P.tile_counts[t]; }, wave_sums);
  const int first = (int)blockIdx.x * kVoxelTile + (int)threadIdx.x * kVoxelItems;
  bool h[kVoxelItems];
  int heads = 0;
#pragma unroll
  for (int e = 0; e < kVoxelItems; ++e) {
    h[e] = first + e < P.N && run_head(P.sorted, first + e);
    heads += h[e] ? 1 : 0;
  }
  int total;
  int rank = before + block_exclusive_sum<kVoxelThreads>(heads, wave_sums, total);  // heads before this thread's keys
#pragma unroll
  for (int e = 0; e < kVoxelItems; ++e) {
    const int i = first + e;
    if (i >= P.N) break;
    rank += h[e] ? 1 : 0;
    const int r = rank - 1;  // 0 <= r <= i: position 0 is a head
    const int64_t src = P.order[i];
    P.order32[i] = (int32_t)src;
    if (src >= 0 && src < P.N) P.inverse[src] = r;  // (a permutation by contract; anything else writes nothing outside)
    if (h[e]) {
      P.sites[r] = P.sorted[i];
      P.first[r] = src;
      P.seg[r] = i;
    }
  }
  if ((int)blockIdx.x == P.tiles - 1 && threadIdx.x == 0) {
    const int M = before + total;
    P.seg[M] = P.N;
    P.count[0] = M;
    // the key of a point out of range sorts first; otherwise the last key holds the highest batch index
    P.count[1] = P.sorted[0] < 0 ? -1 : key_batch(P.sorted[P.N - 1]) + 1;
  }
}

// ---- features ----------------------------------------------------------------------------------------------------------------------
struct VoxelReduceParams {
  int M, N, C, mode;
  const float* x;          // [N, C]
  const int32_t* order;    // [N]
  const int32_t* seg;      // [M + 1]
  float* y;                // [M, C]
  int32_t* arg;            // [M, C] (max)
};

__global__ __launch_bounds__(256) void voxel_reduce_kernel(VoxelReduceParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.M * P.C) return;
  const int c = (int)(t % P.C);
  const int m = (int)(t / P.C);
  int j0 = P.seg[m], j1 = P.seg[m + 1];
  j0 = max(j0, 0);
  j1 = min(j1, P.N);
  if (P.mode == VDETR_VOXEL_MAX) {
    float best = 0.f;
    int win = -1;
    for (int j = j0; j < j1; ++j) {
      const int row = P.order[j];
      if (row < 0 || row >= P.N) continue;
      const float v = P.x[(size_t)row * P.C + c];
      // np.maximum.at: a NaN wins and stays; a tie keeps the earlier (lower) row
      if (win < 0 || v > best || (v != v && best == best)) { best = v; win = row; }
    }
    P.y[t] = best;
    P.arg[t] = win;
    return;
  }
  if (P.mode == VDETR_VOXEL_FIRST) {
    const int row = j0 < j1 ? P.order[j0] : -1;
    P.y[t] = (row >= 0 && row < P.N) ? P.x[(size_t)row * P.C + c] : 0.f;
    return;
  }
  float acc = 0.f;  // (np.add.at on zeros: the fold starts from +0)
  for (int j = j0; j < j1; ++j) {
    const int row = P.order[j];
    if (row < 0 || row >= P.N) continue;
    acc += P.x[(size_t)row * P.C + c];
  }
  if (P.mode == VDETR_VOXEL_AVG) acc = acc / (float)(j1 - j0);
  P.y[t] = acc;
}

struct VoxelGradParams {
  int M, N, C, mode;
  const float* dy;         // [M, C]
  const int32_t* inverse;  // [N]
  const int32_t* seg;      // [M + 1]
  const int32_t* arg;      // [M, C] (max)
  const int32_t* order;    // [N] (first)
  float* dx;               // [N, C]
};

__global__ __launch_bounds__(256) void voxel_reduce_grad_kernel(VoxelGradParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.N * P.C) return;
  const int c = (int)(t % P.C);
  const int i = (int)(t / P.C);
  const int m = P.inverse[i];
  float g = 0.f;
  if (m >= 0 && m < P.M) {
    const size_t at = (size_t)m * P.C + c;
    if (P.mode == VDETR_VOXEL_MAX) {
      g = P.arg[at] == i ? P.dy[at] : 0.f;
    } else if (P.mode == VDETR_VOXEL_FIRST) {
      const int j = P.seg[m];
      g = (j >= 0 && j < P.N && P.order[j] == i) ? P.dy[at] : 0.f;  // the head of the run is the kept row
    } else {
      g = P.dy[at];
      if (P.mode == VDETR_VOXEL_AVG) g = g / (float)(P.seg[m + 1] - P.seg[m]);
    }
  }
  P.dx[t] = g;
}

struct VoxelLabelsParams {
  int M, N, ignore;
  const int32_t* labels;   // [N]
  const int32_t* order;    // [N]
  const int32_t* seg;      // [M + 1]
  int32_t* out;            // [M]
};

__global__ __launch_bounds__(256) void voxel_labels_kernel(VoxelLabelsParams P) {
  const int m = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (m >= P.M) return;
  const int j0 = max(P.seg[m], 0), j1 = min(P.seg[m + 1], P.N);
  int label = P.ignore;
  bool have = false;
  for (int j = j0; j < j1; ++j) {
    const int row = P.order[j];
    if (row < 0 || row >= P.N) continue;
    const int l = P.labels[row];
    if (!have) { label = l; have = true; }
    else if (l != label) { label = P.ignore; break; }
  }
  P.out[m] = label;
}

static int* voxel_lay_out(Carver& c, long n) { return c.take<int>((size_t)((n + kVoxelTile - 1) / kVoxelTile)); }

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_sp_voxel_tile(void) { return kVoxelTile; }

extern "C" int vdetr_sp_voxel_keys_f32(const vdetr_sp_voxel_keys_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_voxel_keys: null descriptor");
  VDETR_REQUIRE(d->N >= 0, "sp_voxel_keys: N=%d is negative", d->N);
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->keys, "sp_voxel_keys: keys is NULL with N=%d", d->N);
  if (d->coords) {
    VDETR_REQUIRE(!d->points, "sp_voxel_keys: both points and coords are given");
    VDETR_REQUIRE(((uintptr_t)d->coords & 15) == 0, "sp_voxel_keys: coords must be 16-byte aligned ([N, 4] int32 rows)");
    CoordKeysParams P{d->N, d->coords, d->keys};
    hipLaunchKernelGGL(coord_keys_kernel, dim3((unsigned)ceil_div(d->N, 256)), dim3(256), 0, (hipStream_t)stream, P);
    return check_launch("sp_voxel_keys");
  }
  VDETR_REQUIRE(d->points, "sp_voxel_keys: points is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->offsets, "sp_voxel_keys: offsets is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->B >= 1 && d->B <= 32768, "sp_voxel_keys: B=%d scenes (1 .. 32768: the key's batch field)", d->B);
  VDETR_REQUIRE(d->stride >= 3, "sp_voxel_keys: row stride %d is less than the three coordinates", d->stride);
  VDETR_REQUIRE(d->voxel_size > 0.0 && d->voxel_size <= 3.0e38, "sp_voxel_keys: voxel_size=%g must be positive and finite",
                d->voxel_size);
  // ATen's device division by a host scalar: ONE reciprocal, taken in double and rounded to float32, then a float32
  // multiplication per element
  const float inv = (float)(1.0 / d->voxel_size);
  VDETR_REQUIRE(inv > 0.f && inv <= 3.0e38f, "sp_voxel_keys: voxel_size=%g has no float32 reciprocal", d->voxel_size);
  VoxelKeysParams P{d->N, d->B, d->stride, inv, d->points, d->offsets, d->keys};
  hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)ceil_div(d->N, 256)), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_voxel_keys");
}

extern "C" int vdetr_sp_region_keys_i64(const vdetr_sp_region_keys_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_region_keys: null descriptor");
  VDETR_REQUIRE(d->N >= 0, "sp_region_keys: N=%d is negative", d->N);
  VDETR_REQUIRE(d->K >= 0, "sp_region_keys: K=%d is negative", d->K);
  const long long total = (long long)d->K * d->N;
  VDETR_REQUIRE(total < (1LL << 31), "sp_region_keys: K=%d x N=%d candidates are more than 31 bits hold", d->K, d->N);
  if (total == 0) return VDETR_OK;
  VDETR_REQUIRE(d->keys, "sp_region_keys: keys is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->offsets, "sp_region_keys: offsets is NULL with K=%d", d->K);
  VDETR_REQUIRE(d->cand, "sp_region_keys: cand is NULL with K=%d x N=%d", d->K, d->N);
  RegionKeysParams P{d->N, total, d->keys, d->offsets, d->cand};
  hipLaunchKernelGGL(region_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_region_keys");
}

extern "C" size_t vdetr_sp_voxel_sites_workspace_bytes(int N) {
  if (N < 0) return 0;
  Carver c(nullptr);
  voxel_lay_out(c, N);
  return c.bytes() + 256;
}

extern "C" int vdetr_sp_voxel_sites_i64(const vdetr_sp_voxel_sites_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_voxel_sites: null descriptor");
  VDETR_REQUIRE(d->N >= 0, "sp_voxel_sites: N=%d is negative", d->N);
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->sorted, "sp_voxel_sites: sorted is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->order, "sp_voxel_sites: order is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->sites, "sp_voxel_sites: sites is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->first, "sp_voxel_sites: first is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->inverse, "sp_voxel_sites: inverse is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->order32, "sp_voxel_sites: order32 is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->seg, "sp_voxel_sites: seg is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->count, "sp_voxel_sites: count is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->workspace, "sp_voxel_sites: workspace is NULL with N=%d", d->N);
  Carver c(d->workspace);
  VoxelSitesParams P;
  P.N = d->N; P.tiles = ceil_div(d->N, kVoxelTile);
  P.sorted = d->sorted; P.order = d->order; P.sites = d->sites; P.first = d->first;
  P.inverse = d->inverse; P.order32 = d->order32; P.seg = d->seg; P.count = d->count;
  P.tile_counts = voxel_lay_out(c, d->N);
  hipLaunchKernelGGL(voxel_heads_kernel, dim3((unsigned)P.tiles), dim3(kVoxelThreads), 0, (hipStream_t)stream, P);
  if (int e = check_launch("sp_voxel_sites")) return e;
  hipLaunchKernelGGL(voxel_fill_kernel, dim3((unsigned)P.tiles), dim3(kVoxelThreads), 0, (hipStream_t)stream, P);
  return check_launch("sp_voxel_sites");
}

static int voxel_mode_ok(int mode) {
  return mode == VDETR_VOXEL_SUM || mode == VDETR_VOXEL_AVG || mode == VDETR_VOXEL_MAX || mode == VDETR_VOXEL_FIRST;
}

extern "C" int vdetr_sp_voxel_reduce_f32(const vdetr_sp_voxel_reduce_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_voxel_reduce: null descriptor");
  VDETR_REQUIRE(voxel_mode_ok(d->mode), "sp_voxel_reduce: mode=%d (0 sum, 1 average, 2 max, 3 first)", d->mode);
  VDETR_REQUIRE(d->C >= 1, "sp_voxel_reduce: C=%d must be positive", d->C);
  VDETR_REQUIRE(d->M >= 0, "sp_voxel_reduce: M=%d is negative", d->M);
  VDETR_REQUIRE(d->N >= d->M, "sp_voxel_reduce: N=%d points for M=%d sites", d->N, d->M);
  if (d->M == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x, "sp_voxel_reduce: x is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->order, "sp_voxel_reduce: order is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->seg, "sp_voxel_reduce: seg is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->y, "sp_voxel_reduce: y is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->arg || d->mode != VDETR_VOXEL_MAX, "sp_voxel_reduce: arg is NULL in max mode");
  const long long blocks = ((long long)d->M * d->C + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_voxel_reduce: M=%d x C=%d is more than one launch covers", d->M, d->C);
  VoxelReduceParams P{d->M, d->N, d->C, d->mode, d->x, d->order, d->seg, d->y, d->arg};
  hipLaunchKernelGGL(voxel_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_voxel_reduce");
}

extern "C" int vdetr_sp_voxel_reduce_grad_f32(const vdetr_sp_voxel_reduce_desc* d, const float* dy, const int32_t* inverse,
                                              float* dx, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_voxel_reduce_grad: null descriptor");
  VDETR_REQUIRE(voxel_mode_ok(d->mode), "sp_voxel_reduce_grad: mode=%d (0 sum, 1 average, 2 max, 3 first)", d->mode);
  VDETR_REQUIRE(d->C >= 1, "sp_voxel_reduce_grad: C=%d must be positive", d->C);
  VDETR_REQUIRE(d->M >= 0, "sp_voxel_reduce_grad: M=%d is negative", d->M);
  VDETR_REQUIRE(d->N >= d->M, "sp_voxel_reduce_grad: N=%d points for M=%d sites", d->N, d->M);
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(dx, "sp_voxel_reduce_grad: dx is NULL with N=%d", d->N);
  VDETR_REQUIRE(inverse, "sp_voxel_reduce_grad: inverse is NULL with N=%d", d->N);
  VDETR_REQUIRE(dy || d->M == 0, "sp_voxel_reduce_grad: dy is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->seg || d->M == 0, "sp_voxel_reduce_grad: seg is NULL with M=%d", d->M);
  // max: the forward's winners [M, C]; first: the int32 permutation, whose entry seg[m] is the kept row of site m
  VDETR_REQUIRE(d->arg || (d->mode != VDETR_VOXEL_MAX) || d->M == 0, "sp_voxel_reduce_grad: arg is NULL in max mode");
  VDETR_REQUIRE(d->order || (d->mode != VDETR_VOXEL_FIRST) || d->M == 0, "sp_voxel_reduce_grad: order is NULL in first mode");
  const long long blocks = ((long long)d->N * d->C + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_voxel_reduce_grad: N=%d x C=%d is more than one launch covers", d->N, d->C);
  VoxelGradParams P{d->M, d->N, d->C, d->mode, dy, inverse, d->seg, d->arg, d->order, dx};
  hipLaunchKernelGGL(voxel_reduce_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_voxel_reduce_grad");
}

extern "C" int vdetr_sp_voxel_labels_i32(const int32_t* labels, const int32_t* order, const int32_t* seg, int M, int N,
                                         int ignore_label, int32_t* out, vdetr_stream_t stream) {
  VDETR_REQUIRE(M >= 0 && N >= M, "sp_voxel_labels: M=%d sites of N=%d points", M, N);
  if (M == 0) return VDETR_OK;
  VDETR_REQUIRE(labels && order && seg && out, "sp_voxel_labels: a NULL operand with M=%d", M);
  VoxelLabelsParams P{M, N, ignore_label, labels, order, seg, out};
  hipLaunchKernelGGL(voxel_labels_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_voxel_labels");
}
