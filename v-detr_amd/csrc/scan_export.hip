// scan_export.hip — a raw ScanNet scan to the arrays of its _vert / _sem_label / _ins_label / _bbox files (DESIGN.md 6.7;
// reference scannet/load_scannet_data.py:60-129 export, scannet/batch_load_scannet_data.py:25-50 export_one_scan).  The host has
// walked the aggregation into per-segment tables (scan_export.py:scan_tables), so that what is left is per vertex and per object.
//   vdetr_scan_export_f32   two launches whatever B, three with a drop table:
//     scan_export_points_kernel   one workgroup per scene-aligned tile of 512 rows, one lane per row: the float64 axis alignment
//                                 rounded once to float32, the two label gathers, and the row's aligned xyz into the [K, 6] table
//                                 of its object in LDS (integer min / max on order-preserving keys) -> one partial table per tile,
//                                 ordinary stores
//     scan_export_boxes_kernel    one workgroup of 1024 lanes per scene: merges the partials (integer min / max per entry, the
//                                 scene's tiles shared out among the lanes of an entry), forms centre and size in float32,
//                                 looks the class up, compacts the kept rows in ascending object id (ballot scan); with a drop
//                                 table also the exclusive scan of the tiles' kept rows
//     scan_export_compact_kernel  drop table only: one workgroup per tile moves its kept rows and labels up, order kept
// Min and max do not depend on the order of their operands and only integers go through atomics: two runs give the same bits.
// -ffp-contract=off as everywhere: the alignment is three products and three sums, each one IEEE float64 operation.
#include "block_scan.h"
#include "scene_tiles.h"

namespace vdetr {
namespace {

constexpr int kTile = VDETR_EXPORT_TILE;
constexpr int kMaxK = VDETR_EXPORT_MAX_INSTANCES;
constexpr int kBoxLanes = 1024;
constexpr int kMergeLoads = 8;              // independent loads per lane and round of the merge: a round costs one trip to L2
constexpr unsigned kNoMin = 0xffffffffu;     // the identities; no finite float has these keys
constexpr unsigned kNoMax = 0u;

struct Work {
  unsigned* partial;    // [tiles, Kmax, 6] keys of min xyz, max xyz
  int32_t* tile_kept;   // [tiles] rows the drop table leaves
  int32_t* tile_base;   // [tiles] kept rows in the scene's earlier tiles
};

Work lay_out(Carver& c, long tiles, int Kmax) {
  Work w;
  w.partial = c.take<unsigned>((size_t)tiles * Kmax * 6);
  w.tile_kept = c.take<int32_t>((size_t)tiles);
  w.tile_base = c.take<int32_t>((size_t)tiles);
  return w;
}

// unsigned keys in the order of the floats (-0 below +0)
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ int scene_objects(const vdetr_scan_export_desc& d, int b) {
  const int cap = d.Kmax < kMaxK ? d.Kmax : kMaxK;
  const int K = d.num_instances[b];
  return K < 0 ? 0 : K > cap ? cap : K;
}

__device__ __forceinline__ bool dropped(const vdetr_scan_export_desc& d, int sem) {
  return sem >= 0 && sem < d.drop_table_len && d.drop_table[sem] != 0;
}

__global__ __launch_bounds__(kTile) void scan_export_points_kernel(vdetr_scan_export_desc d, int total_rows, Work w) {
  __shared__ unsigned table[kMaxK * 6];
  __shared__ int wave_kept[kTile / kWave];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, kTile, t, b, local_tile)) return;          // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  const int K = scene_objects(d, b);
  for (int i = tid; i < K * 6; i += kTile) table[i] = i % 6 < 3 ? kNoMin : kNoMax;
  __syncthreads();
  const int j = local_tile * kTile + tid;
  const long r = (long)begin + j;
  bool keep = false;
  if (j < rows && r < total_rows) {
    const float* src = d.vertices + (size_t)r * d.vert_stride;
    float* dst = d.out_vertices + (size_t)r * d.W;
    const double* m = d.axis_align + (size_t)b * 16;
    const double x = src[0], y = src[1], z = src[2];
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double px = x * m[4 * c], py = y * m[4 * c + 1], pz = z * m[4 * c + 2];   // np.dot's terms, left to right
      a[c] = (float)(((px + py) + pz) + m[4 * c + 3]);                               // the one rounding to float32
      dst[c] = a[c];
    }
    for (int c = 3; c < d.W; ++c) dst[c] = src[c];
    const int seg = d.seg_indices[r];
    int sem = 0, inst = 0;
    if (seg >= 0 && seg < d.num_segments) {
      sem = d.seg_label[seg];
      inst = d.seg_object[seg];
    }
    d.semantic[r] = sem;
    d.instance[r] = inst;
    if (inst >= 1 && inst <= K) {
      unsigned* row = table + (inst - 1) * 6;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned key = order_key(a[c]);
        atomicMin(row + c, key);
        atomicMax(row + 3 + c, key);
      }
    }
    keep = !dropped(d, sem);
  }
  __syncthreads();
  unsigned* out = w.partial + (size_t)t * d.Kmax * 6;
  for (int i = tid; i < K * 6; i += kTile) out[i] = table[i];
  if (d.drop_table_len > 0) {
    int total;
    block_rank<kTile>(keep, wave_kept, total);
    if (tid == 0) w.tile_kept[t] = total;
  }
}

__global__ __launch_bounds__(kBoxLanes) void scan_export_boxes_kernel(vdetr_scan_export_desc d, int num_tiles, Work w) {
  __shared__ unsigned merged[kMaxK * 6];
  __shared__ int wave_count[kBoxLanes / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int rows = d.offsets[b + 1] - d.offsets[b];
  const int first = first_tile(d.offsets, b, kTile), nt = tiles_of(rows, kTile);
  const int K = scene_objects(d, b);
  // every entry of the table is folded over the scene's tiles by as many lanes as the workgroup has to spare, each taking every
  // `slices`-th tile; the lanes of an entry meet in LDS (integer min / max again: any order gives the same bits)
  const int E = K * 6;
  const int n = nt < num_tiles - first ? nt : num_tiles - first;              // the scene's tiles; the second bound is a guard
  for (int e = tid; e < E; e += kBoxLanes) merged[e] = e % 6 < 3 ? kNoMin : kNoMax;
  __syncthreads();
  const int slices = E > 0 && E < kBoxLanes ? kBoxLanes / E : 1;
  for (int at = tid; at < slices * E; at += kBoxLanes) {
    const int e = at % E, slice = at / E;
    const bool low = e % 6 < 3;
    unsigned v = low ? kNoMin : kNoMax;
    const unsigned* q = w.partial + (size_t)first * d.Kmax * 6 + e;
    const size_t stride = (size_t)d.Kmax * 6;
    for (int i = slice; i < n; i += slices * kMergeLoads) {               // kMergeLoads loads in flight, then their fold
      unsigned p[kMergeLoads];
#pragma unroll
      for (int u = 0; u < kMergeLoads; ++u) {
        const int t = i + u * slices;
        p[u] = t < n ? q[(size_t)t * stride] : v;
      }
#pragma unroll
      for (int u = 0; u < kMergeLoads; ++u) v = low ? min(v, p[u]) : max(v, p[u]);
    }
    if (low) atomicMin(&merged[e], v);
    else atomicMax(&merged[e], v);
  }
  __syncthreads();

  int kept = 0;
  for (int k0 = 0; k0 < d.Kmax; k0 += kBoxLanes) {                            // uniform
    const int k = k0 + tid;
    float box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int label = 0, cls = -1;
    if (k < d.Kmax) {
      if (k < K && merged[k * 6] != kNoMin) {                                 // the object has vertices
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float lo = key_value(merged[k * 6 + c]), hi = key_value(merged[k * 6 + 3 + c]);
          box[c] = (lo + hi) / 2.0f;
          box[3 + c] = hi - lo;
        }
        label = d.object_label[(size_t)b * d.Kmax + k];
      }
      float* row = d.instance_bboxes + ((size_t)b * d.Kmax + k) * 7;
#pragma unroll
      for (int c = 0; c < 6; ++c) row[c] = box[c];
      row[6] = (float)label;
      if (label >= 0 && label < d.class_table_len) cls = d.class_table[label];
    }
    const bool keep = k < K && cls >= 0;                                      // a row of zeros has label 0, as in the reference
    int kept_here;
    const int to = kept + block_rank<kBoxLanes>(keep, wave_count, kept_here);
    kept += kept_here;
    if (keep && to < d.Kmax) {
      float* o = d.boxes + ((size_t)b * d.Kmax + to) * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) o[c] = box[c];
      d.box_nyu40[(size_t)b * d.Kmax + to] = label;
      d.box_classes[(size_t)b * d.Kmax + to] = cls;
    }
  }
  for (int g = kept + tid; g < d.Kmax; g += kBoxLanes) {
    float* o = d.boxes + ((size_t)b * d.Kmax + g) * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = 0.f;
    d.box_nyu40[(size_t)b * d.Kmax + g] = 0;
    d.box_classes[(size_t)b * d.Kmax + g] = 0;
  }
  if (tid == 0) d.box_counts[b] = kept;
  if (d.drop_table_len > 0) {                                                 // uniform: exclusive scan of the tiles' kept rows
    const int carry = block_exclusive_sum_array<kBoxLanes>(w.tile_kept + first, w.tile_base + first, n, wave_count);
    if (tid == 0) d.kept_counts[b] = carry;
  }
}

__global__ __launch_bounds__(kTile) void scan_export_compact_kernel(vdetr_scan_export_desc d, int total_rows, Work w) {
  __shared__ int wave_kept[kTile / kWave];
  const int t = blockIdx.x, tid = threadIdx.x;
  int b, local_tile;
  if (!locate_tile(d.offsets, d.B, kTile, t, b, local_tile)) return;          // uniform
  const int begin = d.offsets[b], rows = d.offsets[b + 1] - begin;
  long base = w.tile_base[t];
  for (int i = 0; i < b; ++i) base += d.kept_counts[i];                       // the earlier scenes' kept rows
  const int j = local_tile * kTile + tid;
  const long r = (long)begin + j;
  const bool in = j < rows && r < total_rows;
  const int sem = in ? d.semantic[r] : 0;
  const bool keep = in && !dropped(d, sem);
  int total;
  const long to = base + block_rank<kTile>(keep, wave_kept, total);
  if (keep && to < total_rows) {                                              // the counts and this test agree: the bound is a guard
    const float* src = d.out_vertices + (size_t)r * d.W;
    float* dst = d.kept_vertices + (size_t)to * d.W;
    for (int c = 0; c < d.W; ++c) dst[c] = src[c];
    d.kept_semantic[to] = sem;
    d.kept_instance[to] = d.instance[r];
  }
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_scan_export_workspace_bytes(const int32_t* offsets_host, int B, int Kmax) {
  if (!offsets_host || B <= 0 || Kmax < 0 || Kmax > kMaxK) return 0;
  const long tiles = count_tiles(offsets_host, B, kTile, nullptr);
  if (tiles <= 0) return 0;
  Carver c(nullptr);
  lay_out(c, tiles, Kmax);
  return c.bytes() + 256;
}

extern "C" int vdetr_scan_export_f32(const vdetr_scan_export_desc* desc, const int32_t* offsets_host, const int32_t* num_instances_host,
                                     void* workspace, size_t workspace_bytes, vdetr_stream_t stream) {
  VDETR_REQUIRE(desc && offsets_host && num_instances_host, "scan_export: null descriptor, offsets or instance counts");
  VDETR_REQUIRE(desc->B >= 0 && desc->B <= kMaxScenes, "scan_export: %d scenes (0 .. %d)", desc->B, kMaxScenes);
  if (desc->B == 0) return VDETR_OK;
  const vdetr_scan_export_desc& d = *desc;
  VDETR_REQUIRE(d.Kmax >= 0 && d.Kmax <= kMaxK, "scan_export: %d object slots (0 .. %d)", d.Kmax, kMaxK);
  for (int b = 0; b < d.B; ++b)
    VDETR_REQUIRE(num_instances_host[b] >= 0 && num_instances_host[b] <= d.Kmax, "scan_export: scene %d has %d objects, %d slots", b,
                  num_instances_host[b], d.Kmax);
  VDETR_REQUIRE(d.W >= 3 && d.vert_stride >= d.W, "scan_export: %d floats per output row, %d per row of vertices (3 <= W <= stride)", d.W,
                d.vert_stride);
  VDETR_REQUIRE(d.num_segments >= 0 && d.class_table_len >= 0 && d.drop_table_len >= 0, "scan_export: negative table length");
  VDETR_REQUIRE(offsets_host[0] == 0, "scan_export: offsets start at %d, not at 0", offsets_host[0]);
  const long tiles = count_tiles(offsets_host, d.B, kTile, "scan_export");
  if (tiles < 0) return VDETR_ERR_ARG;
  VDETR_REQUIRE(tiles <= 0x7fffffffL, "scan_export: %ld tiles", tiles);
  VDETR_REQUIRE(d.vertices && d.offsets && d.seg_indices && d.num_instances && d.axis_align && d.out_vertices && d.semantic && d.instance &&
                    d.box_counts,
                "scan_export: null pointer");
  VDETR_REQUIRE(d.num_segments == 0 || (d.seg_label && d.seg_object), "scan_export: %d segments without their tables", d.num_segments);
  VDETR_REQUIRE(d.class_table_len == 0 || d.class_table, "scan_export: null class table");
  VDETR_REQUIRE(d.Kmax == 0 || (d.object_label && d.instance_bboxes && d.boxes && d.box_nyu40 && d.box_classes),
                "scan_export: %d object slots without their arrays", d.Kmax);
  VDETR_REQUIRE(d.drop_table_len == 0 || (d.drop_table && d.kept_vertices && d.kept_semantic && d.kept_instance && d.kept_counts),
                "scan_export: a drop table without the arrays of the kept rows");
  if (int e = require_workspace("scan_export", workspace, workspace_bytes, vdetr_scan_export_workspace_bytes(offsets_host, d.B, d.Kmax)))
    return e;
  Carver carver(workspace);
  const Work w = lay_out(carver, tiles, d.Kmax);
  const int total = (int)offsets_host[d.B];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(scan_export_points_kernel, dim3((unsigned)tiles), dim3(kTile), 0, s, d, total, w);
  hipLaunchKernelGGL(scan_export_boxes_kernel, dim3(d.B), dim3(kBoxLanes), 0, s, d, (int)tiles, w);
  if (d.drop_table_len > 0) hipLaunchKernelGGL(scan_export_compact_kernel, dim3((unsigned)tiles), dim3(kTile), 0, s, d, total, w);
  return check_launch("scan_export");
}
