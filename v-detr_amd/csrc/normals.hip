// normals.hip — area-weighted vertex normals of a scan's mesh, --use_normals (reference
// datasets/scannet.py:394-420).  The reference's serial loop `nv[face[i]] += nf[i]` is a scatter whose result depends on the
// order of additions per vertex only: every vertex adds the weights of its incident faces in ascending face index.
//   vdetr_vertex_normals_f32   seven launches whatever B:
//     normals_clear_kernel     counts = 0
//     normals_face_kernel      one lane per face: w[f] in the reference's operation order; the corners per vertex (integer atomics)
//     normals_tile_sum_kernel  \
//     normals_top_scan_kernel   > exclusive scan of the counts over the packed batch -> starts, cursors
//     normals_starts_kernel    /
//     normals_fill_kernel      one lane per face: the vertex -> faces lists; a corner's slot comes from an integer atomic, so
//                              the order inside a list is arbitrary here
//     normals_vertex_kernel    one lane per vertex: a list of up to VDETR_NORMALS_SHORT faces is walked in ascending order by
//                              repeated selection; a longer one is sorted in place by the vertex's workgroup (a bitonic network
//                              whose exchanges all move the smaller key down, so the list needs no padding to a power of two:
//                              O(k log^2 k) for any k) and summed by one lane from rows staged through LDS
// Only integers go through atomics; the float sums have one fixed order: two runs give the same bits.  A corner outside its
// scene is never followed: the face's weight is NaN and only its in-range corners are listed.  -ffp-contract=off as everywhere:
// every product, difference and sum below is one IEEE float32 operation; `/` and sqrtf are the correctly rounded forms (no
// fast-math, not the native sqrt), float32 subnormals are kept (the compiler's default mode for kernels).
#include "block_scan.h"
#include "scene_tiles.h"

namespace vdetr {
namespace {

constexpr int kTile = VDETR_NORMALS_TILE;
constexpr int kScanTile = VDETR_NORMALS_SCAN_TILE;
constexpr int kScanRows = kScanTile / 256;   // consecutive vertices per lane of the scan kernels
constexpr int kShort = VDETR_NORMALS_SHORT;
constexpr float kEps = 1.0e-8f;              // the reference's 1.0e-8, rounded to float32 when it meets a float32 array

struct Work {
  float* w;       // [F, 3]
  int* count;     // [N] corners that name the vertex
  int* start;     // [N] first slot of the vertex's list
  int* cursor;    // [N] next free slot while the lists are filled
  int* tile_sum;  // [tiles] corners per scan tile, then their exclusive scan
  int* adj;       // [3F] packed face index per slot
  int N, F, tiles;
};

// the scene of packed face g (scenes without faces are skipped) -> its vertices' first row and count; a device offset table
// that does not fit the N rows gives a scene without vertices, so that nothing is followed
__device__ __forceinline__ void scene_of_face(const vdetr_normals_desc& d, int N, int g, int& vbegin, int& n) {
  int lo = 0, hi = d.B - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (d.face_offsets[mid + 1] > g) hi = mid;
    else lo = mid + 1;
  }
  vbegin = d.vert_offsets[lo];
  n = d.vert_offsets[lo + 1] - vbegin;
  if (vbegin < 0 || n < 0 || (long)vbegin + n > (long)N) { vbegin = 0; n = 0; }
}

__device__ __forceinline__ long corner(const vdetr_normals_desc& d, int g, int c) {
  const size_t at = (size_t)g * 3 + c;
  return d.faces_i64 ? (long)static_cast<const int64_t*>(d.faces)[at] : (long)static_cast<const int32_t*>(d.faces)[at];
}

__global__ __launch_bounds__(kTile) void normals_clear_kernel(Work k) {
  const long v = (long)blockIdx.x * kTile + threadIdx.x;
  if (v < k.N) k.count[v] = 0;
}

__global__ __launch_bounds__(kTile) void normals_face_kernel(vdetr_normals_desc d, Work k) {
  const long at = (long)blockIdx.x * kTile + threadIdx.x;
  if (at >= k.F) return;
  const int g = (int)at;
  int vbegin, n;
  scene_of_face(d, k.N, g, vbegin, n);
  long idx[3];
  bool ok[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    idx[c] = corner(d, g, c);
    ok[c] = idx[c] >= 0 && idx[c] < (long)n;
  }
  const float nan = __builtin_nanf("");
  float w0 = nan, w1 = nan, w2 = nan;
  if (ok[0] && ok[1] && ok[2]) {
    const float* p0 = d.vertices + (size_t)(vbegin + idx[0]) * d.vert_stride;
    const float* p1 = d.vertices + (size_t)(vbegin + idx[1]) * d.vert_stride;
    const float* p2 = d.vertices + (size_t)(vbegin + idx[2]) * d.vert_stride;
    const float u0 = p1[0] - p0[0], u1 = p1[1] - p0[1], u2 = p1[2] - p0[2];
    const float v0 = p2[0] - p0[0], v1 = p2[1] - p0[1], v2 = p2[2] - p0[2];
    const float a0 = u1 * v2, b0 = u2 * v1, a1 = u2 * v0, b1 = u0 * v2, a2 = u0 * v1, b2 = u1 * v0;   // np.cross: no fma
    const float c0 = a0 - b0, c1 = a1 - b1, c2 = a2 - b2;
    const float q0 = c0 * c0, q1 = c1 * c1, q2 = c2 * c2;
    const float len = sqrtf((q0 + q1) + q2) + kEps;
    const float area = len * 0.5f;
    w0 = (c0 / len) * area;
    w1 = (c1 / len) * area;
    w2 = (c2 / len) * area;
  }
  float* w = k.w + (size_t)g * 3;
  w[0] = w0; w[1] = w1; w[2] = w2;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (ok[c]) atomicAdd(&k.count[vbegin + (int)idx[c]], 1);
}

__device__ __forceinline__ int lane_counts(const Work& k, int tile, int (&c)[kScanRows]) {
  const long first = (long)tile * kScanTile + (long)threadIdx.x * kScanRows;
  int s = 0;
#pragma unroll
  for (int r = 0; r < kScanRows; ++r) {
    c[r] = first + r < k.N ? k.count[first + r] : 0;
    s += c[r];
  }
  return s;
}

__global__ __launch_bounds__(256) void normals_tile_sum_kernel(Work k) {
  __shared__ int wave_sums[256 / kWave];
  int c[kScanRows];
  int total;
  block_exclusive_sum<256>(lane_counts(k, blockIdx.x, c), wave_sums, total);
  if (threadIdx.x == 0) k.tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void normals_top_scan_kernel(Work k) {   // one workgroup
  __shared__ int wave_sums[256 / kWave];
  block_exclusive_sum_array<256>(k.tile_sum, k.tile_sum, k.tiles, wave_sums);
}

__global__ __launch_bounds__(256) void normals_starts_kernel(Work k) {
  __shared__ int wave_sums[256 / kWave];
  int c[kScanRows], total;
  int at = k.tile_sum[blockIdx.x] + block_exclusive_sum<256>(lane_counts(k, blockIdx.x, c), wave_sums, total);
  const long first = (long)blockIdx.x * kScanTile + (long)threadIdx.x * kScanRows;
#pragma unroll
  for (int r = 0; r < kScanRows; ++r) {
    if (first + r < k.N) {
      k.start[first + r] = at;
      k.cursor[first + r] = at;
    }
    at += c[r];
  }
}

__global__ __launch_bounds__(kTile) void normals_fill_kernel(vdetr_normals_desc d, Work k) {
  const long at = (long)blockIdx.x * kTile + threadIdx.x;
  if (at >= k.F) return;
  const int g = (int)at;
  int vbegin, n;
  scene_of_face(d, k.N, g, vbegin, n);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long idx = corner(d, g, c);
    if (idx >= 0 && idx < (long)n) {                                   // the face pass's own test: the slots were counted
      const int slot = atomicAdd(&k.cursor[vbegin + (int)idx], 1);
      if (slot >= 0 && (long)slot < 3L * k.F) k.adj[slot] = g;
    }
  }
}

__device__ __forceinline__ void write_normal(const vdetr_normals_desc& d, long v, float n0, float n1, float n2) {
  const float q0 = n0 * n0, q1 = n1 * n1, q2 = n2 * n2;
  const float len = sqrtf((q0 + q1) + q2) + kEps;
  float* out = d.out + (size_t)v * d.out_stride;
  out[0] = n0 / len;
  out[1] = n1 / len;
  out[2] = n2 / len;
}

// the workgroup sorts seg[0 .. k) ascending, in place.  Bitonic merges in the form whose every exchange moves the smaller key to
// the lower index (first a mirror step, then halving strides), so the keys a power-of-two length would add sit at the top, are
// never smaller than their partner, and a pair that reaches past k is simply skipped.
__device__ void sort_list(int* seg, long k) {
  long half = 1;
  while (half * 2 < k) half *= 2;                                      // pairs per step: half of the power of two >= k
  for (long size = 2; (size >> 1) < k; size <<= 1) {
    for (long p = threadIdx.x; p < half; p += kTile) {
      const long block = p / (size >> 1), off = p % (size >> 1);
      const long i = block * size + off, l = block * size + (size - 1 - off);
      if (l < k) {
        const int a = seg[i], b = seg[l];
        if (b < a) { seg[i] = b; seg[l] = a; }
      }
    }
    __syncthreads();
    for (long j = size >> 2; j >= 1; j >>= 1) {
      for (long p = threadIdx.x; p < half; p += kTile) {
        const long i = (p / j) * 2 * j + p % j, l = i + j;
        if (l < k) {
          const int a = seg[i], b = seg[l];
          if (b < a) { seg[i] = b; seg[l] = a; }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kTile) void normals_vertex_kernel(vdetr_normals_desc d, Work k) {
  __shared__ int long_list[kTile];
  __shared__ int long_count;
  __shared__ float rows[kTile][3];
  const int tid = threadIdx.x;
  const long v = (long)blockIdx.x * kTile + tid;
  const float nan = __builtin_nanf("");
  if (tid == 0) long_count = 0;
  __syncthreads();
  if (v < k.N) {
    int cnt = k.count[v];
    const int s = k.start[v];
    if (cnt < 0 || s < 0 || (long)s + cnt > 3L * k.F) cnt = 0;         // cannot happen: the lists were counted
    if (cnt <= kShort) {
      float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;                          // np.zeros_like: the sum starts from +0
      int last = -1, done = 0;
      while (done < cnt) {
        int best = 0x7fffffff, copies = 0;                             // the smallest face above `last`; a face may name v twice
        for (int j = 0; j < cnt; ++j) {
          const int f = k.adj[s + j];
          if (f > last) {
            if (f < best) { best = f; copies = 1; }
            else if (f == best) ++copies;
          }
        }
        if (copies == 0) break;
        const bool inside = best < k.F;
        const float* w = k.w + (size_t)(inside ? best : 0) * 3;
        const float w0 = inside ? w[0] : nan, w1 = inside ? w[1] : nan, w2 = inside ? w[2] : nan;
        for (int m = 0; m < copies; ++m) { n0 = n0 + w0; n1 = n1 + w1; n2 = n2 + w2; }
        last = best;
        done += copies;
      }
      write_normal(d, v, n0, n1, n2);
    } else {
      long_list[atomicAdd(&long_count, 1)] = tid;
    }
  }
  __syncthreads();
  const int nlong = long_count;                                        // uniform; the order of the list does not matter
  for (int i = 0; i < nlong; ++i) {
    const long lv = (long)blockIdx.x * kTile + long_list[i];
    const long cnt = k.count[lv];
    int* seg = k.adj + k.start[lv];
    sort_list(seg, cnt);
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    for (long base = 0; base < cnt; base += kTile) {
      if (base + tid < cnt) {
        const int f = seg[base + tid];
        const bool inside = f >= 0 && f < k.F;
        const float* w = k.w + (size_t)(inside ? f : 0) * 3;
        rows[tid][0] = inside ? w[0] : nan;
        rows[tid][1] = inside ? w[1] : nan;
        rows[tid][2] = inside ? w[2] : nan;
      }
      __syncthreads();
      if (tid == 0) {
        const int m = cnt - base < kTile ? (int)(cnt - base) : kTile;
        for (int j = 0; j < m; ++j) { n0 = n0 + rows[j][0]; n1 = n1 + rows[j][1]; n2 = n2 + rows[j][2]; }
      }
      __syncthreads();
    }
    if (tid == 0) write_normal(d, lv, n0, n1, n2);
  }
}

// N, F of the packed batch, or -1 (with a message if `op` is given)
int batch_sizes(const int32_t* vert, const int32_t* face, int B, const char* op, long& N, long& F) {
  if (vert[0] != 0 || face[0] != 0) {
    if (op) set_error("%s: offsets start at %d (vertices) and %d (faces), not at 0", op, vert[0], face[0]);
    return -1;
  }
  for (int b = 0; b < B; ++b) {
    if (vert[b + 1] <= vert[b]) {
      if (op) set_error("%s: scene %d has no vertices (offsets %d .. %d)", op, b, vert[b], vert[b + 1]);
      return -1;
    }
    if (face[b + 1] < face[b]) {
      if (op) set_error("%s: face offsets decrease at scene %d (%d .. %d)", op, b, face[b], face[b + 1]);
      return -1;
    }
  }
  N = vert[B];
  F = face[B];
  if (N >= (1L << 31) || 3 * F >= (1L << 31)) {
    if (op) set_error("%s: %ld vertices, %ld faces: N and 3F must stay below 2^31", op, N, F);
    return -1;
  }
  return 0;
}

// the workspace of a packed batch of N vertices and F faces
Work lay_out(Carver& c, long N, long F) {
  Work k;
  k.N = (int)N;
  k.F = (int)F;
  k.tiles = (int)((N + kScanTile - 1) / kScanTile);
  k.w = c.take<float>((size_t)F * 3);
  k.count = c.take<int>((size_t)N);
  k.start = c.take<int>((size_t)N);
  k.cursor = c.take<int>((size_t)N);
  k.tile_sum = c.take<int>((size_t)k.tiles);
  k.adj = c.take<int>((size_t)F * 3);
  return k;
}

size_t workspace_need(long N, long F) {
  Carver c(nullptr);
  lay_out(c, N, F);
  return c.bytes() + 256;
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

extern "C" size_t vdetr_vertex_normals_workspace_bytes(const int32_t* vert_offsets_host, const int32_t* face_offsets_host, int B) {
  if (!vert_offsets_host || !face_offsets_host || B <= 0) return 0;
  long N, F;
  if (batch_sizes(vert_offsets_host, face_offsets_host, B, nullptr, N, F)) return 0;
  return workspace_need(N, F);
}

extern "C" int vdetr_vertex_normals_f32(const vdetr_normals_desc* desc, const int32_t* vert_offsets_host, const int32_t* face_offsets_host,
                                        void* workspace, size_t workspace_bytes, vdetr_stream_t stream) {
  VDETR_REQUIRE(desc && vert_offsets_host && face_offsets_host, "vertex_normals: null descriptor or offsets");
  VDETR_REQUIRE(desc->B >= 0 && desc->B <= kMaxScenes, "vertex_normals: %d scenes (0 .. %d)", desc->B, kMaxScenes);
  if (desc->B == 0) return VDETR_OK;
  const vdetr_normals_desc& d = *desc;
  VDETR_REQUIRE(d.vert_stride >= 3 && d.out_stride >= 3, "vertex_normals: %d / %d floats per row of vertices / out, xyz needs 3", d.vert_stride,
                d.out_stride);
  long N, F;
  if (batch_sizes(vert_offsets_host, face_offsets_host, d.B, "vertex_normals", N, F)) return VDETR_ERR_ARG;
  VDETR_REQUIRE(d.vertices && d.vert_offsets && d.face_offsets && d.out && (d.faces || F == 0), "vertex_normals: null pointer");
  if (int e = require_workspace("vertex_normals", workspace, workspace_bytes, workspace_need(N, F))) return e;
  Carver c(workspace);
  const Work k = lay_out(c, N, F);
  const unsigned vert_tiles = (unsigned)((N + kTile - 1) / kTile);
  const unsigned face_tiles = (unsigned)((F + kTile - 1) / kTile > 0 ? (F + kTile - 1) / kTile : 1);   // no faces: one idle workgroup
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(normals_clear_kernel, dim3(vert_tiles), dim3(kTile), 0, s, k);
  hipLaunchKernelGGL(normals_face_kernel, dim3(face_tiles), dim3(kTile), 0, s, d, k);
  hipLaunchKernelGGL(normals_tile_sum_kernel, dim3((unsigned)k.tiles), dim3(256), 0, s, k);
  hipLaunchKernelGGL(normals_top_scan_kernel, dim3(1), dim3(256), 0, s, k);
  hipLaunchKernelGGL(normals_starts_kernel, dim3((unsigned)k.tiles), dim3(256), 0, s, k);
  hipLaunchKernelGGL(normals_fill_kernel, dim3(face_tiles), dim3(kTile), 0, s, d, k);
  hipLaunchKernelGGL(normals_vertex_kernel, dim3(vert_tiles), dim3(kTile), 0, s, d, k);
  return check_launch("vertex_normals");
}
