// sparse_union.hip — sparse tensors on DIFFERENT key sets: the union of two sorted key sets with its row maps, the order-preserving
// compaction behind MinkowskiPruning, and the two feature kernels that run through such maps.  gfx950.
//
// Reference: `inputs[i] + x` of the generative neck (models/model_vdetr.py:271 with woexpand_conv = False: the up blocks begin
// with MinkowskiGenerativeConvolutionTranspose, :146-176, so the two operands live on different coordinate maps) and the
// commented `self.pruning = ME.MinkowskiPruning()` beside it.  MinkowskiEngine is un-vendored: the semantics are this package's
// own, DESIGN 6.11.
//
// Geometry.  Both maps are the two-launch compaction of block_scan.h over tiles of kUnionTile keys.
// The outputs are allocated at their bound (na + nb, N) and the total is the ONE 4-byte word the host reads, after launch 2.
//
// Union of A [na] and B [nb] (sorted, unique), symmetric in the two sides.  With q(i) = |{j : B[j] < A[i]}| (sparse_key.h's lower bound) and
// m(i) = |{i' < i : A[i'] in B}| (a prefix over A's OWN flags, which is what makes the scan local to a side):
//   row_a[i] = i + q(i) - m(i)        (the keys of B below A[i] that A does not hold come before it)
// and the same with the sides exchanged.  Launch 1 keeps q and the flag of every key in the workspace, launch 2 only scans.
// A key that both sides hold is written to U by side A; src_a / src_b of a row are written by the side that holds the key, and
// where only one side holds it that side's thread writes the other's -1 as well: every word of every output is written once.
//
// Features.  Whole-row gathers as in sparse_pool.hip: a thread owns one row's channel quad (16 bytes).  A missing operand is
// SELECTED as zero, not multiplied away: an infinity on a row the other side lacks stays an infinity.
#include "block_scan.h"
#include "sparse_key.h"
#include "workspace.h"

namespace vdetr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kUnionThreads = 256;
constexpr int kUnionItems = 4;                             // consecutive keys per thread
constexpr int kUnionTile = kUnionThreads * kUnionItems;    // keys per workgroup (vdetr_sp_union_tile)

struct UnionParams {
  int na, nb, ta, tb;  // keys and tiles per side; tile t < ta belongs to A
  const int64_t *a, *b;
  int64_t* u;
  int *row_a, *row_b, *src_a, *src_b, *count;
  unsigned* found_pos;  // [na + nb]: bit 31 = the other side holds this key, bits 0-30 = the other side's keys below it
  int* tile_matches;    // [ta + tb]
};

__global__ __launch_bounds__(kUnionThreads) void union_search_kernel(UnionParams P) {
  __shared__ int wave_sums[kUnionThreads / kWave];
  const bool side_a = (int)blockIdx.x < P.ta;
  const int tile = side_a ? (int)blockIdx.x : (int)blockIdx.x - P.ta;
  const int64_t* x = side_a ? P.a : P.b;
  const int64_t* y = side_a ? P.b : P.a;
  const int n = side_a ? P.na : P.nb, m = side_a ? P.nb : P.na;
  unsigned* out = P.found_pos + (side_a ? 0 : P.na);
  const int first = tile * kUnionTile + (int)threadIdx.x * kUnionItems;
  int matches = 0;
#pragma unroll
  for (int e = 0; e < kUnionItems; ++e) {
    const int i = first + e;
    if (i >= n) break;
    const int64_t key = x[i];
    const int p = key_lower_bound(y, m, key);
    const bool found = p < m && y[p] == key;
    out[i] = (unsigned)p | (found ? 0x80000000u : 0u);
    matches += found ? 1 : 0;
  }
  int total;
  block_exclusive_sum<kUnionThreads>(matches, wave_sums, total);
  if (threadIdx.x == 0) P.tile_matches[blockIdx.x] = total;
}

__global__ __launch_bounds__(kUnionThreads) void union_fill_kernel(UnionParams P) {
  __shared__ int wave_sums[kUnionThreads / kWave];
  const bool side_a = (int)blockIdx.x < P.ta;
  const int tile = side_a ? (int)blockIdx.x : (int)blockIdx.x - P.ta;
  const int64_t* x = side_a ? P.a : P.b;
  const int n = side_a ? P.na : P.nb;
  const unsigned* fp = P.found_pos + (side_a ? 0 : P.na);
  int* row_x = side_a ? P.row_a : P.row_b;
  int* src_x = side_a ? P.src_a : P.src_b;
  int* src_y = side_a ? P.src_b : P.src_a;
  const int cap = P.na + P.nb;
  const int* counts = P.tile_matches + (side_a ? 0 : P.ta);  // matches in this side's earlier tiles
  const int before = block_sum<kUnionThreads>(tile, [&](int i) { return counts[i]; }, wave_sums);
  const int first = tile * kUnionTile + (int)threadIdx.x * kUnionItems;
  unsigned w[kUnionItems];
  int matches = 0;
#pragma unroll
  for (int e = 0; e < kUnionItems; ++e) {
    w[e] = first + e < n ? fp[first + e] : 0u;
    matches += (int)(w[e] >> 31);
  }
  int total;
  int m = before + block_exclusive_sum<kUnionThreads>(matches, wave_sums, total);
#pragma unroll
  for (int e = 0; e < kUnionItems; ++e) {
    const int i = first + e;
    if (i >= n) break;
    const bool found = (w[e] >> 31) != 0;
    const int row = i + (int)(w[e] & 0x7fffffffu) - m;
    m += found ? 1 : 0;
    row_x[i] = row;
    if (row < 0 || row >= cap) continue;  // (unsorted or repeated input keys: the maps are then wrong, but nothing is written outside)
    src_x[row] = i;
    if (!found) src_y[row] = -1;
    if (!found || side_a) P.u[row] = x[i];
  }
  // nu = na + nb - |A and B|: the matches of one whole side, known to the workgroup of that side's last tile
  const bool counts_here = P.ta > 0 ? (side_a && tile == P.ta - 1) : (tile == P.tb - 1);
  if (counts_here && threadIdx.x == 0) P.count[0] = cap - (before + total);
}

struct PruneParams {
  int n, tiles;
  const unsigned char* mask;
  const int64_t* keys;
  int *kept, *pos, *count;
  int64_t* keys_out;
  int* tile_counts;  // [tiles]
};

__global__ __launch_bounds__(kUnionThreads) void prune_count_kernel(PruneParams P) {
  __shared__ int wave_sums[kUnionThreads / kWave];
  const int first = (int)blockIdx.x * kUnionTile + (int)threadIdx.x * kUnionItems;
  int keep = 0;
#pragma unroll
  for (int e = 0; e < kUnionItems; ++e)
    if (first + e < P.n) keep += P.mask[first + e] ? 1 : 0;
  int total;
  block_exclusive_sum<kUnionThreads>(keep, wave_sums, total);
  if (threadIdx.x == 0) P.tile_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kUnionThreads) void prune_fill_kernel(PruneParams P) {
  __shared__ int wave_sums[kUnionThreads / kWave];
  const int before = block_sum<kUnionThreads>((int)blockIdx.x, [&](int i) { return P.tile_counts[i]; }, wave_sums);
  const int first = (int)blockIdx.x * kUnionTile + (int)threadIdx.x * kUnionItems;
  bool k[kUnionItems];
  int keep = 0;
#pragma unroll
  for (int e = 0; e < kUnionItems; ++e) {
    k[e] = first + e < P.n && P.mask[first + e] != 0;
    keep += k[e] ? 1 : 0;
  }
  int total;
  int rank = before + block_exclusive_sum<kUnionThreads>(keep, wave_sums, total);
#pragma unroll
  for (int e = 0; e < kUnionItems; ++e) {
    const int i = first + e;
    if (i >= P.n) break;
    P.pos[i] = k[e] ? rank : -1;
    if (k[e]) {  // rank <= i < n
      P.kept[rank] = i;
      P.keys_out[rank] = P.keys[i];
      ++rank;
    }
  }
  if ((int)blockIdx.x == P.tiles - 1 && threadIdx.x == 0) P.count[0] = before + total;
}

struct UnionAddParams {
  int nu, na, nb, C4, sign;
  const float *a, *b;
  const int *src_a, *src_b;
  float* y;
};

__global__ __launch_bounds__(256) void union_add_kernel(UnionAddParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.nu * P.C4) return;
  const int c4 = (int)(t % P.C4);
  const int u = (int)(t / P.C4);
  const int ia = P.src_a[u], ib = P.src_b[u];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 va = zero, vb = zero;
  if (ia >= 0 && ia < P.na) va = reinterpret_cast<const f32x4*>(P.a)[(size_t)ia * P.C4 + c4];
  if (ib >= 0 && ib < P.nb) vb = reinterpret_cast<const f32x4*>(P.b)[(size_t)ib * P.C4 + c4];
  reinterpret_cast<f32x4*>(P.y)[t] = P.sign > 0 ? va + vb : va - vb;
}

struct TakeRowsParams {
  int nrows, nsrc, C4, sign;
  const float* x;
  const int* idx;
  float* y;
};

__global__ __launch_bounds__(256) void take_rows_kernel(TakeRowsParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.nrows * P.C4) return;
  const int c4 = (int)(t % P.C4);
  const int r = (int)(t / P.C4);
  const int i = P.idx[r];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i >= 0 && i < P.nsrc) {
    v = reinterpret_cast<const f32x4*>(P.x)[(size_t)i * P.C4 + c4];
    if (P.sign < 0) v = -v;
  }
  reinterpret_cast<f32x4*>(P.y)[t] = v;
}

struct UnionWorkspace {
  unsigned* found_pos;
  int* tile_matches;
};

static UnionWorkspace union_lay_out(Carver& c, long na, long nb) {
  UnionWorkspace w;
  w.found_pos = c.take<unsigned>((size_t)(na + nb));
  w.tile_matches = c.take<int>((size_t)((na + kUnionTile - 1) / kUnionTile + (nb + kUnionTile - 1) / kUnionTile));
  return w;
}

static int* prune_lay_out(Carver& c, long n) { return c.take<int>((size_t)((n + kUnionTile - 1) / kUnionTile)); }

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_sp_union_tile(void) { return kUnionTile; }

extern "C" size_t vdetr_sp_union_map_workspace_bytes(int na, int nb) {
  if (na < 0 || nb < 0) return 0;
  Carver c(nullptr);
  union_lay_out(c, na, nb);
  return c.bytes() + 256;
}

extern "C" int vdetr_sp_union_map_i64(const vdetr_sp_union_map_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_union_map: null descriptor");
  VDETR_REQUIRE(d->na >= 0, "sp_union_map: na=%d is negative", d->na);
  VDETR_REQUIRE(d->nb >= 0, "sp_union_map: nb=%d is negative", d->nb);
  VDETR_REQUIRE((long long)d->na + d->nb <= 0x7fffffffLL, "sp_union_map: na=%d + nb=%d is more than 31 bits hold", d->na, d->nb);
  if (d->na == 0 && d->nb == 0) return VDETR_OK;
  VDETR_REQUIRE(d->a || d->na == 0, "sp_union_map: a is NULL with na=%d", d->na);
  VDETR_REQUIRE(d->b || d->nb == 0, "sp_union_map: b is NULL with nb=%d", d->nb);
  VDETR_REQUIRE(d->row_a || d->na == 0, "sp_union_map: row_a is NULL with na=%d", d->na);
  VDETR_REQUIRE(d->row_b || d->nb == 0, "sp_union_map: row_b is NULL with nb=%d", d->nb);
  VDETR_REQUIRE(d->u, "sp_union_map: u is NULL with na=%d nb=%d", d->na, d->nb);
  VDETR_REQUIRE(d->src_a, "sp_union_map: src_a is NULL with na=%d nb=%d", d->na, d->nb);
  VDETR_REQUIRE(d->src_b, "sp_union_map: src_b is NULL with na=%d nb=%d", d->na, d->nb);
  VDETR_REQUIRE(d->count, "sp_union_map: count is NULL with na=%d nb=%d", d->na, d->nb);
  VDETR_REQUIRE(d->workspace, "sp_union_map: workspace is NULL with na=%d nb=%d", d->na, d->nb);
  Carver c(d->workspace);
  const UnionWorkspace w = union_lay_out(c, d->na, d->nb);
  UnionParams P;
  P.na = d->na; P.nb = d->nb;
  P.ta = ceil_div(d->na, kUnionTile); P.tb = ceil_div(d->nb, kUnionTile);
  P.a = d->a; P.b = d->b; P.u = d->u;
  P.row_a = d->row_a; P.row_b = d->row_b; P.src_a = d->src_a; P.src_b = d->src_b; P.count = d->count;
  P.found_pos = w.found_pos; P.tile_matches = w.tile_matches;
  const dim3 grid((unsigned)(P.ta + P.tb));
  hipLaunchKernelGGL(union_search_kernel, grid, dim3(kUnionThreads), 0, (hipStream_t)stream, P);
  if (int e = check_launch("sp_union_map")) return e;
  hipLaunchKernelGGL(union_fill_kernel, grid, dim3(kUnionThreads), 0, (hipStream_t)stream, P);
  return check_launch("sp_union_map");
}

extern "C" size_t vdetr_sp_prune_map_workspace_bytes(int n) {
  if (n < 0) return 0;
  Carver c(nullptr);
  prune_lay_out(c, n);
  return c.bytes() + 256;
}

extern "C" int vdetr_sp_prune_map_i64(const vdetr_sp_prune_map_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_prune_map: null descriptor");
  VDETR_REQUIRE(d->N >= 0, "sp_prune_map: N=%d is negative", d->N);
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->mask, "sp_prune_map: mask is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->keys, "sp_prune_map: keys is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->kept, "sp_prune_map: kept is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->pos, "sp_prune_map: pos is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->keys_out, "sp_prune_map: keys_out is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->count, "sp_prune_map: count is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->workspace, "sp_prune_map: workspace is NULL with N=%d", d->N);
  Carver c(d->workspace);
  PruneParams P;
  P.n = d->N; P.tiles = ceil_div(d->N, kUnionTile);
  P.mask = d->mask; P.keys = d->keys; P.kept = d->kept; P.pos = d->pos; P.count = d->count; P.keys_out = d->keys_out;
  P.tile_counts = prune_lay_out(c, d->N);
  hipLaunchKernelGGL(prune_count_kernel, dim3((unsigned)P.tiles), dim3(kUnionThreads), 0, (hipStream_t)stream, P);
  if (int e = check_launch("sp_prune_map")) return e;
  hipLaunchKernelGGL(prune_fill_kernel, dim3((unsigned)P.tiles), dim3(kUnionThreads), 0, (hipStream_t)stream, P);
  return check_launch("sp_prune_map");
}

extern "C" int vdetr_sp_union_add_f32(const vdetr_sp_union_add_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_union_add: null descriptor");
  VDETR_REQUIRE(d->C > 0 && d->C % 4 == 0, "sp_union_add: C=%d must be a positive multiple of 4 (float4 rows)", d->C);
  VDETR_REQUIRE(d->sign == 1 || d->sign == -1, "sp_union_add: sign=%d (1 add, -1 subtract)", d->sign);
  VDETR_REQUIRE(d->nu >= 0, "sp_union_add: nu=%d is negative", d->nu);
  VDETR_REQUIRE(d->na >= 0, "sp_union_add: na=%d is negative", d->na);
  VDETR_REQUIRE(d->nb >= 0, "sp_union_add: nb=%d is negative", d->nb);
  if (d->nu == 0) return VDETR_OK;
  VDETR_REQUIRE(d->src_a, "sp_union_add: src_a is NULL with nu=%d", d->nu);
  VDETR_REQUIRE(d->src_b, "sp_union_add: src_b is NULL with nu=%d", d->nu);
  VDETR_REQUIRE(d->y, "sp_union_add: y is NULL with nu=%d", d->nu);
  VDETR_REQUIRE(d->a || d->na == 0, "sp_union_add: a is NULL with na=%d", d->na);
  VDETR_REQUIRE(d->b || d->nb == 0, "sp_union_add: b is NULL with nb=%d", d->nb);
  const long long blocks = ((long long)d->nu * (d->C / 4) + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_union_add: nu=%d x C=%d is more than one launch covers", d->nu, d->C);
  UnionAddParams P{d->nu, d->na, d->nb, d->C / 4, d->sign, d->a, d->b, d->src_a, d->src_b, d->y};
  hipLaunchKernelGGL(union_add_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_union_add");
}

extern "C" int vdetr_sp_take_rows_f32(const vdetr_sp_take_rows_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_take_rows: null descriptor");
  VDETR_REQUIRE(d->C > 0 && d->C % 4 == 0, "sp_take_rows: C=%d must be a positive multiple of 4 (float4 rows)", d->C);
  VDETR_REQUIRE(d->sign == 1 || d->sign == -1, "sp_take_rows: sign=%d (1 copy, -1 negate)", d->sign);
  VDETR_REQUIRE(d->nrows >= 0, "sp_take_rows: nrows=%d is negative", d->nrows);
  VDETR_REQUIRE(d->nsrc >= 0, "sp_take_rows: nsrc=%d is negative", d->nsrc);
  if (d->nrows == 0) return VDETR_OK;
  VDETR_REQUIRE(d->idx, "sp_take_rows: idx is NULL with nrows=%d", d->nrows);
  VDETR_REQUIRE(d->y, "sp_take_rows: y is NULL with nrows=%d", d->nrows);
  VDETR_REQUIRE(d->x || d->nsrc == 0, "sp_take_rows: x is NULL with nsrc=%d", d->nsrc);
  const long long blocks = ((long long)d->nrows * (d->C / 4) + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_take_rows: nrows=%d x C=%d is more than one launch covers", d->nrows, d->C);
  TakeRowsParams P{d->nrows, d->nsrc, d->C / 4, d->sign, d->x, d->idx, d->y};
  hipLaunchKernelGGL(take_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_take_rows");
}
