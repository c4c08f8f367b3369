// sparse_interp.hip — MinkowskiInterpolation: the features of a sparse tensor at float coordinates, trilinear over the 2^3 sites
// around every point; the map, the weighted 8-row gather and its transposed backward.  gfx950.
//
// Reference: ME.MinkowskiInterpolation / SparseTensor.features_at_coordinates.  MinkowskiEngine is un-vendored: the definition
// below is this package's own and tests/interp_restatement.py restates it in NumPy.
//
// Map.  One thread per point, no atomics, no memset, every thread writes only its own 8 + 8 words.  Per axis, at integer tensor
// stride s:  i = (int)floorf(x),  lo = floor_div(i, s) * s (towards minus infinity),  t = (x - (float)lo) / (float)s.
//   The subtraction.  lo is an integer below 2^17 in magnitude, a float32 and a multiple of ulp(x) (|x| <= 32768, so ulp(x) < 1);
//   the difference d = x - lo, 0 <= d < s, is a multiple of ulp(x) too.  For x >= 0, lo >= 0 and d <= x: d < 2^24 ulp(x) and the
//   subtraction is EXACT.  For x < 0 it is exact whenever |lo| / 2 <= |x| (Sterbenz).  What is left is a negative x in the upper
//   half of the cell that ends at zero or of one whose lower site is more than twice as far from zero: there d may need more
//   bits than a float32 has (x = -2^-30, s = 1: d = 1 - 2^-30) and is rounded ONCE, by at most 2^-25 d.  t then comes within
//   two roundings of the real quotient, and may round to exactly 1: the lower corner's weight is then an exact 0 and the upper
//   one's 1, which is the nearest float32 statement of the same point.
// Corner k = 4 bx + 2 by + bz, bit 1 = the upper site lo + s; w = (fx * fy) * fz with f = b ? t : 1 - t.  A corner whose
// coordinate leaves its field of the key (sparse_key.h) is absent (-1): it is tested on the coordinate BEFORE the key is packed, so
// nothing carries into the neighbouring field.  w = 0 wherever nbr = -1.  A row with a non-finite coordinate, a floorf outside
// -32768 .. 32767 or a batch value that is not an integer in 0 .. 32767 gets eight -1.
// The eight corners are four z-adjacent pairs: ONE lower bound per pair (four interleaved binary searches over the sorted keys,
// four independent loads per step).  The upper-z site, if there, is the next sorted key when the sites lie on the lattice of s;
// where some other key sits in between (a key set off the lattice) the pair falls back to a second search, so nbr is the row of
// the corner's key for ANY sorted unique key set.
//
// Forward.  out[n, :] = sum over k ascending, pairs with nbr >= 0 only, of w[n, k] * F[nbr[n, k], :], float32, multiply then add
// (no fused multiply-add), from +0.  A pair of weight 0 is still a pair (0 * inf is a NaN, as IEEE says).  A float4 of channels
// per lane where C % 4 == 0 (the lanes of a row read its eight indices and weights from the same two cache lines), one channel
// per lane otherwise.  M == 0 writes zeros.
//
// Backward.  Many points share a corner, so the transposed sum has no single writer per pair and a scatter would need float
// atomics.  Instead the 8N pair site rows are sorted by a STABLE library sort (the host layer: torch.sort), absent pairs (-1)
// first; interp_seg_kernel writes seg [M + 1] by one lower bound per site — empty sites get an empty run — and the permutation
// as int32; interp_bwd_kernel folds every site's run in sorted order = ascending (n, k):
//   dF[m, :] = sum of w[p] * dy[p >> 3, :] over p = order[seg[m] .. seg[m + 1]),  float32, from +0: a site with no pair gets +0.
// One lane per (site, float4 of channels | channel), four pairs' loads in flight per lane, the adds in order.  No atomics: two
// runs give the same bits.  A site with L pairs is L dependent adds on its lanes: every point in one cell is eight serial walks.
#include "common.h"
#include "sparse_key.h"

namespace vdetr {

constexpr int kInterpTile = 256;  // points per workgroup of the map launch (vdetr_sp_interp_tile)

struct InterpMapParams {
  int M, N, s, steps;      // steps: binary-search steps that empty any range of M keys
  const int64_t* keys;     // [M] ascending, unique
  const float4* tfield;    // [N] (batch, x, y, z)
  int4* nbr;               // [N][2]
  float4* w;               // [N][2]
};

// floor(x) as an index a key may hold, its lower site and the weight of the UPPER site; false where the row has no corner
__device__ __forceinline__ bool interp_axis(float x, int s, int& lo, float& t) {
  const float f = floorf(x);
  if (!(f >= -32768.f && f <= 32767.f)) return false;  // (a NaN fails both comparisons)
  const int i = (int)f;
  const int q = i >= 0 ? i / s : -((-i + s - 1) / s);  // floor_div: towards minus infinity
  lo = q * s;
  t = (x - (float)lo) / (float)s;
  return true;
}

__global__ __launch_bounds__(kInterpTile) void interp_map_kernel(InterpMapParams P) {
  const int n = (int)blockIdx.x * kInterpTile + (int)threadIdx.x;
  if (n >= P.N) return;
  const float4 p = P.tfield[n];
  int lo[3];
  float t[3];
  bool row = p.x >= 0.f && p.x <= 32767.f && floorf(p.x) == p.x;  // (a NaN or an infinity fails)
  row = interp_axis(p.y, P.s, lo[0], t[0]) && row;
  row = interp_axis(p.z, P.s, lo[1], t[1]) && row;
  row = interp_axis(p.w, P.s, lo[2], t[2]) && row;
  int nb[8];
  float wt[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { nb[k] = -1; wt[k] = 0.f; }
  if (row && P.M > 0) {
    const bool zlo_in = key_in_field(lo[2]), zhi_in = key_in_field(lo[2] + P.s);
    // the key of the lower-z corner of pair j = 2 bx + by (z clamped into the field: an absent lower z still places the search)
    int64_t key[4];
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = lo[0] + (j >> 1) * P.s, y = lo[1] + (j & 1) * P.s;
      in[j] = key_in_field(x) && key_in_field(y) && (zlo_in || zhi_in);
      const int z = zlo_in ? lo[2] : lo[2] + P.s;
      key[j] = key_pack_fields((int)p.x, x, y, z);  // (tested above: a pair that is not `in` never reads its key's row)
    }
    // four lower bounds interleaved, four loads in flight per step: deliberately not four calls of key_lower_bound
    int a[4] = {0, 0, 0, 0}, e[4] = {P.M, P.M, P.M, P.M};  // lower bounds: keys[< a] < key <= keys[>= e]
    for (int step = 0; step < P.steps; ++step) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int mid = (int)(((unsigned)a[j] + (unsigned)e[j]) >> 1);  // a == e == M stays put: mid is then not read
        if (a[j] < e[j]) {
          if (P.keys[mid] < key[j]) a[j] = mid + 1; else e[j] = mid;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!in[j]) continue;
      int at = a[j];
      if (zlo_in) {
        if (at < P.M && P.keys[at] == key[j]) nb[2 * j] = at++;
        if (!zhi_in) continue;
        key[j] += P.s;  // (z + s is inside the field: no carry)
      }
      // the upper z: the next sorted key on a lattice of s; a key in between (off the lattice) asks for a search of its own
      if (at < P.M && P.keys[at] < key[j]) at += key_lower_bound(P.keys + at, P.M - at, key[j]);
      if (at < P.M && P.keys[at] == key[j]) nb[2 * j + 1] = at;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float fx = (k & 4) ? t[0] : 1.f - t[0], fy = (k & 2) ? t[1] : 1.f - t[1], fz = (k & 1) ? t[2] : 1.f - t[2];
      wt[k] = nb[k] >= 0 ? (fx * fy) * fz : 0.f;
    }
  }
  P.nbr[2 * (size_t)n] = make_int4(nb[0], nb[1], nb[2], nb[3]);
  P.nbr[2 * (size_t)n + 1] = make_int4(nb[4], nb[5], nb[6], nb[7]);
  P.w[2 * (size_t)n] = make_float4(wt[0], wt[1], wt[2], wt[3]);
  P.w[2 * (size_t)n + 1] = make_float4(wt[4], wt[5], wt[6], wt[7]);
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
struct InterpParams {
  int M, N, C;
  const float* x;          // forward: F [M, C]; backward: dy [N, C]
  const int32_t* nbr;      // [N, 8]
  const float* w;          // [N, 8]
  const int32_t* order;    // [8 N]
  const int32_t* seg;      // [M + 1]
  float* y;                // forward: out [N, C]; backward: dF [M, C]
};

// V = float4 (C % 4 == 0, lanes = C / 4) or float (lanes = C)
template <typename V>
__device__ __forceinline__ V interp_axpy(V acc, float w, V v);
template <>
__device__ __forceinline__ float interp_axpy<float>(float acc, float w, float v) { return acc + w * v; }
template <>
__device__ __forceinline__ float4 interp_axpy<float4>(float4 acc, float w, float4 v) {
  return make_float4(acc.x + w * v.x, acc.y + w * v.y, acc.z + w * v.z, acc.w + w * v.w);
}
template <typename V>
__device__ __forceinline__ V interp_zero();
template <>
__device__ __forceinline__ float interp_zero<float>() { return 0.f; }
template <>
__device__ __forceinline__ float4 interp_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

template <typename V>
__global__ __launch_bounds__(256) void interp_fwd_kernel(InterpParams P, int lanes) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.N * lanes) return;
  const int c = (int)(t % lanes);
  const size_t n = (size_t)(t / lanes);
  const int4 r0 = reinterpret_cast<const int4*>(P.nbr)[2 * n], r1 = reinterpret_cast<const int4*>(P.nbr)[2 * n + 1];
  const float4 w0 = reinterpret_cast<const float4*>(P.w)[2 * n], w1 = reinterpret_cast<const float4*>(P.w)[2 * n + 1];
  const int r[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  const V* x = reinterpret_cast<const V*>(P.x);
  V v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)  // the eight row loads are independent: all in flight before the first add
    v[k] = (unsigned)r[k] < (unsigned)P.M ? x[(size_t)r[k] * lanes + c] : interp_zero<V>();
  V acc = interp_zero<V>();
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((unsigned)r[k] < (unsigned)P.M) acc = interp_axpy<V>(acc, w[k], v[k]);
  reinterpret_cast<V*>(P.y)[t] = acc;
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
struct InterpSegParams {
  int M, P;                // sites, pairs (8 N)
  const int32_t* sorted;   // [P] the pair site rows ascending, -1 (absent) first
  const int64_t* order;    // [P] the stable sort's permutation
  int32_t* order32;        // [P]
  int32_t* seg;            // [M + 1]
};

__global__ __launch_bounds__(256) void interp_seg_kernel(InterpSegParams P) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < P.P) P.order32[i] = (int32_t)P.order[i];
  if (i <= P.M) {  // seg[m] = the first sorted position whose site row is >= m; seg[M] = P (rows are below M)
    P.seg[i] = key_lower_bound(P.sorted, P.P, (int32_t)i);
  }
}

template <typename V>
__global__ __launch_bounds__(256) void interp_bwd_kernel(InterpParams P, int lanes) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.M * lanes) return;
  const int c = (int)(t % lanes);
  const int m = (int)(t / lanes);
  const long long pairs = 8ll * P.N;
  const long long j0 = max(P.seg[m], 0), j1 = min((long long)P.seg[m + 1], pairs);
  const V* dy = reinterpret_cast<const V*>(P.x);
  V acc = interp_zero<V>();
  long long j = j0;
  for (; j + 4 <= j1; j += 4) {  // four pairs' loads in flight, the adds in order
    int p[4];
    float w[4];
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) p[u] = P.order[j + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = (unsigned)p[u] < (unsigned long long)pairs;
      w[u] = ok ? P.w[p[u]] : 0.f;
      v[u] = ok ? dy[(size_t)(p[u] >> 3) * lanes + c] : interp_zero<V>();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if ((unsigned)p[u] < (unsigned long long)pairs) acc = interp_axpy<V>(acc, w[u], v[u]);
  }
  for (; j < j1; ++j) {
    const int p = P.order[j];
    if ((unsigned)p >= (unsigned long long)pairs) continue;
    acc = interp_axpy<V>(acc, P.w[p], dy[(size_t)(p >> 3) * lanes + c]);
  }
  reinterpret_cast<V*>(P.y)[t] = acc;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_sp_interp_tile(void) { return kInterpTile; }

extern "C" int vdetr_sp_interp_map_f32(const vdetr_sp_interp_map_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d, "sp_interp_map: null descriptor");
  VDETR_REQUIRE(d->N >= 0, "sp_interp_map: N=%d is negative", d->N);
  VDETR_REQUIRE(d->M >= 0, "sp_interp_map: M=%d is negative", d->M);
  VDETR_REQUIRE(d->stride >= 1 && d->stride <= 32768, "sp_interp_map: tensor stride s=%d (1 .. 32768)", d->stride);
  VDETR_REQUIRE(d->N <= 0x7fffffff / 8, "sp_interp_map: N=%d points have more than 2^31 pairs", d->N);
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->keys || d->M == 0, "sp_interp_map: keys is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->tfield, "sp_interp_map: tfield is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->nbr, "sp_interp_map: nbr is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->w, "sp_interp_map: w is NULL with N=%d", d->N);
  VDETR_REQUIRE(aligned16(d->tfield) && aligned16(d->nbr) && aligned16(d->w),
                "sp_interp_map: tfield, nbr and w must be 16-byte aligned ([N, 4] and [N, 8] rows)");
  int steps = 0;
  while ((1ll << steps) <= (long long)d->M) ++steps;  // a range of M keys is empty after floor(log2 M) + 1 halvings
  InterpMapParams P{d->M, d->N, d->stride, steps, d->keys, reinterpret_cast<const float4*>(d->tfield),
                    reinterpret_cast<int4*>(d->nbr), reinterpret_cast<float4*>(d->w)};
  hipLaunchKernelGGL(interp_map_kernel, dim3((unsigned)ceil_div(d->N, kInterpTile)), dim3(kInterpTile), 0, (hipStream_t)stream, P);
  return check_launch("sp_interp_map");
}

static int interp_common(const char* op, const vdetr_sp_interp_desc* d) {
  VDETR_REQUIRE(d, "%s: null descriptor", op);
  VDETR_REQUIRE(d->C >= 1, "%s: C=%d must be positive", op, d->C);
  VDETR_REQUIRE(d->M >= 0, "%s: M=%d is negative", op, d->M);
  VDETR_REQUIRE(d->N >= 0, "%s: N=%d is negative", op, d->N);
  VDETR_REQUIRE(d->N <= 0x7fffffff / 8, "%s: N=%d points have more than 2^31 pairs", op, d->N);
  return VDETR_OK;
}

extern "C" int vdetr_sp_interp_fwd_f32(const vdetr_sp_interp_desc* d, vdetr_stream_t stream) {
  if (int e = interp_common("sp_interp_fwd", d)) return e;
  if (d->N == 0) return VDETR_OK;
  VDETR_REQUIRE(d->x || d->M == 0, "sp_interp_fwd: x is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->nbr, "sp_interp_fwd: nbr is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->w, "sp_interp_fwd: w is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->y, "sp_interp_fwd: y is NULL with N=%d", d->N);
  VDETR_REQUIRE(aligned16(d->nbr) && aligned16(d->w), "sp_interp_fwd: nbr and w must be 16-byte aligned ([N, 8] rows)");
  const bool wide = d->C % 4 == 0 && aligned16(d->x) && aligned16(d->y);
  const int lanes = wide ? d->C / 4 : d->C;
  const long long blocks = ((long long)d->N * lanes + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_interp_fwd: N=%d x C=%d is more than one launch covers", d->N, d->C);
  InterpParams P{d->M, d->N, d->C, d->x, d->nbr, d->w, nullptr, nullptr, d->y};
  if (wide) hipLaunchKernelGGL(interp_fwd_kernel<float4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, lanes);
  else hipLaunchKernelGGL(interp_fwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, lanes);
  return check_launch("sp_interp_fwd");
}

extern "C" int vdetr_sp_interp_seg_i32(const int32_t* sorted, const int64_t* order, int M, int N, int32_t* order32, int32_t* seg,
                                       vdetr_stream_t stream) {
  VDETR_REQUIRE(M >= 0, "sp_interp_seg: M=%d is negative", M);
  VDETR_REQUIRE(N >= 0, "sp_interp_seg: N=%d is negative", N);
  VDETR_REQUIRE(N <= 0x7fffffff / 8, "sp_interp_seg: N=%d points have more than 2^31 pairs", N);
  VDETR_REQUIRE(seg, "sp_interp_seg: seg is NULL");
  VDETR_REQUIRE((sorted && order && order32) || N == 0, "sp_interp_seg: a NULL operand with N=%d", N);
  InterpSegParams P{M, 8 * N, sorted, order, order32, seg};
  const long long threads = (long long)P.P > (long long)M + 1 ? (long long)P.P : (long long)M + 1;
  hipLaunchKernelGGL(interp_seg_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("sp_interp_seg");
}

extern "C" int vdetr_sp_interp_bwd_f32(const vdetr_sp_interp_desc* d, vdetr_stream_t stream) {
  if (int e = interp_common("sp_interp_bwd", d)) return e;
  if (d->M == 0) return VDETR_OK;
  VDETR_REQUIRE(d->y, "sp_interp_bwd: y is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->seg, "sp_interp_bwd: seg is NULL with M=%d", d->M);
  VDETR_REQUIRE(d->x || d->N == 0, "sp_interp_bwd: x is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->w || d->N == 0, "sp_interp_bwd: w is NULL with N=%d", d->N);
  VDETR_REQUIRE(d->order || d->N == 0, "sp_interp_bwd: order is NULL with N=%d", d->N);
  const bool wide = d->C % 4 == 0 && aligned16(d->x) && aligned16(d->y);
  const int lanes = wide ? d->C / 4 : d->C;
  const long long blocks = ((long long)d->M * lanes + 255) / 256;
  VDETR_REQUIRE(blocks <= 0x7fffffffLL, "sp_interp_bwd: M=%d x C=%d is more than one launch covers", d->M, d->C);
  InterpParams P{d->M, d->N, d->C, d->x, nullptr, d->w, d->order, d->seg, d->y};
  if (wide) hipLaunchKernelGGL(interp_bwd_kernel<float4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, lanes);
  else hipLaunchKernelGGL(interp_bwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, lanes);
  return check_launch("sp_interp_bwd");
}
