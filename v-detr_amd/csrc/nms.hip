// nms.hip — greedy 3-D non-maximum suppression of a scene's box predictions on the device (the
// evaluation's post-processing; reference utils/nms.py:78-162 called from utils/ap_calculator.py:165-220).
//
// The reference copies corners / scores to the host and runs a numpy loop per scene: pick the best remaining box, delete
// every remaining box of the same class whose IoU with it exceeds the threshold, repeat (~K numpy round trips of K-long
// vectors; 50-100 ms for 1024 boxes).  Here one workgroup per scene:
//   1. axis-aligned extents = min / max over the 8 corners (ap_calculator.py:168-214), volumes in fp64 as numpy has them
//      (np.zeros((K, 8)) is a float64 array filled with float32 values);
//   2. the K x K "i suppresses j" relation as a bit matrix in the caller's workspace, all threads, same fp64 expression
//      `inter / (area_i + area_j - inter) > thr` (or inter / area_j for old_type) times the class equality;
//   3. one wave walks the boxes in score order: a box still alive is kept and ORs its row into the dead set.
// Greedy suppression is inherently sequential in the kept boxes; the walk costs ~100 cycles per box.
// The rotated form (vdetr_nms3d_rot_f32) replaces steps 1 and 2: the corners themselves in rank order, and
// the relation from the reference's box3d_iou of the two boxes (nms3d_rot_relation_kernel, next to the clip routine below).
#include "wave.h"
#include "workspace.h"

namespace vdetr {
namespace {

struct NmsParams {
  const float* corners;       // [B,K,8,3]
  const int32_t* cls;         // [B,K] or NULL (class-agnostic)
  const uint8_t* valid;       // [B,K] or NULL
  const int64_t* order;       // [B,K] ascending stable arg-sort of score
  uint8_t* keep;              // [B,K]
  // workspace
  float* ext;                 // [B,K,6] extents in rank order (rank r = r-th best box: order[K-1-r])
  int* rcls;                  // [B,K] class in rank order; < 0: invalid box (matches nothing)
  unsigned long long* rel;    // [B,K,W] "rank r suppresses rank 64w+t" bits, W = ceil(K/64)
  float* rcorn;               // [B,K,8,3] corners in rank order (rotated NMS; then ext is unused), else NULL
  int K, W, old_type;
  double thr;
};

// 1. extents (or, for the rotated relation, the 24 corner floats) + classes in rank order
__global__ __launch_bounds__(256) void nms3d_prepare_kernel(NmsParams P) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x, K = P.K;
  if (r >= K) return;
  const int i = (int)P.order[(size_t)b * K + K - 1 - r];
  const float* c = P.corners + ((size_t)b * K + i) * 24;
  if (P.rcorn) {  // rotated NMS: the relation needs the box itself, not its hull
    float* o = P.rcorn + ((size_t)b * K + r) * 24;
    for (int k = 0; k < 24; ++k) o[k] = c[k];
  } else {
    float lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
    for (int k = 1; k < 8; ++k)
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(lo[a], c[k * 3 + a]);
        hi[a] = fmaxf(hi[a], c[k * 3 + a]);
      }
    float* e = P.ext + ((size_t)b * K + r) * 6;
    for (int a = 0; a < 3; ++a) e[a] = lo[a], e[3 + a] = hi[a];
  }
  const bool ok = P.valid == nullptr || P.valid[(size_t)b * K + i] != 0;
  P.rcls[(size_t)b * K + r] = ok ? (P.cls ? P.cls[(size_t)b * K + i] : 0) : -1 - r;
}

// 2. the K x K relation over the whole GPU: grid (K/256, 4W, B).  A thread owns rank r and builds a quarter (16 bits) of
//    word blockIdx.y/4 of its row; the 16 partner boxes are staged in LDS as float64 extents + volume (broadcast
//    reads), and only ranks worse than r are evaluated.  The division is skipped where no lane has an intersection.
constexpr int kNmsQuarter = 16;
__global__ __launch_bounds__(256) void nms3d_relation_kernel(NmsParams P) {
  __shared__ double sbox[kNmsQuarter][8];
  __shared__ int scls[kNmsQuarter];
  const int b = blockIdx.z, piece = blockIdx.y, K = P.K, W = P.W;
  const int r = blockIdx.x * 256 + threadIdx.x, s0 = piece * kNmsQuarter;
  unsigned short* out = reinterpret_cast<unsigned short*>(P.rel + (size_t)b * K * W);
  if (s0 + kNmsQuarter - 1 <= (int)(blockIdx.x * 256) || s0 >= K) {  // every pair of this block has s <= r
    if (r < K) out[(size_t)r * W * 4 + piece] = 0;
    return;
  }
  const float* __restrict__ ext = P.ext + (size_t)b * K * 6;
  const int* __restrict__ cls = P.rcls + (size_t)b * K;
  if (threadIdx.x < kNmsQuarter) {
    const int s = s0 + threadIdx.x;
    double c[6];
    for (int q = 0; q < 6; ++q) c[q] = s < K ? (double)ext[(size_t)s * 6 + q] : 0.0;
    for (int q = 0; q < 6; ++q) sbox[threadIdx.x][q] = c[q];
    sbox[threadIdx.x][6] = ((c[3] - c[0]) * (c[4] - c[1])) * (c[5] - c[2]);  // float64 volumes, as numpy computes them
    scls[threadIdx.x] = s < K ? cls[s] : -1;  // a negative class (invalid box, see prepare) matches nothing
  }
  __syncthreads();
  if (r >= K) return;
  unsigned bits = 0u;
  const int cr = cls[r];
  double a[6];
  for (int q = 0; q < 6; ++q) a[q] = (double)ext[(size_t)r * 6 + q];
  const double va = ((a[3] - a[0]) * (a[4] - a[1])) * (a[5] - a[2]);
  const bool always_divide = !(P.thr >= 0.0);
#pragma unroll
  for (int t = 0; t < kNmsQuarter; ++t) {
    const double* c = sbox[t];
    const bool pair = s0 + t > r && scls[t] == cr;
    const double l = fmax(0.0, fmin(a[3], c[3]) - fmax(a[0], c[0]));
    const double wd = fmax(0.0, fmin(a[4], c[4]) - fmax(a[1], c[1]));
    const double h = fmax(0.0, fmin(a[5], c[5]) - fmax(a[2], c[2]));
    const double inter = (l * wd) * h;
    if (pair && (inter > 0.0 || always_divide)) {  // inter == 0: the ratio is 0 or NaN, never above a threshold >= 0
      const double o = P.old_type ? inter / c[6] : inter / ((va + c[6]) - inter);
      if (o > P.thr) bits |= 1u << t;
    }
  }
  out[(size_t)r * W * 4 + piece] = (unsigned short)(cr >= 0 ? bits : 0u);
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// 3. the greedy walk, one workgroup per scene.  The relation is pulled into LDS when it fits (K <= 1024: 128 KB); then
//    ONE wave walks the ranks 64 at a time: lane l owns word l of the dead set (K <= 4096: <= 64 words); inside a block
//    of 64 ranks only the diagonal word decides, which is resolved with scalar instructions (lane t holds row t's
//    diagonal word); the rows of the block's survivors are then OR-ed into every lane's word with 64 unconditional,
//    masked loads (no dependent latency chain).  A box is kept iff its bit is still clear at the end: a row only has
//    bits of worse ranks, so nothing can kill a rank after its own turn.
constexpr int kNmsThreads = 1024;
template <bool IN_LDS>
__global__ __launch_bounds__(kNmsThreads) void nms3d_walk_kernel(NmsParams P) {
  extern __shared__ unsigned long long srel[];
  __shared__ unsigned long long dead0[64];
  const int b = blockIdx.x, tid = threadIdx.x, K = P.K, W = P.W;
  const unsigned long long* __restrict__ grel = P.rel + (size_t)b * K * W;
  const int* cls = P.rcls + (size_t)b * K;
  for (int r0 = 0; r0 < 64 * W; r0 += kNmsThreads) {  // invalid boxes and the tail of the last word start out dead
    const int r = r0 + tid;
    const unsigned long long m = __ballot(r >= K || cls[min(r, K - 1)] < 0);
    if ((tid & 63) == 0 && (r >> 6) < W) dead0[r >> 6] = m;
  }
  if (IN_LDS) {  // 8 loads in flight per thread: the copy is one memory round trip, not sixteen
    const int n = K * W;
    for (int e0 = 0; e0 < n; e0 += 8 * kNmsThreads) {
      unsigned long long v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = e0 + q * kNmsThreads + tid;
        v[q] = e < n ? grel[e] : 0ull;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = e0 + q * kNmsThreads + tid;
        if (e < n) srel[e] = v[q];
      }
    }
  }
  __syncthreads();
  // one address space per instantiation: a pointer that may be either would compile to flat loads
  auto rel_at = [&](int e) -> unsigned long long { return IN_LDS ? srel[e] : grel[e]; };
  if (tid < 64) {
    // lane layout of the apply step: W2 = W rounded up to a power of two; lane = q * W2 + word, so one load instruction
    // fetches 64 / W2 rows of the block at once
    int W2 = 1;
    while (W2 < W) W2 <<= 1;
    const int rows_per_load = 64 / W2, q = tid / W2, wd = tid & (W2 - 1);
    const bool word_ok = wd < W;
    const int lw = min(wd, W - 1);
    unsigned long long mine = tid < W ? dead0[tid] : ~0ull;
    for (int w = 0; w < W; ++w) {
      const unsigned long long diag = rel_at(min(64 * w + tid, K - 1) * W + w);
      unsigned long long dw = readlane_u64(mine, w);
#pragma unroll
      for (int t = 0; t < 64; ++t) {
        const unsigned long long d = readlane_u64(diag, t);
        if (!((dw >> t) & 1ull)) dw |= d;
      }
      const unsigned long long alive = ~dw;  // survivors of this block (wave-uniform)
      const int last = K - 1 - 64 * w;       // rows beyond the last box are clamped; their alive bit is clear
      unsigned long long acc = 0ull;
#pragma unroll 4
      for (int i = 0; i < W2; ++i) {
        const int t = i * rows_per_load + q;
        const unsigned long long row = rel_at((64 * w + min(t, last)) * W + lw);
        acc |= ((alive >> t) & 1ull) && word_ok ? row : 0ull;
      }
      for (int off = W2; off < 64; off <<= 1) acc |= __shfl_xor(acc, off);  // OR over the q groups
      mine |= acc;                                                          // lane l < W: word l
    }
    dead0[tid] = mine;
  }
  __syncthreads();
  for (int r = tid; r < K; r += kNmsThreads)
    P.keep[(size_t)b * K + (int)P.order[(size_t)b * K + K - 1 - r]] = (uint8_t)(((~dead0[r >> 6]) >> (r & 63)) & 1ull);
}

// ---------------------------------------------------------------------------------------------------------------------
// points inside every predicted box (parse_predictions' remove_empty_box, utils/ap_calculator.py:78-93: mmcv
// points_in_boxes_all -> [B,N,K] flags -> sum over the points).  The flags are never materialised: a thread owns a box, a
// workgroup walks a slice of the scene's points through LDS (broadcast reads) and adds its count with one integer atomic.
// The test is mmcv's check_pt_in_box3d (bottom-centre z convention, strict x / y bounds in the box frame, yaw by -rz).
constexpr int kCountChunk = 1024;  // points staged per round
__global__ __launch_bounds__(256) void box_point_count_kernel(const float* __restrict__ points, const float* __restrict__ boxes,
                                                              int N, int K, int slice, int* __restrict__ counts) {
  __shared__ float4 pts[kCountChunk];
  const int b = blockIdx.z, k = blockIdx.y * 256 + threadIdx.x;
  const int n0 = blockIdx.x * slice, n1 = min(N, n0 + slice);
  float cx = 0.f, cy = 0.f, zc = 0.f, hx = -1.f, hy = -1.f, hz = -1.f, ca = 1.f, sa = 0.f;
  if (k < K) {
    const float* r = boxes + ((size_t)b * K + k) * 7;  // centre xyz, sizes, yaw
    const float zb = r[2] - r[5] / 2.f;                // the caller's bottom-centre shift (ap_calculator.py:80) ...
    zc = zb + r[5] / 2.f;                              // ... and mmcv's shift back to the centre
    cx = r[0]; cy = r[1];
    hx = r[3] / 2.f; hy = r[4] / 2.f; hz = r[5] / 2.f;
    ca = cosf(-r[6]); sa = sinf(-r[6]);
  }
  int cnt = 0;
  for (int c0 = n0; c0 < n1; c0 += kCountChunk) {
    const int m = min(kCountChunk, n1 - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += 256) {
      const float* p = points + ((size_t)b * N + c0 + i) * 3;
      pts[i] = make_float4(p[0], p[1], p[2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
      const float4 p = pts[i];
      const float sx = p.x - cx, sy = p.y - cy;
      const float lx = sx * ca - sy * sa, ly = sx * sa + sy * ca;
      const bool in = !(fabsf(p.z - zc) > hz) && lx > -hx && lx < hx && ly > -hy && ly < hy;
      cnt += in ? 1 : 0;
    }
  }
  if (k < K && cnt) atomicAdd(counts + (size_t)b * K + k, cnt);
}

// ---------------------------------------------------------------------------------------------------------------------
// best ground-truth box of every detection (utils/eval_det.py:160-172 -> get_iou_obb -> utils/box_util.py:122-147
// box3d_iou): float64 on the float32 corners, the reference's Sutherland-Hodgman clip of the two x-z footprints
// (box_util.py:37-84: strict `inside`, the same intersection formula and operation order), heights from corners 0 / 4,
// volumes from three edge lengths.  The overlap area is the area of the convex hull of the clipped points, as the reference
// takes it from qhull (see the end of footprint_intersection).
struct P2 {
  double x, y;
};
__device__ __forceinline__ double box3d_vol64(const float* c) {
  auto len = [&](int i, int j) {
    const double dx = (double)c[i * 3] - (double)c[j * 3], dy = (double)c[i * 3 + 1] - (double)c[j * 3 + 1],
                 dz = (double)c[i * 3 + 2] - (double)c[j * 3 + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
  };
  return (len(0, 1) * len(1, 2)) * len(0, 4);
}
// subject / clip: the two footprints as float64 (x, z) of corners 3, 2, 1, 0: counter-clockwise (box_util.py:135-136)
__device__ double footprint_intersection(const P2* subject, const P2* clip) {
  P2 out[10], in[10];
  int n = 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = subject[i];
  P2 cp1 = clip[3];
  for (int cv = 0; cv < 4; ++cv) {
    const P2 cp2 = clip[cv];
    const int m = n;
    for (int i = 0; i < m; ++i) in[i] = out[i];
    n = 0;
    auto inside = [&](const P2& p) { return (cp2.x - cp1.x) * (p.y - cp1.y) > (cp2.y - cp1.y) * (p.x - cp1.x); };
    auto cross_point = [&](const P2& s, const P2& e) {
      const double dc0 = cp1.x - cp2.x, dc1 = cp1.y - cp2.y, dp0 = s.x - e.x, dp1 = s.y - e.y;
      const double n1 = cp1.x * cp2.y - cp1.y * cp2.x, n2 = s.x * e.y - s.y * e.x;
      const double n3 = 1.0 / (dc0 * dp1 - dc1 * dp0);
      return P2{(n1 * dp0 - n2 * dc0) * n3, (n1 * dp1 - n2 * dc1) * n3};
    };
    P2 sv = in[m - 1];
    for (int i = 0; i < m; ++i) {
      const P2 e = in[i];
      if (inside(e)) {
        if (!inside(sv) && n < 10) out[n++] = cross_point(sv, e);
        if (n < 10) out[n++] = e;
      } else if (inside(sv)) {
        if (n < 10) out[n++] = cross_point(sv, e);
      }
      sv = e;
    }
    cp1 = cp2;
    if (n == 0) return 0.0;
  }
  // The reference hands the clipped points to qhull and takes the hull's area (box_util.py:92-105).  For a well-conditioned
  // clip that is the polygon itself; for nearly coincident rotated boxes the intersection formula divides by ~0 and the
  // "polygon" is garbage whose HULL the reference still measures (IoU > 1 happens) -- so the hull it is: monotone chain
  // over <= 10 points.  qhull raises on non-finite or degenerate input and the reference then counts no overlap.
  if (n < 3) return 0.0;
  for (int i = 0; i < n; ++i)
    if (!(fabs(out[i].x) < INFINITY) || !(fabs(out[i].y) < INFINITY)) return 0.0;
  for (int i = 1; i < n; ++i) {  // insertion sort by (x, y)
    const P2 v = out[i];
    int j = i - 1;
    while (j >= 0 && (out[j].x > v.x || (out[j].x == v.x && out[j].y > v.y))) {
      out[j + 1] = out[j];
      --j;
    }
    out[j + 1] = v;
  }
  auto turn = [](const P2& o, const P2& a, const P2& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); };
  P2 chain[20];
  int h = 0;
  for (int i = 0; i < n; ++i) {  // lower chain
    while (h >= 2 && turn(chain[h - 2], chain[h - 1], out[i]) <= 0.0) --h;
    chain[h++] = out[i];
  }
  const int lower = h + 1;
  for (int i = n - 2; i >= 0; --i) {  // upper chain
    while (h >= lower && turn(chain[h - 2], chain[h - 1], out[i]) <= 0.0) --h;
    chain[h++] = out[i];
  }
  --h;  // the last point repeats the first
  if (h < 3) return 0.0;
  double acc = 0.0;
  for (int i = 0; i < h; ++i) {
    const P2 a = chain[i], b = chain[(i + 1) % h];
    acc += a.x * b.y - a.y * b.x;
  }
  return 0.5 * fabs(acc);
}
__device__ __forceinline__ void footprint64(const float* c, P2* rect) {
#pragma unroll
  for (int i = 0; i < 4; ++i) rect[i] = P2{(double)c[(3 - i) * 3], (double)c[(3 - i) * 3 + 2]};
}
__device__ __forceinline__ double footprint_intersection(const float* c1, const float* c2) {
  P2 r1[4], r2[4];
  footprint64(c1, r1);
  footprint64(c2, r2);
  return footprint_intersection(r1, r2);
}
__global__ __launch_bounds__(128) void box3d_iou_max_kernel(const float* __restrict__ pred, const int* __restrict__ pred_img,
                                                            const int* __restrict__ pred_cls, int P, const float* __restrict__ gt,
                                                            const int* __restrict__ gt_cls, const int* __restrict__ img_gt_begin,
                                                            double* __restrict__ ovmax, int* __restrict__ jmax) {
  const int d = blockIdx.x * 128 + threadIdx.x;
  if (d >= P) return;
  float c1[24];
  for (int k = 0; k < 24; ++k) c1[k] = pred[(size_t)d * 24 + k];
  const int img = pred_img[d], cls = pred_cls[d];
  const double vol1 = box3d_vol64(c1);
  double best = -INFINITY;
  int arg = -1;
  for (int j = img_gt_begin[img]; j < img_gt_begin[img + 1]; ++j) {
    if (gt_cls[j] != cls) continue;
    float c2[24];
    for (int k = 0; k < 24; ++k) c2[k] = gt[(size_t)j * 24 + k];
    const double area = footprint_intersection(c1, c2);
    const double ymax = fmin((double)c1[1], (double)c2[1]), ymin = fmax((double)c1[13], (double)c2[13]);
    const double inter_vol = area * fmax(0.0, ymax - ymin);
    const double iou = inter_vol / ((vol1 + box3d_vol64(c2)) - inter_vol);
    if (iou > best) best = iou, arg = j;  // the first of equal maxima stays (eval_det.py:169-171)
  }
  ovmax[d] = best;
  jmax[d] = arg;
}

// The same matching with the detections given as (box row, class) pairs of the evaluation's device store (eval_store.hip,
// DESIGN.md 6.12): thread e = r * max(C, 1) + c takes box row r and class c (C = 0: the stored class) and writes detection
// d = C box_begin[s] + c n_s + (r - box_begin[s]) of the reference's per-scan class-major list order, with its class and
// score.  The loop over the scan's ground truth is box3d_iou_max_kernel's, expression for expression.  Everything read from
// the store is device data: rows and scans outside the host's counts write nothing.
//
// kSized (vdetr_box3d_iou_max_size_f64): the size split of --test_size.  box_size / gt_size hold the volume class of
// every box row and ground-truth row (box3d_size_class_kernel below); a ground-truth row is a candidate only if it is of the
// box's class, a box of class 3 (on a bound, or NaN) has no candidate, and det_size[d] is the box's class.
template <bool kSized>
__global__ __launch_bounds__(128) void box3d_iou_max_idx_kernel(vdetr_det_store st, int nboxes, int nscans, int ngt, int C,
                                                                const uint8_t* __restrict__ box_size,
                                                                const uint8_t* __restrict__ gt_size, double* __restrict__ ovmax,
                                                                int* __restrict__ jmax, int* __restrict__ det_cls,
                                                                float* __restrict__ det_score, uint8_t* __restrict__ det_size) {
  const int per = C > 0 ? C : 1;
  const long e = (long)blockIdx.x * 128 + threadIdx.x;
  if (e >= (long)nboxes * per) return;
  const int r = (int)(e / per), c = (int)(e % per);
  const int s = st.box_scan[r];
  if (s < 0 || s >= nscans) return;
  const int b0 = st.box_begin[s], ns = st.box_begin[s + 1] - b0, j = r - b0;
  if (j < 0 || j >= ns) return;
  const long d = C > 0 ? (long)C * b0 + (long)c * ns + j : r;
  if (d < 0 || d >= (long)nboxes * per) return;
  float c1[24];
  for (int k = 0; k < 24; ++k) c1[k] = st.box_corners[(size_t)r * 24 + k];
  const int cls = C > 0 ? c : st.box_cls[r];
  const double vol1 = box3d_vol64(c1);
  double best = -INFINITY;
  int arg = -1;
  const int size = kSized ? box_size[r] : 0;
  const int g0 = max(st.gt_begin[s], 0), g1 = kSized && size > 2 ? g0 : min(st.gt_begin[s + 1], ngt);
  for (int g = g0; g < g1; ++g) {
    if (st.gt_cls[g] != cls) continue;
    if (kSized && gt_size[g] != size) continue;
    float c2[24];
    for (int k = 0; k < 24; ++k) c2[k] = st.gt_corners[(size_t)g * 24 + k];
    const double area = footprint_intersection(c1, c2);
    const double ymax = fmin((double)c1[1], (double)c2[1]), ymin = fmax((double)c1[13], (double)c2[13]);
    const double inter_vol = area * fmax(0.0, ymax - ymin);
    const double iou = inter_vol / ((vol1 + box3d_vol64(c2)) - inter_vol);
    if (iou > best) best = iou, arg = g;
  }
  ovmax[d] = best;
  jmax[d] = arg;
  det_cls[d] = cls;
  det_score[d] = st.box_scores[(size_t)r * st.S + (C > 0 ? c : 0)];
  if (kSized) det_size[d] = (uint8_t)size;
}

// The volume class of the size split (utils/eval_det.py:62-67 box3d_vol_batch, :89-104): three axis differences of the float32
// corners, every operation a rounded float32 operation as numpy does them (the library is built with -ffp-contract=off), compared
// with the float32 bounds.  0 = S, 1 = M, 2 = L, 3 = none (a volume equal to a bound, or NaN).
__global__ __launch_bounds__(256) void box3d_size_class_kernel(const float* __restrict__ corners, int n, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* c = corners + (size_t)i * 24;
  const float dz = c[2] - c[5], dx = c[3] - c[6], dy = c[1] - c[13];
  // sqrtf is the correctly rounded square root here; HIP's __fsqrt_rn is the hardware approximation
  const float a = sqrtf(dz * dz), b = sqrtf(dx * dx), h = sqrtf(dy * dy);
  const float vol = (a * b) * h;
  const float lo = (float)0.17, hi = (float)0.44;
  out[i] = vol < lo ? 0 : (vol > lo && vol < hi) ? 1 : vol > hi ? 2 : 3;
}

// ---------------------------------------------------------------------------------------------------------------------
// The reference's box3d_iou for all pairs: out[a, b] = box3d_iou(corners_a[a], corners_b[b]) (box a is the subject of the
// clip, box b the clip polygon, as in box_util.py:139).  One thread per pair.
__global__ __launch_bounds__(128) void box3d_iou_pairs_kernel(const float* __restrict__ ca, const float* __restrict__ cb, int Na,
                                                              int Nb, double* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (e >= (size_t)Na * Nb) return;
  const float* c1 = ca + (e / Nb) * 24;
  const float* c2 = cb + (e % Nb) * 24;
  float a[24], b[24];
  for (int k = 0; k < 24; ++k) a[k] = c1[k], b[k] = c2[k];
  const double area = footprint_intersection(a, b);
  const double ymax = fmin((double)a[1], (double)b[1]), ymin = fmax((double)a[13], (double)b[13]);
  const double inter_vol = area * fmax(0.0, ymax - ymin);
  out[e] = inter_vol / ((box3d_vol64(a) + box3d_vol64(b)) - inter_vol);
}

// 2r. the rotated relation: the overlap of ranks r and s is the reference's box3d_iou(corners_r, corners_s)
//     instead of the IoU of the two hulls.  Grid (K/64, 4W, B): ONE wave owns 64 ranks r and a quarter word (16 partners s),
//     staged in LDS as float64 footprint, top / bottom height and volume.  The clip is ~40 doubles of polygon state with
//     dynamic indices (private memory) and a few hundred fp64 operations, so a lane first collects the partners that pass
//     the exact pre-tests (s > r, same class, heights overlap: otherwise inter is exactly 0 or NaN and never above a threshold
//     >= 0) as a bit mask and then clips only those: the wave runs as many clips as its busiest lane has candidates, not 16.
struct RotBox {
  P2 rect[4];
  double top, bottom, vol;
};
__global__ __launch_bounds__(64) void nms3d_rot_relation_kernel(NmsParams P) {
  __shared__ RotBox sbox[kNmsQuarter];
  __shared__ int scls[kNmsQuarter];
  const int b = blockIdx.z, piece = blockIdx.y, K = P.K, W = P.W;
  const int r = blockIdx.x * 64 + threadIdx.x, s0 = piece * kNmsQuarter;
  unsigned short* out = reinterpret_cast<unsigned short*>(P.rel + (size_t)b * K * W);
  if (s0 + kNmsQuarter - 1 <= (int)(blockIdx.x * 64) || s0 >= K) {  // every pair of this wave has s <= r
    if (r < K) out[(size_t)r * W * 4 + piece] = 0;
    return;
  }
  const float* __restrict__ rc = P.rcorn + (size_t)b * K * 24;
  const int* __restrict__ cls = P.rcls + (size_t)b * K;
  auto load = [&](int i, RotBox& o) {
    float c[24];
    for (int k = 0; k < 24; ++k) c[k] = rc[(size_t)i * 24 + k];
    footprint64(c, o.rect);
    o.top = (double)c[1];
    o.bottom = (double)c[13];
    o.vol = box3d_vol64(c);
  };
  if (threadIdx.x < kNmsQuarter) {
    const int s = s0 + threadIdx.x;
    load(min(s, K - 1), sbox[threadIdx.x]);
    scls[threadIdx.x] = s < K ? cls[s] : -1;  // a negative class (invalid box, see prepare) matches nothing
  }
  __syncthreads();
  if (r >= K) return;
  const int cr = cls[r];
  RotBox A;
  load(r, A);
  const bool always_divide = !(P.thr >= 0.0);
  unsigned cand = 0u, bits = 0u;
#pragma unroll
  for (int t = 0; t < kNmsQuarter; ++t) {
    const double h = fmax(0.0, fmin(A.top, sbox[t].top) - fmax(A.bottom, sbox[t].bottom));
    if (s0 + t > r && scls[t] == cr && cr >= 0 && (h > 0.0 || always_divide)) cand |= 1u << t;
  }
  while (cand) {
    const int t = __ffs(cand) - 1;
    cand &= cand - 1u;
    const RotBox& S = sbox[t];
    const double area = footprint_intersection(A.rect, S.rect);
    const double inter = area * fmax(0.0, fmin(A.top, S.top) - fmax(A.bottom, S.bottom));
    const double o = P.old_type ? inter / S.vol : inter / ((A.vol + S.vol) - inter);
    if (o > P.thr) bits |= 1u << t;
  }
  out[(size_t)r * W * 4 + piece] = (unsigned short)bits;
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

// the workspace, as the fields of the kernels' parameters that point into it: the relation bit matrix, the prepared boxes
// (extents, or the rotated form's corners) and their classes
static NmsParams lay_out(Carver& c, bool rotated, int B, int K) {
  const size_t rows = (size_t)B * K, W = (K + 63) / 64;
  NmsParams P{};
  P.rel = c.take<unsigned long long>(rows * W);
  (rotated ? P.rcorn : P.ext) = c.take<float>(rows * (rotated ? 24 : 6));
  P.rcls = c.take<int>(rows);
  return P;
}
static size_t nms3d_bytes(bool rotated, int B, int K) {
  if (B <= 0 || K <= 0) return 0;
  Carver c(nullptr);
  lay_out(c, rotated, B, K);
  return c.bytes() + 256;
}

extern "C" size_t vdetr_nms3d_workspace_bytes(int B, int K) { return nms3d_bytes(false, B, K); }
extern "C" size_t vdetr_nms3d_rot_workspace_bytes(int B, int K) { return nms3d_bytes(true, B, K); }

static int nms3d_launch(bool rotated, const float* corners, const float* score, const int32_t* cls, const uint8_t* valid,
                        const int64_t* order, int B, int K, double iou_threshold, int old_type, uint8_t* keep, void* workspace,
                        size_t workspace_bytes, vdetr_stream_t stream) {
  const char* op = rotated ? "nms3d_rot" : "nms3d";
  VDETR_REQUIRE(B >= 0 && K >= 0, "%s: negative dimension", op);
  if (B == 0 || K == 0) return VDETR_OK;
  VDETR_REQUIRE(corners && score && order && keep, "%s: null pointer", op);
  VDETR_REQUIRE(K <= 4096 && B <= 65535, "%s: %d scenes x %d boxes: limits are 65535 x 4096", op, B, K);
  if (int e = require_workspace(op, workspace, workspace_bytes, nms3d_bytes(rotated, B, K))) return e;
  Carver carver(workspace);
  NmsParams P = lay_out(carver, rotated, B, K);
  P.corners = corners; P.cls = cls; P.valid = valid; P.order = order; P.keep = keep;
  P.K = K; P.W = (K + 63) / 64; P.old_type = old_type; P.thr = iou_threshold;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nms3d_prepare_kernel, dim3(ceil_div(K, 256), B), dim3(256), 0, st, P);
  if (int e = check_launch("nms3d_prepare")) return e;
  if (rotated) {
    hipLaunchKernelGGL(nms3d_rot_relation_kernel, dim3(ceil_div(K, 64), P.W * 4, B), dim3(64), 0, st, P);
    if (int e = check_launch("nms3d_rot_relation")) return e;
  } else {
    hipLaunchKernelGGL(nms3d_relation_kernel, dim3(ceil_div(K, 256), P.W * 4, B), dim3(256), 0, st, P);
    if (int e = check_launch("nms3d_relation")) return e;
  }
  const size_t relb = (size_t)K * P.W * sizeof(unsigned long long);
  const int in_lds = relb <= 150 * 1024;
  const size_t lds = in_lds ? relb : 0;
  if (in_lds) {
    if (int rc = set_lds(nms3d_walk_kernel<true>, lds, "nms3d")) return rc;
    hipLaunchKernelGGL(nms3d_walk_kernel<true>, dim3(B), dim3(kNmsThreads), lds, st, P);
  } else {
    hipLaunchKernelGGL(nms3d_walk_kernel<false>, dim3(B), dim3(kNmsThreads), 0, st, P);
  }
  return check_launch("nms3d_walk");
}

extern "C" int vdetr_nms3d_f32(const float* corners, const float* score, const int32_t* cls, const uint8_t* valid,
                               const int64_t* order, int B, int K, double iou_threshold, int old_type, uint8_t* keep,
                               void* workspace, size_t workspace_bytes, vdetr_stream_t stream) {
  return nms3d_launch(false, corners, score, cls, valid, order, B, K, iou_threshold, old_type, keep, workspace, workspace_bytes,
                      stream);
}

extern "C" int vdetr_nms3d_rot_f32(const float* corners, const float* score, const int32_t* cls, const uint8_t* valid,
                                   const int64_t* order, int B, int K, double iou_threshold, int old_type, uint8_t* keep,
                                   void* workspace, size_t workspace_bytes, vdetr_stream_t stream) {
  return nms3d_launch(true, corners, score, cls, valid, order, B, K, iou_threshold, old_type, keep, workspace, workspace_bytes,
                      stream);
}

extern "C" int vdetr_box3d_iou_pairs_f64(const float* corners_a, int Na, const float* corners_b, int Nb, double* out,
                                         vdetr_stream_t stream) {
  VDETR_REQUIRE(Na >= 0 && Nb >= 0, "box3d_iou_pairs: negative count");
  if (Na == 0 || Nb == 0) return VDETR_OK;
  VDETR_REQUIRE(corners_a && corners_b && out, "box3d_iou_pairs: null pointer");
  VDETR_REQUIRE((size_t)Na * Nb <= ((size_t)1 << 30), "box3d_iou_pairs: %d x %d pairs > 2^30", Na, Nb);
  hipLaunchKernelGGL(box3d_iou_pairs_kernel, dim3((unsigned)(((size_t)Na * Nb + 127) / 128)), dim3(128), 0, (hipStream_t)stream,
                     corners_a, corners_b, Na, Nb, out);
  return check_launch("box3d_iou_pairs");
}

extern "C" int vdetr_box_point_count_f32(const float* points, const float* boxes, int B, int N, int K, int32_t* counts,
                                         vdetr_stream_t stream) {
  VDETR_REQUIRE(B >= 0 && N >= 0 && K >= 0, "box_point_count: negative dimension");
  if (B == 0 || N == 0 || K == 0) return VDETR_OK;
  VDETR_REQUIRE(points && boxes && counts, "box_point_count: null pointer");
  VDETR_REQUIRE(B <= 65535, "box_point_count: %d scenes > 65535", B);
  // enough point slices to fill the chip (~1024 workgroups = 4 per CU)
  const int kb = ceil_div(K, 256);
  int splits = 1024 / (kb * B > 0 ? kb * B : 1);
  splits = splits < 1 ? 1 : splits;
  int slice = ceil_div(ceil_div(N, splits), 64) * 64;
  hipLaunchKernelGGL(box_point_count_kernel, dim3(ceil_div(N, slice), kb, B), dim3(256), 0, (hipStream_t)stream, points, boxes, N, K,
                     slice, counts);
  return check_launch("box_point_count");
}

extern "C" int vdetr_box3d_iou_max_f64(const float* pred_corners, const int32_t* pred_img, const int32_t* pred_cls, int P,
                                       const float* gt_corners, const int32_t* gt_cls, const int32_t* img_gt_begin,
                                       double* ovmax, int32_t* jmax, vdetr_stream_t stream) {
  VDETR_REQUIRE(P >= 0, "box3d_iou_max: negative count");
  if (P == 0) return VDETR_OK;
  VDETR_REQUIRE(pred_corners && pred_img && pred_cls && img_gt_begin && ovmax && jmax, "box3d_iou_max: null pointer");
  hipLaunchKernelGGL(box3d_iou_max_kernel, dim3(ceil_div(P, 128)), dim3(128), 0, (hipStream_t)stream, pred_corners, pred_img, pred_cls,
                     P, gt_corners, gt_cls, img_gt_begin, ovmax, jmax);
  return check_launch("box3d_iou_max");
}

extern "C" int vdetr_box3d_iou_max_idx_f64(const vdetr_det_store* store, int nboxes, int nscans, int ngt, int num_classes,
                                           double* ovmax, int32_t* jmax, int32_t* det_cls, float* det_score,
                                           vdetr_stream_t stream) {
  VDETR_REQUIRE(store, "box3d_iou_max_idx: null store");
  const vdetr_det_store& s = *store;
  VDETR_REQUIRE(nboxes >= 0 && nscans >= 0 && ngt >= 0 && num_classes >= 0, "box3d_iou_max_idx: negative count");
  VDETR_REQUIRE(nboxes <= s.box_capacity && nscans <= s.scan_capacity && ngt <= s.gt_capacity,
                "box3d_iou_max_idx: %d boxes, %d scans, %d ground-truth boxes exceed the store's %d, %d, %d", nboxes, nscans, ngt,
                s.box_capacity, s.scan_capacity, s.gt_capacity);
  VDETR_REQUIRE(s.S >= (num_classes > 0 ? num_classes : 1), "box3d_iou_max_idx: %d scores per box < %d classes", s.S, num_classes);
  const long P = (long)nboxes * (num_classes > 0 ? num_classes : 1);
  VDETR_REQUIRE(P < ((long)1 << 31), "box3d_iou_max_idx: %ld detections >= 2^31", P);
  if (P == 0) return VDETR_OK;
  VDETR_REQUIRE(s.box_corners && s.box_scores && s.box_cls && s.box_scan && s.box_begin && s.gt_begin && ovmax && jmax &&
                    det_cls && det_score && (ngt == 0 || (s.gt_corners && s.gt_cls)),
                "box3d_iou_max_idx: null pointer");
  hipLaunchKernelGGL(box3d_iou_max_idx_kernel<false>, dim3(ceil_div(P, 128)), dim3(128), 0, (hipStream_t)stream, s, nboxes, nscans,
                     ngt, num_classes, nullptr, nullptr, ovmax, jmax, det_cls, det_score, nullptr);
  return check_launch("box3d_iou_max_idx");
}

extern "C" int vdetr_box3d_iou_max_size_f64(const vdetr_det_store* store, int nboxes, int nscans, int ngt, int num_classes,
                                            const uint8_t* box_size, const uint8_t* gt_size, double* ovmax, int32_t* jmax,
                                            int32_t* det_cls, float* det_score, uint8_t* det_size, vdetr_stream_t stream) {
  VDETR_REQUIRE(store, "box3d_iou_max_size: null store");
  const vdetr_det_store& s = *store;
  VDETR_REQUIRE(nboxes >= 0 && nscans >= 0 && ngt >= 0 && num_classes >= 0, "box3d_iou_max_size: negative count");
  VDETR_REQUIRE(nboxes <= s.box_capacity && nscans <= s.scan_capacity && ngt <= s.gt_capacity,
                "box3d_iou_max_size: %d boxes, %d scans, %d ground-truth boxes exceed the store's %d, %d, %d", nboxes, nscans, ngt,
                s.box_capacity, s.scan_capacity, s.gt_capacity);
  VDETR_REQUIRE(s.S >= (num_classes > 0 ? num_classes : 1), "box3d_iou_max_size: %d scores per box < %d classes", s.S, num_classes);
  const long P = (long)nboxes * (num_classes > 0 ? num_classes : 1);
  VDETR_REQUIRE(P < ((long)1 << 31), "box3d_iou_max_size: %ld detections >= 2^31", P);
  if (P == 0) return VDETR_OK;
  VDETR_REQUIRE(s.box_corners && s.box_scores && s.box_cls && s.box_scan && s.box_begin && s.gt_begin && box_size && ovmax && jmax &&
                    det_cls && det_score && det_size && (ngt == 0 || (s.gt_corners && s.gt_cls && gt_size)),
                "box3d_iou_max_size: null pointer");
  hipLaunchKernelGGL(box3d_iou_max_idx_kernel<true>, dim3(ceil_div(P, 128)), dim3(128), 0, (hipStream_t)stream, s, nboxes, nscans,
                     ngt, num_classes, box_size, gt_size, ovmax, jmax, det_cls, det_score, det_size);
  return check_launch("box3d_iou_max_size");
}

extern "C" int vdetr_box3d_size_class_f32(const float* corners, int n, uint8_t* out, vdetr_stream_t stream) {
  VDETR_REQUIRE(n >= 0, "box3d_size_class: negative count");
  if (n == 0) return VDETR_OK;
  VDETR_REQUIRE(corners && out, "box3d_size_class: null pointer");
  hipLaunchKernelGGL(box3d_size_class_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, corners, n, out);
  return check_launch("box3d_size_class");
}
