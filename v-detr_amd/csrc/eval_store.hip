// eval_store.hip — the evaluation loop's detections kept on the device (reference utils/ap_calculator.py:430-470
// APCalculator.step and utils/eval_det.py:23-56, 127-141).
//
// The reference (and the host path of v-detr_amd/ap_calculator.py) copies every batch's predictions to the host and keeps
// the kept boxes as per-scan lists.  Here the kept boxes and the present ground-truth boxes of a batch are appended to a
// store whose arrays AND cursors are device memory (vdetr_det_store), so that a step of the evaluation loop reads nothing
// back; the matching over the store is vdetr_box3d_iou_max_idx_f64 (nms.hip, next to the clip routine) and the curves and
// the average precision of every class and threshold are ONE launch here (vdetr_voc_ap_f64).  The size split of --test_size
//  reuses that launch over 3C (size, class) segments; its volume classes and its matching are in nms.hip too.
//
// Append = two launches.  `rows`: grid (tiles of 256 boxes + tiles of 256 ground-truth boxes, B); a workgroup counts the
// flags in front of its tile (all earlier scenes and the earlier tiles of its own: at most B*K bytes), adds the cursor it
// reads from the store and compacts its tile with a ballot, so the rows land in (scene, ascending index) order whatever
// order the workgroups run in.  `cursors`: one workgroup recounts every scene and writes box_begin / gt_begin, the cursors
// and the dropped-row count.  Counting is integer arithmetic and every row has exactly one writer: two runs, same bits.
#include "block_scan.h"

namespace vdetr {
namespace {

constexpr int kTile = 256;

typedef int WaveRow[kTile / kWave];

// number of non-zero flags in f[0 .. n), the same value in every thread of the workgroup
__device__ int flag_count(const uint8_t* __restrict__ f, long n, WaveRow& sh) {
  return block_sum<kTile>(n, [&](long i) { return (int)(f[i] != 0); }, sh);
}

// Rows i of tile `tile` of scene b with flag[b,i] != 0 -> positions base + (number of flags in front), in ascending order.
// Returns the row's position or -1 (not flagged, or outside [0, capacity): the store's cursor is device data).
__device__ long tile_position(const uint8_t* __restrict__ flag, int b, int n, int tile, long base, int capacity, WaveRow& sh) {
  const long front = flag_count(flag, (long)b * n + (long)tile * kTile, sh);
  const int i = tile * kTile + threadIdx.x;
  const bool on = i < n && flag[(size_t)b * n + i] != 0;
  int in_tile;
  const long pos = base + front + block_rank<kTile>(on, sh, in_tile);
  return on && pos >= 0 && pos < capacity ? pos : -1;
}

__global__ __launch_bounds__(kTile) void det_append_rows_kernel(vdetr_det_store st, const uint8_t* __restrict__ keep,
                                                                const float* __restrict__ corners, const float* __restrict__ scores,
                                                                const int32_t* __restrict__ cls, const float* __restrict__ gt_corners,
                                                                const int32_t* __restrict__ gt_cls, const uint8_t* __restrict__ present,
                                                                int K, int G, int box_tiles, int scan_base) {
  __shared__ WaveRow sh;
  const int b = blockIdx.y;
  if ((int)blockIdx.x < box_tiles) {
    const long pos = tile_position(keep, b, K, blockIdx.x, st.counters[0], st.box_capacity, sh);
    if (pos < 0) return;
    const size_t src = (size_t)b * K + blockIdx.x * kTile + threadIdx.x;
    for (int k = 0; k < 24; ++k) st.box_corners[pos * 24 + k] = corners[src * 24 + k];
    for (int k = 0; k < st.S; ++k) st.box_scores[pos * st.S + k] = scores[src * st.S + k];
    st.box_cls[pos] = cls[src];
    st.box_scan[pos] = scan_base + b;
  } else {
    const int tile = blockIdx.x - box_tiles;
    const long pos = tile_position(present, b, G, tile, st.counters[1], st.gt_capacity, sh);
    if (pos < 0) return;
    const size_t src = (size_t)b * G + tile * kTile + threadIdx.x;
    for (int k = 0; k < 24; ++k) st.gt_corners[pos * 24 + k] = gt_corners[src * 24 + k];
    st.gt_cls[pos] = gt_cls[src];
  }
}

// rows of [start, end) that lie at or beyond the capacity
__device__ __forceinline__ long beyond(long start, long end, long capacity) {
  const long from = start > capacity ? start : capacity;
  return end > from ? end - from : 0;
}

__global__ __launch_bounds__(kTile) void det_append_cursors_kernel(vdetr_det_store st, const uint8_t* __restrict__ keep,
                                                                   const uint8_t* __restrict__ present, int B, int K, int G,
                                                                   int scan_base) {
  __shared__ WaveRow sh;
  const long box0 = st.counters[0], gt0 = st.counters[1];
  long box = box0, gt = gt0;
  for (int b = 0; b < B; ++b) {  // (scan_base + B <= scan_capacity: checked on the host, both are host values)
    if (threadIdx.x == 0) st.box_begin[scan_base + b] = (int)box, st.gt_begin[scan_base + b] = (int)gt;
    box += flag_count(keep + (size_t)b * K, K, sh);
    if (G > 0) gt += flag_count(present + (size_t)b * G, G, sh);
  }
  if (threadIdx.x == 0) {
    st.box_begin[scan_base + B] = (int)box;
    st.gt_begin[scan_base + B] = (int)gt;
    st.counters[0] = (int)box;
    st.counters[1] = (int)gt;
    st.counters[2] = scan_base + B;
    st.counters[3] += (int)(beyond(box0, box, st.box_capacity) + beyond(gt0, gt, st.gt_capacity));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Curves and VOC-12 AP: grid (C, T), one workgroup per (class, threshold) walks the class's segment of the ranked tp flags
// BACKWARDS in chunks of 2048 ranks (8 consecutive ranks per thread; thread 0 owns the last ones), because both things the
// sum needs run from the end: the precision envelope is a suffix maximum, and with the segment's total known the inclusive
// true-positive count of a rank is total - (true positives behind it).  Per chunk: a workgroup scan of the threads' counts,
// the 8 precisions, a workgroup scan-max of the threads' maxima, then the terms.  A rank adds a term only where the recall
// changes (voc_ap: mrec[i+1] != mrec[i]), i.e. at a true positive of a class with ground truth; the appended (1, 0) point
// adds (1 - rec) * 0.
constexpr int kApItems = 8, kApChunk = kTile * kApItems;

__global__ __launch_bounds__(kTile) void voc_ap_kernel(const uint8_t* __restrict__ tp, const int* __restrict__ seg,
                                                       const int* __restrict__ npos, int P, int C, double* __restrict__ out,
                                                       double* __restrict__ rec, double* __restrict__ prec) {
  __shared__ WaveRow row_i;
  __shared__ double row_d[kTile / kWave];
  __shared__ double s_acc[kTile];  // the final sum of acc
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  int lo = seg[c], hi = seg[c + 1];  // device data: clamped to the flags that exist
  lo = lo < 0 ? 0 : (lo > P ? P : lo);
  hi = hi < lo ? lo : (hi > P ? P : hi);
  const int n = hi - lo, np = npos[c];
  const double dnp = (double)np;
  const uint8_t* __restrict__ f = tp + (size_t)t * P + lo;
  double* r_out = rec ? rec + (size_t)t * P + lo : nullptr;
  double* p_out = prec ? prec + (size_t)t * P + lo : nullptr;
  auto vmax = [](double a, double b) { return fmax(a, b); };

  const int total = flag_count(f, n, row_i);

  int behind = 0;      // true positives behind the chunk
  double env = 0.0;    // envelope behind the chunk; voc_ap's mpre ends in 0
  double acc = 0.0;
  for (int top = n; top > 0; top -= kApChunk) {
    const int first = top - 1 - tid * kApItems;  // this thread's ranks: first, first - 1, ..
    bool fl[kApItems];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kApItems; ++k) {
      fl[k] = first - k >= 0 && f[first - k] != 0;
      cnt += fl[k];
    }
    int chunk_cnt;
    int later = behind + block_exclusive_sum<kTile>(cnt, row_i, chunk_cnt);
    int tpc[kApItems];
    double pr[kApItems], mx = 0.0;
#pragma unroll
    for (int k = 0; k < kApItems; ++k) {
      tpc[k] = total - later;  // inclusive count at rank first - k
      later += fl[k];
      pr[k] = first - k >= 0 ? (double)tpc[k] / (double)(first - k + 1) : 0.0;  // tp + fp = rank + 1 >= 1 > eps
      mx = fmax(mx, pr[k]);
    }
    double chunk_max;
    double e = fmax(env, block_exclusive_scan<kTile>(mx, 0.0, vmax, row_d, chunk_max));
#pragma unroll
    for (int k = 0; k < kApItems; ++k) {
      if (first - k < 0) continue;
      e = fmax(e, pr[k]);
      const double rk = np > 0 ? (double)tpc[k] / dnp : 0.0;
      if (r_out) r_out[first - k] = rk, p_out[first - k] = pr[k];
      if (fl[k] && np > 0) acc += (rk - (double)(tpc[k] - 1) / dnp) * e;
    }
    behind += chunk_cnt;
    env = fmax(env, chunk_max);
  }
  __syncthreads();
  s_acc[tid] = acc;
  __syncthreads();
  for (int o = kTile / 2; o > 0; o >>= 1) {
    if (tid < o) s_acc[tid] = s_acc[tid] + s_acc[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double* o = out + (size_t)t * 4 * C;
    o[c] = n > 0 ? s_acc[0] : 0.0;
    o[C + c] = n > 0 && np > 0 ? (double)total / dnp : 0.0;
    o[2 * C + c] = (double)n;
    o[3 * C + c] = dnp;
  }
}

}  // namespace
}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_det_append_f32(const vdetr_det_store* store, const uint8_t* keep, const float* corners, const float* scores,
                                    const int32_t* cls, const float* gt_corners, const int32_t* gt_cls, const uint8_t* gt_present,
                                    int B, int K, int G, int scan_base, vdetr_stream_t stream) {
  VDETR_REQUIRE(store, "det_append: null store");
  const vdetr_det_store& s = *store;
  VDETR_REQUIRE(B >= 0 && K >= 0 && G >= 0 && scan_base >= 0, "det_append: negative dimension");
  VDETR_REQUIRE(s.box_capacity >= 0 && s.gt_capacity >= 0 && s.scan_capacity >= 0 && s.S >= 1, "det_append: bad store sizes");
  if (B == 0) return VDETR_OK;
  VDETR_REQUIRE(B <= 65535, "det_append: %d scenes > 65535", B);
  VDETR_REQUIRE((long)scan_base + B <= s.scan_capacity, "det_append: scans %d + %d exceed the store's %d", scan_base, B,
                s.scan_capacity);
  VDETR_REQUIRE((long)B * K < ((long)1 << 31) && (long)B * G < ((long)1 << 31), "det_append: batch of >= 2^31 rows");
  VDETR_REQUIRE(s.box_begin && s.gt_begin && s.counters, "det_append: null pointer");
  VDETR_REQUIRE(K == 0 || (keep && corners && scores && cls && s.box_corners && s.box_scores && s.box_cls && s.box_scan),
                "det_append: null pointer");
  VDETR_REQUIRE(G == 0 || (gt_corners && gt_cls && gt_present && s.gt_corners && s.gt_cls), "det_append: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int box_tiles = ceil_div(K, kTile), gt_tiles = ceil_div(G, kTile);
  if (box_tiles + gt_tiles > 0) {
    hipLaunchKernelGGL(det_append_rows_kernel, dim3(box_tiles + gt_tiles, B), dim3(kTile), 0, st, s, keep, corners, scores, cls,
                       gt_corners, gt_cls, gt_present, K, G, box_tiles, scan_base);
    if (int e = check_launch("det_append_rows")) return e;
  }
  hipLaunchKernelGGL(det_append_cursors_kernel, dim3(1), dim3(kTile), 0, st, s, keep, gt_present, B, K, G, scan_base);
  return check_launch("det_append_cursors");
}

extern "C" int vdetr_voc_ap_f64(const uint8_t* tp, const int32_t* seg, const int32_t* npos, int T, int P, int C, double* out,
                                double* rec, double* prec, vdetr_stream_t stream) {
  VDETR_REQUIRE(T >= 0 && P >= 0 && C >= 0, "voc_ap: negative dimension");
  if (T == 0 || C == 0) return VDETR_OK;
  VDETR_REQUIRE(T <= 65535, "voc_ap: %d thresholds > 65535", T);
  VDETR_REQUIRE(seg && npos && out && (P == 0 || tp), "voc_ap: null pointer");
  VDETR_REQUIRE((rec == nullptr) == (prec == nullptr), "voc_ap: rec and prec come together");
  hipLaunchKernelGGL(voc_ap_kernel, dim3(C, T), dim3(kTile), 0, (hipStream_t)stream, tp, seg, npos, P, C, out, rec, prec);
  return check_launch("voc_ap");
}
