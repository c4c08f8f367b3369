// rot_iou.h — rotated 3-D IoU / DIoU of one (prediction, ground truth) box pair, and its gradient with respect to the
// prediction (reference criterion.py:25-64, diff_diou_rotated_3d, and mmcv-full 1.6.1 diff_iou_rotated_3d /
// box2corners / oriented_box_intersection_2d, restated from their published semantics: tests/rot_iou_restatement.py).
//
// A box is (x, y, z, w, h, l, alpha); its footprint is the rectangle (+-w/2, +-h/2) turned by alpha about (x, y), corners
// in box2corners order (+,+), (-,+), (-,-), (+,-) (counter-clockwise).
//   I2    = exact area of the footprints' intersection
//   zo    = clamp(min(z1 + l1/2, z2 + l2/2) - max(z1 - l1/2, z2 - l2/2), min=0)
//   iou   = I2 zo / (w1 h1 l1 + w2 h2 l2 - I2 zo)                      (no epsilon, as in mmcv)
//   diou  = iou - r2 / c2,  r2 = (x1-x2)^2 + (y1-y2)^2 + (w1-w2)^2     (the reference's box1[..., :3] of (x, y, w, h, alpha))
//                           c2 = squared diagonal of the enclosing box: x / y extents over both boxes' rotated corners
//
// One routine serves both uses through its scalar type S: `float` (matcher cost, value only) or Dual<7> (set loss:
// forward-mode tangents with respect to the prediction's 7 parameters).  Gradient tie rules follow torch: the extent over
// the 4 corners is torch.max / min(dim), the first extreme corner takes the gradient; the elementwise max / min of the two
// boxes' extents splits it evenly on a tie; clamp(min=0) passes it at 0.
//
// Intersection area.  Everything runs relative to the ground truth's centre (scene coordinates reach ~10 m and an
// absolute shoelace sum cancels badly there) and, for the area, in the ground truth's own frame, where its footprint is
// the axis-aligned [-a, a] x [-b, b].  Green's theorem on the boundary of R = A ∩ box (A = prediction footprint):
//   area = -∮ y dx = sum over A's edges of -∫ y dx along the part inside the box   (Liang-Barsky clip of the edge)
//                  + b * |{x in [-a, a] : (x, +b) in A}| + b * |{x in [-a, a] : (x, -b) in A}|
// (the box's vertical edges contribute nothing to ∮ y dx).  Both kinds of pieces meet where an edge of A crosses y = +-b,
// and both take that crossing from the same quotient (b - Py) / Dy, so they agree to rounding however the edge is
// inclined: no clip list, no data-dependent indexing, a fixed sequence of selects.  Collinear edges (exactly horizontal A
// edge on y = +-b, e.g. identical or touching axis-aligned boxes) are counted once when the two regions lie on the same
// side and cancel when they lie on opposite sides.
#pragma once
#include "common.h"

namespace vdetr {

template <int N>
struct Dual {
  float v;
  float t[N];
};

__device__ __forceinline__ float val(float a) { return a; }
template <int N>
__device__ __forceinline__ float val(const Dual<N>& a) {
  return a.v;
}

__device__ __forceinline__ void set_const(float& r, float v) { r = v; }
template <int N>
__device__ __forceinline__ void set_const(Dual<N>& r, float v) {
  r.v = v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = 0.f;
}
template <typename S>
__device__ __forceinline__ S cst(float v) {
  S r;
  set_const(r, v);
  return r;
}

__device__ __forceinline__ void rot_sincos(float a, float& s, float& c) { sincosf(a, &s, &c); }
template <int N>
__device__ __forceinline__ void rot_sincos(const Dual<N>& a, Dual<N>& s, Dual<N>& c) {
  float sv, cv;
  sincosf(a.v, &sv, &cv);
  s.v = sv, c.v = cv;
#pragma unroll
  for (int i = 0; i < N; ++i) s.t[i] = cv * a.t[i], c.t[i] = -sv * a.t[i];
}

template <int N>
__device__ __forceinline__ Dual<N> operator+(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = a.t[i] + b.t[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = a.t[i] - b.t[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& a) {
  Dual<N> r;
  r.v = -a.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = -a.t[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = a.t[i] * b.v + a.v * b.t[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator/(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v / b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = (a.t[i] - r.v * b.t[i]) / b.v;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator+(const Dual<N>& a, float b) {
  Dual<N> r = a;
  r.v = a.v + b;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator+(float a, const Dual<N>& b) {
  return b + a;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& a, float b) {
  Dual<N> r = a;
  r.v = a.v - b;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(float a, const Dual<N>& b) {
  return -(b - a);
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& a, float b) {
  Dual<N> r;
  r.v = a.v * b;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = a.t[i] * b;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(float a, const Dual<N>& b) {
  return b * a;
}
template <int N>
__device__ __forceinline__ Dual<N> operator/(const Dual<N>& a, float b) {
  Dual<N> r;
  r.v = a.v / b;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = a.t[i] / b;
  return r;
}

// torch.maximum / minimum(a, b): the larger (smaller) one; on a tie the value with the mean of the two tangents
__device__ __forceinline__ float tie_mean(float a, float) { return a; }
template <int N>
__device__ __forceinline__ Dual<N> tie_mean(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.t[i] = 0.5f * (a.t[i] + b.t[i]);
  return r;
}
template <typename S>
__device__ __forceinline__ S max2(const S& a, const S& b) {
  return val(a) > val(b) ? a : (val(a) < val(b) ? b : tie_mean(a, b));
}
template <typename S>
__device__ __forceinline__ S min2(const S& a, const S& b) {
  return val(a) < val(b) ? a : (val(a) > val(b) ? b : tie_mean(a, b));
}

// Clip the edge P + t D (t in [0, 1]) against `p t <= q`; p == 0: the whole edge is in (q >= 0) or out.
template <typename S>
__device__ __forceinline__ void clip_t(const S& p, const S& q, S& t0, S& t1, bool& empty) {
  if (val(p) == 0.f) {
    if (val(q) < 0.f) empty = true;
  } else {
    const S r = q / p;
    if (val(p) > 0.f) {
      if (val(r) < val(t1)) t1 = r;
    } else {
      if (val(r) > val(t0)) t0 = r;
    }
  }
}

// prediction p = (x, y, z, w, h, l, alpha) with (sp, cp) = sincos(alpha); ground truth g (plain floats) with (sg, cg).
// diou: subtract the enclosing-box term.
template <typename S>
__device__ __forceinline__ S rot_iou_pair(const S* p, const S& sp, const S& cp, const float* g, float sg, float cg, bool diou) {
  const S dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
  const S hw = p[3] * 0.5f, hh = p[4] * 0.5f;
  const float a = g[3] * 0.5f, b = g[4] * 0.5f;
  // ---- footprint intersection, in the ground truth's frame: relative angle by the difference formulas (exactly 0 for
  // equal angles, so equal orientations give exactly parallel edges)
  const S c1 = cp * cg + sp * sg, s1 = sp * cg - cp * sg;
  const S ox = dx * cg + dy * sg, oy = dy * cg - dx * sg;
  S X[4], Y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const S lx = (k == 0 || k == 3) ? hw : -hw, ly = k < 2 ? hh : -hh;
    X[k] = ox + (lx * c1 - ly * s1);
    Y[k] = oy + (lx * s1 + ly * c1);
  }
  S area = cst<S>(0.f);
  S lo_t = cst<S>(-a), hi_t = cst<S>(a), lo_b = cst<S>(-a), hi_b = cst<S>(a);
  bool none_t = false, none_b = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int k1 = (k + 1) & 3;
    const S Dx = X[k1] - X[k], Dy = Y[k1] - Y[k];
    // this edge's part inside the box: -∫ y dx = -(t1 - t0) Dx (Py + (t0 + t1) Dy / 2)
    S t0 = cst<S>(0.f), t1 = cst<S>(1.f);
    bool empty = false;
    clip_t(Dx, a - X[k], t0, t1, empty);
    clip_t(-Dx, a + X[k], t0, t1, empty);
    clip_t(Dy, b - Y[k], t0, t1, empty);
    clip_t(-Dy, b + Y[k], t0, t1, empty);
    if (!empty && val(t1) > val(t0)) area = area - ((t1 - t0) * Dx) * (Y[k] + ((t0 + t1) * 0.5f) * Dy);
    // where the lines y = +b (top, run in -x) and y = -b (bottom, run in +x) are on this edge's inner side
    if (val(Dy) == 0.f) {
      // parallel: (Y - Py) Dx >= 0 is inside; an edge lying on the line counts once (same direction) or cancels
      const float ft = (b - val(Y[k])) * val(Dx), fb = (-b - val(Y[k])) * val(Dx);
      if (val(Dx) < 0.f ? !(ft > 0.f) : ft < 0.f) none_t = true;
      if (val(Dx) > 0.f ? !(fb > 0.f) : fb < 0.f) none_b = true;
    } else {
      // the same quotient as clip_t's for y <= b / y >= -b: ((b - Py) / Dy and (b + Py) / -Dy == (-b - Py) / Dy)
      const S xt = X[k] + Dx * ((b - Y[k]) / Dy);
      const S xb = X[k] + Dx * ((b + Y[k]) / -Dy);
      if (val(Dy) > 0.f) {
        if (val(xt) < val(hi_t)) hi_t = xt;
        if (val(xb) < val(hi_b)) hi_b = xb;
      } else {
        if (val(xt) > val(lo_t)) lo_t = xt;
        if (val(xb) > val(lo_b)) lo_b = xb;
      }
    }
  }
  if (!none_t && val(hi_t) > val(lo_t)) area = area + (hi_t - lo_t) * b;
  if (!none_b && val(hi_b) > val(lo_b)) area = area + (hi_b - lo_b) * b;
  // ---- height overlap, volumes
  const S zmax1 = dz + p[5] * 0.5f, zmin1 = dz - p[5] * 0.5f;
  const float zmax2 = g[5] * 0.5f, zmin2 = -(g[5] * 0.5f);
  const S zr = min2(zmax1, cst<S>(zmax2)) - max2(zmin1, cst<S>(zmin2));
  const S zo = val(zr) >= 0.f ? zr : cst<S>(0.f);
  const S inter = area * zo;
  const S vol1 = (p[3] * p[4]) * p[5];
  const float vol2 = (g[3] * g[4]) * g[5];
  const S uni = (vol1 + vol2) - inter;
  S iou = inter / uni;
  if (!diou) return iou;
  // ---- enclosing box: the corners in the scene's axes (relative to the ground truth's centre)
  S x1max, x1min, y1max, y1min;
  float x2max = 0.f, x2min = 0.f, y2max = 0.f, y2min = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const S lx = (k == 0 || k == 3) ? hw : -hw, ly = k < 2 ? hh : -hh;
    const S xs = dx + (lx * cp - ly * sp), ys = dy + (lx * sp + ly * cp);
    const float gx = (k == 0 || k == 3) ? a : -a, gy = k < 2 ? b : -b;
    const float xg = gx * cg - gy * sg, yg = gx * sg + gy * cg;
    if (k == 0) {
      x1max = x1min = xs, y1max = y1min = ys;
      x2max = x2min = xg, y2max = y2min = yg;
    } else {  // strict comparisons: the first extreme corner wins (torch.max / min over dim)
      if (val(xs) > val(x1max)) x1max = xs;
      if (val(xs) < val(x1min)) x1min = xs;
      if (val(ys) > val(y1max)) y1max = ys;
      if (val(ys) < val(y1min)) y1min = ys;
      x2max = fmaxf(x2max, xg), x2min = fminf(x2min, xg), y2max = fmaxf(y2max, yg), y2min = fminf(y2min, yg);
    }
  }
  const S ex = min2(x1min, cst<S>(x2min)) - max2(x1max, cst<S>(x2max));
  const S ey = min2(y1min, cst<S>(y2min)) - max2(y1max, cst<S>(y2max));
  const S ez = min2(zmin1, cst<S>(zmin2)) - max2(zmax1, cst<S>(zmax2));
  const S c2 = (ex * ex + ey * ey) + ez * ez;
  const S dw = p[3] - g[3];
  const S r2 = (dx * dx + dy * dy) + dw * dw;
  return iou - r2 / c2;
}

}  // namespace vdetr
