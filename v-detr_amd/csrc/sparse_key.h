// sparse_key.h — the key of a sparse site and the search of a sorted key vector, said once.
//
//   key = batch << 48 | (x + 32768) << 32 | (y + 32768) << 16 | (z + 32768)        batch in 0 .. 32767, x, y, z in -32768 .. 32767
//
// A legal key is non-negative, and ascending key order is lexicographic (batch, x, y, z) order: a sparse tensor keeps its keys
// sorted, so a neighbour look-up is a lower bound and scene b begins at the lower bound of key_scene_floor(b).  -1 is the one
// invalid key: what no key can hold packs to it, a move that takes a field out of its range gives it, and it sorts first.
// Plain functions, host and device, no HIP header: tests/sparse_key_check.cpp holds them to restatements without a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SK_HD __host__ __device__ __forceinline__
#else
#define SK_HD inline
#endif

namespace vdetr {

constexpr int kKeyBias = 32768;       // added to a coordinate: the field holds 0 .. 65535
constexpr int kKeyFieldEnd = 65536;   // one past the largest biased coordinate
constexpr int kKeyBatchEnd = 32768;   // one past the largest batch index: the key stays non-negative
constexpr int kKeyBatchShift = 48, kKeyXShift = 32, kKeyYShift = 16;

SK_HD bool key_in_field(int c) { return (unsigned)c + (unsigned)kKeyBias < (unsigned)kKeyFieldEnd; }
// the key of fields that are known to be in range (no test: the caller made it)
SK_HD int64_t key_pack_fields(int b, int x, int y, int z) {
  return ((int64_t)b << kKeyBatchShift) | ((int64_t)(x + kKeyBias) << kKeyXShift) | ((int64_t)(y + kKeyBias) << kKeyYShift) | (int64_t)(z + kKeyBias);
}
// ... or -1 where the batch index or a coordinate is outside its field
SK_HD int64_t key_pack(int b, int x, int y, int z) {
  const bool ok = (unsigned)b < (unsigned)kKeyBatchEnd && key_in_field(x) && key_in_field(y) && key_in_field(z);
  return ok ? key_pack_fields(b, x, y, z) : (int64_t)-1;
}

SK_HD int64_t key_field(int64_t key, int shift) { return (key >> shift) & (int64_t)(kKeyFieldEnd - 1); }  // biased: 0 .. 65535
SK_HD int key_batch(int64_t key) { return (int)(key >> kKeyBatchShift); }
SK_HD int key_x(int64_t key) { return (int)key_field(key, kKeyXShift) - kKeyBias; }
SK_HD int key_y(int64_t key) { return (int)key_field(key, kKeyYShift) - kKeyBias; }
SK_HD int key_z(int64_t key) { return (int)key_field(key, 0) - kKeyBias; }
SK_HD int64_t key_scene_floor(int b) { return (int64_t)b << kKeyBatchShift; }  // the smallest key of scene b

// The key of the site at (x + dx, y + dy, z + dz) of the same scene; -1 where a coordinate leaves its field or `key` is negative.
// Each field is moved in 64 bits (an offset is any int32) and tested on its own: nothing carries into the field beside it.
SK_HD int64_t key_shift(int64_t key, int dx, int dy, int dz) {
  const int64_t x = key_field(key, kKeyXShift) + dx, y = key_field(key, kKeyYShift) + dy, z = key_field(key, 0) + dz;
  const bool ok = key >= 0 && x >= 0 && x < kKeyFieldEnd && y >= 0 && y < kKeyFieldEnd && z >= 0 && z < kKeyFieldEnd;
  return ok ? (((key >> kKeyBatchShift) << kKeyBatchShift) | (x << kKeyXShift) | (y << kKeyYShift) | z) : (int64_t)-1;
}

// the midpoint of lo <= hi <= INT_MAX (the signed sum would overflow)
SK_HD int key_mid(int lo, int hi) { return (int)(((unsigned)lo + (unsigned)hi) >> 1); }
// the first index of the ascending keys[0 .. n) whose element is >= key, n where none is (int64 keys; int32 site rows as well)
template <class T>
SK_HD int key_lower_bound(const T* keys, int n, T key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = key_mid(lo, hi);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the row of `key`, or -1 where the keys do not hold it
template <class T>
SK_HD int key_find(const T* keys, int n, T key) {
  const int lo = key_lower_bound(keys, n, key);
  return (lo < n && keys[lo] == key) ? lo : -1;
}

}  // namespace vdetr
