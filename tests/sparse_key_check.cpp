// sparse_key_check.cpp — csrc/sparse_key.h on the host (tests/test_sparse_key.py builds and runs this): the key codec, the field
// move and the sorted-key search against restatements written out here (products and quotients of powers of two in int64,
// std::lower_bound), at the edges of every field and with offsets up to INT_MAX / INT_MIN.  Exit status 1 and a line on stderr at
// the first disagreement.  On success it prints the keys of a fixed coordinate list, which the Python side compares with its own.
//   sparse_key_check [random pairs]
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <tuple>
#include <vector>

#include "sparse_key.h"

using namespace vdetr;

static long g_checks = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    ++g_checks;                                                \
    if (!(cond)) {                                             \
      std::fprintf(stderr, "sparse key check failed: ");       \
      std::fprintf(stderr, __VA_ARGS__);                       \
      std::fprintf(stderr, "  [%s:%d]\n", __FILE__, __LINE__); \
      std::exit(1);                                            \
    }                                                          \
  } while (0)

// ---- the model: the layout as sums of products, every field in int64 -----------------------------------------------------------
static const int64_t kTwo16 = 65536, kTwo32 = kTwo16 * kTwo16, kTwo48 = kTwo32 * kTwo16;
static bool m_coord_ok(int64_t c) { return c >= -32768 && c <= 32767; }
static int64_t m_pack(int64_t b, int64_t x, int64_t y, int64_t z) {
  if (b < 0 || b > 32767 || !m_coord_ok(x) || !m_coord_ok(y) || !m_coord_ok(z)) return -1;
  return b * kTwo48 + (x + 32768) * kTwo32 + (y + 32768) * kTwo16 + (z + 32768);
}
struct Site { int64_t b, x, y, z; };
static Site m_unpack(int64_t key) {  // of a non-negative key
  return {key / kTwo48, key / kTwo32 % kTwo16 - 32768, key / kTwo16 % kTwo16 - 32768, key % kTwo16 - 32768};
}
static int64_t m_shift(int64_t key, int64_t dx, int64_t dy, int64_t dz) {
  if (key < 0) return -1;
  const Site s = m_unpack(key);
  return m_pack(s.b, s.x + dx, s.y + dy, s.z + dz);
}

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static const int kEdge[7] = {-32768, -32767, -1, 0, 1, 32766, 32767};
static const int kBatch[3] = {0, 1, 32767};

static void pack_and_fields() {
  for (int b : kBatch)
    for (int x : kEdge)
      for (int y : kEdge)
        for (int z : kEdge) {
          const int64_t key = key_pack(b, x, y, z);
          CHECK(key >= 0 && key == m_pack(b, x, y, z), "pack(%d, %d, %d, %d) = %lld", b, x, y, z, (long long)key);
          CHECK(key == key_pack_fields(b, x, y, z), "pack_fields(%d, %d, %d, %d)", b, x, y, z);
          CHECK(key_batch(key) == b && key_x(key) == x && key_y(key) == y && key_z(key) == z,
                "fields of pack(%d, %d, %d, %d): %d, %d, %d, %d", b, x, y, z, key_batch(key), key_x(key), key_y(key), key_z(key));
          CHECK(key_in_field(x) && key_in_field(y) && key_in_field(z), "in_field of an edge value");
        }
  const int out[2] = {-32769, 32768};
  for (int c : out) {
    CHECK(!key_in_field(c), "in_field(%d)", c);
    CHECK(key_pack(1, c, 0, 0) == -1 && key_pack(1, 0, c, 0) == -1 && key_pack(1, 0, 0, c) == -1, "pack with a coordinate at %d", c);
  }
  CHECK(!key_in_field(INT_MAX) && !key_in_field(INT_MIN), "in_field at the ends of int");
  CHECK(key_pack(-1, 0, 0, 0) == -1 && key_pack(32768, 0, 0, 0) == -1, "pack with the batch index at -1 / 32768");
  CHECK(kKeyBias == 32768 && kKeyFieldEnd == 65536 && kKeyBatchEnd == 32768, "constants");
  for (int b : kBatch) {
    CHECK(key_scene_floor(b) == b * kTwo48 && key_scene_floor(b) == key_pack(b, -32768, -32768, -32768), "scene floor of %d", b);
    if (b > 0) CHECK(key_pack(b - 1, 32767, 32767, 32767) == key_scene_floor(b) - 1, "the last key of scene %d", b - 1);
  }
}

// a coordinate that often ties with another draw's, and often sits at an edge
static int rnd_coord() {
  const uint64_t r = rnd64();
  return (r & 3) == 0 ? (int)((r >> 8) % 65536) - 32768 : kEdge[(r >> 8) % 7];
}

static void order(long pairs) {
  for (long i = 0; i < pairs; ++i) {
    const int a[4] = {kBatch[rnd64() % 3], rnd_coord(), rnd_coord(), rnd_coord()};
    const int b[4] = {kBatch[rnd64() % 3], rnd_coord(), rnd_coord(), rnd_coord()};
    const int64_t ka = key_pack(a[0], a[1], a[2], a[3]), kb = key_pack(b[0], b[1], b[2], b[3]);
    const bool less = std::make_tuple(a[0], a[1], a[2], a[3]) < std::make_tuple(b[0], b[1], b[2], b[3]);
    CHECK(ka >= 0 && kb >= 0 && (ka < kb) == less && (ka == kb) == std::equal(a, a + 4, b),
          "order of (%d, %d, %d, %d) and (%d, %d, %d, %d)", a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
  }
}

static const int kOffset[9] = {0, 1, -1, 65535, -65535, 65536, -65536, INT_MAX, INT_MIN};

static void shift_case(int b, const int (&c)[3], const int (&d)[3]) {
  const int64_t key = key_pack(b, c[0], c[1], c[2]);
  const int64_t got = key_shift(key, d[0], d[1], d[2]);
  bool inside = true;
  for (int a = 0; a < 3; ++a) inside = inside && m_coord_ok((int64_t)c[a] + (int64_t)d[a]);
  CHECK(got == m_shift(key, d[0], d[1], d[2]), "shift of (%d, %d, %d, %d) by (%d, %d, %d) = %lld, model %lld", b, c[0], c[1], c[2],
        d[0], d[1], d[2], (long long)got, (long long)m_shift(key, d[0], d[1], d[2]));
  CHECK((got == -1) == !inside && (got >= 0) == inside, "shift of (%d, %d, %d, %d) by (%d, %d, %d): -1 exactly outside", b, c[0],
        c[1], c[2], d[0], d[1], d[2]);
  if (inside)  // every field holds its own sum: nothing carried, and a field that was not moved is as it was
    CHECK(key_batch(got) == b && key_x(got) == c[0] + d[0] && key_y(got) == c[1] + d[1] && key_z(got) == c[2] + d[2],
          "fields after the shift of (%d, %d, %d, %d) by (%d, %d, %d): %d, %d, %d, %d", b, c[0], c[1], c[2], d[0], d[1], d[2],
          key_batch(got), key_x(got), key_y(got), key_z(got));
}

static void shift() {
  const int at[3] = {-32768, 0, 32767}, batches[2] = {0, 32767};
  for (int b : batches)
    for (int x : at)
      for (int y : at)
        for (int z : at) {
          const int c[3] = {x, y, z};
          for (int axis = 0; axis < 3; ++axis)
            for (int o : kOffset) {
              int d[3] = {0, 0, 0};
              d[axis] = o;
              shift_case(b, c, d);
            }
          for (int dx : kOffset)
            for (int dy : kOffset)
              for (int dz : kOffset) {
                const int d[3] = {dx, dy, dz};
                shift_case(b, c, d);
              }
        }
  // a negative key is no site: -1 whatever the offsets (the fields of -1 are all ones: moved by -1 they would still be "legal")
  const int64_t negative[5] = {-1, -2, -kTwo48, std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::min() + 5};
  for (int64_t key : negative)
    for (int o : kOffset) {
      CHECK(key_shift(key, o, 0, 0) == -1 && key_shift(key, 0, o, 0) == -1 && key_shift(key, 0, 0, o) == -1 && key_shift(key, o, o, o) == -1,
            "shift of the negative key %lld by %d", (long long)key, o);
    }
}

// ascending arrays with a guard element on either side, every element and its two neighbours as probes
template <class T>
static void search(uint64_t max_gap) {
  const int lengths[10] = {0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025};
  for (int n : lengths) {
    std::vector<T> buf((size_t)n + 2);
    buf[0] = std::numeric_limits<T>::min();
    buf[(size_t)n + 1] = std::numeric_limits<T>::max();
    T v = (T)-5;  // (a sorted key vector may begin with invalid keys)
    for (int i = 0; i < n; ++i) {
      buf[(size_t)i + 1] = v;
      v = (T)(v + (T)(1 + rnd64() % max_gap));
    }
    const T* keys = buf.data() + 1;
    std::vector<T> probes = {(T)-1000, (T)(v + 1000)};  // below the first, above the last
    for (int i = 0; i < n; ++i) {
      probes.push_back(keys[i]);
      probes.push_back((T)(keys[i] - 1));
      probes.push_back((T)(keys[i] + 1));
    }
    for (T p : probes) {
      const T* it = std::lower_bound(keys, keys + n, p);
      const int want = (int)(it - keys), row = (it != keys + n && *it == p) ? want : -1;
      const int got = key_lower_bound(keys, n, p), found = key_find(keys, n, p);
      CHECK(got == want, "lower bound of %lld in %d keys: %d, std %d", (long long)p, n, got, want);
      CHECK(found == row, "find of %lld in %d keys: %d, expected %d", (long long)p, n, found, row);
    }
  }
}

static void midpoint() {
  CHECK(key_mid(INT_MAX - 1, INT_MAX) == INT_MAX - 1, "mid(INT_MAX - 1, INT_MAX) = %d", key_mid(INT_MAX - 1, INT_MAX));
  CHECK(key_mid(INT_MAX, INT_MAX) == INT_MAX && key_mid(0, INT_MAX) == INT_MAX / 2 && key_mid(0, 0) == 0 && key_mid(0, 1) == 0 &&
            key_mid(3, 8) == 5, "midpoints");
}

// 16 rows (batch, x, y, z) whose keys tests/test_sparse_key.py packs again in Python
static const int kRows[16][4] = {{0, 0, 0, 0},          {0, -32768, -32768, -32768}, {0, 32767, 32767, 32767}, {0, 1, -1, 0},
                                 {0, -1, 32767, -32768}, {1, 0, 0, 0},                {1, -32768, 32767, 0},    {1, 7, -300, 12345},
                                 {2, 100, 200, -300},    {2, -32767, 32766, 1},       {5, 0, 0, -1},            {300, -5, 5, -5},
                                 {32766, 1, 2, 3},       {32767, -32768, -32768, -32768}, {32767, 0, 0, 0},     {32767, 32767, 32767, 32767}};

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 1000;
  pack_and_fields();
  order(n);
  shift();
  search<int64_t>((uint64_t)1 << 40);
  search<int64_t>(2);
  search<int32_t>(1000);
  search<int32_t>(2);
  midpoint();
  for (const auto& r : kRows) {  // row: batch x y z | key, its batch, the floor of its scene, the origin site of its scene
    const int64_t key = key_pack(r[0], r[1], r[2], r[3]);
    std::printf("row %d %d %d %d %lld %d %lld %lld\n", r[0], r[1], r[2], r[3], (long long)key, key_batch(key),
                (long long)key_scene_floor(r[0]), (long long)key_pack(r[0], 0, 0, 0));
  }
  std::printf("sparse key ok: %ld random pairs, %ld checks\n", n, g_checks);
  return 0;
}
