// drop_stream_check.cpp — csrc/drop_stream.h on the host (tests/test_drop_stream.py builds and runs this): known answers computed
// apart from the library, and every hoisted form the kernels use against a model of the generator written out here in one piece, on
// random (seed, offset, coordinates).  Exit status 1 and a line on stderr at the first disagreement.
//   drop_stream_check [random cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "drop_stream.h"

using namespace vdetr;

static long g_checks = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    ++g_checks;                                              \
    if (!(cond)) {                                           \
      std::fprintf(stderr, "drop stream check failed: ");    \
      std::fprintf(stderr, __VA_ARGS__);                     \
      std::fprintf(stderr, "  [%s:%d]\n", __FILE__, __LINE__); \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

// ---- the model: MurmurHash3's finaliser and the two key forms, from (seed, offset) as 64-bit words ----------------------------
static uint32_t m_fmix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
struct Model {
  uint64_t seed, offset;
  uint32_t keyed(uint32_t major, uint32_t minor, uint32_t j) const {
    const uint32_t a = m_fmix((major * 2654435761u + (uint32_t)offset) ^ (uint32_t)seed);
    const uint32_t b = m_fmix(a ^ (minor * 668265263u + (uint32_t)(offset >> 32)) ^ (uint32_t)(seed >> 32));
    return m_fmix(b ^ (j * 374761393u));
  }
  uint32_t flat(uint64_t i) const {
    const uint32_t a = m_fmix((((uint32_t)i) * 2654435761u + (uint32_t)offset) ^ (uint32_t)seed ^ ((uint32_t)(i >> 32) * 668265263u));
    return m_fmix(a ^ (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32));
  }
  static uint32_t next(uint32_t x) { return m_fmix(x + 2654435769u); }
  // draw d (0..3) of word x: low, high half, then those of its successor
  static uint32_t draw(uint32_t x, int d) {
    const uint32_t w = d < 2 ? x : next(x);
    return (d & 1) ? w >> 16 : w & 0xFFFFu;
  }
};

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void known_answers() {
  CHECK(fmix32(1u) == 0x514E28B7u, "fmix32(1) = %08x", fmix32(1u));
  CHECK(fmix32(0xDEADBEEFu) == 0x0DE5C6A9u, "fmix32(0xDEADBEEF) = %08x", fmix32(0xDEADBEEFu));
  const DropStream g = drop_stream(0.3f, 0x01234567D746CDEEull, 0x100000009ull, (const uint64_t*)nullptr);
  CHECK(g.seed_lo == 0xD746CDEEu && g.seed_hi == 0x01234567u && g.off_lo == 9u && g.off_hi == 1u, "halves of the by-value pair");
  unsigned p = drop_prefix(g, 5, 1), x = drop_word(p, 3);
  CHECK(p == 0x6B7DE35Eu && x == 0x25B29DB6u && drop_next(x) == 0x497B87EEu, "rows: prefix %08x word %08x next %08x", p, x, drop_next(x));
  p = drop_prefix(g, 9, 129);
  x = drop_word(p, 17);
  CHECK(p == 0xF4DF84C5u && x == 0xA4235674u && drop_next(x) == 0x7AF32DE2u, "attention: prefix %08x word %08x next %08x", p, x, drop_next(x));
  x = drop_flat(g, 1000);
  CHECK(x == 0xF2B2F064u && drop_next(x) == 0x1E4E30E9u, "flat(1000) = %08x, %08x", x, drop_next(x));
  const float ps[4] = {0.1f, 0.3f, 1e-6f, 0.99999f};
  const unsigned ts[4] = {6554u, 19661u, 1u, 65535u};
  for (int i = 0; i < 4; ++i) {
    const DropRate r = drop_rate(ps[i]);
    CHECK(r.thresh == ts[i], "threshold of p = %g is %u", ps[i], r.thresh);
    CHECK(r.scale == 65536.f / (float)(65536u - ts[i]), "scale of p = %g is %g", ps[i], r.scale);
  }
}

static void fold() {
  const uint64_t seed = 0x8000000100000003ull, off = 0x00000001FFFFFFFFull;
  const uint64_t state[2] = {0xFEDCBA9876543210ull, 0x0000000000000002ull};  // the sum carries into the offset's high half
  const DropStream a = drop_stream(0.5f, seed, off, (const uint64_t*)nullptr), b = drop_stream(0.5f, seed, off, state);
  CHECK(a.seed_lo == 3u && a.seed_hi == 0x80000001u && a.off_lo == 0xFFFFFFFFu && a.off_hi == 1u, "fold without a device state");
  const uint64_t s = seed ^ state[0], o = off + state[1];
  CHECK(b.seed_lo == (uint32_t)s && b.seed_hi == (uint32_t)(s >> 32) && b.off_lo == 1u && b.off_hi == 2u && (uint32_t)(o >> 32) == 2u,
        "fold with a device state: seed ^= state[0], offset += state[1]");
  const unsigned long long state2[2] = {state[0], state[1]};  // (the attention descriptors carry the state as unsigned long long)
  const DropStream c = drop_stream(0.5f, seed, off, state2);
  CHECK(c.seed_lo == b.seed_lo && c.seed_hi == b.seed_hi && c.off_lo == b.off_lo && c.off_hi == b.off_hi, "fold: pointer type");
  CHECK(a.thresh == 32768u && a.scale == 2.f && b.thresh == 32768u, "p = 0.5");
}

static void no_dropout() {
  const float ps[3] = {0.f, -1.f, -0.f};
  for (float p : ps) {
    const DropStream g = drop_stream(p, rnd64(), rnd64(), (const uint64_t*)nullptr);
    CHECK(g.thresh == 0u && g.scale == 1.f, "p = %g: thresh %u scale %g", p, g.thresh, g.scale);
    for (int k = 0; k < 64; ++k) {
      bool k4[4], f4[4];
      const unsigned pre = drop_prefix(g, (unsigned)rnd64(), 1);
      drop_keep4(g, pre, (unsigned)k, k4);
      drop_keep4(g, drop_flat(g, (long long)(rnd64() >> 1)), f4);
      CHECK(k4[0] && k4[1] && k4[2] && k4[3] && f4[0] && f4[1] && f4[2] && f4[3] && drop_keep_pair(g, pre, k), "thresh 0 keeps everything");
    }
  }
}

static void random_case() {
  const uint64_t seed = rnd64(), offset = (rnd64() & 1) ? rnd64() : rnd64() >> 40, st[2] = {rnd64(), rnd64()};
  const bool with_state = rnd64() & 1;
  const float p = (float)((rnd64() >> 11) * (1.0 / 9007199254740992.0));
  const DropStream g = drop_stream(p, seed, offset, with_state ? st : (const uint64_t*)nullptr);
  const Model M = {with_state ? seed ^ st[0] : seed, with_state ? offset + st[1] : offset};
  const unsigned t = g.thresh;
  CHECK(t >= 1u && t <= 65535u, "threshold %u of p = %g", t, p);

  // attention: the prefix of (b, head group, q) once, a word per key (attn_fwd_self.hip), head h & 3 by `second` and `shift`
  const unsigned b = (unsigned)(rnd64() % 64), H = 4u * (1 + (unsigned)(rnd64() % 4)), q = (unsigned)(rnd64() % 100000), key0 = (unsigned)(rnd64() % 100000);
  for (unsigned h = 0; h < H; ++h) {
    const unsigned pre = drop_prefix(g, q, b * 64u + (h >> 2));
    const bool second = (h & 2) != 0;
    const int shift = (int)(h & 1) * 16;
    for (unsigned key = key0; key < key0 + 3; ++key) {
      const unsigned x = drop_word(pre, key), y = drop_next(x);
      const unsigned want = Model::draw(M.keyed(q, b * 64u + (h >> 2), key), (int)(h & 3));
      const unsigned hoisted = ((second ? drop_next(x) : x) >> shift) & 0xFFFFu;
      const unsigned picked = drop_pick4(drop_lo(x), drop_hi(x), drop_lo(y), drop_hi(y), (int)(h & 3));
      CHECK(hoisted == want && picked == want, "attention draw of (b %u, h %u, q %u, key %u): %u / %u, model %u", b, h, q, key, hoisted, picked, want);
    }
  }
  // rows: prefix per row, word per four channels; channels: prefix per channel, pair words (heads.hip) against per-element keep (bn_act.hip)
  const unsigned major = (unsigned)rnd64(), pre = drop_prefix(g, major, 1);
  for (int it = 0; it < 3; ++it) {
    const unsigned j = (unsigned)(rnd64() % (1u << 20));
    bool k4[4];
    drop_keep4(g, pre, j, k4);
    for (int d = 0; d < 4; ++d) CHECK(k4[d] == (Model::draw(M.keyed(major, 1, j), d) >= t), "row %u word %u draw %d", major, j, d);
    const int e0 = 2 * (int)j;  // four consecutive elements e0 .. e0 + 3 of a channel, e0 even
    const unsigned x0 = drop_word(pre, (unsigned)(e0 >> 1)), x1 = drop_word(pre, (unsigned)((e0 >> 1) + 1));
    const bool pair[4] = {drop_lo(x0) >= t, drop_hi(x0) >= t, drop_lo(x1) >= t, drop_hi(x1) >= t};
    for (int d = 0; d < 4; ++d) {
      const bool want = Model::draw(M.keyed(major, 1, (unsigned)((e0 + d) >> 1)), (e0 + d) & 1) >= t;
      CHECK(pair[d] == want && drop_keep_pair(g, pre, e0 + d) == want, "channel %u element %d", major, e0 + d);
    }
  }
  // the flat form, below and above 2^32 float4s (no tensor of a test reaches the high term)
  for (int it = 0; it < 2; ++it) {
    const uint64_t i = it ? (rnd64() >> 24) | (1ull << 32) : rnd64() >> 40;
    bool k4[4];
    drop_keep4(g, drop_flat(g, (long long)i), k4);
    for (int d = 0; d < 4; ++d) CHECK(k4[d] == (Model::draw(M.flat(i), d) >= t), "flat %llu draw %d", (unsigned long long)i, d);
    CHECK(drop_flat(g, (long long)i) == M.flat(i), "flat word of %llu", (unsigned long long)i);
  }
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 1000;
  known_answers();
  fold();
  no_dropout();
  for (long i = 0; i < n; ++i) random_case();
  std::printf("drop stream ok: %ld random cases, %ld checks\n", n, g_checks);
  return 0;
}
