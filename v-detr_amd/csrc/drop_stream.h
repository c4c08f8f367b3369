// drop_stream.h — the one dropout generator of the library: counter-based (stateless), so a backward pass regenerates the mask
// its forward drew and a fused launch draws the masks of the launches it replaces.  A chain of murmur3 finalisers (fmix32: a
// bijection of 32 bits with full avalanche) keyed by (seed, offset) and the element's coordinates; a 32-bit word holds two 16-bit
// draws, its successor two more; keep iff draw >= thresh.  A Philox4x32-10 here cost ~100 ops per attention pair, this ~16.
//
//   keyed form  word = fmix32(prefix(major, minor) ^ j * c):  the prefix is hoisted out of the loop over j
//     add_ln.hip, rowblock.hip   major row,     minor 1,                  j = channel / 4,            4 draws: channels 4 j .. 4 j + 3
//     bn_act.hip, heads.hip      major channel, minor 1,                  j = e / 2 (e in the B*N),   2 draws: elements 2 j, 2 j + 1
//     attn_*.hip                 major query,   minor b * 64 + head / 4,  j = key,                    4 draws: heads 4 (head / 4) ..
//   flat form   word = drop_flat(i):  float4 number i of a flat tensor, 4 draws (relu_dropout in bn_act.hip, rowblock.hip)
//
// Plain functions, host and device, no other header: tests/drop_stream_check.cpp holds them to known answers without a GPU, and
// tests/drop_stream_restatement.py restates every stream in numpy for the masks the kernels return.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DS_HD __host__ __device__ __forceinline__
#else
#define DS_HD inline
#endif

namespace vdetr {

DS_HD unsigned fmix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

struct DropStream {
  unsigned seed_lo, seed_hi, off_lo, off_hi;
  unsigned thresh;  // keep iff 16-bit draw >= thresh; 0: no dropout
  float scale;      // 65536 / (65536 - thresh): unbiased for the quantised rate
};

// the rate in 1/65536 steps, never 0 (that means "no dropout") and never everything
struct DropRate {
  unsigned thresh;
  float scale;
};
DS_HD DropRate drop_rate(float p) {
  DropRate r = {0u, 1.f};
  if (p > 0.f) {
    int t = (int)((double)p * 65536.0 + 0.5);
    t = t < 1 ? 1 : (t > 65535 ? 65535 : t);
    r.thresh = (unsigned)t;
    r.scale = 65536.f / (float)(65536 - t);
  }
  return r;
}
// The device-resident {seed, offset} pair (optional) is COMBINED with the by-value one: seed ^= state.seed, offset += state.offset,
// so that many modules share one per-step device state and still draw independent masks through their by-value salt.
template <class U64>
DS_HD DropStream drop_stream(float p, unsigned long long seed, unsigned long long offset, const U64* rng_state) {
  static_assert(sizeof(U64) == 8, "the device state is two 64-bit words");
  DropStream g;
  unsigned long long s = seed, o = offset;
  if (rng_state) { s ^= rng_state[0]; o += rng_state[1]; }
  g.seed_lo = (unsigned)s; g.seed_hi = (unsigned)(s >> 32); g.off_lo = (unsigned)o; g.off_hi = (unsigned)(o >> 32);
  const DropRate r = drop_rate(p);
  g.thresh = r.thresh; g.scale = r.scale;
  return g;
}

DS_HD unsigned drop_prefix(const DropStream& g, unsigned major, unsigned minor) {
  const unsigned x = fmix32((major * 0x9E3779B1u + g.off_lo) ^ g.seed_lo);
  return fmix32(x ^ (minor * 0x27D4EB2Fu + g.off_hi) ^ g.seed_hi);
}
DS_HD unsigned drop_word(unsigned prefix, unsigned j) { return fmix32(prefix ^ (j * 0x165667B1u)); }
DS_HD unsigned drop_next(unsigned x) { return fmix32(x + 0x9E3779B9u); }
DS_HD unsigned drop_flat(const DropStream& g, long long i) {
  const unsigned x = fmix32(((unsigned)i * 0x9E3779B1u + g.off_lo) ^ g.seed_lo ^ ((unsigned)(i >> 32) * 0x27D4EB2Fu));
  return fmix32(x ^ g.seed_hi ^ g.off_hi);
}

// the two draws of a word
DS_HD unsigned drop_lo(unsigned x) { return x & 0xFFFFu; }
DS_HD unsigned drop_hi(unsigned x) { return x >> 16; }
// draw i of the four (lo, hi of a word, lo, hi of its successor): attention head 4 g + i reads it
DS_HD unsigned drop_pick4(unsigned d0, unsigned d1, unsigned d2, unsigned d3, int i) { return i == 0 ? d0 : (i == 1 ? d1 : (i == 2 ? d2 : d3)); }
// keep flags of the four draws of word x and its successor; everything is kept without dropout
DS_HD void drop_keep4(const DropStream& g, unsigned x, bool (&keep)[4]) {
  if (!g.thresh) { keep[0] = keep[1] = keep[2] = keep[3] = true; return; }
  const unsigned y = drop_next(x);
  keep[0] = drop_lo(x) >= g.thresh; keep[1] = drop_hi(x) >= g.thresh;
  keep[2] = drop_lo(y) >= g.thresh; keep[3] = drop_hi(y) >= g.thresh;
}
// ... of word j behind a hoisted prefix
DS_HD void drop_keep4(const DropStream& g, unsigned prefix, unsigned j, bool (&keep)[4]) { drop_keep4(g, drop_word(prefix, j), keep); }
// keep flag of element e of a pair stream (word e / 2, its low draw for even e)
DS_HD bool drop_keep_pair(const DropStream& g, unsigned prefix, int e) {
  if (!g.thresh) return true;
  const unsigned x = drop_word(prefix, (unsigned)(e >> 1));
  return ((e & 1) ? drop_hi(x) : drop_lo(x)) >= g.thresh;
}

}  // namespace vdetr
