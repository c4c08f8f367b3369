// Host check of v-detr_amd/csrc/box4_walk.h (the routing of attn_bwd_box4.hip's walk): test_box4_walk_plan.py compiles this
// file with a host sanitizer and runs it.  A scalar model walks the slots one by one and holds the walk to three rules:
//   1. every slot is added to exactly one half of the tile, and that half is the one its group is flushed from
//   2. at no matrix instruction do two different live groups share a half
//   3. the groups are flushed once each, in slot order, and a half is empty (zero) when a new group enters it
// Cases: all 16 end patterns of a quad x both incoming parities, and random end masks with bit ns - 1 set.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "box4_walk.h"

namespace {

int g_fail = 0;
unsigned long long g_mask = 0;
int g_ns = 0;

void fail(const char* what, int slot) {
  if (g_fail < 20) std::fprintf(stderr, "FAIL mask %016llx ns %d slot %d: %s\n", g_mask, g_ns, slot, what);
  ++g_fail;
}

struct Model {
  int gid[64];         // the group of a slot: the ends in front of it, counted slot by slot
  int added[64] = {};  // matrix instructions that took the slot into a row half
  int half_of[64];     // ... and into which
  int live[2] = {-1, -1};  // the group a half holds sums of (-1: the half is zero)
  int next_flush = 0, mmas = 0, cuts = 0;
};

// walks the first ns slots (ns a multiple of 4, bit ns - 1 of emask set, no bit above it)
void check_mask(unsigned long long emask, int ns) {
  g_mask = emask;
  g_ns = ns;
  Model m;
  int ends = 0;
  for (int s = 0; s < ns; ++s) {
    m.gid[s] = ends;
    m.half_of[s] = -1;
    ends += (int)(emask >> s) & 1;
  }
  const int ngroups = ends;
  const unsigned long long par = vdetr::b4_parity_word(emask);
  for (int s = 0; s < ns; ++s) {
    if (vdetr::b4_half_of_slot(par, s) != (m.gid[s] & 1)) fail("parity word differs from the count of ends in front", s);
    for (int row = 0; row < 16; ++row) {  // the lane of row `row` whose slots are 4 i + kk: its keep bit of this slot
      const int kept = (int)(vdetr::b4_keep_word(par, row, s & 3) >> (s & ~3)) & 1;
      if (kept != ((row >> 3) == vdetr::b4_half_of_slot(par, s))) fail("keep word: a row takes a slot of the other half", s);
    }
  }
  for (int i = 0; 4 * i < ns; ++i) {
    const unsigned eb = (unsigned)(emask >> (4 * i)) & 0xFu;
    const int before = m.mmas;
    vdetr::b4_walk_quad(
        eb, 4 * i,
        [&](int lo, int hi) {
          ++m.mmas;
          if (lo < 0 || hi > 3 || lo > hi) fail("instruction over no slot", 4 * i);
          for (int k = lo; k <= hi; ++k) {
            const int s = 4 * i + k, h = vdetr::b4_half_of_slot(par, s);
            if (m.live[h] == -1) m.live[h] = m.gid[s];  // (rule 3: it enters an empty half)
            else if (m.live[h] != m.gid[s]) fail("two live groups in one half", s);  // rule 2
            ++m.added[s];
            m.half_of[s] = h;
          }
        },
        [&](int s) {
          if (s < 0 || s >= ns || !((emask >> s) & 1)) {
            fail("flush at a slot that ends no group", s);
            return;
          }
          const int g = m.gid[s], h = vdetr::b4_half_of_slot(par, s);
          if (g != m.next_flush) fail("groups not flushed once each in slot order", s);  // rule 3
          m.next_flush = g + 1;
          if (m.live[h] != g) fail("flush from a half that does not hold the group", s);
          for (int q = 0; q < ns; ++q)
            if (m.gid[q] == g && (m.added[q] != 1 || m.half_of[q] != h)) fail("flushed group misses a slot, or holds it twice or elsewhere", q);  // rule 1
          m.live[h] = -1;
        });
    const int used = m.mmas - before, cut = vdetr::b4_quad_cut(eb);
    const int inside = __builtin_popcount(eb & 7u);
    if ((cut >= 0) != (inside >= 2)) fail("cut decision", 4 * i);
    if (used != (inside >= 2 ? 2 : 1)) fail("matrix instructions of the quad", 4 * i);
  }
  for (int s = 0; s < ns; ++s)
    if (m.added[s] != 1) fail("slot not added exactly once", s);  // rule 1
  if (m.next_flush != ngroups) fail("groups left unflushed", ns - 1);
  if (m.live[0] != -1 || m.live[1] != -1) fail("a half is not empty at the chunk's end", ns - 1);
}

}  // namespace

int main(int argc, char** argv) {
  const int nrandom = argc > 1 ? std::atoi(argv[1]) : 4000;
  long cases = 0;
  // every end pattern of a quad, behind a quad that hands it parity 0 (no end) or 1 (an end in its last slot), in front of
  // the quad that closes the chunk
  for (unsigned eb = 0; eb < 16; ++eb)
    for (int p = 0; p < 2; ++p) {
      check_mask((p ? 0x8ull : 0x0ull) | ((unsigned long long)eb << 4) | (0x8ull << 8), 12);
      check_mask((p ? 0x8ull : 0x0ull) | ((unsigned long long)eb << 4) | (0x8ull << 60), 64);
      cases += 2;
    }
  for (unsigned eb = 0; eb < 16; ++eb) {  // ... as the first quad, and as the last (bit 3: the chunk's end is always set)
    check_mask((unsigned long long)eb | (0x8ull << 4), 8);
    check_mask(((unsigned long long)(eb | 8u)) << 60, 64);
    check_mask(0x8ull | ((unsigned long long)(eb | 8u)) << 60, 64);
    cases += 3;
  }
  std::mt19937_64 rng(20240607);
  for (int r = 0; r < nrandom; ++r) {
    unsigned long long mask = rng();
    const int density = (int)(rng() % 4);  // from one end in 2 slots to one in 16
    for (int d = 0; d < density; ++d) mask &= rng();
    const int ns = r % 3 == 0 ? 4 * (1 + (int)(rng() % 16)) : 64;
    if (ns < 64) mask &= (1ull << ns) - 1ull;
    mask |= 1ull << (ns - 1);
    check_mask(mask, ns);
    ++cases;
  }
  check_mask(~0ull, 64);               // every slot its own group
  check_mask(1ull << 63, 64);          // one group
  check_mask(0x8888888888888888ull, 64);  // groups of four: ends in slot 3 only
  cases += 3;
  if (g_fail) {
    std::fprintf(stderr, "%d failures in %ld masks\n", g_fail, cases);
    return 1;
  }
  std::printf("box4 walk ok: %ld masks\n", cases);
  return 0;
}
