// box4_walk.h — routing of attn_bwd_box4.hip's walk over a sorted 64-slot chunk: which half of the 16 x 16 tile a group's
// sums live in, which half a flush empties, and where a quad of four slots has to be cut.  Plain functions, host and device:
// tests/box4_walk_check.cpp runs them against a slot-by-slot model without a GPU.
//
// The matrix instruction v_mfma_f32_16x16x4_f32 has 16 rows, a group's sums need 8 (the products w_z w_y).  Rows 0..7
// (half 0) hold the groups of even parity, rows 8..15 (half 1) those of odd parity, where a slot's parity is the number of
// group ends in front of it in the chunk, mod 2: consecutive groups alternate, so the group that begins behind an end inside a
// quad accumulates beside the one that ends there, and the quad is ONE instruction.  Only a quad with two or three ends among
// its slots 0..2 would bring groups g and g + 2 into one half: it is cut behind the second of them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define B4_HD __host__ __device__ __forceinline__
#else
#define B4_HD inline
#endif

namespace vdetr {

// bit s = parity of the number of set bits of `emask` (the slots that end a group) strictly below s
B4_HD unsigned long long b4_parity_word(unsigned long long emask) {
  unsigned long long x = emask << 1;
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x ^= x << 16;
  x ^= x << 32;
  return x;
}

// the half (0: rows 0..7, lanes 0..31 of the result; 1: rows 8..15, lanes 32..63) that accumulates `slot`, and that the
// flush of a group ending in `slot` empties
B4_HD int b4_half_of_slot(unsigned long long par, int slot) { return (int)(par >> slot) & 1; }

// Row m of a lane whose slots are 4 i + kk: bit 4 i of the returned word is set where the lane's A operand of quad i is
// U[m & 7], clear where it is 0
B4_HD unsigned long long b4_keep_word(unsigned long long par, int m, int kk) { return ((m & 8) ? par : ~par) >> kk; }

// -1: the quad is one instruction.  Otherwise the in-quad slot (1 or 2) of the second end among slots 0..2: the quad is cut
// behind it.  eb: the quad's four end bits.
B4_HD int b4_quad_cut(unsigned eb) {
  const unsigned in = eb & 7u, in2 = in & (in - 1u);
  // (tests/test_box4_walk_plan.py replaces the next line, matched as text, in a copy of this file to show that the host check
  // catches a walk without the cut: reword it there too)
  return in2 ? __builtin_ctz(in2) : -1;
}

// One quad (slots base .. base + 3, end bits eb): mma(lo, hi) stands for one matrix instruction over the in-quad slots
// lo .. hi (the A operand of the other slots zeroed), flush(slot) for the flush of the group that ends in `slot`.
template <class Mma, class Flush>
B4_HD void b4_walk_quad(unsigned eb, int base, Mma&& mma, Flush&& flush) {
  const int cut = b4_quad_cut(eb);
  if (cut < 0) {  // no end, or groups g and g + 1 side by side: the end inside first, then the one in slot 3
    mma(0, 3);
    if (eb & 7u) flush(base + __builtin_ctz(eb & 7u));
    if (eb & 8u) flush(base + 3);
  } else {  // ends e0 < cut inside: groups g, g + 1 up to the cut, then g + 2 (and g + 3 behind an end in slot 2)
    mma(0, cut);
    flush(base + __builtin_ctz(eb));
    flush(base + cut);
    mma(cut + 1, 3);
    if (cut == 1 && (eb & 4u)) flush(base + 2);
    if (eb & 8u) flush(base + 3);
  }
}

}  // namespace vdetr
