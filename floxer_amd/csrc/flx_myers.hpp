// One column of the Myers/Hyyro bit-vector recurrence over one 64-row word, as the DP kernels (K3/K4, ed_block_body) and the traceback's
// window recomputation (K5) share it, and the per-block patch of the reference symbols past a window's end.
// The step is written on the two 32-bit halves of the word: gfx950 computes any boolean of three inputs in one instruction
// (v_bitop3_b32), but the compiler only splits 64-bit logic into halves after it has selected instructions and so never forms one from
// u64 source. Only the addition and the two shifts by one, whose carries cross the halves, stay 64-bit operations.
// A host compiler gets a portable bit3 and runs the identical step (tests/myers_step_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>

namespace flx {

#if defined(__HIPCC__)
#define FLX_MYERS_FN __host__ __device__ __forceinline__
#else
#define FLX_MYERS_FN inline
#endif

// The truth table of a boolean of three inputs, as v_bitop3_b32 takes it: bit (a << 2 | b << 1 | c) of the table is f(a, b, c), which is
// the expression evaluated on these three words.
constexpr std::uint32_t kBit3A = 0xF0u, kBit3B = 0xCCu, kBit3C = 0xAAu;
#define FLX_BIT3_TABLE(expr) ([] { constexpr std::uint32_t a = ::flx::kBit3A, b = ::flx::kBit3B, c = ::flx::kBit3C; return (std::uint32_t)(expr) & 0xFFu; }())
constexpr std::uint32_t kTtAndOfOr = FLX_BIT3_TABLE((a | b) & c);        // (eq | mv) & pv
constexpr std::uint32_t kTtXorOr = FLX_BIT3_TABLE((a ^ b) | c);          // (tt ^ pv) | x
constexpr std::uint32_t kTtOrNor = FLX_BIT3_TABLE(a | ~(b | c));         // mv | ~(pv | d0), (hn << 1) | ~(xh | d0)
constexpr std::uint32_t kTtMerge = FLX_BIT3_TABLE((a & c) | (b & ~c));   // c ? a : b, bit by bit

template <std::uint32_t TT>
FLX_MYERS_FN std::uint32_t bit3(std::uint32_t a, std::uint32_t b, std::uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
#else
    std::uint32_t r = 0;                              // the sum of the table's minterms (TT is a constant: the unused ones fold away)
    for (std::uint32_t i = 0; i < 8u; ++i)
        if ((TT >> i) & 1u) r |= ((i & 4u) ? a : ~a) & ((i & 2u) ? b : ~b) & ((i & 1u) ? c : ~c);
    return r;
#endif
}

// a 64-bit word as its two halves (x: bits 0..31), bit-cast both ways: never rebuilt by shifting and or-ing
#if defined(__HIP_DEVICE_COMPILE__)
typedef std::uint32_t MyersHalves __attribute__((ext_vector_type(2)));
FLX_MYERS_FN MyersHalves myers_halves(std::uint64_t v) { return __builtin_bit_cast(MyersHalves, v); }
FLX_MYERS_FN std::uint64_t myers_word(MyersHalves h) { return __builtin_bit_cast(std::uint64_t, h); }
#else
struct MyersHalves { std::uint32_t x, y; };          // (little-endian hosts, as the device)
FLX_MYERS_FN MyersHalves myers_halves(std::uint64_t v) { MyersHalves h; std::memcpy(&h, &v, 8); return h; }
FLX_MYERS_FN std::uint64_t myers_word(MyersHalves h) { std::uint64_t v; std::memcpy(&v, &h, 8); return v; }
#endif

// the high half of a word shifted up by one: its bits move up, bit 31 of the low half comes in below (v_alignbit_b32)
FLX_MYERS_FN std::uint32_t funnel_up1(std::uint32_t hi, std::uint32_t lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, 31);
#else
    return (hi << 1) | (lo >> 31);
#endif
}

// One column of one word. eq: the rows that match the column's symbol; vp, vn: the word's vertical deltas (+1, -1), updated in place;
// c_hp, c_hn (0 or 1): the horizontal delta that enters the word's row 0 from the word above; hp, hn: the word's horizontal deltas in
// this column (bit 63 is what the next word, or the next group, takes as its c_hp, c_hn).
FLX_MYERS_FN void myers_step(std::uint64_t eq, std::uint64_t& vp, std::uint64_t& vn, std::uint32_t c_hp, std::uint32_t c_hn, std::uint64_t& hp,
                             std::uint64_t& hn) {
    MyersHalves const e = myers_halves(eq), p = myers_halves(vp), m = myers_halves(vn);
    MyersHalves x, xp, d0, hnh, hph, vnh, vph;
    x.x = e.x | m.x;
    x.y = e.y | m.y;
    xp.x = bit3<kTtAndOfOr>(e.x, m.x, p.x);
    xp.y = bit3<kTtAndOfOr>(e.y, m.y, p.y);
    MyersHalves const t = myers_halves(vp + myers_word(xp) + c_hn);
    d0.x = bit3<kTtXorOr>(t.x, p.x, x.x);
    d0.y = bit3<kTtXorOr>(t.y, p.y, x.y);
    hnh.x = p.x & d0.x;
    hnh.y = p.y & d0.y;
    hph.x = bit3<kTtOrNor>(m.x, p.x, d0.x);
    hph.y = bit3<kTtOrNor>(m.y, p.y, d0.y);
    hp = myers_word(hph);
    hn = myers_word(hnh);
    MyersHalves xh, ns;
    xh.x = (hph.x << 1) | c_hp;
    xh.y = funnel_up1(hph.y, hph.x);
    ns.x = (hnh.x << 1) | c_hn;
    ns.y = funnel_up1(hnh.y, hnh.x);
    vnh.x = xh.x & d0.x;
    vnh.y = xh.y & d0.y;
    vph.x = bit3<kTtOrNor>(ns.x, xh.x, d0.x);
    vph.y = bit3<kTtOrNor>(ns.y, xh.y, d0.y);
    vn = myers_word(vnh);
    vp = myers_word(vph);
}

// The same step as plain 64-bit source, as the compiler splits it into two-input operations. Kept for the kernel instantiations whose
// register allocation does not hold the form above without scratch (ed_block_body: kPlainStep).
FLX_MYERS_FN void myers_step_u64(std::uint64_t eq, std::uint64_t& vp, std::uint64_t& vn, std::uint32_t c_hp, std::uint32_t c_hn, std::uint64_t& hp,
                                 std::uint64_t& hn) {
    std::uint64_t const pv = vp, mv = vn;
    std::uint64_t const x = eq | mv;
    std::uint64_t const tt = pv + (x & pv) + c_hn;
    std::uint64_t const d0 = (tt ^ pv) | x;
    hn = pv & d0;
    hp = mv | ~(pv | d0);
    std::uint64_t const xh = (hp << 1) | c_hp;
    vn = xh & d0;
    vp = (hn << 1) | ~(xh | d0) | c_hn;
}

// A block's outgoing carry word from two 16-bit accumulators. A column pushes bit 63 of its last word's hp (hn) into its accumulator
// from below, funnel_up1(acc, high half), so that column j of sixteen ends up at bit 15 - j. The carry word holds column j's pair at
// bits 2j (hp) and 2j + 1 (hn): both accumulators in one word, its bits reversed (column j at bit j and at bit 16 + j), and the two halves
// shuffled into each other.
FLX_MYERS_FN std::uint32_t myers_carry_word(std::uint32_t acc_hp, std::uint32_t acc_hn) {
    std::uint32_t x = (acc_hp << 16) | (acc_hn & 0xFFFFu);
#if defined(__HIP_DEVICE_COMPILE__)
    x = __builtin_bitreverse32(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    x = (x >> 16) | (x << 16);
#endif
    std::uint32_t t;
    t = (x ^ (x >> 8)) & 0x0000FF00u; x = x ^ t ^ (t << 8);
    t = (x ^ (x >> 4)) & 0x00F000F0u; x = x ^ t ^ (t << 4);
    t = (x ^ (x >> 2)) & 0x0C0C0C0Cu; x = x ^ t ^ (t << 2);
    t = (x ^ (x >> 1)) & 0x22222222u; x = x ^ t ^ (t << 1);
    return x;
}

// The four symbol registers of a 16-column block (column j in byte j % 4 of register j / 4) with symbol 6, which matches no row, in
// every column from `inside` on: the columns past the end of the window. inside <= 0: all sixteen; >= 16: none. One merge per register.
FLX_MYERS_FN std::uint32_t myers_patch_register(std::uint32_t q, int keep) {      // keep: columns of this register inside the window
    std::uint32_t const mask = keep >= 4 ? 0xFFFFFFFFu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u;
    return bit3<kTtMerge>(q, 0x06060606u, mask);
}
FLX_MYERS_FN void myers_patch_symbols(std::uint32_t (&q)[4], int inside) {
    q[0] = myers_patch_register(q[0], inside);
    q[1] = myers_patch_register(q[1], inside - 4);
    q[2] = myers_patch_register(q[2], inside - 8);
    q[3] = myers_patch_register(q[3], inside - 12);
}

}  // namespace flx
