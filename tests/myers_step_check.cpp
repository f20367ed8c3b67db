// The column step the DP kernels and the traceback share (floxer_amd/csrc/flx_myers.hpp), compiled for the host and run against the plain
// 64-bit formula written out here: vp, vn, hp and hn must be equal for every carry-in pair on structured words (zeros, ones, alternating
// bits, single bits at 0 / 31 / 32 / 63, runs that end at bit 31 and at bit 63 so that the addition's carry crosses the halves and leaves
// the word), on a million random triples and on a chain of 250 000 columns that feeds a word's outputs back in. Each truth table is checked against its expression on the eight input combinations, the
// portable bit3 against a bit-by-bit lookup in its table, and the symbol patch for every count of in-window columns. Test infrastructure.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../floxer_amd/csrc/flx_myers.hpp"
using namespace flx;
using u32 = std::uint32_t;
using u64 = std::uint64_t;

static int bad = 0;
static long checked = 0;

// Myers' column, Hyyro's block form, as the kernels had it before the step moved into the header
static void plain_step(u64 eq, u64& vp, u64& vn, u64 c_hp, u64 c_hn, u64& hp, u64& hn) {
    u64 const pv = vp, mv = vn;
    u64 const x = eq | mv;
    u64 const tt = pv + (x & pv) + c_hn;
    u64 const d0 = (tt ^ pv) | x;
    hn = pv & d0;
    hp = mv | ~(pv | d0);
    u64 const xh = (hp << 1) | c_hp;
    vn = xh & d0;
    vp = (hn << 1) | ~(xh | d0) | c_hn;
}

static void check_triple(u64 eq, u64 pv, u64 mv) {
    for (u32 c = 0; c < 4u; ++c) {
        u64 vp0 = pv, vn0 = mv, hp0, hn0, vp1 = pv, vn1 = mv, hp1, hn1;
        plain_step(eq, vp0, vn0, c & 1u, c >> 1, hp0, hn0);
        myers_step(eq, vp1, vn1, c & 1u, c >> 1, hp1, hn1);
        ++checked;
        u64 vp2 = pv, vn2 = mv, hp2, hn2;                 // (the header's 64-bit form, which one kernel instantiation keeps)
        myers_step_u64(eq, vp2, vn2, c & 1u, c >> 1, hp2, hn2);
        if (vp0 != vp2 || vn0 != vn2 || hp0 != hp2 || hn0 != hn2) { if (bad++ < 5) printf("FAIL myers_step_u64 on eq %016llx\n", (unsigned long long)eq); }
        if (vp0 != vp1 || vn0 != vn1 || hp0 != hp1 || hn0 != hn1) {
            if (bad++ < 5)
                printf("FAIL step eq %016llx vp %016llx vn %016llx c_hp %u c_hn %u: vp %016llx/%016llx vn %016llx/%016llx hp %016llx/%016llx hn %016llx/%016llx\n",
                       (unsigned long long)eq, (unsigned long long)pv, (unsigned long long)mv, c & 1u, c >> 1, (unsigned long long)vp1, (unsigned long long)vp0,
                       (unsigned long long)vn1, (unsigned long long)vn0, (unsigned long long)hp1, (unsigned long long)hp0, (unsigned long long)hn1,
                       (unsigned long long)hn0);
        }
    }
}

template <u32 TT, class F>
static void check_table(const char* name, F f) {
    for (u32 i = 0; i < 8u; ++i) {
        u32 const a = (i >> 2) & 1u, b = (i >> 1) & 1u, c = i & 1u;
        u32 const want = f(a, b, c) & 1u;
        if (((TT >> i) & 1u) != want) { if (bad++ < 5) printf("FAIL table %s: entry %u is %u, the expression gives %u\n", name, i, (TT >> i) & 1u, want); }
        // the portable bit3 on whole words: every bit of the word carries the same combination
        u32 const got = bit3<TT>(a ? ~0u : 0u, b ? ~0u : 0u, c ? ~0u : 0u);
        if (got != (want ? ~0u : 0u)) { if (bad++ < 5) printf("FAIL bit3 %s: inputs %u %u %u give %08x\n", name, a, b, c, got); }
    }
    if (TT > 0xFFu) { if (bad++ < 5) printf("FAIL table %s: %x is wider than 8 bits\n", name, TT); }
}

int main() {
    // ---- truth tables against their expressions
    check_table<kTtAndOfOr>("(a|b)&c", [](u32 a, u32 b, u32 c) { return (a | b) & c; });
    check_table<kTtXorOr>("(a^b)|c", [](u32 a, u32 b, u32 c) { return (a ^ b) | c; });
    check_table<kTtOrNor>("a|~(b|c)", [](u32 a, u32 b, u32 c) { return a | ~(b | c); });
    check_table<kTtMerge>("c?a:b", [](u32 a, u32 b, u32 c) { return c ? a : b; });
    std::mt19937_64 rng(11);
    for (int it = 0; it < 1000; ++it) {                   // bit3 on mixed words, bit by bit from the table
        u32 const a = (u32)rng(), b = (u32)rng(), c = (u32)rng();
        u32 want = 0;
        for (u32 bit = 0; bit < 32u; ++bit) {
            u32 const idx = (((a >> bit) & 1u) << 2) | (((b >> bit) & 1u) << 1) | ((c >> bit) & 1u);
            want |= ((kTtXorOr >> idx) & 1u) << bit;
        }
        if (bit3<kTtXorOr>(a, b, c) != want) { if (bad++ < 5) printf("FAIL bit3 on %08x %08x %08x\n", a, b, c); }
    }
    if (funnel_up1(0x80000001u, 0x80000000u) != 0x00000003u || funnel_up1(0x40000000u, 0x7FFFFFFFu) != 0x80000000u) { ++bad; printf("FAIL funnel_up1\n"); }

    // ---- the step on structured words
    std::vector<u64> words = {0ull, ~0ull, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull};
    for (int bit : {0, 31, 32, 63}) { words.push_back(1ull << bit); words.push_back(~(1ull << bit)); }
    for (int lo : {0, 1, 17, 30, 31}) words.push_back(((1ull << 32) - 1ull) & ~((1ull << lo) - 1ull));          // runs that end at bit 31
    for (int lo : {0, 1, 31, 32, 33, 47, 62, 63}) words.push_back(~0ull & ~((1ull << lo) - 1ull));              // runs that end at bit 63
    words.push_back(0x00000000FFFFFFFFull);
    words.push_back(0xFFFFFFFF00000000ull);
    words.push_back(0x7FFFFFFFFFFFFFFFull);
    words.push_back(0x000000007FFFFFFFull);
    for (u64 eq : words)
        for (u64 pv : words)
            for (u64 mv : words) check_triple(eq, pv, mv);
    // (a valid column never has vp and vn set in the same row; the formula is checked on every triple all the same, and on valid ones)
    for (u64 eq : words)
        for (u64 pv : words) { check_triple(eq, pv, ~pv); check_triple(eq, pv, 0ull); }
    long const structured = checked;
    // ---- random triples, sparse and dense, and chains of columns that feed a word's outputs back in
    for (int it = 0; it < 1000000; ++it) {
        u64 eq = rng(), pv = rng(), mv = rng();
        if (it & 1) { eq &= rng(); mv &= ~pv; }           // (every other one a valid state with a sparser match mask)
        if ((it & 6) == 6) { pv |= rng() | rng(); mv &= ~pv; }   // (long runs of +1: long carry chains through the addition)
        check_triple(eq, pv, mv);
    }
    {
        u64 vp0 = ~0ull, vn0 = 0, vp1 = ~0ull, vn1 = 0;
        for (int it = 0; it < 250000; ++it) {
            u64 const eq = rng() & rng();
            u32 const c = (u32)rng() & 3u;
            u64 hp0, hn0, hp1, hn1;
            plain_step(eq, vp0, vn0, c & 1u, c >> 1, hp0, hn0);
            myers_step(eq, vp1, vn1, c & 1u, c >> 1, hp1, hn1);
            ++checked;
            if (vp0 != vp1 || vn0 != vn1 || hp0 != hp1 || hn0 != hn1) { if (bad++ < 5) printf("FAIL chained column %d\n", it); vp1 = vp0; vn1 = vn0; }
        }
    }

    // ---- the symbol patch: column j (byte j % 4 of register j / 4) keeps its symbol when j < inside and is 6 otherwise
    int patched = 0;
    for (int inside = -20; inside <= 40; ++inside) {
        u32 q[4], q0[4];
        for (int r = 0; r < 4; ++r) q[r] = q0[r] = (u32)rng();
        myers_patch_symbols(q, inside);
        for (int j = 0; j < 16; ++j) {
            u32 const got = (q[j >> 2] >> (8 * (j & 3))) & 0xFFu, was = (q0[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            u32 const want = j < inside ? was : 6u;
            if (got != want) { if (bad++ < 5) printf("FAIL patch: %d columns inside, column %d is %u, not %u\n", inside, j, got, want); }
        }
        ++patched;
    }
    // ---- the carry word: sixteen columns' bits pushed into the two accumulators, against each pair placed at bits 2j, 2j + 1
    int words_packed = 0;
    for (int it = 0; it < 20000; ++it) {
        u32 acc_hp = 0, acc_hn = 0, want = 0;
        u32 const bits_hp = it < 4 ? ((it & 1) ? 0xFFFFu : 0u) : (u32)rng() & 0xFFFFu, bits_hn = it < 4 ? ((it & 2) ? 0xFFFFu : 0u) : (u32)rng() & 0xFFFFu;
        for (int j = 0; j < 16; ++j) {
            u32 const hp_hi = (((bits_hp >> j) & 1u) << 31) | ((u32)rng() >> 1), hn_hi = (((bits_hn >> j) & 1u) << 31) | ((u32)rng() >> 1);
            acc_hp = funnel_up1(acc_hp, hp_hi);
            acc_hn = funnel_up1(acc_hn, hn_hi);
            want |= (((bits_hp >> j) & 1u) | (((bits_hn >> j) & 1u) << 1)) << (2 * j);
        }
        if (myers_carry_word(acc_hp, acc_hn) != want) { if (bad++ < 5) printf("FAIL carry word: hp %04x hn %04x give %08x, not %08x\n", bits_hp, bits_hn, myers_carry_word(acc_hp, acc_hn), want); }
        ++words_packed;
    }
    if (bad) { printf("FAILED: %d\n", bad); return 1; }
    printf("ok %ld steps (%ld on structured words), 4 tables, %d symbol patches, %d carry words\n", checked, structured, patched, words_packed);
    return 0;
}
