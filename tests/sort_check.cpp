// flx_sort.hpp alone, under ASan + UBSan (built and run by tests/test_sort_host.py): key packing at the extremes, every case of a
// record's end, every refusal of sort_plan, the digits of a key against a byte walk, the order against a brute-force comparison,
// reg2bin against the definition, and the rule that keeps the digit table within two scan levels.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../include/floxer_amd.h"
#include "../floxer_amd/csrc/flx_sort.hpp"

using namespace flx;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static flx_record record(uint32_t flag, int32_t ref, int32_t pos, uint64_t off, uint32_t len) {
    flx_record r{};
    r.flag = flag; r.reference_id = ref; r.position = pos; r.cigar_offset = off; r.cigar_length = len;
    return r;
}
static uint32_t word(char op, uint32_t n) {
    uint32_t const code = op == '=' ? 7u : op == 'X' ? 8u : op == 'I' ? 1u : op == 'D' ? 2u : op == 'S' ? 4u : op == 'M' ? 0u : 5u;
    return n << 4 | code;
}

struct Plan { bool ok; std::vector<SortKey> keys; std::vector<SortMeta> meta; std::string error; };
static Plan plan(uint32_t n_refs, std::vector<flx_record> const& recs, std::vector<uint32_t> const& words, uint64_t first, const uint64_t* ordinals = nullptr) {
    Plan p;
    // something in front: a refusal must leave it alone
    p.keys.push_back(SortKey{1, 2});
    p.meta.push_back(SortMeta{3, 4});
    p.ok = sort_plan(n_refs, recs.data(), recs.size(), words.empty() ? nullptr : words.data(), words.size(), first, ordinals, "check", p.keys, p.meta, &p.error);
    CHECK(p.keys.size() == p.meta.size());
    CHECK(p.keys[0].hi == 1 && p.keys[0].lo == 2 && p.meta[0].end == 3 && p.meta[0].flag == 4);
    if (!p.ok) { CHECK(p.keys.size() == 1); CHECK(!p.error.empty()); }
    else CHECK(p.keys.size() == 1 + recs.size());
    return p;
}

int main() {
    // ---- key packing at the extremes
    {
        SortKey const k = sort_key(0, 0, 0, 0);
        CHECK(k.hi == 0 && k.lo == 0);
        SortKey const top = sort_key(16, 0x7FFFFFFF, 0x7FFFFFFE, SORT_MAX_ORDINAL - 1);
        CHECK(top.hi == (0x7FFFFFFFull << 32 | 0x7FFFFFFEull) && top.lo == ~0ull);
        CHECK(sort_key_ordinal(top) == SORT_MAX_ORDINAL - 1 && sort_key_reference(top) == 0x7FFFFFFF && sort_key_position(top) == 0x7FFFFFFE);
        SortKey const un = sort_key(4, 3, 17, 5), neg = sort_key(0, -1, -1, 6);
        CHECK(un.hi == (0xFFFFFFFFull << 32 | 17ull) && un.lo == 5);
        CHECK(neg.hi == ~0ull && neg.lo == 6 && sort_key_reference(neg) == -1 && sort_key_position(neg) == -1);
        CHECK(sort_key_less(top, un) && !sort_key_less(un, top) && !sort_key_less(un, un));
        // forward before reverse at one place, whatever the ordinals; the ordinal behind the strand
        CHECK(sort_key_less(sort_key(0, 1, 9, 1000), sort_key(16, 1, 9, 0)));
        CHECK(sort_key_less(sort_key(272, 1, 9, 0), sort_key(2064, 1, 9, 1)));
        CHECK(sort_key_less(sort_key(16, 1, 9, 5), sort_key(0, 1, 10, 0)));
        CHECK(sort_key_less(sort_key(16, 1, 0x7FFFFFFE, 5), sort_key(0, 2, 0, 0)));
        // the digits are the key's bytes, least significant first
        SortKey const d = SortKey{0x0F0E0D0C0B0A0908ull, 0x0706050403020100ull};
        for (uint32_t i = 0; i < SORT_DIGITS; ++i) CHECK(sort_digit(d, i) == i);
    }
    // ---- every case of end
    {
        CHECK(sort_end(false, 0, 0) == 1);                   // a mapped record without words
        CHECK(sort_end(false, 10, 1) == 11 && sort_end(false, 10, 7) == 17);
        CHECK(sort_end(false, 0x7FFFFFFE, 1) == 0x7FFFFFFFull);
        CHECK(sort_end(true, 10, 99) == 11);                 // an unplaced one: its words do not count
        CHECK(sort_end(true, -1, 0) == 0x100000000ull);
        std::vector<uint32_t> const words{word('S', 5), word('=', 10), word('I', 3), word('X', 2), word('D', 4), word('S', 1), word('I', 2)};
        Plan const p = plan(2, {record(0, 1, 100, 0, 6), record(16, 0, 7, 6, 1), record(0, 0, 7, 0, 0), record(4, -1, 0, 0, 0), record(4, 1, 50, 0, 6)}, words, 10);
        CHECK(p.ok);
        if (p.ok) {
            CHECK(p.meta[1].end == 116 && p.meta[1].flag == 0);
            CHECK(p.meta[2].end == 8 && p.meta[2].flag == 16);   // only an insertion: span 0
            CHECK(p.meta[3].end == 8);
            CHECK(p.meta[4].end == 1 && p.meta[5].end == 51);
            CHECK(p.keys[1].lo == 10 && p.keys[2].lo == (1ull << 63 | 11) && p.keys[5].lo == 14 && p.keys[5].hi == (0xFFFFFFFFull << 32 | 50));
        }
    }
    // ---- refusals
    {
        std::vector<uint32_t> const words{word('=', 10), word('M', 3), word('=', 0), word('=', 0x7FFFFFF), word('D', 0xFFFFFFF)};
        CHECK(plan(2, {record(0, 1, 0, 0, 1)}, words, 0).ok);
        CHECK(!plan(2, {record(0, 2, 0, 0, 1)}, words, 0).ok);                     // reference_id >= n_refs
        CHECK(!plan(0, {record(0, 0, 0, 0, 0)}, words, 0).ok);
        CHECK(plan(0, {record(4, 5, 0, 0, 0)}, words, 0).ok);                      // an unplaced record names no reference
        CHECK(!plan(2, {record(0, 1, -1, 0, 1)}, words, 0).ok);                    // position < 0
        CHECK(!plan(2, {record(0, 1, 0, 0, 2)}, words, 0).ok);                     // an op other than = X I D S
        CHECK(!plan(2, {record(0, 1, 0, 2, 1)}, words, 0).ok);                     // a zero-length word
        CHECK(!plan(2, {record(0, 1, 0, 5, 1)}, words, 0).ok);                     // words behind the pool
        CHECK(!plan(2, {record(0, 1, 0, 4, 2)}, words, 0).ok);
        CHECK(!plan(2, {record(0, 1, 0, ~0ull, 2)}, words, 0).ok);
        CHECK(!plan(2, {record(0, 1, 0, 0, 1)}, {}, 0).ok);                        // no pool at all
        CHECK(plan(2, {record(0, 1, 0, 5, 0)}, words, 0).ok);                      // no words: the offset is not read
        CHECK(plan(2, {record(0, 1, 0x7FFFFFFE, 0, 0)}, words, 0).ok);             // end = 2^31 - 1
        CHECK(!plan(2, {record(0, 1, 0x7FFFFFFF, 0, 0)}, words, 0).ok);            // end = 2^31
        CHECK(plan(2, {record(0, 1, 0x7FFFFFFF - 10, 0, 1)}, words, 0).ok);
        CHECK(!plan(2, {record(0, 1, 0x7FFFFFFF - 9, 0, 1)}, words, 0).ok);
        // spans beyond 32 bits are summed in 64: sixteen words of 2^28 - 1 columns
        std::vector<uint32_t> const big(20, word('D', 0xFFFFFFF));
        CHECK(!plan(2, {record(0, 1, 0, 0, 20)}, big, 0).ok);
        CHECK(plan(2, {record(0, 1, 0, 0, 7)}, big, 0).ok && !plan(2, {record(0, 1, 0, 0, 9)}, big, 0).ok);
        CHECK(plan(2, {record(0, 1, 0, 0, 1)}, words, SORT_MAX_ORDINAL - 1).ok);   // ordinals
        CHECK(!plan(2, {record(0, 1, 0, 0, 1)}, words, SORT_MAX_ORDINAL).ok);
        CHECK(!plan(2, {record(0, 1, 0, 0, 1), record(0, 1, 0, 0, 1)}, words, SORT_MAX_ORDINAL - 1).ok);
        uint64_t const given[2] = {7, SORT_MAX_ORDINAL};
        CHECK(!plan(2, {record(0, 1, 0, 0, 1), record(0, 1, 0, 0, 1)}, words, 0, given).ok);
        // a refusal behind good records takes them back
        CHECK(!plan(2, {record(0, 1, 0, 0, 1), record(0, 0, 5, 0, 1), record(0, 1, 0, 1, 1)}, words, 0).ok);
    }
    // ---- the order on random keys against a comparison of the fields
    {
        std::mt19937_64 rng(7);
        struct Row { uint32_t flag; int32_t ref, pos; uint64_t ordinal; };
        std::vector<Row> rows(3000);
        int32_t const positions[] = {0, 1, 255, 256, 65535, 65536, 0x7FFFFFFE};
        uint32_t const flags[] = {0, 16, 256, 272, 4, 2048, 2064, 20};
        for (auto& r : rows) r = Row{flags[rng() % 8], (int32_t)(rng() % 4) - 1, positions[rng() % 7], rng() >> 1 >> (rng() % 3 ? 40 : 0)};
        auto less = [](Row const& a, Row const& b) {
            bool const ua = (a.flag & 4) || a.ref < 0, ub = (b.flag & 4) || b.ref < 0;
            if (ua != ub) return ub;
            if (!ua && a.ref != b.ref) return a.ref < b.ref;
            if ((uint32_t)a.pos != (uint32_t)b.pos) return (uint32_t)a.pos < (uint32_t)b.pos;
            if (((a.flag >> 4) & 1) != ((b.flag >> 4) & 1)) return ((a.flag >> 4) & 1) < ((b.flag >> 4) & 1);
            return a.ordinal < b.ordinal;
        };
        for (size_t i = 0; i + 1 < rows.size(); ++i) {
            Row const &a = rows[i], &b = rows[i + 1];
            CHECK(sort_key_less(sort_key(a.flag, a.ref, a.pos, a.ordinal), sort_key(b.flag, b.ref, b.pos, b.ordinal)) == less(a, b));
        }
        // sixteen stable passes over the digits, least significant first, give that order
        std::vector<SortKey> keys;
        for (auto const& r : rows) keys.push_back(sort_key(r.flag, r.ref, r.pos, r.ordinal));
        std::vector<SortKey> radix = keys, want = keys;
        for (uint32_t d = 0; d < SORT_DIGITS; ++d) std::stable_sort(radix.begin(), radix.end(), [d](SortKey const& a, SortKey const& b) { return sort_digit(a, d) < sort_digit(b, d); });
        std::stable_sort(want.begin(), want.end(), sort_key_less);
        for (size_t i = 0; i < keys.size(); ++i) CHECK(radix[i].hi == want[i].hi && radix[i].lo == want[i].lo);
    }
    // ---- reg2bin: the smallest bin whose interval holds [beg, end)
    {
        std::mt19937_64 rng(11);
        int64_t const edges[] = {0, 1, 16383, 16384, 16385, 1 << 17, (1 << 17) + 1, 1 << 20, 1 << 23, 1 << 26, (1 << 29) - 1};
        auto brute = [](int64_t beg, int64_t end) {
            int const shifts[] = {14, 17, 20, 23, 26};
            uint32_t const firsts[] = {4681, 585, 73, 9, 1};
            for (int l = 0; l < 5; ++l) if (beg >> shifts[l] == (end - 1) >> shifts[l]) return firsts[l] + (uint32_t)(beg >> shifts[l]);
            return 0u;
        };
        for (int64_t a : edges) for (int64_t b : edges) if (a < b) CHECK(reg2bin(a, b) == brute(a, b));
        for (int i = 0; i < 20000; ++i) {
            int64_t const a = (int64_t)(rng() % (1ull << 29)), b = std::min<int64_t>(a + 1 + (int64_t)(rng() % (1ull << (rng() % 28))), 1ll << 29);
            CHECK(reg2bin(a, b) == brute(a, b));
        }
        CHECK(reg2bin(0, 1) == 4681 && reg2bin(16383, 16385) == 585 && reg2bin(0, 1 << 29) == 0 && reg2bin((1 << 29) - 1, 1 << 29) == 37448);
    }
    // ---- the digit table stays within two scan levels
    {
        uint64_t const block = 256, scan = 4096, max_tiles = scan * scan / SORT_RADIX;
        uint64_t const sizes[] = {0, 1, 255, 2048, 2049, max_tiles * 2048, max_tiles * 2048 + 1, max_tiles * 2304, max_tiles * 2304 + 1, (1ull << 32) - 1};
        for (uint64_t n : sizes)
            for (uint64_t tile : {256ull, 2048ull, 4096ull}) {
                uint64_t const t = sort_effective_tile(n, tile, block, scan);
                CHECK(t >= tile && t % block == 0 && (n + t - 1) / t <= max_tiles);
                CHECK(t == tile || (n + (t - block) - 1) / (t - block) > max_tiles);      // grown no further than needed
                CHECK(t < (1ull << 32));
            }
        CHECK(sort_effective_tile(max_tiles * 2048, 2048, block, scan) == 2048 && sort_effective_tile(max_tiles * 2048 + 1, 2048, block, scan) == 2304);
    }
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("ok sort_check\n");
    return 0;
}
