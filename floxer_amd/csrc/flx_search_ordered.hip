// K1' for gfx950: the FM-index walk in the reference's own order of discovery (fm_search_ordered_kernel). The default walk is in
// flx_fm_core.hpp / flx_search.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "flx_internal.hpp"

namespace flx {

// ================================================================================================ K1: FM search, the reference's order
// The default walk (error children first, stack in LDS, presence filter, one-row subtrees against the text) is in flx_fm_core.hpp /
// flx_search.hip. fm_search_ordered_kernel below walks the DFS of search_ng21 in the reference's own order with an explicit stack in
// HBM: for first_reported (the first n rows in emission order) and the raw-emission test hook, where the order of discovery itself
// is the result. One lane serves one seed; a rank query reads one 32-byte block (32 BWT positions: five absolute counters + three
// bit-planes) with two 16-byte loads and pop-counts the positions below the offset.

// r[c] = number of symbol c in bwt[0, pos) for c = 0..4
__device__ __forceinline__ void rank5(const OccBlock* __restrict__ tab, u32 pos, u32 r[5]) {
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(tab + (pos >> 5));
    uint4 const a = q[0], b = q[1];
    u32 const mask = (1u << (pos & 31u)) - 1u;
    u32 const p0 = b.y, p1 = b.z, p2 = b.w;
    u32 const n2 = ~p2 & mask;
    r[0] = a.x + (u32)__popc(n2 & ~(p1 | p0));
    r[1] = a.y + (u32)__popc(n2 & ~p1 & p0);
    r[2] = a.z + (u32)__popc(n2 & p1 & ~p0);
    r[3] = a.w + (u32)__popc(n2 & p1 & p0);
    r[4] = b.x + (u32)__popc(p2 & mask & ~(p1 | p0));
}

// both ends of the interval [lo, lo + nlen): cl[c] = rows of the child of symbol c (c = 0..5), ab[c] = its lower bound on the
// extended side (symbol 0, the sequence delimiter, is only ever a match child: a read holding the character '$', input.cpp:165-176)
__device__ __forceinline__ void extend_all(const DevIndex& idx, const OccBlock* __restrict__ tab, u32 lo, u32 nlen, u32 ab[6], u32 cl[6]) {
    u32 ra[5], rb[5];
    rank5(tab, lo, ra);
    rank5(tab, lo + nlen, rb);
    u32 sum_a = 0, sum_l = 0;
#pragma unroll
    for (u32 c = 0; c < 5; ++c) { cl[c] = rb[c] - ra[c]; sum_a += ra[c]; sum_l += cl[c]; }
    cl[5] = nlen - sum_l;
    ab[0] = ra[0];                                                    // C[0] = 0
#pragma unroll
    for (u32 c = 1; c < 5; ++c) ab[c] = idx.C[c] + ra[c];
    ab[5] = idx.C[5] + (lo - sum_a);
}

// frame state word: x:20 | e:3 | linfo:2 | rinfo:2 | next_sym:3 | right:1
enum : u32 { INFO_M = 0, INFO_I = 1, INFO_D = 2, INFO_S = 3 };
__device__ __forceinline__ u32 st_pack(u32 x, u32 e, u32 li, u32 ri, u32 sym, u32 right) {
    return x | (e << 20) | (li << 23) | (ri << 25) | (sym << 27) | (right << 30);
}
#define ST_X(s) ((s) & 0xFFFFFu)
#define ST_E(s) (((s) >> 20) & 7u)
#define ST_LI(s) (((s) >> 23) & 3u)
#define ST_RI(s) (((s) >> 25) & 3u)
#define ST_SYM(s) (((s) >> 27) & 7u)
#define ST_RIGHT(s) (((s) >> 30) & 1u)

__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (u32)__shfl_xor((int)v, off);
    return v;
}

// counters: [0] hit slots reserved, [1] stack overflow flag, [2] cursor extensions (rank pairs), [3] unused,
//           [4] wave-iterations, [5] max iterations of a wave, [6] busy lane-iterations, [7] seed queue head,
//           [8] wave-iterations after the seed queue ran dry, [9] their maximum over the waves
//
// DFS sizes differ by orders of magnitude between seeds, so neither lanes nor waves are bound to seeds: the launch is a fixed
// number of waves, a wave takes FM_GRAB consecutive seeds at a time from a global counter (counters[7]) and hands them to its lanes
// as they finish (wave-uniform bookkeeping in scalar registers). One loop iteration = one DFS step of every busy lane (at most one
// rank pair), which keeps the divergent part of the loop short.
constexpr u32 FM_GRAB = 64;
constexpr u32 FM_HIT_GRAB = 64;
constexpr u32 FM_MAX_WAVES = 4096;
constexpr u32 FM_SEEDS_PER_WAVE = 256;      // a launch has at most n_seeds / this many waves, so that every wave gets several ranges
constexpr u32 FM_KEY_MAX_X = 0x3FFFu;

// hit slots for the hits the lanes found in the last iteration. Slots are reserved FM_HIT_GRAB at a time per wave (one global
// atomic per range instead of one per hit, all on one address); the unused rest of a range is filled with entries of seed
// 0xFFFFFFFF, which the consumers skip. The hit's ordinal within its seed (the order the kernel found them in) rides in the upper
// bits of the error count (errors <= 3): the hits of a seed are put into one segment without a sort.
#define FM_EMIT_HITS()                                                                                                              \
    do {                                                                                                                            \
        u64 const emit = __ballot(hit_pending);                                                                                     \
        if (emit) {                                                                                                                 \
            u32 const n_emit = (u32)__popcll(emit);                                                                                 \
            if (h_end - h_next < n_emit) {                                                                                          \
                { u32 const at = h_next + lane; if (at < h_end && at < hit_cap) hits[at] = DevHit{0xFFFFFFFFu, 0u, 0u, 0u, 0ull}; } \
                u32 b = 0;                                                                                                          \
                if (lane == 0) b = atomicAdd(&counters[0], FM_HIT_GRAB);                                                            \
                h_next = (u32)__builtin_amdgcn_readfirstlane((int)b);                                                               \
                h_end = h_next + FM_HIT_GRAB;                                                                                       \
            }                                                                                                                       \
            if (hit_pending) {                                                                                                      \
                u32 const slot = h_next + (u32)__popcll(emit & lanes_below);                                                        \
                if (slot < hit_cap) hits[slot] = DevHit{sid, nlb, hit_rep, seed_cnt ? ne | (min(hit_idx, 0xFFFFFFu) << 8) : ne, hit_key}; \
                if (seed_cnt) seed_cnt[sid] = hit_idx + 1u;                                                                         \
                ++hit_idx;                                                                                                          \
            }                                                                                                                       \
            h_next += n_emit;                                                                                                       \
            hit_pending = false;                                                                                                    \
        }                                                                                                                           \
    } while (0)

// seeds for the idle lanes: k = index of this lane's new seed or 0xFFFFFFFF (wave-uniform bookkeeping of the grabbed range)
#define FM_ASSIGN_SEEDS(k)                                                                                                          \
    do {                                                                                                                            \
        u32 const n_idle = (u32)__popcll(idle);                                                                                     \
        u32 const avail = q_end - q_next;                                                                                           \
        u32 new_base = 0;                                                                                                           \
        bool grabbed = false;                                                                                                       \
        if (avail < n_idle && !queue_done) {                                                                                        \
            u32 b = 0;                                                                                                              \
            if (lane == 0) b = atomicAdd(&counters[7], FM_GRAB);                                                                    \
            new_base = (u32)__builtin_amdgcn_readfirstlane((int)b);                                                                 \
            grabbed = true;                                                                                                         \
        }                                                                                                                           \
        u32 const r = (u32)__popcll(idle & lanes_below);                                                                            \
        if (want) {                                                                                                                 \
            if (r < avail) k = q_next + r;                                                                                          \
            else if (grabbed && new_base + (r - avail) < n_seeds) k = new_base + (r - avail);                                       \
        }                                                                                                                           \
        if (grabbed) {                                                                                                              \
            if (new_base >= n_seeds) { q_next = 0; q_end = 0; queue_done = true; }                                                  \
            else {                                                                                                                  \
                q_end = min(new_base + FM_GRAB, n_seeds);                                                                           \
                q_next = min(new_base + (n_idle - avail), q_end);                                                                   \
                queue_done = new_base + FM_GRAB >= n_seeds;                                                                         \
            }                                                                                                                       \
        } else q_next += min(n_idle, avail);                                                                                        \
    } while (0)

// start of search `srch` of the seed: the root cursor, or the cursor of the seed's first KMER_Q characters when the search begins
// with an exact, rightward part that long and free of N. false: the search finds nothing.
__device__ __forceinline__ bool fm_begin_search(DevIndex const& idx, const u64* __restrict__ ex, const u8* __restrict__ q, u32 len,
                                                u32& nlb, u32& nlbr, u32& nlen, u32& nx) {
    nlb = 0; nlbr = 0; nlen = idx.n; nx = 0;
    if (len >= KMER_Q && ((ex[KMER_Q - 1] >> 27) & 1u)) {
        u32 const p0 = (u32)ex[0] & SCH_POS_MASK;
        u32 w[2];
        __builtin_memcpy(w, q + p0, 8);                                  // eight ranks, first character in the low byte
        u32 const t0 = w[0] - 0x01010101u, t1 = w[1] - 0x01010101u;      // A,C,G,T -> 0..3; anything else leaves bits 2..7 set
        if (((t0 | t1) & 0xFCFCFCFCu) == 0u) {
            // gather the four 2-bit fields of a word, first character most significant: b0<<6 | b1<<4 | b2<<2 | b3
            u32 const code = (((t0 * 0x40100401u) >> 24) << 8) | ((t1 * 0x40100401u) >> 24);
            const u32* __restrict__ e = idx.kmer + 3u * code;
            nlb = e[0]; nlbr = e[1]; nlen = e[2];
            nx = KMER_Q;
            if (nlen == 0) return false;
        }
    }
    return true;
}

// the children of a branching node that exist: bit 0 match, bits 2c-1 / 2c deletion / substitution of symbol c, bit 11 insertion
__device__ __forceinline__ u32 fm_child_mask(const u32 cl[6], u32 next_sym, bool match_allowed, bool deletion, bool insertion) {
    u32 mask = 0;
#pragma unroll
    for (u32 c = 1; c < 6; ++c) {
        if (cl[c] > 0u) {
            if (deletion) mask |= 1u << (2u * c - 1u);
            if (c != next_sym) mask |= 1u << (2u * c);
            else if (match_allowed) mask |= 1u;
        }
    }
    if (next_sym == 0u && match_allowed && cl[0] > 0u) mask |= 1u;      // a '$' of the query matches a sequence delimiter
    if (insertion) mask |= 1u << 11;
    return mask;
}

// The DFS in the reference's own order (match child first): frames are written to the seed's stack in HBM when they are made
// (64 B = four 16-byte stores) and read back when the DFS returns to them; the children of the top frame are in LDS.
__global__ void __launch_bounds__(64) fm_search_ordered_kernel(DevIndex idx, const u8* __restrict__ seq, const u64* __restrict__ scheme,
                                                               const DevSeed* __restrict__ seeds, u32 n_seeds, u32 max_hits,
                                                               DevFrame* __restrict__ stack, DevHit* __restrict__ hits, u32 hit_cap,
                                                               u32* __restrict__ counters, u32* __restrict__ seed_cnt) {
    __shared__ uint4 child[6][64];              // top frame: {abs, oth, len, -} of the child cursor of symbol s+1 (entry 5: symbol 0), per lane
    u32 q_next = 0, q_end = 0;
    bool queue_done = false;
    u32 h_next = 0, h_end = 0;
    u32 const lane = threadIdx.x & 63u;
    u64 const lanes_below = (1ull << lane) - 1ull;

    u32 n_ext = 0, n_iter = 0, n_busy_iter = 0, n_tail_iter = 0;
    bool busy = false, exhausted = false;
    u32 sid = 0, srch = 0, num_searches = 0, len = 0, ct = 0, stack_frames = 0;
    const u8* __restrict__ q = seq;
    uint4* __restrict__ stk = reinterpret_cast<uint4*>(stack);
    const u64* __restrict__ ex_base = scheme;
    bool in_search = false;
    const u64* __restrict__ ex = scheme;
    u32 l_last = 0, u_last = 0;
    u32 nlb = 0, nlbr = 0, nlen = 0, nx = 0, ne = 0, nli = INFO_M, nri = INFO_M;
    // top frame (frame depth-1 of the stack): its node and the mask of children not taken yet
    u32 f_lb = 0, f_lbr = 0, f_len = 0, f_state = 0, f_mask = 0;
    u32 depth = 0;                              // frames on the stack, the top one included
    bool need_child = false;
    bool hit_pending = false;
    u32 hit_rep = 0, hit_idx = 0;
    u64 const hit_key = 0;                      // the ordinals of this kernel's hits are the emission order

    while (true) {
        FM_EMIT_HITS();
        bool const want = !busy && !exhausted;
        u64 const idle = __ballot(want);
        if (idle) {                                                     // wave-uniform
            u32 k = 0xFFFFFFFFu;
            FM_ASSIGN_SEEDS(k);
            if (want) {
                if (k != 0xFFFFFFFFu) {
                    DevSeed const seed = seeds[k];
                    sid = seed.id;
                    q = seq + seed.seq_off;
                    stk = reinterpret_cast<uint4*>(stack + seed.stack_off);
                    len = seed.length;
                    num_searches = seed.frames_searches >> 24;
                    stack_frames = seed.frames_searches & 0xFFFFFFu;
                    ex_base = scheme + seed.scheme_off;
                    srch = 0; ct = 0; hit_idx = 0;
                    busy = true;
                    in_search = false;
                } else exhausted = true;
            }
        }
        if (__all(exhausted && !busy)) break;
        ++n_iter;
        if (queue_done && q_next == q_end) ++n_tail_iter;
        if (!busy) continue;
        ++n_busy_iter;

        if (!in_search) {
            if (srch >= num_searches) { busy = false; continue; }
            ex = ex_base + (u64)srch * len;
            u32 const last_entry = (u32)ex[len - 1];
            l_last = (last_entry >> 20) & 7u;
            u_last = (last_entry >> 23) & 7u;
            ne = 0; nli = INFO_M; nri = INFO_M;
            f_mask = 0;
            depth = 0;
            need_child = false;
            in_search = true;
            if (!fm_begin_search(idx, ex, q, len, nlb, nlbr, nlen, nx)) { in_search = false; ++srch; continue; }
        }

        // ---- one DFS step
        if (need_child) {
            if (f_mask == 0u) {
                // the top frame has no child left (or there is no frame): back to the frame below it
                if (depth <= 1u) { in_search = false; ++srch; continue; }    // search exhausted
                --depth;
                const uint4* __restrict__ g = stk + (depth - 1u) * 4u;
                uint4 const v0 = g[0], v1 = g[1], v2 = g[2], v3 = g[3];
                f_lb = v2.w; f_lbr = v3.x; f_state = v3.z;
                f_mask = v3.w;                                             // never empty: see where frames are made
                // bounds of the children on the other side: prefix sums of their lengths, symbol 0 first
                u32 const o0 = ST_RIGHT(f_state) ? f_lb : f_lbr;
                u32 const o1 = o0 + v1.y;
                u32 const o2 = o1 + v1.z, o3 = o2 + v1.w, o4 = o3 + v2.x, o5 = o4 + v2.y;
                f_len = o5 + v2.z - o0;                                    // the children's rows are the node's
                child[0][lane] = uint4{v0.x, o1, v1.z, 0u};
                child[1][lane] = uint4{v0.y, o2, v1.w, 0u};
                child[2][lane] = uint4{v0.z, o3, v2.x, 0u};
                child[3][lane] = uint4{v0.w, o4, v2.y, 0u};
                child[4][lane] = uint4{v1.x, o5, v2.z, 0u};
                child[5][lane] = uint4{v3.y, o0, v1.y, 0u};
            }
            u32 const ci = (u32)__ffs((int)f_mask) - 1u;
            f_mask &= f_mask - 1u;
            u32 const st = f_state;
            u32 const right = ST_RIGHT(st);
            u32 const px = ST_X(st), pe = ST_E(st);
            u32 info, sym;
            if (ci == 0) { sym = ST_SYM(st); nx = px + 1; ne = pe; info = INFO_M; }
            else if (ci == 11) { sym = 1; nx = px + 1; ne = pe + 1; info = INFO_I; }
            else {
                sym = (ci + 1) >> 1;
                bool const del = ci & 1u;
                nx = del ? px : px + 1;
                ne = pe + 1;
                info = del ? INFO_D : INFO_S;
            }
            uint4 const c = child[sym ? sym - 1u : 5u][lane];              // sym is 1..5 for every child but the match of a '$'
            if (ci == 11) { nlb = f_lb; nlbr = f_lbr; nlen = f_len; }
            else { nlen = c.z; nlb = right ? c.y : c.x; nlbr = right ? c.x : c.y; }
            nli = right ? ST_LI(st) : info;
            nri = right ? info : ST_RI(st);
            need_child = false;
        }

        // ---- inspect node (nlb, nlbr, nlen, nx, ne, nli, nri); nlen > 0 by construction
        if (nx == len) {
            bool const ok_l = nli == INFO_M || nli == INFO_I, ok_r = nri == INFO_M || nri == INFO_I;
            if (ok_l && ok_r && l_last <= ne && ne <= u_last) {
                u32 rep = nlen;
                if (ct + rep > max_hits) rep = max_hits - ct;        // search_n truncates the last cursor
                ct += rep;
                hit_pending = true;                                  // written at the top of the next iteration
                hit_rep = rep;
                if (ct == max_hits) { busy = false; continue; }      // search_n aborts all remaining searches of the seed
            }
            need_child = true;
            continue;
        }
        u32 const sch = (u32)ex[nx];
        u32 const lower = (sch >> 20) & 7u, upper = (sch >> 23) & 7u, right = (sch >> 26) & 1u;
        if (ne > upper) { need_child = true; continue; }
        bool const mismatch_allowed = lower <= ne + 1 && ne + 1 <= upper;
        bool const match_allowed = lower <= ne && ne <= upper;
        if (!mismatch_allowed && !match_allowed) { need_child = true; continue; }

        u32 const next_sym = q[sch & SCH_POS_MASK];
        u32 const lo = right ? nlbr : nlb, other = right ? nlb : nlbr;
        u32 ab[6], cl[6];
        extend_all(idx, idx.occ[right], lo, nlen, ab, cl);
        ++n_ext;

        if (mismatch_allowed) {
            // this node branches: it becomes the top frame. The frame below keeps its place on the stack if it still has children
            // (its mask is brought up to date), else its place is taken.
            if (depth > 0u) {
                if (f_mask != 0u) reinterpret_cast<u32*>(stk + (depth - 1u) * 4u)[15] = f_mask;
                else --depth;
            }
            if (depth >= stack_frames) { atomicOr(&counters[1], 1u); busy = false; continue; }
            u32 const tinfo = right ? nri : nli;
            f_lb = nlb; f_lbr = nlbr; f_len = nlen;
            f_state = st_pack(nx, ne, nli, nri, next_sym, right);
            f_mask = fm_child_mask(cl, next_sym, match_allowed, tinfo == INFO_M || tinfo == INFO_D, tinfo == INFO_M || tinfo == INFO_I);
            uint4* __restrict__ g = stk + depth * 4u;
            g[0] = uint4{ab[1], ab[2], ab[3], ab[4]};
            g[1] = uint4{ab[5], cl[0], cl[1], cl[2]};
            g[2] = uint4{cl[3], cl[4], cl[5], nlb};
            g[3] = uint4{nlbr, ab[0], f_state, f_mask};
            ++depth;
            u32 const o1 = other + cl[0], o2 = o1 + cl[1], o3 = o2 + cl[2], o4 = o3 + cl[3], o5 = o4 + cl[4];
            child[0][lane] = uint4{ab[1], o1, cl[1], 0u};
            child[1][lane] = uint4{ab[2], o2, cl[2], 0u};
            child[2][lane] = uint4{ab[3], o3, cl[3], 0u};
            child[3][lane] = uint4{ab[4], o4, cl[4], 0u};
            child[4][lane] = uint4{ab[5], o5, cl[5], 0u};
            child[5][lane] = uint4{ab[0], other, cl[0], 0u};
            need_child = true;
        } else {
            // only an exact extension is possible: continue in place (no frame)
            if (next_sym > 5u) { need_child = true; continue; }
            u32 clen = cl[0], cabs = ab[0], coth = other;
#pragma unroll
            for (u32 c = 1; c < 6; ++c) {
                coth += c <= next_sym ? cl[c - 1u] : 0u;
                bool const take = c == next_sym;
                clen = take ? cl[c] : clen;
                cabs = take ? ab[c] : cabs;
            }
            if (clen == 0) { need_child = true; continue; }
            nlb = right ? coth : cabs;
            nlbr = right ? cabs : coth;
            if (right) nri = INFO_M; else nli = INFO_M;
            nlen = clen;
            nx = nx + 1;
        }
    }
    { u32 const at = h_next + lane; if (at < h_end && at < hit_cap) hits[at] = DevHit{0xFFFFFFFFu, 0u, 0u, 0u, 0ull}; }
    n_ext = wave_sum_u32(n_ext);
    n_busy_iter = wave_sum_u32(n_busy_iter);
    if (lane == 0) {
        atomicAdd(&counters[2], n_ext); atomicAdd(&counters[6], n_busy_iter);
        atomicAdd(&counters[4], n_iter); atomicMax(&counters[5], n_iter); atomicAdd(&counters[8], n_tail_iter); atomicMax(&counters[9], n_tail_iter);
    }
}
#undef FM_EMIT_HITS
#undef FM_ASSIGN_SEEDS

static u32 fm_seeds_per_wave() {
    static u32 const v = [] { const char* e = getenv("FLX_FM_SEEDS_PER_WAVE"); u32 const x = e ? (u32)strtoul(e, nullptr, 10) : 0u; return x ? x : FM_SEEDS_PER_WAVE; }();
    return v;
}

u32 fm_search_max_keyed_length() { return FM_KEY_MAX_X; }

// the walk in the reference's order (fm_search_ordered_kernel); the default walk is DeviceApi::search_filtered (flx_search.hip)
int DeviceApi::search(void* stream, const DevIndex& idx, const u8* d_seq, const u64* d_scheme, const DevSeed* d_seeds, u32 n_seeds,
                      u32 max_hits_per_seed, DevFrame* d_stack, DevHit* d_hits, u32 hit_cap, u32* d_counters, u32* d_seed_cnt) {
    if (n_seeds == 0) return 0;
    if (!d_stack) return (int)hipErrorInvalidValue;
    u32 const spw = fm_seeds_per_wave();
    dim3 const grid(std::min<u32>((n_seeds + spw - 1) / spw, FM_MAX_WAVES));
    hipLaunchKernelGGL(fm_search_ordered_kernel, grid, dim3(64), 0, (hipStream_t)stream, idx, d_seq, d_scheme, d_seeds, n_seeds,
                       max_hits_per_seed, d_stack, d_hits, hit_cap, d_counters, d_seed_cnt);
    return (int)hipGetLastError();
}

}  // namespace flx
