// Read-backed phasing on the device (the rule: flx_phase.hpp; the object and the C ABI: flx_phase_api.cpp). Wave64 integer work:
//   phase_observe    the hot path, in every add: one wave per counted record, 64 CIGAR words per pass, the walk of variants_indel_keys
//                    (prefix sums over columns and rows, position and row carried wave-uniform across passes; that walk's any_before
//                    carry has no reader here: an I or D word is only looked at from a column of its own record in front of it, so it
//                    is always preceded). The lane whose word owns the column of an anchor writes the slots of every site anchored
//                    there: a lower bound into the record's stretch of the anchors, then the sites while they lie inside the word.
//                    For an indel site on its word's last column it reads the words behind its own straight from memory while they
//                    are I or D, across the 64-word pass boundary where needed. An X word loads one letter per SNV site, an I word
//                    only the letters its key packs (and only when anchor, kind and length agree). A column belongs to one word: no
//                    two lanes share a slot, and every slot of the record is written once. A record without a slot is left at once.
//   phase_links      one thread per observation slot of the add: its record by a search over the records' first slots, then, with a
//                    successor in the same record and both REF or ALT, one add to cis or trans of its site. Needs the observations.
//   phase_chain      three steps with two ScanDriver sum scans between the first and the second: the flip and break flags per site
//                    (they need all links: the finish); the set starts scattered by their ordinal (they need the scanned breaks);
//                    p(i) as the parity of the flips since the set's start and the phased bit (they need the scattered starts).
//   phase_tags       one thread per record: phase_tag_record over its slots. Needs the chain, or the revote.
//   phase_votes      one thread per slot: keep or swap of its site from its record's tag. Needs the tags.
//   phase_revote     one thread per site: p flips where swap > keep. Needs all votes.
//   phase_results    one thread per site: the result row.
// Every dependence between these is a launch boundary. All adds are device-scope integer atomicAdd, all stores plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_scan_dev.hpp"
#include "flx_phase.hpp"

namespace flx {

// ------------------------------------------------------------------------------------------------ phase_observe
__global__ void __launch_bounds__(THREADS) phase_observe_kernel(const PileupJob* __restrict__ jobs, const PhaseRecord* __restrict__ recs, u32 n_jobs, const u32* __restrict__ words,
                                                                const u8* __restrict__ letters, const u32* __restrict__ anchors, const flx_phase_site* __restrict__ sites,
                                                                u8* __restrict__ obs) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * (THREADS / 64u);
    for (u32 id = blockIdx.x * (THREADS / 64u) + (threadIdx.x >> 6); id < n_jobs; id += waves) {       // (id is wave-uniform)
        PhaseRecord const rec = recs[id];
        if (rec.n_slots == 0u) continue;                               // (wave-uniform: no site in the record's span)
        PileupJob const job = jobs[id];
        const u8* __restrict__ const seq = letters + job.seq_off;
        const u32* __restrict__ const mine = words + job.word_off;
        const u32* __restrict__ const my_anchors = anchors + rec.first;
        const flx_phase_site* __restrict__ const my_sites = sites + rec.first;
        u8* __restrict__ const out = obs + rec.obs_off;
        u64 pos = job.text_off, row = 0;                               // the wave-uniform carries: position and row behind the last pass
        for (u32 base = 0; base < job.n_words; base += 64u) {
            u32 const t = base + lane;
            u32 const word = t < job.n_words ? mine[t] : 0u;           // (op 0 consumes nothing and owns no column)
            u32 const op = word & 15u, len = word >> 4;
            u32 const cols = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            u32 const rows = (op == 7u || op == 8u || op == 1u || op == 4u) ? len : 0u;
            u32 const incl = wave_inclusive_scan(cols), incl_rows = wave_inclusive_scan(rows);
            if (cols)
                // (the host judged the record: the words behind this one end with n_words, the rows with the read; the host found the
                // slots: k < n_slots lies in the record's own stretch of the observations)
                phase_observe_word(rec.n_slots, op, len, pos + incl - cols, row + incl_rows - rows, rec.text_end, t, job.n_words, [&](u32 k) { return my_anchors[k]; },
                                   [&](u32 k) { return my_sites[k]; }, [&](u32 u) { return mine[u]; }, [&](u64 r) { return seq[r]; }, [&](u32 k, u32 o) { out[k] = (u8)o; });
            pos += __shfl(incl, 63);
            row += __shfl(incl_rows, 63);
        }
    }
}

// ------------------------------------------------------------------------------------------------ phase_links, phase_votes
// the record that holds slot g: the last one whose first slot is not behind g (a record without slots shares its first slot with its
// successor, so the last one has slots)
__device__ __forceinline__ u64 owner_of(const PhaseRecord* __restrict__ recs, u64 n_recs, u64 g) {
    u64 lo = 0, hi = n_recs;                                           // the answer lies in [lo, hi)
    while (hi - lo > 1u) {
        u64 const mid = lo + (hi - lo) / 2u;
        if (recs[mid].obs_off <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(THREADS) phase_links_kernel(const PhaseRecord* __restrict__ recs, u32 n_recs, u64 slot0, u64 n_slots, const u8* __restrict__ obs,
                                                              u32* __restrict__ cis, u32* __restrict__ trans) {
    u64 const i = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_slots) return;
    u64 const g = slot0 + i;
    PhaseRecord const rec = recs[owner_of(recs, n_recs, g)];
    u64 const k = g - rec.obs_off;
    if (k + 1u >= (u64)rec.n_slots) return;                            // (the record's last slot has no successor)
    u32 const a = obs[g], b = obs[g + 1u];
    if (a > PHASE_ALT || b > PHASE_ALT) return;
    atomicAdd((a == b ? cis : trans) + (rec.first + (u32)k), 1u);
}

__global__ void __launch_bounds__(THREADS) phase_votes_kernel(const PhaseRecord* __restrict__ recs, u64 n_recs, u64 n_slots, const u8* __restrict__ obs,
                                                              const u32* __restrict__ set, const u32* __restrict__ state, const flx_phase_tag* __restrict__ tags,
                                                              u32* __restrict__ keep, u32* __restrict__ swap) {
    u64 const g = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_slots) return;
    u64 const j = owner_of(recs, n_recs, g);
    PhaseRecord const rec = recs[j];
    u32 const s = rec.first + (u32)(g - rec.obs_off);
    u32 const v = phase_vote(tags[j].hap, tags[j].phase_set, obs[g], state[s], set[s]);
    if (v == 1u) atomicAdd(keep + s, 1u);
    else if (v == 2u) atomicAdd(swap + s, 1u);
}

// ------------------------------------------------------------------------------------------------ phase_chain
__global__ void __launch_bounds__(THREADS) phase_chain_flags_kernel(const flx_phase_site* __restrict__ sites, u32 n_sites, const u32* __restrict__ cis,
                                                                    const u32* __restrict__ trans, u32 min_link, u32* __restrict__ flips, u32* __restrict__ starts) {
    u64 const i64_ = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i64_ >= n_sites) return;
    u32 const i = (u32)i64_;
    bool joined = false, flip = false;
    if (i > 0u) {
        u32 const c = cis[i - 1u], t = trans[i - 1u];
        joined = phase_connected(c, t, sites[i - 1u].reference_id == sites[i].reference_id, min_link);
        flip = joined && phase_flip(c, t);
    }
    flips[i] = flip ? 1u : 0u;
    starts[i] = joined ? 0u : 1u;
}
// (flips and starts hold their inclusive sums: starts[i] is the 1-based ordinal of site i's set)
__global__ void __launch_bounds__(THREADS) phase_chain_scatter_kernel(u32 n_sites, const u32* __restrict__ starts, u32* __restrict__ set_start) {
    u64 const i64_ = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i64_ >= n_sites) return;
    u32 const i = (u32)i64_, ord = starts[i];
    if (i == 0u || starts[i - 1u] != ord) set_start[ord - 1u] = i;     // (one site per set stores: its first)
    if (i == n_sites - 1u) set_start[ord] = n_sites;                   // (the end behind the last set: ord <= n_sites entries before it)
}
__global__ void __launch_bounds__(THREADS) phase_chain_phase_kernel(u32 n_sites, const u32* __restrict__ flips, const u32* __restrict__ starts, const u32* __restrict__ set_start,
                                                                    u32* __restrict__ set, u32* __restrict__ state) {
    u64 const i64_ = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i64_ >= n_sites) return;
    u32 const i = (u32)i64_, ord = starts[i], first = set_start[ord - 1u], next = set_start[ord];
    set[i] = first;
    state[i] = ((flips[i] - flips[first]) & PHASE_BIT_P) | (next - first > 1u ? PHASE_BIT_PHASED : 0u);      // (the set's first site adds no flip of its own)
}

// ------------------------------------------------------------------------------------------------ phase_tags, phase_revote, phase_results
__global__ void __launch_bounds__(THREADS) phase_tags_kernel(const PhaseRecord* __restrict__ recs, u64 n_recs, const u8* __restrict__ obs, const u32* __restrict__ set,
                                                             const u32* __restrict__ state, u32 min_margin, flx_phase_tag* __restrict__ tags) {
    u64 const j = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (j >= n_recs) return;
    PhaseRecord const rec = recs[j];
    const u8* __restrict__ const mine = obs + rec.obs_off;
    flx_phase_tag t;
    t.add = rec.add; t.read = rec.read; t.n_slots = rec.n_slots; t.reserved = 0;
    phase_tag_record(rec.n_slots, min_margin, [&](u32 k) { return (u32)mine[k]; }, [&](u32 k) { return state[rec.first + k]; }, [&](u32 k) { return set[rec.first + k]; }, t.hap,
                     t.phase_set, t.h1, t.h2);
    tags[j] = t;
}
__global__ void __launch_bounds__(THREADS) phase_revote_kernel(u32 n_sites, const u32* __restrict__ keep, const u32* __restrict__ swap, u32* __restrict__ state) {
    u64 const i = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_sites) return;
    if (swap[i] > keep[i]) state[i] ^= PHASE_BIT_P;
}
__global__ void __launch_bounds__(THREADS) phase_results_kernel(u32 n_sites, const u32* __restrict__ set, const u32* __restrict__ state, const u32* __restrict__ cis,
                                                                const u32* __restrict__ trans, const u32* __restrict__ keep, const u32* __restrict__ swap,
                                                                flx_phase_result* __restrict__ out) {
    u64 const i = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_sites) return;
    out[i] = phase_result_row(set[i], state[i], cis[i], trans[i], keep[i], swap[i]);
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
namespace {
dim3 per_element(u64 n) { return dim3((u32)((n + THREADS - 1) / THREADS)); }
}  // namespace

int PhaseDevice::observe(void* stream, const PileupJob* d_jobs, const PhaseRecord* d_recs, u32 n_jobs, const u32* d_words, const u8* d_letters, const u32* d_anchors,
                         const flx_phase_site* d_sites, u8* d_obs) {
    if (n_jobs == 0) return 0;
    static_assert(OBSERVE_WAVES == THREADS / 64u, "a block of phase_observe is four waves");
    u32 const blocks = std::min<u32>((n_jobs + OBSERVE_WAVES - 1) / OBSERVE_WAVES, OBSERVE_GRID_CAP);
    hipLaunchKernelGGL(phase_observe_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, d_recs, n_jobs, d_words, d_letters, d_anchors, d_sites, d_obs);
    return (int)hipGetLastError();
}
int PhaseDevice::links(void* stream, const PhaseRecord* d_recs, u32 n_recs, u64 slot0, u64 n_slots, const u8* d_obs, u32* d_cis, u32* d_trans) {
    if (n_slots == 0 || n_recs == 0) return 0;
    hipLaunchKernelGGL(phase_links_kernel, per_element(n_slots), dim3(THREADS), 0, (hipStream_t)stream, d_recs, n_recs, slot0, n_slots, d_obs, d_cis, d_trans);
    return (int)hipGetLastError();
}
int PhaseDevice::chain(void* stream, int step, const flx_phase_site* d_sites, u32 n_sites, const u32* d_cis, const u32* d_trans, u32 min_link, u32* d_flips, u32* d_starts,
                       u32* d_set_start, u32* d_set, u32* d_state) {
    if (n_sites == 0) return 0;
    if (step == 0) hipLaunchKernelGGL(phase_chain_flags_kernel, per_element(n_sites), dim3(THREADS), 0, (hipStream_t)stream, d_sites, n_sites, d_cis, d_trans, min_link, d_flips, d_starts);
    else if (step == 1) hipLaunchKernelGGL(phase_chain_scatter_kernel, per_element(n_sites), dim3(THREADS), 0, (hipStream_t)stream, n_sites, d_starts, d_set_start);
    else hipLaunchKernelGGL(phase_chain_phase_kernel, per_element(n_sites), dim3(THREADS), 0, (hipStream_t)stream, n_sites, d_flips, d_starts, d_set_start, d_set, d_state);
    return (int)hipGetLastError();
}
int PhaseDevice::tags(void* stream, const PhaseRecord* d_recs, u64 n_recs, const u8* d_obs, const u32* d_set, const u32* d_state, u32 min_margin, flx_phase_tag* d_tags) {
    if (n_recs == 0) return 0;
    hipLaunchKernelGGL(phase_tags_kernel, per_element(n_recs), dim3(THREADS), 0, (hipStream_t)stream, d_recs, n_recs, d_obs, d_set, d_state, min_margin, d_tags);
    return (int)hipGetLastError();
}
int PhaseDevice::votes(void* stream, const PhaseRecord* d_recs, u64 n_recs, u64 n_slots, const u8* d_obs, const u32* d_set, const u32* d_state, const flx_phase_tag* d_tags,
                       u32* d_keep, u32* d_swap) {
    if (n_slots == 0 || n_recs == 0) return 0;
    hipLaunchKernelGGL(phase_votes_kernel, per_element(n_slots), dim3(THREADS), 0, (hipStream_t)stream, d_recs, n_recs, n_slots, d_obs, d_set, d_state, d_tags, d_keep, d_swap);
    return (int)hipGetLastError();
}
int PhaseDevice::revote(void* stream, u32 n_sites, const u32* d_keep, const u32* d_swap, u32* d_state) {
    if (n_sites == 0) return 0;
    hipLaunchKernelGGL(phase_revote_kernel, per_element(n_sites), dim3(THREADS), 0, (hipStream_t)stream, n_sites, d_keep, d_swap, d_state);
    return (int)hipGetLastError();
}
int PhaseDevice::results(void* stream, u32 n_sites, const u32* d_set, const u32* d_state, const u32* d_cis, const u32* d_trans, const u32* d_keep, const u32* d_swap,
                         flx_phase_result* d_out) {
    if (n_sites == 0) return 0;
    hipLaunchKernelGGL(phase_results_kernel, per_element(n_sites), dim3(THREADS), 0, (hipStream_t)stream, n_sites, d_set, d_state, d_cis, d_trans, d_keep, d_swap, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
