// Diploid small-variant calls on the device (the rule: flx_variants.hpp; the object and the C ABI: flx_variants_api.cpp). The seven planes
// are pileup's and are added to by pileup_add (flx_pileup.hip) as it stands; the runs of equal sorted keys are found by the consensus's
// consensus_allele_heads and consensus_allele_fill (flx_consensus.hip) as they stand. Wave64 integer work:
//   variants_indel_keys       one wave per counted record, 64 CIGAR words per pass: consensus_ins_keys' walk (prefix sums over columns and
//                             rows, the any_before carry, the key slots used so far as the fourth wave-uniform carry) with two event
//                             kinds. The lane of an I word packs its letters from the oriented sequence; the lane of a D word makes its
//                             key from the anchor and the length alone and loads no letter, as does a word that is void for its length
//                             or for the missing column in front. Each stores its key at the job's first slot plus the word's slot: no
//                             two lanes share a slot.
//   variants_anchor_winners   one thread per allele: its table row; the first allele of an anchor walks the anchor's alleles (they are
//                             neighbours, and few: at most the depth) and stores the index of the one with the largest count, the
//                             first among equals, at the anchor's entry of the INS plane, which nothing reads any more, and the sum of
//                             their counts, events(a), at the anchor's entry of an eighth plane behind pileup's seven. Both are then
//                             strip-loaded by the call like the counts; a per-anchor table would cost the call a search per position.
//   variants_call             SCAN_TILE positions per block, strip loads of the six count planes, the winners and the events: mode 0
//                             counts the tile's rows (up to two per position) and adds them to one u64; mode 1, behind the scan of the
//                             counts, makes the calls again and writes the rows in order, the SNV row in front of the indel row
// Every dependence between these is a launch boundary. All adds are device-scope integer atomicAdd, all stores plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_scan_dev.hpp"
#include "flx_variants.hpp"

namespace flx {

// ------------------------------------------------------------------------------------------------ variants_indel_keys
__global__ void __launch_bounds__(THREADS) variants_indel_keys_kernel(const PileupJob* __restrict__ jobs, const u64* __restrict__ key_off, u32 n_jobs,
                                                                      const u32* __restrict__ words, const u8* __restrict__ letters, u32 max_del, SortKey* __restrict__ keys) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * (THREADS / 64u);
    for (u32 id = blockIdx.x * (THREADS / 64u) + (threadIdx.x >> 6); id < n_jobs; id += waves) {       // (id is wave-uniform)
        PileupJob const job = jobs[id];
        const u8* __restrict__ const seq = letters + job.seq_off;
        SortKey* __restrict__ const out = keys + key_off[id];
        u64 pos = job.text_off, row = 0;                               // the wave-uniform carries: position and row behind the last pass,
        bool any_before = false;                                       // whether a reference-consuming column lies in front of this pass,
        u64 slots = 0;                                                 // and the key slots the passes so far have used
        for (u32 base = 0; base < job.n_words; base += 64u) {
            u32 const word = base + lane < job.n_words ? words[job.word_off + base + lane] : 0u;      // (op 0 consumes nothing and is no event)
            u32 const op = word & 15u, len = word >> 4;
            u32 const cols = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            u32 const rows = (op == 7u || op == 8u || op == 1u || op == 4u) ? len : 0u;
            u32 const event = (op == 1u || op == 2u) ? 1u : 0u;
            u32 const incl = wave_inclusive_scan(cols), incl_rows = wave_inclusive_scan(rows), incl_events = wave_inclusive_scan(event);
            if (event) {
                // first: an I word's cursor, a D word's first column; either way the column in front of it is the anchor
                u64 const first = pos + incl - cols, first_row = row + incl_rows - rows;
                bool const preceded = any_before || incl - cols > 0u;   // (a word has at least one column)
                // (the host judged the rows: they end with the read; the host counted the I and D words: the slot lies in the job's own)
                out[slots + incl_events - 1u] = variants_key(op == 1u ? VARIANTS_KEY_INS : VARIANTS_KEY_DEL, preceded, first - 1, len, max_del,
                                                             [&](u32 i) { return (u32)seq[first_row + i]; });
            }
            u32 const pass_cols = __shfl(incl, 63);
            pos += pass_cols;
            row += __shfl(incl_rows, 63);
            slots += __shfl(incl_events, 63);
            any_before = any_before || pass_cols > 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------ variants_anchor_winners
__global__ void __launch_bounds__(THREADS) variants_anchor_winners_kernel(const SortKey* __restrict__ sorted, const u32* __restrict__ run_start,
                                                                          const u32* __restrict__ run_end, u32 n_alleles, const u32* __restrict__ starts, u32 n_refs,
                                                                          flx_variant_allele* __restrict__ alleles, u32* __restrict__ winner, u32* __restrict__ events) {
    u64 const j64 = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (j64 >= n_alleles) return;
    u32 const j = (u32)j64;
    SortKey const k = sorted[run_start[j]];
    u64 const anchor = variants_key_anchor(k);
    u32 const ref = find_ref(starts, n_refs, anchor);                  // (the host judged the records: an anchor lies inside a sequence)
    alleles[j] = variants_allele_of(k, run_end[j] - run_start[j], ref, starts[ref]);
    if (j > 0u && variants_key_anchor(sorted[run_start[j - 1u]]) == anchor) return;
    u32 best = j, best_count = run_end[j] - run_start[j], sum = best_count;
    for (u32 x = j + 1u; x < n_alleles && variants_key_anchor(sorted[run_start[x]]) == anchor; ++x) {
        u32 const c = run_end[x] - run_start[x];
        sum += c;                                                      // (all events are fewer than 2^32)
        if (c > best_count) { best = x; best_count = c; }              // (key order: an earlier allele keeps a tie)
    }
    winner[anchor] = best;
    events[anchor] = sum;
}

// ------------------------------------------------------------------------------------------------ variants_call
// the rows of position p0 + i of a thread's strips: bit 0 the SNV row (row[0]), bit 1 the indel row (row[1])
struct Strips { u32 depth[STRIP], del[STRIP], a[STRIP], c[STRIP], g[STRIP], t[STRIP], win[STRIP], events[STRIP]; };
__device__ __forceinline__ u32 position_rows(Strips const& s, u32 i, u32 R, const flx_variant_allele* __restrict__ alleles, VariantsModel const& v, flx_variant (&row)[2]) {
    u32 const acgt[4] = {s.a[i], s.c[i], s.g[i], s.t[i]};
    u32 n = variants_snv(R, s.depth[i], s.del[i], acgt, v, row[0]) ? 1u : 0u;
    if (s.win[i] != CONSENSUS_NO_WINNER) {
        flx_variant_allele const al = alleles[s.win[i]];
        if (variants_indel(R, s.depth[i], s.del[i], s.events[i], variants_allele_key_kind(al), al.length, al.count, al.letters, v, row[1])) n |= 2u;
    }
    return n;
}

template <int MODE>
__global__ void __launch_bounds__(THREADS) variants_call_kernel(const u32* __restrict__ acc, u64 stride, u64 total, const u32* __restrict__ starts, u32 n_refs,
                                                                const u8* __restrict__ text, const i64* __restrict__ text_delta,
                                                                const flx_variant_allele* __restrict__ alleles, VariantsModel v, u32* __restrict__ count,
                                                                unsigned long long* __restrict__ n_rows, flx_variant* __restrict__ out) {
    __shared__ u32 lds[THREADS / 64u];
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    Strips s;
    load_strip(acc + (u64)PILEUP_DEPTH * stride, total, p0, s.depth);
    load_strip(acc + (u64)PILEUP_DEL * stride, total, p0, s.del);
    load_strip(acc + (u64)PILEUP_A * stride, total, p0, s.a);
    load_strip(acc + (u64)PILEUP_C * stride, total, p0, s.c);
    load_strip(acc + (u64)PILEUP_G * stride, total, p0, s.g);
    load_strip(acc + (u64)PILEUP_T * stride, total, p0, s.t);
    load_strip(acc + (u64)PILEUP_INS * stride, total, p0, s.win);
    load_strip(acc + (u64)VARIANTS_PLANE_EVENTS * stride, total, p0, s.events);
    u32 const ref0 = p0 < total ? find_ref(starts, n_refs, p0) : 0u;
    u32 ref = ref0, rows = 0;
    u32 made = 0;                                                      // two bits per position of the strip: its rows
    flx_variant row[2];
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) {
        u64 const p = p0 + i;
        if (p >= total) continue;                                      // (a strip past the end read 0 for the winners too: nothing of it is used)
        while ((u64)starts[ref + 1] <= p) ++ref;                       // (p < total = starts[n_refs]: ref stays below n_refs)
        u32 const R = text[(i64)p + text_delta[ref]];
        u32 const n = position_rows(s, i, R, alleles, v, row);
        made |= n << (2u * i);
        rows += (n & 1u) + (n >> 1);
    }
    u32 tile_rows;
    u32 const before = block_exclusive_scan(rows, lds, tile_rows);
    if (MODE == 0) {
        if (threadIdx.x == 0) {
            count[blockIdx.x] = tile_rows;
            if (tile_rows) atomicAdd(n_rows, (unsigned long long)tile_rows);
        }
        return;
    }
    if (!rows) return;
    u64 index = (u64)before + (blockIdx.x > 0 ? count[blockIdx.x - 1] : 0u);       // (count holds the inclusive scan; all rows are fewer than 2^32)
    ref = ref0;
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) {
        if (!(made >> (2u * i) & 3u)) continue;
        u64 const p = p0 + i;
        while ((u64)starts[ref + 1] <= p) ++ref;
        u32 const R = text[(i64)p + text_delta[ref]];
        u32 const n = position_rows(s, i, R, alleles, v, row);
#pragma unroll
        for (u32 k = 0; k < 2u; ++k) {
            if (!(n >> k & 1u)) continue;
            row[k].reference_id = (int32_t)ref;
            row[k].position = (u32)(p - starts[ref]);
            out[index++] = row[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
namespace {
dim3 per_element(u64 n) { return dim3((u32)((n + THREADS - 1) / THREADS)); }
}  // namespace

int VariantsDevice::indel_keys(void* stream, const PileupJob* d_jobs, const u64* d_key_off, u32 n_jobs, const u32* d_words, const u8* d_letters, u32 max_del, SortKey* d_keys) {
    if (n_jobs == 0) return 0;
    static_assert(KEYS_WAVES == THREADS / 64u, "a block of variants_indel_keys is four waves");
    u32 const blocks = std::min<u32>((n_jobs + KEYS_WAVES - 1) / KEYS_WAVES, KEYS_GRID_CAP);
    hipLaunchKernelGGL(variants_indel_keys_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, d_key_off, n_jobs, d_words, d_letters, max_del, d_keys);
    return (int)hipGetLastError();
}
int VariantsDevice::anchor_winners(void* stream, const SortKey* d_sorted, const u32* d_run_start, const u32* d_run_end, u32 n_alleles, const u32* d_starts, u32 n_refs,
                                   flx_variant_allele* d_alleles, u32* d_winner, u32* d_events) {
    if (n_alleles == 0) return 0;
    hipLaunchKernelGGL(variants_anchor_winners_kernel, per_element(n_alleles), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, d_run_start, d_run_end, n_alleles, d_starts,
                       n_refs, d_alleles, d_winner, d_events);
    return (int)hipGetLastError();
}
int VariantsDevice::call(void* stream, int mode, const u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, const u8* d_text, const i64* d_text_delta,
                         const flx_variant_allele* d_alleles, VariantsModel v, u32* d_count, unsigned long long* d_rows, flx_variant* d_out) {
    dim3 const grid((u32)((total + TILE - 1) / TILE)), block(THREADS);
    if (mode == 0) hipLaunchKernelGGL(variants_call_kernel<0>, grid, block, 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, d_text, d_text_delta, d_alleles, v, d_count, d_rows, d_out);
    else hipLaunchKernelGGL(variants_call_kernel<1>, grid, block, 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, d_text, d_text_delta, d_alleles, v, d_count, d_rows, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
