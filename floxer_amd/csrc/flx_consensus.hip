// Consensus sequence on the device (the rule: flx_consensus.hpp; the object and the C ABI: flx_consensus_api.cpp). The seven planes are
// pileup's and are added to by pileup_add (flx_pileup.hip) as it stands. Wave64 integer work:
//   consensus_ins_keys        one wave per counted record, 64 CIGAR words per pass: pileup_add's walk (prefix sums over columns and rows,
//                             the any_before carry) with a fourth wave-uniform carry, the key slots used so far. The lane of an I word
//                             packs its letters from the oriented sequence and stores its key at the job's first slot plus the word's
//                             slot; a word longer than 32 letters is void without a letter being loaded. No two lanes share a slot.
//   consensus_allele_heads    over the sorted keys: 1 where a run of equal keys that are not void begins (scanned by flx_scan.hip)
//   consensus_allele_fill     every run's first key and the key behind its last, by the lanes that see those boundaries
//   consensus_allele_winners  one thread per allele: its table row; the first allele of an anchor walks the anchor's alleles (they are
//                             neighbours, and few: at most the depth) and stores the index of the one with the largest count, the
//                             first among equals, at the anchor's entry of the INS plane, which nothing reads any more
//   consensus_call            SCAN_TILE positions per block, strip loads of the six planes and the winners: mode 0 counts the tile's
//                             change rows and adds its letters to one u64; mode 1, behind the scan of the counts, writes the rows and
//                             then replaces DEPTH by out_len and DEL by the call word, each thread its own strip
//   consensus_emit            behind the scan of out_len: one thread per position stores its letter and its inserted letters
//   consensus_offsets         one thread per sequence: the offset of its first position
// Every dependence between these is a launch boundary. All adds are device-scope integer atomicAdd, all stores plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_scan_dev.hpp"
#include "flx_consensus.hpp"

namespace flx {

// ------------------------------------------------------------------------------------------------ consensus_ins_keys
__global__ void __launch_bounds__(THREADS) consensus_ins_keys_kernel(const PileupJob* __restrict__ jobs, const u64* __restrict__ key_off, u32 n_jobs,
                                                                     const u32* __restrict__ words, const u8* __restrict__ letters, SortKey* __restrict__ keys) {
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
            u32 const event = op == 1u ? 1u : 0u;
            u32 const incl = wave_inclusive_scan(cols), incl_rows = wave_inclusive_scan(rows), incl_events = wave_inclusive_scan(event);
            if (event) {
                u64 const first = pos + incl - cols, first_row = row + incl_rows - rows;
                bool const preceded = any_before || incl - cols > 0u;   // (a word has at least one column)
                // (the host judged the rows: they end with the read; the host counted the I words: the slot lies in the job's own)
                out[slots + incl_events - 1u] = consensus_key(preceded, first - 1, len, [&](u32 i) { return (u32)seq[first_row + i]; });
            }
            u32 const pass_cols = __shfl(incl, 63);
            pos += pass_cols;
            row += __shfl(incl_rows, 63);
            slots += __shfl(incl_events, 63);
            any_before = any_before || pass_cols > 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------ alleles
__global__ void __launch_bounds__(THREADS) consensus_allele_heads_kernel(const SortKey* __restrict__ sorted, u64 n, u32* __restrict__ flags) {
    u64 const i = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    SortKey const k = sorted[i];
    flags[i] = !consensus_key_is_void(k) && (i == 0 || !consensus_key_equal(sorted[i - 1], k)) ? 1u : 0u;
}

__global__ void __launch_bounds__(THREADS) consensus_allele_fill_kernel(const SortKey* __restrict__ sorted, const u32* __restrict__ ids, u64 n,
                                                                        u32* __restrict__ run_start, u32* __restrict__ run_end) {
    u64 const i = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n || consensus_key_is_void(sorted[i])) return;
    u32 const id = ids[i];                                             // (a key that is not void lies in a run: id >= 1)
    if (i == 0 || ids[i - 1] != id) run_start[id - 1u] = (u32)i;
    if (i + 1 == n || consensus_key_is_void(sorted[i + 1]) || ids[i + 1] != id) run_end[id - 1u] = (u32)(i + 1);      // (n < 2^32)
}

__global__ void __launch_bounds__(THREADS) consensus_allele_winners_kernel(const SortKey* __restrict__ sorted, const u32* __restrict__ run_start,
                                                                           const u32* __restrict__ run_end, u32 n_alleles, const u32* __restrict__ starts, u32 n_refs,
                                                                           flx_consensus_allele* __restrict__ alleles, u32* __restrict__ winner) {
    u64 const j64 = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (j64 >= n_alleles) return;
    u32 const j = (u32)j64;
    SortKey const k = sorted[run_start[j]];
    u64 const anchor = consensus_key_anchor(k);
    u32 const ref = find_ref(starts, n_refs, anchor);                  // (the host judged the records: an anchor lies inside a sequence)
    alleles[j] = consensus_allele_of(k, run_end[j] - run_start[j], ref, starts[ref]);
    if (j > 0u && consensus_key_anchor(sorted[run_start[j - 1u]]) == anchor) return;
    u32 best = j, best_count = run_end[j] - run_start[j];
    for (u32 x = j + 1u; x < n_alleles && consensus_key_anchor(sorted[run_start[x]]) == anchor; ++x) {
        u32 const c = run_end[x] - run_start[x];
        if (c > best_count) { best = x; best_count = c; }              // (key order: an earlier allele keeps a tie)
    }
    winner[anchor] = best;
}

// ------------------------------------------------------------------------------------------------ consensus_call
// the tile's words carry, above the call word's fields, what mode 1 needs to write a row without making the call again
__device__ __forceinline__ u32 row_word(u32 word, ConsensusCall const& c, u32 R) { return word | c.sub_or_del << 16 | c.alt << 17 | R << 20; }

template <int MODE>
__global__ void __launch_bounds__(THREADS) consensus_call_kernel(u32* __restrict__ acc, u64 stride, u64 total, const u32* __restrict__ starts, u32 n_refs,
                                                                 const u8* __restrict__ text, const i64* __restrict__ text_delta,
                                                                 const flx_consensus_allele* __restrict__ alleles, ConsensusThresholds t, u32* __restrict__ count,
                                                                 unsigned long long* __restrict__ n_letters, flx_consensus_change* __restrict__ out) {
    __shared__ u32 lds[THREADS / 64u];
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    u32 depth[STRIP], del[STRIP], a[STRIP], c[STRIP], g[STRIP], tt[STRIP], win[STRIP];
    load_strip(acc + (u64)PILEUP_DEPTH * stride, total, p0, depth);
    load_strip(acc + (u64)PILEUP_DEL * stride, total, p0, del);
    load_strip(acc + (u64)PILEUP_A * stride, total, p0, a);
    load_strip(acc + (u64)PILEUP_C * stride, total, p0, c);
    load_strip(acc + (u64)PILEUP_G * stride, total, p0, g);
    load_strip(acc + (u64)PILEUP_T * stride, total, p0, tt);
    load_strip(acc + (u64)PILEUP_INS * stride, total, p0, win);
    u32 word[STRIP];
    u32 rows = 0, letters = 0;
    u32 const ref0 = p0 < total ? find_ref(starts, n_refs, p0) : 0u;
    u32 ref = ref0;
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) {
        u64 const p = p0 + i;
        word[i] = 0u;
        if (p >= total) continue;
        while ((u64)starts[ref + 1] <= p) ++ref;                       // (p < total = starts[n_refs]: ref stays below n_refs)
        u32 const R = text[(i64)p + text_delta[ref]];
        u32 const acgt[4] = {a[i], c[i], g[i], tt[i]};
        ConsensusCall const call = consensus_call(R, depth[i], del[i], acgt, t);
        u32 ins = 0;
        if (call.called && win[i] != CONSENSUS_NO_WINNER) {
            flx_consensus_allele const al = alleles[win[i]];
            if (consensus_meets(al.count, (u64)depth[i] + (u64)del[i], t)) ins = al.length;
        }
        word[i] = row_word(consensus_call_word(call.emit, ins), call, R);
        rows += call.sub_or_del + (ins ? 1u : 0u);
        letters += consensus_word_len(word[i]);
    }
    u32 tile_rows, tile_letters;
    u32 const before = block_exclusive_scan(rows, lds, tile_rows);
    if (MODE == 0) {
        (void)block_exclusive_scan(letters, lds, tile_letters);
        if (threadIdx.x == 0) {
            count[blockIdx.x] = tile_rows;
            atomicAdd(n_letters, (unsigned long long)tile_letters);
        }
        return;
    }
    if (rows) {
        u64 index = (u64)before + (blockIdx.x > 0 ? count[blockIdx.x - 1] : 0u);
        ref = ref0;
#pragma unroll
        for (u32 i = 0; i < STRIP; ++i) {
            u32 const w = word[i], ins = consensus_word_ins(w);
            if (!(w >> 16 & 1u) && !ins) continue;
            u64 const p = p0 + i;
            while ((u64)starts[ref + 1] <= p) ++ref;
            u32 const position = (u32)(p - starts[ref]), R = w >> 20 & 7u, alt = w >> 17 & 7u;
            u64 const cov64 = (u64)depth[i] + (u64)del[i];
            u32 const cov = cov64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)cov64;
            if (w >> 16 & 1u) {
                u32 const acgt[4] = {a[i], c[i], g[i], tt[i]};
                bool const is_del = alt == CONSENSUS_CALL_DEL;
                out[index++] = consensus_change_row(ref, position, is_del ? CONSENSUS_DEL : CONSENSUS_SUB, R, is_del ? 0u : alt, 1u, is_del ? del[i] : acgt[(alt - 1u) & 3u], cov, 0);
            }
            if (ins) {
                flx_consensus_allele const al = alleles[win[i]];
                out[index++] = consensus_change_row(ref, position, CONSENSUS_INS, R, 0u, al.length, al.count, cov, al.letters);
            }
        }
    }
    // out_len over DEPTH, the call word over DEL: this thread read its strip of both above, and no other thread reads it
    u32 len[STRIP];
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) { len[i] = consensus_word_len(word[i]); word[i] &= 0xFFFFu; }
    store_strip(acc + (u64)PILEUP_DEPTH * stride, total, p0, len);
    store_strip(acc + (u64)PILEUP_DEL * stride, total, p0, word);
}

// ------------------------------------------------------------------------------------------------ consensus_emit, consensus_offsets
__global__ void __launch_bounds__(THREADS) consensus_emit_kernel(const u32* __restrict__ acc, u64 stride, u64 total, const flx_consensus_allele* __restrict__ alleles,
                                                                 char* __restrict__ pool) {
    u64 const p = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (p >= total) return;
    u32 const w = acc[(u64)PILEUP_DEL * stride + p], len = consensus_word_len(w);
    if (len == 0u) return;
    u64 at = (u64)(acc[(u64)PILEUP_DEPTH * stride + p] - len);         // (the inclusive scan less the position's own: below 2^32, the host saw to it)
    if (consensus_word_emit(w)) pool[at++] = consensus_letter(consensus_word_emit(w));
    u32 const ins = consensus_word_ins(w);
    if (ins) {
        u64 const lo = alleles[acc[(u64)PILEUP_INS * stride + p]].letters;
        for (u32 i = 0; i < ins; ++i) pool[at + i] = consensus_letter(consensus_key_letter(lo, i));
    }
}

__global__ void __launch_bounds__(THREADS) consensus_offsets_kernel(const u32* __restrict__ acc, u64 stride, u64 total, const u32* __restrict__ starts, u32 n_refs,
                                                                    u32* __restrict__ offsets) {
    u32 const r = blockIdx.x * THREADS + threadIdx.x;
    if (r > n_refs) return;
    const u32* __restrict__ const incl = acc + (u64)PILEUP_DEPTH * stride;
    if (r == n_refs) { offsets[r] = incl[total - 1]; return; }
    u64 const p = starts[r];                                           // (no sequence is empty: p < total)
    offsets[r] = incl[p] - consensus_word_len(acc[(u64)PILEUP_DEL * stride + p]);
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
namespace {
dim3 per_element(u64 n) { return dim3((u32)((n + THREADS - 1) / THREADS)); }
}  // namespace

int ConsensusDevice::ins_keys(void* stream, const PileupJob* d_jobs, const u64* d_key_off, u32 n_jobs, const u32* d_words, const u8* d_letters, SortKey* d_keys) {
    if (n_jobs == 0) return 0;
    static_assert(KEYS_WAVES == THREADS / 64u, "a block of consensus_ins_keys is four waves");
    u32 const blocks = std::min<u32>((n_jobs + KEYS_WAVES - 1) / KEYS_WAVES, KEYS_GRID_CAP);
    hipLaunchKernelGGL(consensus_ins_keys_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, d_key_off, n_jobs, d_words, d_letters, d_keys);
    return (int)hipGetLastError();
}
int ConsensusDevice::allele_heads(void* stream, const SortKey* d_sorted, u64 n, u32* d_flags) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(consensus_allele_heads_kernel, per_element(n), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, n, d_flags);
    return (int)hipGetLastError();
}
int ConsensusDevice::allele_fill(void* stream, const SortKey* d_sorted, const u32* d_ids, u64 n, u32* d_run_start, u32* d_run_end) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(consensus_allele_fill_kernel, per_element(n), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, d_ids, n, d_run_start, d_run_end);
    return (int)hipGetLastError();
}
int ConsensusDevice::allele_winners(void* stream, const SortKey* d_sorted, const u32* d_run_start, const u32* d_run_end, u32 n_alleles, const u32* d_starts, u32 n_refs,
                                    flx_consensus_allele* d_alleles, u32* d_winner) {
    if (n_alleles == 0) return 0;
    hipLaunchKernelGGL(consensus_allele_winners_kernel, per_element(n_alleles), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, d_run_start, d_run_end, n_alleles, d_starts,
                       n_refs, d_alleles, d_winner);
    return (int)hipGetLastError();
}
int ConsensusDevice::call(void* stream, int mode, u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, const u8* d_text, const i64* d_text_delta,
                          const flx_consensus_allele* d_alleles, ConsensusThresholds t, u32* d_count, unsigned long long* d_letters, flx_consensus_change* d_out) {
    dim3 const grid((u32)((total + TILE - 1) / TILE)), block(THREADS);
    if (mode == 0) hipLaunchKernelGGL(consensus_call_kernel<0>, grid, block, 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, d_text, d_text_delta, d_alleles, t, d_count, d_letters, d_out);
    else hipLaunchKernelGGL(consensus_call_kernel<1>, grid, block, 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, d_text, d_text_delta, d_alleles, t, d_count, d_letters, d_out);
    return (int)hipGetLastError();
}
int ConsensusDevice::emit(void* stream, const u32* d_acc, u64 stride, u64 total, const flx_consensus_allele* d_alleles, char* d_pool) {
    hipLaunchKernelGGL(consensus_emit_kernel, per_element(total), dim3(THREADS), 0, (hipStream_t)stream, d_acc, stride, total, d_alleles, d_pool);
    return (int)hipGetLastError();
}
int ConsensusDevice::offsets(void* stream, const u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, u32* d_offsets) {
    hipLaunchKernelGGL(consensus_offsets_kernel, per_element((u64)n_refs + 1), dim3(THREADS), 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, d_offsets);
    return (int)hipGetLastError();
}

}  // namespace flx
