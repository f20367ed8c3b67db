// Error profile on the device (the rule: flx_errprof.hpp; the object and the C ABI: flx_errprof_api.cpp). Wave64 integer work:
//   errprof_add    one wave per counted record, 64 CIGAR words per pass, as pileup_add: two wave prefix sums, over the reference-consuming
//                  and over the query-consuming lengths, each with a wave-uniform carry between passes, give every word its first position
//                  in the text and its first row of the oriented sequence. (pileup_add's third carry, "a reference column precedes", has no
//                  use here: an I word's position is the walk's cursor whether or not a column lies in front of it.) Every lane adds what
//                  its word adds once (errprof_word_events). A word of fewer than 64 columns is then walked by its own lane with the
//                  header's errprof_word_columns, the host's code. A word of 64 columns or more (a clean read is one = word of 10 000) is
//                  walked by the whole wave: a ballot picks the long words of the pass and the wave takes them one at a time, 64 columns
//                  per step; lanes that hold the same (t, q) pair or the same letter are counted with one ballot and added once, the
//                  word's rows go to their position bins one bin per lane (no division per column: a bin's first row follows from the
//                  read's length), and the two homopolymer scans are one load per lane, 32 lanes a side.
//   the counters   every wave keeps a private u32 copy of the table in LDS (ERRPROF_ENTRIES * 4 bytes; four waves a block: 18 KB) and
//                  adds to it with LDS atomics, which order the adds of its own lanes; no other wave touches it, so the record loop has
//                  no __syncthreads(): the waves of a block take different numbers of records. At its end, and between two records once
//                  the columns plus rows walked since the last flush reach flush_threshold, the wave adds its non-zero entries to the
//                  global u64 table with device-scope atomicAdd and clears them.
//                  The u32 bound: no entry grows by more than 1 per column or row walked, or by more than a record's own sums per record
//                  (errprof_record_end: each at most its columns plus rows). A flush happens as soon as `walked` >= flush_threshold
//                  between records, so in front of a record walked < flush_threshold <= 2^31 (errprof_options_valid), and a record adds
//                  less than 2^31 (ERRPROF_MAX_RECORD, judged on the host): every entry, and `walked` itself, stays below 2^32.
// All adds are integer atomics (LDS, or device scope on the table), all stores plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_errprof.hpp"
#include "flx_wave.hpp"

namespace flx {
namespace {

constexpr u32 EP_THREADS = 256, EP_WAVES = EP_THREADS / 64u;

// + (number of lanes with `valid` and this lane's `entry`) to tab[entry], once per distinct entry among the lanes; every lane calls it
__device__ __forceinline__ void wave_count(u32* tab, u32 entry, bool valid) {
    u32 const lane = lane_id();
    unsigned long long todo = __ballot(valid);
    while (todo) {                                                      // (wave-uniform)
        u32 const leader = (u32)__ffsll((long long)todo) - 1u;
        u32 const e = (u32)__shfl((int)entry, (int)leader);
        unsigned long long const same = __ballot(valid && entry == e);
        if (lane == leader) atomicAdd(&tab[e], (u32)__popcll(same));
        todo &= ~same;
    }
}
__device__ __forceinline__ u32 wave_sum32(u32 v) {
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) v += (u32)__shfl_xor((int)v, (int)d);
    return v;
}
// the wave's entries added to the table and cleared (atomicExch reads and clears in one step, ordered behind the wave's LDS adds)
__device__ __forceinline__ void flush(u32* tab, unsigned long long* __restrict__ table) {
    for (u32 i = lane_id(); i < ERRPROF_ENTRIES; i += 64u) {
        u32 const v = atomicExch(&tab[i], 0u);
        if (v) atomicAdd(&table[i], (unsigned long long)v);
    }
}

// one word of 64 columns or more, by the whole wave; all arguments are wave-uniform
__device__ __forceinline__ void wave_word(u32* tab, u32 op, u32 L, u64 p, u64 row, ErrprofJob const& job, const u8* __restrict__ text, const u8* __restrict__ seq) {
    u32 const lane = lane_id();
    bool const reverse = job.reverse != 0;
    if (op == 7u || op == 8u) {
        u32* const pair = tab + (op == 7u ? EP_PAIR_EQ : EP_PAIR_X);
        for (u32 c0 = 0; c0 < L; c0 += 64u) {
            u32 const c = c0 + lane;
            bool const valid = c < L;                                   // (the host judged the columns and the rows: they end with the sequence and the read)
            u32 const code = valid ? errprof_rank(text[p + c]) * 6u + errprof_rank(seq[row + c]) : 0u;
            wave_count(pair, code, valid);
        }
    } else if (op == 1u || op == 2u) {
        const u8* __restrict__ const letters = op == 1u ? seq + row : text + p;
        u32 const a = errprof_rank(letters[0]);
        bool differs = false;
        for (u32 c0 = 0; c0 < L; c0 += 64u) {
            u32 const c = c0 + lane;
            bool const valid = c < L;
            u32 const x = valid ? errprof_rank(letters[c]) : a;
            wave_count(tab + (op == 1u ? EP_INS_LETTER : EP_DEL_LETTER), x, valid);
            differs = differs || x != a;
        }
        bool const uniform = __ballot(differs) == 0ull;
        u64 run = op == 2u ? L : 0u;                                    // (a D of 64: bin 32 whatever stands next to it, so only an I scans)
        if (op == 1u && uniform && a >= 1u && a <= 4u) {
            // lanes 0..31: position p - 1 - lane, not below s0; lanes 32..63: position p + lane - 32, below s1
            u32 const k = lane & 31u;
            bool const left = lane < 32u;
            bool const inside = left ? p - job.s0 > k : job.s1 - p > k;      // (s0 <= p <= s1: neither difference wraps, nothing outside the sequence is read)
            bool const equal = inside && text[left ? p - 1 - k : p + k] == a;
            unsigned long long const unequal = ~__ballot(equal);
            u32 const lo = (u32)unequal, hi = (u32)(unequal >> 32);
            run = (u64)(lo ? (u32)__ffs((int)lo) - 1u : 32u) + (hi ? (u32)__ffs((int)hi) - 1u : 32u);
        }
        if (lane == 0u) atomicAdd(&tab[(op == 1u ? EP_HP_INS : EP_HP_DEL) + errprof_hp_bin(a, uniform, run)], 1u);
    }
    if (op != 2u) {                                                     // the rows' position bins, one bin per lane
        u32 const section = op == 7u ? EP_POS_MATCH : op == 8u ? EP_POS_MISMATCH : op == 1u ? EP_POS_INS : EP_POS_CLIP;
        u64 ga, gb;
        errprof_given_rows(row, L, job.read_len, reverse, ga, gb);
        u32 const first = errprof_bin(ga, job.read_len), last = errprof_bin(gb - 1, job.read_len);
        for (u32 b = first + lane; b <= last; b += 64u) {
            u32 const k = errprof_rows_in_bin(b, ga, gb, job.read_len);
            if (k) atomicAdd(&tab[section + b], k);
        }
    }
}

__global__ void __launch_bounds__(EP_THREADS) errprof_add_kernel(const ErrprofJob* __restrict__ jobs, u32 n_jobs, const u32* __restrict__ words, const u8* __restrict__ text,
                                                                 const u8* __restrict__ letters, unsigned long long* __restrict__ table, u32 flush_threshold) {
    __shared__ u32 lds[EP_WAVES * ERRPROF_ENTRIES];
    u32 const lane = lane_id();
    u32* const tab = lds + (threadIdx.x >> 6) * ERRPROF_ENTRIES;        // this wave's own table
    for (u32 i = lane; i < ERRPROF_ENTRIES; i += 64u) atomicExch(&tab[i], 0u);
    auto add = [tab](u32 entry, u32 count) { atomicAdd(&tab[entry], count); };
    u32 const waves = gridDim.x * EP_WAVES;
    u32 walked = 0;                                                     // columns plus rows since the last flush (wave-uniform)
    for (u32 id = blockIdx.x * EP_WAVES + (threadIdx.x >> 6); id < n_jobs; id += waves) {       // (id is wave-uniform)
        ErrprofJob const job = jobs[id];
        const u8* __restrict__ const seq = letters + job.seq_off;
        auto q = [seq](u64 r) { return (u32)seq[r]; };
        u64 pos = job.text_off, row = 0;                               // the wave-uniform carries: position and row behind the last pass
        ErrprofSums sums{};                                            // this lane's words
        for (u32 base = 0; base < job.n_words; base += 64u) {
            u32 const word = base + lane < job.n_words ? words[job.word_off + base + lane] : 0u;      // (op 0 consumes and counts nothing)
            u32 const op = word & 15u, len = word >> 4;
            u32 const cols = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            u32 const rows = (op == 7u || op == 8u || op == 1u || op == 4u) ? len : 0u;
            u32 const incl = wave_inclusive_scan(cols), incl_rows = wave_inclusive_scan(rows);
            u32 const before = incl - cols, before_rows = incl_rows - rows;
            errprof_word_events(op, len, row + before_rows, job.read_len, job.reverse != 0, add);
            errprof_sums_word(sums, op, len);
            if (len < 64u) errprof_word_columns(op, len, pos + before, row + before_rows, job, text, q, add);
            unsigned long long long_words = __ballot(len >= 64u);
            while (long_words) {                                        // (wave-uniform)
                int const src = __ffsll((long long)long_words) - 1;
                long_words &= long_words - 1ull;
                wave_word(tab, (u32)__shfl((int)op, src), (u32)__shfl((int)len, src), pos + (u32)__shfl((int)before, src), row + (u32)__shfl((int)before_rows, src), job, text, seq);
            }
            u32 const pass_cols = (u32)__shfl((int)incl, 63), pass_rows = (u32)__shfl((int)incl_rows, 63);
            pos += pass_cols;
            row += pass_rows;
            walked += pass_cols + pass_rows;
        }
        ErrprofSums total;
        total.matches = wave_sum32(sums.matches); total.mismatches = wave_sum32(sums.mismatches);
        total.ins_events = wave_sum32(sums.ins_events); total.ins_bases = wave_sum32(sums.ins_bases);
        total.del_events = wave_sum32(sums.del_events); total.del_bases = wave_sum32(sums.del_bases);
        total.clip_bases = wave_sum32(sums.clip_bases);
        if (lane == 0u) errprof_record_end(total, add);
        if (walked >= flush_threshold) { flush(tab, table); walked = 0; }
    }
    flush(tab, table);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the launch (checked by its caller)
int ErrprofDevice::add(void* stream, const ErrprofJob* d_jobs, u32 n_jobs, const u32* d_words, const u8* d_text, const u8* d_letters, unsigned long long* d_table,
                       u32 flush_threshold) {
    if (n_jobs == 0) return 0;
    // capped as pileup_add's grid is, but lower: every wave ends with a flush of its table, so a wave should take several records
    u32 const blocks = std::min<u32>((n_jobs + EP_WAVES - 1) / EP_WAVES, ADD_GRID_CAP);
    hipLaunchKernelGGL(errprof_add_kernel, dim3(blocks), dim3(EP_THREADS), 0, (hipStream_t)stream, d_jobs, n_jobs, d_words, d_text, d_letters, d_table, flush_threshold);
    return (int)hipGetLastError();
}

}  // namespace flx
