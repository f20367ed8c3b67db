// PAF summaries on the device (the rule: flx_paf.hpp; the object and the C ABI: flx_paf_api.cpp). Wave64 integer work over CIGAR words:
//   paf_summarise   one wave per record, a stride loop over the records, one lane per word and 64 words per pass. A pass sums the lengths
//                   of its = X I D words (64-bit wave sums) and counts its gap opens with a ballot: an I or D lane whose left neighbour
//                   (the carried op of the previous pass's last word for lane 0) has another op. Soft clips: ballots give the pass's
//                   first and last non-S lane; S lanes below the first add to `lead` while no non-S word has been seen, S lanes above the
//                   last become the pending length, which is `trail` at the end; an S lane between the two, or a pending length in front
//                   of a non-S word, is an interior clip. The wave-uniform carries between passes: the six sums, whether a non-S word
//                   has been seen, the pending S length, the previous pass's last op.
// The host has judged every record (paf_judge); a record that still breaks the rule gets 0xFFFFFFFF in every field. Lanes 0..7 store the
// eight fields of a summary, one plain 32-byte stretch per record. No text or query letters are read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_paf.hpp"
#include "flx_wave.hpp"

namespace flx {

__global__ void __launch_bounds__(64) paf_summarise_kernel(const PafJob* __restrict__ jobs, u32 n_jobs, const u32* __restrict__ words,
                                                           u32* __restrict__ out) {
    u32 const lane = lane_id();
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {          // (id is wave-uniform)
        PafJob const job = jobs[id];
        u64 eq = 0, x = 0, ins = 0, del = 0, lead = 0, pending = 0, gap_opens = 0;
        bool seen = false, violation = false;
        u32 prev_last = 0;                                             // the op of the previous pass's last word (no op is 0)
        for (u64 base = 0; base < job.n_words; base += 64u) {
            bool const valid = base + lane < job.n_words;
            u32 const word = valid ? words[job.word_off + base + lane] : 0u;
            u32 const op = word & 15u;
            u64 const len = word >> 4;
            bool const is_s = valid && op == 4u, non_s = valid && op != 4u;
            eq += wave_sum(op == 7u ? len : 0ull);
            x += wave_sum(op == 8u ? len : 0ull);
            ins += wave_sum(op == 1u ? len : 0ull);
            del += wave_sum(op == 2u ? len : 0ull);
            if (__ballot(valid && (len == 0 || !(op == 7u || op == 8u || op == 1u || op == 2u || op == 4u))) != 0ull) violation = true;
            u32 const left = __shfl_up(op, 1);
            u32 const prev = lane == 0u ? prev_last : left;
            gap_opens += (u64)__popcll(__ballot(valid && (op == 1u || op == 2u) && prev != op));
            prev_last = __shfl(op, 63);                                // (a pass that is not full is the last one)
            unsigned long long const s_mask = __ballot(is_s), n_mask = __ballot(non_s);
            if (n_mask == 0ull) {                                      // S words only
                u64 const s = wave_sum(is_s ? len : 0ull);
                if (seen) pending += s; else lead += s;
            } else {
                u32 const first = (u32)__ffsll((long long)n_mask) - 1u, last = 63u - (u32)__clzll((long long)n_mask);
                unsigned long long const below = (1ull << first) - 1ull, above = last == 63u ? 0ull : ~0ull << (last + 1u);
                u64 const head = wave_sum(is_s && lane < first ? len : 0ull), tail = wave_sum(is_s && lane > last ? len : 0ull);
                if ((s_mask & ~below & ~above) != 0ull) violation = true;
                if (seen && (pending != 0 || head != 0)) violation = true;
                if (!seen) lead += head;
                pending = tail;
                seen = true;
            }
        }
        u64 const trail = pending;
        u32 field = 0;
        if (job.n_words != 0) {
            u64 const ref_end = (u64)job.position + eq + x + del;
            if (!seen || eq + x + del == 0 || lead + eq + x + ins + trail != (u64)job.read_len) violation = true;
            if (lead >= PAF_MAX_SUM || trail >= PAF_MAX_SUM || eq >= PAF_MAX_SUM || x >= PAF_MAX_SUM || ins >= PAF_MAX_SUM || del >= PAF_MAX_SUM ||
                gap_opens >= PAF_MAX_SUM || ref_end >= PAF_MAX_SUM)
                violation = true;
            u64 const q_start = job.reverse ? trail : lead, q_end = (u64)job.read_len - (job.reverse ? lead : trail);
            u64 const v = lane == 0u ? q_start : lane == 1u ? q_end : lane == 2u ? ref_end : lane == 3u ? eq : lane == 4u ? x : lane == 5u ? ins : lane == 6u ? del : gap_opens;
            field = violation ? PAF_VIOLATION : (u32)v;
        }
        if (lane < 8u) out[(u64)id * 8u + lane] = field;
    }
}

int PafDevice::summarise(void* stream, const PafJob* d_jobs, u32 n_jobs, const u32* d_words, flx_paf_summary* d_out) {
    if (n_jobs == 0) return 0;
    static_assert(sizeof(flx_paf_summary) == 32, "eight u32 fields");
    hipLaunchKernelGGL(paf_summarise_kernel, dim3(std::min(n_jobs, PAF_GRID_CAP)), dim3(64), 0, (hipStream_t)stream, d_jobs, n_jobs, d_words,
                       reinterpret_cast<u32*>(d_out));
    return (int)hipGetLastError();
}

}  // namespace flx
