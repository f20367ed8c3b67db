// K5b md_build: the MD string of every traced path, built on the device from the CIGAR words K5 (ed_traceback, flx_device.hip) has just
// written and the reference text in HBM. It is queued on the lane's stream directly behind K5 and reads K5's DevTraceOut there: the host
// does not wait in between, and it needs no reference text of its own (a context made on an index image has none).
//
// The rule is samtools calmd's, defined on the CIGAR's ops; nothing is compared again. Walk the reference-consuming columns from `begin`:
// '=' columns increment a counter; every X column emits the counter (decimal, possibly 0), the reference letter, and resets the counter;
// every D op emits the counter, '^', the op's reference letters, and resets the counter; I emits nothing and resets nothing; the end emits
// the counter. So X X gives A0C, D then X gives ^AC0T, D I D gives ^A0^C, a perfect match of 2000 gives 2000. Letters come from the
// index's ranks: 1..4 -> ACGT, anything else -> N (IUPAC and lower-case letters of the FASTA are not recoverable: the index stores ranks).
// The string is in reference-forward orientation for both strands (a reverse-strand record was traced with the reverse-complemented read).
//
// One wave per job, one lane per CIGAR word, 64 words per pass. A wave scan of the ops' reference lengths gives every lane its reference
// position; a scan of the '=' lengths, cut at the last X / D op below the lane (ballot + one shuffle: the segmented scan), gives the match
// count in front of every X / D op, an I between two '=' runs merging them; from that a lane knows the bytes it emits, and an exclusive scan
// gives it its output offset. Three wave-uniform values carry from pass to pass: reference position, pending match count, output position.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {

__device__ __forceinline__ u32 dec_digits(u32 v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ void put_dec(u8* p, u32 v, u32 digits) {
    for (u32 i = digits; i-- > 0;) { p[i] = (u8)('0' + v % 10u); v /= 10u; }
}
__device__ __forceinline__ u8 md_letter(u8 rank) {                     // 1..4 -> ACGT, else N
    u32 const r = (u32)rank - 1u;
    return r < 4u ? (u8)(0x54474341u >> (8u * r)) : (u8)'N';
}

}  // namespace

__global__ void __launch_bounds__(64) md_build_kernel(const u8* __restrict__ text, const u32* __restrict__ cigar, const DevTraceOut* __restrict__ trace_out,
                                                      const DevMdJob* __restrict__ jobs, u32 n_jobs, u8* __restrict__ md, DevMdOut* __restrict__ out) {
    u32 const lane = lane_id();
    // (a grid no larger than the job list: a wave takes jobs in turn, as K5's do)
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
        DevMdJob const job = jobs[id];
        DevTraceOut const t = trace_out[job.out_index];
        if (t.cigar_len == 0xFFFFFFFFu) {                              // K5 ran out of its slab: the host fails on that
            if (lane == 0) out[job.out_index] = DevMdOut{0u, 0u};
            continue;
        }
        const u8* __restrict__ r = text + job.ref_off;
        const u32* __restrict__ words = cigar + job.cigar_off + t.cigar_start;
        u8* __restrict__ dst = md + job.md_off;
        u32 const cap = job.md_cap, n = job.n;
        auto letter_at = [&](u32 col) { return md_letter(col < n ? r[col] : (u8)0); };      // (the passes check that the path stays in the window)
        u32 ref_pos = t.begin, pending = 0, out_pos = 0;               // the wave-uniform carries
        bool overflow = false;
        for (u32 base = 0; base < t.cigar_len; base += 64u) {
            u32 const w = base + lane < t.cigar_len ? words[base + lane] : 0u;
            u32 const op = w & 15u, len = w >> 4;
            bool const is_eq = op == 7u, is_x = op == 8u, is_d = op == 2u;
            bool const event = (is_x || is_d) && len > 0u;
            // reference position of the op's first column
            u32 const ref_len = (is_eq || is_x || is_d) ? len : 0u;
            u32 const ref_incl = wave_inclusive_scan(ref_len);
            u32 const my_ref = ref_pos + ref_incl - ref_len;
            // (a path that leaves its window - K5 never writes one - is reported like a slab that is too small, not written with N's)
            if (__shfl(ref_incl, 63) > n - min(ref_pos, n)) { overflow = true; break; }
            // '=' columns since the last X / D op in front of this one (an event's own '=' length is 0: inclusive = exclusive there)
            u32 const eq_incl = wave_inclusive_scan(is_eq ? len : 0u);
            u64 const ev_mask = __ballot(event);
            u64 const ev_below = ev_mask & ((1ull << lane) - 1ull);
            u32 const eq_at_prev = __shfl(eq_incl, ev_below ? 63 - __builtin_clzll(ev_below) : 0);
            u32 const cnt = ev_below ? eq_incl - eq_at_prev : pending + eq_incl;
            // bytes: the count, then X: letter (0 letter)*, D: ^ letters. (Clamped above the slab's size: the sums stay small.)
            u32 const digits = dec_digits(cnt);
            u32 bytes = 0;
            if (event) bytes = len > cap ? cap + 1u : digits + (is_x ? 2u * len - 1u : 1u + len);
            if (bytes > cap) bytes = cap + 1u;
            u32 const out_incl = wave_inclusive_scan(bytes);
            u32 const total = __shfl(out_incl, 63);
            if (total > cap - out_pos) { overflow = true; break; }     // (out_pos <= cap always; cap < 2^26 from a 32-bit NM <= query rows)
            u32 const my_out = out_pos + out_incl - bytes;
            u32 const head = digits + (is_d ? 1u : 0u);                // bytes in front of the op's letters
            if (event) {
                u8* p = dst + my_out;
                put_dec(p, cnt, digits);
                if (is_d) p[digits] = (u8)'^';
                if (len <= 64u) {
                    p += head;
                    for (u32 c = 0; c < len; ++c) {
                        if (is_x && c) *p++ = (u8)'0';
                        *p++ = letter_at(my_ref + c);
                    }
                }
            }
            // a run of more than 64 symbols is copied by the whole wave
            u64 long_mask = __ballot(event && len > 64u);
            while (long_mask) {
                int const src = __builtin_ctzll(long_mask);
                long_mask &= long_mask - 1ull;
                u32 const l_len = __shfl(len, src), l_ref = __shfl(my_ref, src), l_out = __shfl(my_out + head, src);
                bool const l_x = __shfl((int)is_x, src) != 0;
                for (u32 c = lane; c < l_len; c += 64u) {
                    u8 const ch = letter_at(l_ref + c);
                    if (l_x) { if (c) dst[l_out + 2u * c - 1u] = (u8)'0'; dst[l_out + 2u * c] = ch; }
                    else dst[l_out + c] = ch;
                }
            }
            // carries
            u32 const eq_total = __shfl(eq_incl, 63);
            u32 const eq_at_last = __shfl(eq_incl, ev_mask ? 63 - __builtin_clzll(ev_mask) : 0);
            pending = ev_mask ? eq_total - eq_at_last : pending + eq_total;
            ref_pos += __shfl(ref_incl, 63);
            out_pos += total;
        }
        if (!overflow) {                                               // the trailing count
            u32 const digits = dec_digits(pending);
            if (digits > cap - out_pos) overflow = true;
            else { if (lane == 0) put_dec(dst + out_pos, pending, digits); out_pos += digits; }
        }
        if (lane == 0) out[job.out_index] = DevMdOut{overflow ? 0xFFFFFFFFu : out_pos, 0u};
    }
}

int DeviceApi::md_build(void* stream, const u8* d_text, const u32* d_cigar, const DevTraceOut* d_trace_out, const DevMdJob* d_jobs, u32 n_jobs,
                        u8* d_md, DevMdOut* d_out) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(md_build_kernel, dim3(std::min(n_jobs, MD_GRID_CAP)), dim3(64), 0, (hipStream_t)stream, d_text, d_cigar, d_trace_out, d_jobs, n_jobs,
                       d_md, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
