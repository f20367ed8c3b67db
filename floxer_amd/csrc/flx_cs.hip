// K5s cs_build: the cs string (minimap2's difference string, short or long form; the rule: flx_cs.hpp) of every traced path, built on the
// device from the CIGAR words K5 (ed_traceback, flx_device.hip) has written - or cigar_realign / cigar_left_align behind it -, the
// reference text in HBM and the oriented query in the query pool. It is queued on the lane's stream directly behind md_build's place in
// the chain and reads the same DevTraceOut and words there: the host does not wait in between, and it needs no reference text of its own
// (a context made on an index image has none).
//
// One wave per job, one lane per CIGAR word, 64 words per pass. Unlike MD nothing merges across words: the bytes a word emits follow from
// (op, len, form) alone, so one exclusive scan gives every lane its output offset and two more its reference column and query row; no
// segmented scan. Three wave-uniform values carry from pass to pass: reference position, query position, output position. The scans are
// 64-bit: a word's length has 28 bits, and the sums are compared with the window, the query and the slab before anything is read or
// written, whatever the words say. Runs of up to 64 letters are written by their lane; longer ones by the whole wave, consecutive lanes
// on consecutive bytes, four letters per lane and store where the run is not X triples. With the long form that copy is most of the
// kernel's work: its output is about as long as the read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {

__device__ __forceinline__ u32 cs_dec_digits(u32 v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : 9u;      // (28 bits)
}
__device__ __forceinline__ void cs_put_dec(u8* p, u32 v, u32 digits) {
    for (u32 i = digits; i-- > 0;) { p[i] = (u8)('0' + v % 10u); v /= 10u; }
}
// 1..4 -> acgt, else n; upper: 32 (ACGT / N) or 0
__device__ __forceinline__ u32 cs_letter(u8 rank, u32 upper) {
    u32 const r = (u32)rank - 1u;
    return (r < 4u ? (0x74676361u >> (8u * r)) & 0xFFu : (u32)'n') - upper;
}

enum : u32 { CS_NONE = 0, CS_REF_UPPER = 1, CS_REF = 2, CS_QUERY = 3, CS_TRIPLES = 4 };     // what a word's letters are

}  // namespace

__global__ void __launch_bounds__(64) cs_build_kernel(const u8* __restrict__ text, const u8* __restrict__ query, const u32* __restrict__ cigar,
                                                      const DevTraceOut* __restrict__ trace_out, const DevCsJob* __restrict__ jobs, u32 n_jobs, u32 form,
                                                      u8* __restrict__ cs, DevCsOut* __restrict__ out) {
    u32 const lane = lane_id();
    bool const long_form = form == 2u;
    // (a grid no larger than the job list: a wave takes jobs in turn, as md_build's do)
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
        DevCsJob const job = jobs[id];
        DevTraceOut const t = trace_out[job.out_index];
        if (t.cigar_len == 0xFFFFFFFFu) {                              // a stage in front ran out of its slab: the host fails on that
            if (lane == 0) out[job.out_index] = DevCsOut{0u, 0u};
            continue;
        }
        const u8* __restrict__ r = text + job.ref_off;
        const u8* __restrict__ q = query + job.q_off;
        const u32* __restrict__ words = cigar + job.cigar_off + t.cigar_start;
        u8* __restrict__ dst = cs + job.cs_off;
        u32 const cap = job.cs_cap, n = job.n, m = job.m;
        u32 ref_pos = min(t.begin, n), q_pos = 0, out_pos = 0;         // the wave-uniform carries
        bool overflow = t.begin > n;
        for (u32 base = 0; base < t.cigar_len && !overflow; base += 64u) {
            u32 const w = base + lane < t.cigar_len ? words[base + lane] : 0u;
            u32 const op = w & 15u, len = w >> 4;
            bool const is_eq = op == 7u && len, is_x = op == 8u && len, is_i = op == 1u && len, is_d = op == 2u && len;
            // the word's first reference column and query row; a path that leaves its window or its query - K5 never writes one - is
            // reported like a slab that is too small
            i64 const ref_len = (is_eq || is_x || is_d) ? (i64)len : 0, q_len = (is_eq || is_x || is_i) ? (i64)len : 0;
            i64 const ref_incl = wave_inclusive_scan(ref_len), q_incl = wave_inclusive_scan(q_len);
            i64 const ref_total = __shfl(ref_incl, 63), q_total = __shfl(q_incl, 63);
            if (ref_total > (i64)(n - ref_pos) || q_total > (i64)(m - q_pos)) { overflow = true; break; }
            u32 const my_ref = ref_pos + (u32)(ref_incl - ref_len), my_q = q_pos + (u32)(q_incl - q_len);
            // bytes, from (op, len, form) alone
            u32 const digits = cs_dec_digits(len);
            u32 const kind = is_eq ? (long_form ? CS_REF_UPPER : CS_NONE) : is_x ? CS_TRIPLES : is_d ? CS_REF : is_i ? CS_QUERY : CS_NONE;
            u32 const head = (is_eq || is_i || is_d) ? 1u : 0u;        // the op's own character in front of its letters or digits
            i64 const bytes = is_x ? 3 * (i64)len : is_eq && !long_form ? (i64)(1u + digits) : head ? 1 + (i64)len : 0;
            i64 const out_incl = wave_inclusive_scan(bytes);
            i64 const total = __shfl(out_incl, 63);
            if (total > (i64)(cap - out_pos)) { overflow = true; break; }     // (out_pos <= cap always)
            u32 const my_out = out_pos + (u32)(out_incl - bytes);
            if (head) dst[my_out] = is_eq ? (long_form ? (u8)'=' : (u8)':') : is_i ? (u8)'+' : (u8)'-';
            if (is_eq && !long_form) cs_put_dec(dst + my_out + 1u, len, digits);
            if (kind != CS_NONE && len <= 64u) {
                u8* p = dst + my_out + head;
                if (kind == CS_TRIPLES) {
                    for (u32 c = 0; c < len; ++c) { *p++ = (u8)'*'; *p++ = (u8)cs_letter(r[my_ref + c], 0u); *p++ = (u8)cs_letter(q[my_q + c], 0u); }
                } else {
                    const u8* __restrict__ s = kind == CS_QUERY ? q + my_q : r + my_ref;
                    u32 const upper = kind == CS_REF_UPPER ? 32u : 0u;
                    for (u32 c = 0; c < len; ++c) p[c] = (u8)cs_letter(s[c], upper);
                }
            }
            // a run of more than 64 letters is copied by the whole wave
            u64 long_mask = __ballot(kind != CS_NONE && len > 64u);
            while (long_mask) {
                int const src = __builtin_ctzll(long_mask);
                long_mask &= long_mask - 1ull;
                u32 const l_kind = __shfl(kind, src), l_len = __shfl(len, src), l_ref = __shfl(my_ref, src), l_q = __shfl(my_q, src);
                u8* __restrict__ p = dst + __shfl(my_out + head, src);
                if (l_kind == CS_TRIPLES) {
                    // one lane per output byte: byte b belongs to column b / 3
                    for (u32 b = lane; b < 3u * l_len; b += 64u) {
                        u32 const c = b / 3u, role = b - 3u * c;
                        p[b] = role == 0u ? (u8)'*' : role == 1u ? (u8)cs_letter(r[l_ref + c], 0u) : (u8)cs_letter(q[l_q + c], 0u);
                    }
                    continue;
                }
                const u8* __restrict__ s = l_kind == CS_QUERY ? q + l_q : r + l_ref;
                u32 const upper = l_kind == CS_REF_UPPER ? 32u : 0u;
                // the bytes up to the first 4-byte boundary of the output one by one, then one aligned 4-byte store per lane, then the rest
                u32 const lead = min(l_len, (4u - (u32)((size_t)p & 3u)) & 3u), n_quads = (l_len - lead) / 4u;
                if (lane < lead) p[lane] = (u8)cs_letter(s[lane], upper);
                for (u32 d = lane; d < n_quads; d += 64u) {
                    u32 const c = lead + 4u * d;
                    u32 const v = cs_letter(s[c], upper) | cs_letter(s[c + 1u], upper) << 8 | cs_letter(s[c + 2u], upper) << 16 | cs_letter(s[c + 3u], upper) << 24;
                    *reinterpret_cast<u32*>(p + c) = v;
                }
                u32 const tail = lead + 4u * n_quads + lane;
                if (tail < l_len) p[tail] = (u8)cs_letter(s[tail], upper);
            }
            // carries
            ref_pos += (u32)ref_total;
            q_pos += (u32)q_total;
            out_pos += (u32)total;
        }
        if (lane == 0) out[job.out_index] = DevCsOut{overflow ? 0xFFFFFFFFu : out_pos, 0u};
    }
}

int DeviceApi::cs_build(void* stream, const u8* d_text, const u8* d_query, const u32* d_cigar, const DevTraceOut* d_trace_out, const DevCsJob* d_jobs,
                        u32 n_jobs, u32 form, u8* d_cs, DevCsOut* d_out) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(cs_build_kernel, dim3(std::min(n_jobs, CS_GRID_CAP)), dim3(64), 0, (hipStream_t)stream, d_text, d_query, d_cigar, d_trace_out, d_jobs,
                       n_jobs, form, d_cs, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
