// Coordinate order of records on the device (the rule: flx_sort.hpp; the object and the C ABI: flx_sort_api.cpp). Wave64 integer work:
//   sort_keys_add     one wave per record: the lanes stride the record's CIGAR words and sum the lengths of = X D, the wave reduces the
//                     sums, lane 0 packs {hi, lo} and {end, flag} into the record's slot of the table.
//   sort_census       one launch over all 16 digits of the keys: 16 x 256 counters per block in LDS (integer atomics), added to the
//                     global counters at the end. A digit with one value in every key has a counter equal to n: the host skips its pass.
//   sort_histogram    a pass's digit counts per tile, in LDS with integer atomics; table[value * n_tiles + tile].
//   (the scan)        the table's inclusive prefix sum with the reduce-then-scan launches of flx_scan.hip, two levels at most:
//                     the host grows the tiles before the table outgrows them (sort_effective_tile).
//   sort_scatter      stable: a block walks its tile 256 keys at a time. Within a wave the lanes with equal digits find each other with
//                     eight ballots (one per bit of the digit); a key's rank among them is the number of lower lanes in that mask. The
//                     first lane of each mask leaves the wave's count of the digit in LDS; a key's place is its digit's running base,
//                     plus the counts of the lower waves, plus its rank. The bases then advance by the step's counts.
// Least significant digit first, 8 bits a pass, keys and their u32 payload ping-pong between two buffers. No block waits for another
// block: no look-back, no flags, no spins. All stores are plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_sort.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {
constexpr u32 THREADS = SortDevice::THREADS;
constexpr u32 WAVES = THREADS / 64u;
static_assert(THREADS == SORT_RADIX, "thread t of a block owns digit value t");

__device__ __forceinline__ SortKey load_key(const SortKey* __restrict__ keys, u64 i) {
    ulonglong2 const x = reinterpret_cast<const ulonglong2*>(keys)[i];      // one 16-byte load
    return SortKey{x.x, x.y};
}
__device__ __forceinline__ void store_key(SortKey* __restrict__ keys, u64 i, SortKey const& k) {
    reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(k.hi, k.lo);
}
}  // namespace

// ------------------------------------------------------------------------------------------------ sort_keys_add
__global__ void __launch_bounds__(THREADS) sort_keys_add_kernel(const flx_record* __restrict__ records, u32 n, const u32* __restrict__ words,
                                                                u64 first_ordinal, SortKey* __restrict__ keys, SortMeta* __restrict__ meta) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * WAVES;
    for (u32 id = blockIdx.x * WAVES + (threadIdx.x >> 6); id < n; id += waves) {       // (id is wave-uniform)
        flx_record const r = records[id];
        u64 span = 0;
        for (u32 t = lane; t < r.cigar_length; t += 64u) {
            u32 const w = words[r.cigar_offset + t];
            if (sort_op_consumes(w & 15u)) span += w >> 4;
        }
#pragma unroll
        for (u32 d = 32u; d >= 1u; d >>= 1) span += __shfl_xor(span, d);
        if (lane == 0u) {
            bool const unplaced = sort_unplaced(r.flag, r.reference_id);
            store_key(keys, id, sort_key(r.flag, r.reference_id, r.position, first_ordinal + id));
            meta[id] = SortMeta{(u32)sort_end(unplaced, r.position, span), r.flag};
        }
    }
}

__global__ void __launch_bounds__(THREADS) sort_iota_kernel(u32* __restrict__ payload, u64 n) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) payload[i] = (u32)i;
}

// ------------------------------------------------------------------------------------------------ sort_census
__global__ void __launch_bounds__(THREADS) sort_census_kernel(const SortKey* __restrict__ keys, u64 n, u32* __restrict__ counts) {
    __shared__ u32 lds[SORT_DIGITS * SORT_RADIX];
    for (u32 c = threadIdx.x; c < SORT_DIGITS * SORT_RADIX; c += THREADS) lds[c] = 0u;
    __syncthreads();
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) {
        SortKey const k = load_key(keys, i);
        unsigned long long const active = __ballot(1);
        u32 const leader = (u32)__ffsll((long long)active) - 1u;
#pragma unroll
        for (u32 d = 0; d < SORT_DIGITS; ++d) {
            u32 const v = sort_digit(k, d);
            if (__all(v == (u32)__shfl((int)v, (int)leader))) {         // the common case, a digit that is constant: one add for the wave
                if (lane_id() == leader) atomicAdd(&lds[d * SORT_RADIX + v], (u32)__popcll(active));
            } else atomicAdd(&lds[d * SORT_RADIX + v], 1u);
        }
    }
    __syncthreads();
    for (u32 c = threadIdx.x; c < SORT_DIGITS * SORT_RADIX; c += THREADS)
        if (lds[c] != 0u) atomicAdd(&counts[c], lds[c]);
}

// ------------------------------------------------------------------------------------------------ sort_histogram
__global__ void __launch_bounds__(THREADS) sort_histogram_kernel(const SortKey* __restrict__ keys, u64 n, u32 digit, u32 tile_keys, u32* __restrict__ table) {
    __shared__ u32 lds[SORT_RADIX];
    lds[threadIdx.x] = 0u;
    __syncthreads();
    u64 const first = (u64)blockIdx.x * tile_keys, last = std::min<u64>(first + tile_keys, n);
    for (u64 i = first + threadIdx.x; i < last; i += THREADS) atomicAdd(&lds[sort_digit(load_key(keys, i), digit)], 1u);
    __syncthreads();
    table[(u64)threadIdx.x * gridDim.x + blockIdx.x] = lds[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ sort_scatter
// table: the histogram's table after its inclusive scan (entry e - 1 is the first place of entry e's keys)
__global__ void __launch_bounds__(THREADS) sort_scatter_kernel(const SortKey* __restrict__ keys, const u32* __restrict__ payload, u64 n, u32 digit,
                                                               u32 tile_keys, const u32* __restrict__ table, SortKey* __restrict__ keys_out,
                                                               u32* __restrict__ payload_out) {
    __shared__ u32 base[SORT_RADIX];                   // the next place of every digit value's keys
    __shared__ u32 wave_count[WAVES][SORT_RADIX];      // this step's keys per wave and digit value
    u32 const lane = lane_id(), wave = threadIdx.x >> 6;
    {
        u64 const e = (u64)threadIdx.x * gridDim.x + blockIdx.x;
        base[threadIdx.x] = e > 0 ? table[e - 1] : 0u;
#pragma unroll
        for (u32 w = 0; w < WAVES; ++w) wave_count[w][threadIdx.x] = 0u;
    }
    __syncthreads();
    u64 const first = (u64)blockIdx.x * tile_keys, last = std::min<u64>(first + tile_keys, n);
    for (u64 at = first; at < last; at += THREADS) {                   // (at is block-uniform: every thread takes every barrier)
        u64 const i = at + threadIdx.x;
        bool const valid = i < last;
        SortKey k{0, 0};
        u32 p = 0, v = 0;
        if (valid) { k = load_key(keys, i); p = payload[i]; v = sort_digit(k, digit); }
        unsigned long long peers = __ballot(valid);                    // the valid lanes of this wave with this lane's digit value
#pragma unroll
        for (u32 b = 0; b < SORT_DIGIT_BITS; ++b) {
            bool const set = (v >> b & 1u) != 0u;
            unsigned long long const with = __ballot(valid && set);
            peers &= set ? with : ~with;
        }
        u32 const rank = (u32)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wave_count[wave][v] = (u32)__popcll(peers);
        __syncthreads();
        if (valid) {
            u32 place = base[v] + rank;
            for (u32 w = 0; w < wave; ++w) place += wave_count[w][v];
            store_key(keys_out, place, k);                             // (place < n: the table counted exactly these keys)
            payload_out[place] = p;
        }
        __syncthreads();
        {
            u32 step = 0;
#pragma unroll
            for (u32 w = 0; w < WAVES; ++w) { step += wave_count[w][threadIdx.x]; wave_count[w][threadIdx.x] = 0u; }
            base[threadIdx.x] += step;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ sort_entries
__global__ void __launch_bounds__(THREADS) sort_entries_kernel(const SortKey* __restrict__ keys, const u32* __restrict__ payload, const SortMeta* __restrict__ meta,
                                                               u64 n, flx_sort_entry* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) {
        SortKey const k = load_key(keys, i);
        SortMeta const m = meta[payload[i]];
        flx_sort_entry e;
        e.ordinal = sort_key_ordinal(k);
        e.reference_id = sort_key_reference(k);
        e.position = sort_key_position(k);
        e.end = m.end;
        e.flag = m.flag;
        out[i] = e;
    }
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
static inline u32 strided_blocks(u64 n, u32 cap) { return (u32)std::min<u64>((n + THREADS - 1) / THREADS, cap); }
static inline u32 tiles_of(u64 n, u32 tile_keys) { return (u32)((n + tile_keys - 1) / tile_keys); }

int SortDevice::keys_add(void* stream, const flx_record* d_records, uint32_t n, const uint32_t* d_words, uint64_t first_ordinal, SortKey* d_keys, SortMeta* d_meta) {
    if (n == 0) return 0;
    u32 const blocks = std::min<u32>((n + WAVES - 1) / WAVES, KEYS_GRID_CAP);
    hipLaunchKernelGGL(sort_keys_add_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_records, n, d_words, first_ordinal, d_keys, d_meta);
    return (int)hipGetLastError();
}
int SortDevice::iota(void* stream, uint32_t* d_payload, uint64_t n) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sort_iota_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_payload, n);
    return (int)hipGetLastError();
}
int SortDevice::digit_census(void* stream, const SortKey* d_keys, uint64_t n, uint32_t* d_counts) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sort_census_kernel, dim3(strided_blocks(n, CENSUS_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_keys, n, d_counts);
    return (int)hipGetLastError();
}
int SortDevice::histogram(void* stream, const SortKey* d_keys, uint64_t n, uint32_t digit, uint32_t tile_keys, uint32_t* d_table) {
    hipLaunchKernelGGL(sort_histogram_kernel, dim3(tiles_of(n, tile_keys)), dim3(THREADS), 0, (hipStream_t)stream, d_keys, n, digit, tile_keys, d_table);
    return (int)hipGetLastError();
}
int SortDevice::scatter(void* stream, const SortKey* d_keys, const uint32_t* d_payload, uint64_t n, uint32_t digit, uint32_t tile_keys, const uint32_t* d_table,
                        SortKey* d_keys_out, uint32_t* d_payload_out) {
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles_of(n, tile_keys)), dim3(THREADS), 0, (hipStream_t)stream, d_keys, d_payload, n, digit, tile_keys, d_table,
                       d_keys_out, d_payload_out);
    return (int)hipGetLastError();
}
int SortDevice::entries(void* stream, const SortKey* d_keys, const uint32_t* d_payload, const SortMeta* d_meta, uint64_t n, void* d_entries) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sort_entries_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_keys, d_payload, d_meta, n,
                       reinterpret_cast<flx_sort_entry*>(d_entries));
    return (int)hipGetLastError();
}

}  // namespace flx
