// The host driver of the least-significant-digit radix sort over SortKey arrays (the launches: SortDevice, flx_sort.hpp; the kernels:
// flx_sort.hip), shared by the objects that order 128-bit keys on the device (flx_sort, flx_sv). It owns what a sort needs besides the
// keys themselves: the digit census, a pass's tile x digit table with its scan, and the ping-pong buffers, which its user sizes.
#pragma once
#include <utility>
#include <vector>

#include "flx_scan.hpp"
#include "flx_sort.hpp"

namespace flx {

struct RadixSorter {
    u32 tile_keys = SortDevice::TILE_KEYS;             // the keys one block orders per pass (a test hook of flx_sort)
    DeviceBuffer keys_a, keys_b, pay_a, pay_b;         // the ping-pong buffers: the user ensures the ones it passes to sort()
    DeviceBuffer table, census;                        // a pass's tile x digit table, the 16 x 256 digit counters
    ScanDriver scan;                                   // the table's scan

    // Orders a[0, n) with its payload pa; b and pb are the second buffers. On return *sorted_keys / *sorted_payload name the buffers that
    // hold the result, *passes the passes run. The stream is idle on return.
    int sort(hipStream_t stream, SortKey* a, SortKey* b, u32* pa, u32* pb, u64 n, SortKey** sorted_keys, u32** sorted_payload, u32* passes) {
        *sorted_keys = a;
        *sorted_payload = pa;
        *passes = 0;
        if (n <= 1) return FLX_OK;
        u32 const tile = (u32)sort_effective_tile(n, tile_keys, SortDevice::THREADS, ScanDevice::SCAN_TILE);
        u64 const n_tiles = (n + tile - 1) / tile, n_table = n_tiles * SORT_RADIX;
        int rc;
        if ((rc = census.ensure(SORT_DIGITS * SORT_RADIX * 4, true)) || (rc = table.ensure(n_table * 4)) || (rc = scan.reserve(n_table))) return rc;
        FLX_HIP(hipMemsetAsync(census.ptr, 0, SORT_DIGITS * SORT_RADIX * 4, stream));
        FLX_LAUNCH("sort_census", SortDevice::digit_census(stream, a, n, census.as<u32>()));
        std::vector<u32> counts(SORT_DIGITS * SORT_RADIX);
        FLX_HIP(hipMemcpyAsync(counts.data(), census.ptr, counts.size() * 4, hipMemcpyDeviceToHost, stream));
        FLX_HIP(hipStreamSynchronize(stream));
        for (u32 d = 0; d < SORT_DIGITS; ++d) {
            bool constant = false;                                          // one value in every key: the pass would move nothing
            for (u32 v = 0; v < SORT_RADIX; ++v) constant = constant || counts[d * SORT_RADIX + v] == n;
            if (constant) continue;
            u32* const t = table.as<u32>();
            FLX_LAUNCH("sort_histogram", SortDevice::histogram(stream, a, n, d, tile, t));
            if ((rc = scan.inclusive(stream, t, n_table))) return rc;       // (two levels at most: sort_effective_tile saw to it)
            FLX_LAUNCH("sort_scatter", SortDevice::scatter(stream, a, pa, n, d, tile, t, b, pb));
            std::swap(a, b);
            std::swap(pa, pb);
            ++*passes;
        }
        FLX_HIP(hipStreamSynchronize(stream));
        *sorted_keys = a;
        *sorted_payload = pa;
        return FLX_OK;
    }
    void release() { keys_a.release(); keys_b.release(); pay_a.release(); pay_b.release(); table.release(); }
};

}  // namespace flx
