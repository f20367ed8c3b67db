// The inclusive prefix sum over u32 arrays that the side objects share (coverage, pileup, sort): the launches of flx_scan.hip and the one
// host driver of their levels. Reduce-then-scan: sums per tile, the scan of the tile sums (the same launches again while there are more
// sums than one tile), the apply pass. All of it u32 sums modulo 2^32.
#pragma once
#include <vector>

#include "flx_context.hpp"

namespace flx {

// ---- the launches of flx_scan.hip (each returns the hipError_t of its launch; pointers are device pointers, the arrays 256-byte aligned)
struct ScanDevice {
    static constexpr u32 SCAN_TILE = 4096;             // elements per scan tile, and tile sums one block of the next level scans
    static int scan_sums(void* stream, const u32* d_a, u64 n, u32* d_sums);
    static int scan_apply(void* stream, u32* d_a, u64 n, const u32* d_scanned);      // d_scanned: null for an array of one tile
    static int sum(void* stream, u32* d_into, const u32* d_from, u64 n);              // into += from
};

// The tile sums of every level, one array per level. Level k has room for the sums of an array of tiles^k(n_reserved) elements, so any
// array of up to n_reserved elements is scanned from level 0.
struct ScanDriver {
    DeviceBuffer sums;
    std::vector<u64> level_off;                        // in entries; every level starts 256-byte aligned
    u64 n_reserved = 0;

    static u64 tiles(u64 n) { return (n + ScanDevice::SCAN_TILE - 1) / ScanDevice::SCAN_TILE; }

    // grow-only (contents are not kept: the stream must be done with an earlier scan)
    int reserve(u64 n) {
        if (n <= n_reserved) return FLX_OK;
        std::vector<u64> off;
        u64 entries = 0;
        for (u64 nt = tiles(n); nt > 1; nt = tiles(nt)) { off.push_back(entries); entries += (nt + 63) / 64 * 64; }
        if (entries) { int const rc = sums.ensure(entries * 4, true); if (rc) return rc; }
        level_off.swap(off);
        n_reserved = n;
        return FLX_OK;
    }
    // inclusive prefix sum of a[0, n) in place, n <= n_reserved
    int inclusive(hipStream_t stream, u32* a, u64 n) {
        if (n > n_reserved) { set_error("scan: an array beyond the reserved size"); return FLX_ERR_INTERNAL; }
        return level(stream, a, n, 0);
    }

private:
    int level(hipStream_t stream, u32* a, u64 n, size_t k) {
        u64 const nt = tiles(n);
        if (nt <= 1) { FLX_LAUNCH("scan_apply", ScanDevice::scan_apply(stream, a, n, nullptr)); return FLX_OK; }
        u32* const s = sums.as<u32>() + level_off[k];
        FLX_LAUNCH("scan_sums", ScanDevice::scan_sums(stream, a, n, s));
        int const rc = level(stream, s, nt, k + 1);
        if (rc) return rc;
        FLX_LAUNCH("scan_apply", ScanDevice::scan_apply(stream, a, n, s));
        return FLX_OK;
    }
};

}  // namespace flx
