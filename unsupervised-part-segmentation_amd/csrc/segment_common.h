// What the kernels over the packed planes of the segmentation export share (segexport.hip, components.hip): the packing table's
// layout and checks, and the overlay blend.  The definitions are DESIGN.md section 8's; tests/segexport_ref.py restates them.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace ups_segment {

constexpr int kWords = 4;                        // int32 words per table row: pixel_offset, h, w, first_block
constexpr int kChunk = 1024;                     // pixels of one block of the render kernels (ops.SEGMENT_CHUNK)

__device__ __forceinline__ unsigned to_byte(double v) {          // clamp(floor(v + 0.5), 0, 255)
    return (unsigned)fmin(fmax(floor(v + 0.5), 0.0), 255.0);
}

// one channel of the overlay over a source byte: clamp(floor(alpha * colour + (1 - alpha) * src + 0.5), 0, 255); oma = 1.0 - alpha
__device__ __forceinline__ unsigned blend(double alpha, double oma, unsigned col, unsigned src) {
    return to_byte(alpha * (double)col + oma * (double)src);
}

// the checks of a packing table, shared by the launchers: UPS_OK and the number of chunks (the grid of the render kernels)
inline int check_table(const int32_t* table_host, int n, long long total, long long* blocks_out) {
    long long blocks = 0, end = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* r = table_host + (long long)i * kWords;
        const long long off = r[0], h = r[1], w = r[2];
        UPS_CHECK_ARG(h >= 1 && w >= 1 && h * w <= 0x7fffffffLL);
        UPS_CHECK_ARG(off >= 0 && (off & 15) == 0);
        UPS_CHECK_ARG(off >= end && off + h * w <= total);                   // ascending, no overlap, inside the planes
        UPS_CHECK_ARG(r[3] == blocks);                                       // the prefix sum of the chunk counts
        end = off + h * w;
        blocks += (h * w + kChunk - 1) / kChunk;
        UPS_CHECK_ARG(blocks <= 0x7fffffffLL);
    }
    *blocks_out = blocks;
    return UPS_OK;
}

}  // namespace ups_segment
