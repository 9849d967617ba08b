// Segmentation export (declared in include/upsparts_hip.h): ups_segment_render -- label maps, colour overlays, confidence maps and
// per-part pixel counts of a whole pass of images from the S x S soft-max maps, every image at ITS OWN output size, in one launch.
// (Its edge-aware variant, ups_segment_guide + ups_segment_render_guided, is further down with its own header.)
//
// The reference never leaves the model's resolution (it resizes the ground truth DOWN to it): the definitions are this project's
//  and tests/segexport_ref.py restates them in NumPy float64.  For output pixel (y, x) of an h x w image:
//     sy = ((y + 0.5) * S) / h - 0.5, clamped to [0, S-1];  y0 = floor(sy), y1 = min(y0 + 1, S-1), fy = sy - y0      (x alike)
//     top = (1-fx) a00 + fx a01,  bot = (1-fx) a10 + fx a11,  v_p = (1-fy) top + fy bot         on the fp32 values widened to fp64
//     label = first p with maximal v_p;   confidence = clamp(floor(v_label * 255 + 0.5), 0, 255)
//     overlay_c = clamp(floor(alpha * colour[label][c] + (1-alpha) * src_c + 0.5), 0, 255);   without src: colour[label][c]
// Every decision is taken in fp64 with contraction off and the correctly rounded fp64 division: each operation is the IEEE operation
// NumPy performs in the same order, so the bytes are the restatement's bytes.  At h = w = S the weights are exactly 0 and 1 and the
// label is the first maximal index of the soft-max itself (out_parts_hard).  `soft` is expected finite (a soft-max is).
//
// Form.  The outputs of image i are packed at table[i].pixel_offset (a multiple of 16: every image starts 16-byte aligned in the
// uint8 planes).  An image is cut into chunks of kChunk = 1024 consecutive pixels, one 256-thread block per chunk; table[i].first_block
// is the prefix sum of the chunk counts, and a block finds its image by a binary search on it (wave-uniform: scalar loads) -- a pass of
// many small images fills the chip as well as one of few large ones, as ups_part_confusion's chunking does.
// A lane owns 4 CONSECUTIVE pixels (they may wrap into the next row): it stores its labels and its confidences as one dword each,
// its overlay as three dwords, and reads its 12 source bytes as three dwords.  Only the last lane of an image whose pixel count is no
// multiple of 4 stores bytes, at most 3 of each plane: the alignment gap behind an image is never written.
// The four corner rows of a pixel are P contiguous floats each.  They are read straight from global memory, NOT staged in LDS: a
// chunk's footprint in `soft` is a few source rows when the image is enlarged (the common case: 1024 pixels of a 500-wide image touch
// 2 .. 3 of the 128 source rows, ~15 KB, and neighbouring lanes hit the same lines in L1) but the whole map when it is shrunk, so a
// staged form would need this direct form as its fall-back anyway -- two paths to keep bit-equal for a kernel whose bytes to move are
// the outputs.  There is no dynamic LDS; the static LDS is the 1 KB histogram and the 768-byte colour table.
// Counts: a lane carries a (label, run length) pair over its 4 pixels, LDS sees one integer atomic per run, and the block adds its
// non-zero bins to counts[image] with one global integer atomic per part: integer sums, independent of geometry and block order.
// `counts` is ADDED to (caller-zeroed, or holding earlier launches' counts), as ups_part_confusion's.
#include "common.h"
#include "segment_common.h"

#pragma clang fp contract(off)

namespace {

using ups_segment::blend;
using ups_segment::check_table;
using ups_segment::to_byte;

constexpr int kBlock = 256;                      // threads per block
constexpr int kPerLane = 4;                      // consecutive pixels of one lane: one dword of labels
constexpr int kChunk = ups_segment::kChunk;      // pixels of one block: 1024 (ops.SEGMENT_CHUNK)
constexpr int kWords = ups_segment::kWords;      // int32 words per table row: pixel_offset, h, w, first_block
static_assert(kChunk == kBlock * kPerLane, "a block covers one chunk");
constexpr int kMaxP = 255;                       // a label is a byte
static_assert(kBlock == 256, "the histogram is cleared one bin per thread");

// source coordinate of output index i of an extent n: the two taps and the weight of the second
__device__ __forceinline__ void source_coord(int i, int n, int S, int& i0, int& i1, double& f) {
    double s = (((double)i + 0.5) * (double)S) / (double)n - 0.5;
    s = fmin(fmax(s, 0.0), (double)(S - 1));
    const double fl = floor(s);
    i0 = (int)fl;
    i1 = min(i0 + 1, S - 1);
    f = s - fl;
}

__global__ __launch_bounds__(kBlock) void segment_render_kernel(const float* __restrict__ soft, const int* __restrict__ table, int n,
                                                                int S, int P, const uint8_t* __restrict__ src,
                                                                const uint8_t* __restrict__ colors, double alpha,
                                                                uint8_t* __restrict__ labels, uint8_t* __restrict__ overlay,
                                                                uint8_t* __restrict__ conf, int* __restrict__ counts) {
    __shared__ int bins[256];
    __shared__ uint8_t scol[256 * 3];
    const int tid = threadIdx.x;
    bins[tid] = 0;
    if (overlay)
        for (int t = tid; t < 3 * P; t += kBlock) scol[t] = colors[t];
    // the image of this block: the last row whose first_block is <= blockIdx.x (first_block is strictly increasing from 0)
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * kWords + 3] <= b) lo = mid;
        else hi = mid - 1;
    }
    const int img = lo;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int hw = h * w;                                                    // <= 2^31 - 1 (checked by the launcher)
    const long long q0l = (long long)(b - table[img * kWords + 3]) * kChunk + (long long)tid * kPerLane;
    __syncthreads();

    const int npx = q0l >= hw ? 0 : (hw - q0l >= kPerLane ? kPerLane : (int)(hw - q0l));      // pixels of this lane
    if (npx > 0) {
        const int q0 = (int)q0l;
        const float* simg = soft + (long long)img * S * S * P;
        const double oma = 1.0 - alpha;
        int y = q0 / w, x = q0 - y * w;
        int row0 = 0, row1 = 0;                                              // element offsets of the two source rows in the image's map
        double fy = 0.0;
        unsigned lab[kPerLane] = {0, 0, 0, 0}, cf[kPerLane] = {0, 0, 0, 0};
        unsigned sw[3] = {0, 0, 0};                                          // the lane's 12 source bytes
        if (overlay && src) {
            const uint8_t* sp = src + 3 * (off + q0);
            if (npx == kPerLane) {
#pragma unroll
                for (int k = 0; k < 3; ++k) sw[k] = reinterpret_cast<const unsigned*>(sp)[k];
            } else {
#pragma unroll
                for (int k = 0; k < 3 * kPerLane; ++k)
                    if (k < 3 * npx) sw[k >> 2] |= (unsigned)sp[k] << (8 * (k & 3));
            }
        }
        unsigned ow[3] = {0, 0, 0};                                          // the lane's 12 overlay bytes
        int run_key = -1, run_len = 0;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            if (k < npx) {
                if (k == 0 || x == 0) {                                      // a new output row
                    int y0, y1;
                    source_coord(y, h, S, y0, y1, fy);
                    row0 = y0 * S * P;                                       // S * S * P < 2^29 (launcher): int offsets
                    row1 = y1 * S * P;
                }
                int x0, x1;
                double fx;
                source_coord(x, w, S, x0, x1, fx);
                const double gx = 1.0 - fx, gy = 1.0 - fy;
                const float* r00 = simg + (row0 + x0 * P);
                const float* r01 = simg + (row0 + x1 * P);
                const float* r10 = simg + (row1 + x0 * P);
                const float* r11 = simg + (row1 + x1 * P);
                double best = 0.0;
                int arg = 0;
#pragma unroll 2
                for (int p = 0; p < P; ++p) {
                    const double top = gx * (double)r00[p] + fx * (double)r01[p];
                    const double bot = gx * (double)r10[p] + fx * (double)r11[p];
                    const double v = gy * top + fy * bot;
                    if (p == 0 || v > best) {
                        best = v;
                        arg = p;
                    }
                }
                lab[k] = (unsigned)arg;
                cf[k] = to_byte(best * 255.0);
                if (overlay) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int e = 3 * k + c;
                        const unsigned col = scol[arg * 3 + c];
                        unsigned o = col;
                        if (src) o = blend(alpha, oma, col, (sw[e >> 2] >> (8 * (e & 3))) & 255u);
                        ow[e >> 2] |= o << (8 * (e & 3));
                    }
                }
                if (arg == run_key) {
                    ++run_len;
                } else {
                    if (counts && run_key >= 0) atomicAdd(&bins[run_key], run_len);
                    run_key = arg;
                    run_len = 1;
                }
                if (++x == w) {
                    x = 0;
                    ++y;
                }
            }
        }
        if (counts) atomicAdd(&bins[run_key], run_len);
        const long long at = off + q0;                                       // a multiple of 4
        if (npx == kPerLane) {
            if (labels) *reinterpret_cast<unsigned*>(labels + at) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            if (conf) *reinterpret_cast<unsigned*>(conf + at) = cf[0] | (cf[1] << 8) | (cf[2] << 16) | (cf[3] << 24);
            if (overlay) {
                unsigned* op = reinterpret_cast<unsigned*>(overlay + 3 * at);
#pragma unroll
                for (int k = 0; k < 3; ++k) op[k] = ow[k];
            }
        } else {                                                             // the last 1 .. 3 pixels of an image: the gap stays untouched
#pragma unroll
            for (int k = 0; k < kPerLane - 1; ++k) {
                if (k < npx) {
                    if (labels) labels[at + k] = (uint8_t)lab[k];
                    if (conf) conf[at + k] = (uint8_t)cf[k];
                }
            }
            if (overlay) {
#pragma unroll
                for (int k = 0; k < 3 * (kPerLane - 1); ++k)
                    if (k < 3 * npx) overlay[3 * at + k] = (uint8_t)(ow[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
    if (counts) {
        __syncthreads();
        if (tid < P) {
            const int v = bins[tid];
            if (v) atomicAdd(&counts[(long long)img * P + tid], v);
        }
    }
}

// ---------------------------------------------------------------------------------------------- edge-aware refinement
// Joint bilateral upsampling (Kopf et al. 2007) guided by the photograph; the definitions are DESIGN.md section 8's and
// tests/segrefine_ref.py restates them with equal bytes.  Two launches per pass:
//   ups_segment_guide          G[i] uint8 [S,S,3]: the rounded box mean of the source pixels tap (ty, tx) covers.  Integer only.
//   ups_segment_render_guided  ups_segment_render's outer form (planes, chunks, binary search, 4 pixels per lane, dword stores, LDS
//                              histogram) with the 4 bilinear taps replaced by the (2R+2)^2 window around (y0, x0): tap weight
//                              w = (wy * wx) * wr[d1], a tent of radius R+1 times the range table at the L1 distance d1 of the output
//                              pixel's source bytes from the guide under the tap; a tap outside the map is skipped.
//                              num_p = sum w soft_p and den = sum w in tap order (j outer), each product and sum rounded once;
//                              label = first p of maximal num_p, confidence = to_byte((num_label / den) * 255).
// The range table (766 doubles, built on the host: the kernel evaluates no transcendental) is read into LDS once per block.
constexpr int kRange = 766;                      // d1 = 0 .. 3 * 255
constexpr int kMaxR = 3;                         // window radius: (2R+2)^2 <= 64 taps
constexpr int kPB = 16;                          // part accumulators a lane holds in registers: P > 16 takes further passes over the taps
constexpr int kGTile = 256;                      // taps of a guide row summed in LDS at a time

// the source rows [ya, yb), columns [qa, qb) of one tile of taps t0 .. tl, added to the tile's LDS sums.  I: the integer type of the
// byte index and of q * S (unsigned where 3 w and (w + 1) S fit in 31 bits -- every photograph -- else 64-bit)
template <typename I>
__device__ __forceinline__ void guide_rows(unsigned long long* sum, const uint8_t* simg, int ya, int yb, int qa, int qb, int w, int S,
                                           int t0, int tl, int tid) {
    for (int r = ya; r < yb; ++r) {
        const uint8_t* rp = simg + 3LL * r * w;
        for (I e = (I)3 * (I)qa + (I)tid; e < (I)3 * (I)qb; e += (I)kBlock) {
            const I q = e / 3;
            const int c = (int)(e - 3 * q);
            int thi = (int)(((q + 1) * (I)S - 1) / (I)w);                                        // the last tap with a_t <= q
            int tlo = w >= S ? thi : (int)((q * (I)S + (I)(w - 1)) / (I)w);                      // w < S: the first tap with a_t == q
            tlo = max(tlo, t0);
            thi = min(thi, tl);
            const unsigned long long v = rp[e];
            for (int t = tlo; t <= thi; ++t) atomicAdd(&sum[(t - t0) * 3 + c], v);
        }
    }
}

// One block per (image, tap row ty): consecutive lanes read consecutive bytes of the source rows [ya, yb) and add them to the LDS sums
// of the taps whose column range holds the byte's pixel -- exactly one tap when w >= S (the ranges partition the row); when w < S every
// tap is the single column a_t and several taps share it.  Integer LDS atomics: the sums do not depend on the order.
__global__ __launch_bounds__(kBlock) void segment_guide_kernel(const uint8_t* __restrict__ src, const int* __restrict__ table, int S,
                                                               uint8_t* __restrict__ guide) {
    __shared__ unsigned long long sum[kGTile * 3];
    const int tid = threadIdx.x;
    const int img = (int)blockIdx.x / S, ty = (int)blockIdx.x - img * S;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int ya = (int)(((long long)ty * h) / S);
    const int yb = max(ya + 1, (int)(((long long)(ty + 1) * h) / S));
    const uint8_t* simg = src + 3 * off;
    uint8_t* grow = guide + (long long)blockIdx.x * S * 3;
    const bool narrow = ((long long)w + 1) * S < 0x7fffffffLL && 3LL * w < 0x7fff0000LL;
    for (int t0 = 0; t0 < S; t0 += kGTile) {
        const int tc = min(kGTile, S - t0), tl = t0 + tc - 1;
        for (int i = tid; i < 3 * tc; i += kBlock) sum[i] = 0ull;
        __syncthreads();
        const int qa = (int)(((long long)t0 * w) / S);                                           // the columns of taps t0 .. tl
        const int qb = max((int)(((long long)tl * w) / S) + 1, (int)(((long long)(tl + 1) * w) / S));
        if (narrow) guide_rows<unsigned>(sum, simg, ya, yb, qa, qb, w, S, t0, tl, tid);
        else guide_rows<long long>(sum, simg, ya, yb, qa, qb, w, S, t0, tl, tid);
        __syncthreads();
        for (int i = tid; i < 3 * tc; i += kBlock) {
            const int t = t0 + i / 3;
            const int xa = (int)(((long long)t * w) / S);
            const int xb = max(xa + 1, (int)(((long long)(t + 1) * w) / S));
            const unsigned long long cnt = (unsigned long long)(yb - ya) * (unsigned long long)(xb - xa);
            grow[3 * t0 + i] = (uint8_t)((2ull * sum[i] + cnt) / (2ull * cnt));
        }
        __syncthreads();
    }
}

// v / (double)(R + 1): where R + 1 is a power of two (R = 0, 1, 3) the correctly rounded quotient IS the product with the exact
// reciprocal (v is in [0, R + 1], far from the subnormals), which spares the ~40 instructions of an fp64 division per weight
template <int R>
__device__ __forceinline__ double over_radius(double v) {
    if constexpr (((R + 1) & R) == 0) return v * (1.0 / (double)(R + 1));
    else return v / (double)(R + 1);
}

template <int R>
__global__ __launch_bounds__(kBlock) void segment_render_guided_kernel(const float* __restrict__ soft, const int* __restrict__ table, int n,
                                                                       int S, int P, const uint8_t* __restrict__ src,
                                                                       const uint8_t* __restrict__ guide, const double* __restrict__ range_w,
                                                                       const uint8_t* __restrict__ colors, double alpha,
                                                                       uint8_t* __restrict__ labels, uint8_t* __restrict__ overlay,
                                                                       uint8_t* __restrict__ conf, int* __restrict__ counts) {
    constexpr int T = 2 * R + 2;                                             // taps per axis: j, k = -R .. R+1
    __shared__ int bins[256];
    __shared__ uint8_t scol[256 * 3];
    __shared__ double swr[kRange];
    const int tid = threadIdx.x;
    bins[tid] = 0;
    if (overlay)
        for (int t = tid; t < 3 * P; t += kBlock) scol[t] = colors[t];
    for (int t = tid; t < kRange; t += kBlock) swr[t] = range_w[t];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * kWords + 3] <= b) lo = mid;
        else hi = mid - 1;
    }
    const int img = lo;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int hw = h * w;
    const long long q0l = (long long)(b - table[img * kWords + 3]) * kChunk + (long long)tid * kPerLane;
    __syncthreads();

    const int npx = q0l >= hw ? 0 : (hw - q0l >= kPerLane ? kPerLane : (int)(hw - q0l));
    if (npx > 0) {
        const int q0 = (int)q0l;
        const float* simg = soft + (long long)img * S * S * P;
        const uint8_t* gimg = guide + (long long)img * S * S * 3;            // 3 S S < 2^31 (launcher): int offsets
        const double oma = 1.0 - alpha;
        int y = q0 / w, x = q0 - y * w;
        int y0 = 0;
        double fy = 0.0;
        unsigned lab[kPerLane] = {0, 0, 0, 0}, cf[kPerLane] = {0, 0, 0, 0};
        unsigned sw[3] = {0, 0, 0};                                          // the lane's 12 source bytes
        {
            const uint8_t* sp = src + 3 * (off + q0);
            if (npx == kPerLane) {
#pragma unroll
                for (int k = 0; k < 3; ++k) sw[k] = reinterpret_cast<const unsigned*>(sp)[k];
            } else {
#pragma unroll
                for (int k = 0; k < 3 * kPerLane; ++k)
                    if (k < 3 * npx) sw[k >> 2] |= (unsigned)sp[k] << (8 * (k & 3));
            }
        }
        unsigned ow[3] = {0, 0, 0};
        int run_key = -1, run_len = 0;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            if (k < npx) {
                if (k == 0 || x == 0) {                                      // a new output row
                    int y1;
                    source_coord(y, h, S, y0, y1, fy);
                }
                int x0, x1;
                double fx;
                source_coord(x, w, S, x0, x1, fx);
                int px[3];                                                   // this pixel's source bytes
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c] = (int)((sw[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255u);
                double wx[T];
#pragma unroll
                for (int kk = 0; kk < T; ++kk) wx[kk] = 1.0 - over_radius<R>(fabs(fx - (double)(kk - R)));
                double best = 0.0, den = 0.0;
                int arg = 0;
                for (int pb = 0; pb < P; pb += kPB) {                        // every num_p is its own chain: a pass per 16 parts
                    double acc[kPB];
#pragma unroll
                    for (int q = 0; q < kPB; ++q) acc[q] = 0.0;
                    double d = 0.0;
                    for (int jj = 0; jj < T; ++jj) {
                        const int ty = y0 + jj - R;
                        if (ty < 0 || ty >= S) continue;                     // a tap outside the map is skipped, not repeated
                        const double wy = 1.0 - over_radius<R>(fabs(fy - (double)(jj - R)));
#pragma unroll
                        for (int kk = 0; kk < T; ++kk) {
                            const int tx = x0 + kk - R;
                            if (tx < 0 || tx >= S) continue;
                            const int tap = ty * S + tx;
                            const uint8_t* g = gimg + 3 * tap;
                            const int d1 = abs(px[0] - (int)g[0]) + abs(px[1] - (int)g[1]) + abs(px[2] - (int)g[2]);
                            const double wt = (wy * wx[kk]) * swr[d1];
                            d = d + wt;
                            const float* row = simg + (tap * P + pb);        // S * S * P < 2^29 (launcher)
#pragma unroll
                            for (int q = 0; q < kPB; ++q)
                                if (pb + q < P) acc[q] = acc[q] + wt * (double)row[q];
                        }
                    }
                    den = d;                                                 // the same chain in every pass
#pragma unroll
                    for (int q = 0; q < kPB; ++q) {
                        if (pb + q < P && (pb + q == 0 || acc[q] > best)) {
                            best = acc[q];
                            arg = pb + q;
                        }
                    }
                }
                lab[k] = (unsigned)arg;
                cf[k] = to_byte((best / den) * 255.0);
                if (overlay) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int e = 3 * k + c;
                        const unsigned o = blend(alpha, oma, scol[arg * 3 + c], (unsigned)px[c]);
                        ow[e >> 2] |= o << (8 * (e & 3));
                    }
                }
                if (arg == run_key) {
                    ++run_len;
                } else {
                    if (counts && run_key >= 0) atomicAdd(&bins[run_key], run_len);
                    run_key = arg;
                    run_len = 1;
                }
                if (++x == w) {
                    x = 0;
                    ++y;
                }
            }
        }
        if (counts) atomicAdd(&bins[run_key], run_len);
        const long long at = off + q0;                                       // a multiple of 4
        if (npx == kPerLane) {
            if (labels) *reinterpret_cast<unsigned*>(labels + at) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            if (conf) *reinterpret_cast<unsigned*>(conf + at) = cf[0] | (cf[1] << 8) | (cf[2] << 16) | (cf[3] << 24);
            if (overlay) {
                unsigned* op = reinterpret_cast<unsigned*>(overlay + 3 * at);
#pragma unroll
                for (int k = 0; k < 3; ++k) op[k] = ow[k];
            }
        } else {                                                             // the last 1 .. 3 pixels of an image: the gap stays untouched
#pragma unroll
            for (int k = 0; k < kPerLane - 1; ++k) {
                if (k < npx) {
                    if (labels) labels[at + k] = (uint8_t)lab[k];
                    if (conf) conf[at + k] = (uint8_t)cf[k];
                }
            }
            if (overlay) {
#pragma unroll
                for (int k = 0; k < 3 * (kPerLane - 1); ++k)
                    if (k < 3 * npx) overlay[3 * at + k] = (uint8_t)(ow[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
    if (counts) {
        __syncthreads();
        if (tid < P) {
            const int v = bins[tid];
            if (v) atomicAdd(&counts[(long long)img * P + tid], v);
        }
    }
}

}  // namespace

extern "C" int32_t ups_segment_chunk(void) { return kChunk; }
extern "C" int32_t ups_segment_table_words(void) { return kWords; }

extern "C" int ups_segment_render(const float* soft, int32_t n, int32_t S, int32_t P, const int32_t* table_host, const int32_t* table,
                                  int64_t total, const uint8_t* src, const uint8_t* colors, double alpha, uint8_t* labels,
                                  uint8_t* overlay, uint8_t* confidence, int32_t* counts, void* stream) {
    UPS_CHECK_ARG(soft && table_host && table);
    UPS_CHECK_ARG(n >= 1 && S >= 1 && P >= 1);
    if (P > kMaxP) {
        ups_set_error("ups_segment_render: P <= 255, a label is a byte (got P = %d)", P);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG(labels || overlay || confidence || counts);
    UPS_CHECK_ARG(!overlay || colors);
    UPS_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0);
    UPS_CHECK_ARG(total >= 1 && total <= 0x7fffffffLL);
    UPS_CHECK_ARG((long long)S * S * P < (1LL << 29) && (long long)n * P <= 0x7fffffffLL);      // int element and byte offsets in a map
    // dword stores and loads: every plane starts on a dword (an image's pixel_offset is a multiple of 16, a lane's first pixel of 4)
    UPS_CHECK_ARG((((uintptr_t)labels | (uintptr_t)overlay | (uintptr_t)confidence | (uintptr_t)src | (uintptr_t)counts) & 3) == 0);
    long long blocks = 0;
    if (const int rc = check_table(table_host, n, total, &blocks)) return rc;
    hipLaunchKernelGGL(segment_render_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, soft, table, n, S, P, src,
                       colors, alpha, labels, overlay, confidence, counts);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_segment_guide(const uint8_t* src, int32_t n, int32_t S, const int32_t* table_host, const int32_t* table, int64_t total,
                                 uint8_t* guide, void* stream) {
    UPS_CHECK_ARG(src && table_host && table && guide);
    UPS_CHECK_ARG(n >= 1 && S >= 1);
    UPS_CHECK_ARG(total >= 1 && total <= 0x7fffffffLL);
    UPS_CHECK_ARG((long long)S * S < (1LL << 29) && (long long)n * S <= 0x7fffffffLL);           // int offsets in a guide; one block per tap row
    long long blocks = 0;
    if (const int rc = check_table(table_host, n, total, &blocks)) return rc;
    hipLaunchKernelGGL(segment_guide_kernel, dim3((unsigned)((long long)n * S)), dim3(kBlock), 0, (hipStream_t)stream, src, table, S, guide);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_segment_render_guided(const float* soft, int32_t n, int32_t S, int32_t P, const int32_t* table_host,
                                         const int32_t* table, int64_t total, const uint8_t* src, const uint8_t* guide,
                                         const double* range_w, int32_t R, const uint8_t* colors, double alpha, uint8_t* labels,
                                         uint8_t* overlay, uint8_t* confidence, int32_t* counts, void* stream) {
    UPS_CHECK_ARG(soft && table_host && table);
    UPS_CHECK_ARG(src && guide && range_w);
    UPS_CHECK_ARG(n >= 1 && S >= 1 && P >= 1);
    if (P > kMaxP) {
        ups_set_error("ups_segment_render_guided: P <= 255, a label is a byte (got P = %d)", P);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG(R >= 0 && R <= kMaxR);
    UPS_CHECK_ARG(labels || overlay || confidence || counts);
    UPS_CHECK_ARG(!overlay || colors);
    UPS_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0);
    UPS_CHECK_ARG(total >= 1 && total <= 0x7fffffffLL);
    UPS_CHECK_ARG((long long)S * S * P < (1LL << 29) && (long long)n * P <= 0x7fffffffLL);
    UPS_CHECK_ARG((((uintptr_t)labels | (uintptr_t)overlay | (uintptr_t)confidence | (uintptr_t)src | (uintptr_t)counts) & 3) == 0);
    UPS_CHECK_ARG(((uintptr_t)range_w & 7) == 0);
    long long blocks = 0;
    if (const int rc = check_table(table_host, n, total, &blocks)) return rc;
    const dim3 grid((unsigned)blocks), block(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define UPS_GUIDED(RR)                                                                                                                  \
    hipLaunchKernelGGL(segment_render_guided_kernel<RR>, grid, block, 0, s, soft, table, n, S, P, src, guide, range_w, colors, alpha,   \
                       labels, overlay, confidence, counts)
    switch (R) {
        case 0: UPS_GUIDED(0); break;
        case 1: UPS_GUIDED(1); break;
        case 2: UPS_GUIDED(2); break;
        default: UPS_GUIDED(3); break;
    }
#undef UPS_GUIDED
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
