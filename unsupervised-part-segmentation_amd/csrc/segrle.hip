// COCO run-length annotations of the packed label planes of the segmentation export (declared in include/upsparts_hip.h; the
// definitions are DESIGN.md section 8 "Run-length annotations", restated twice by tests/segrle_ref.py).  Integer arithmetic only:
// every output is a function of the label plane, whatever the schedule.
//
//   ups_segment_rle_count   offsets int64 [n P + 1], area int32 [n, P], bbox int32 [n, P, 4]; per-chunk positions in the scratch
//   ups_segment_rle_write   counts int32 [offsets[n P]]: the count lists in (image, part) order
//
// For image i (h x w at `off`) and part p the mask in COCO's column-major order is m[k] = (labels[off + y w + x] == p), k = x h + y.
// T = the ascending positions with m[k] != m[k-1] (m[-1] = 0); the list is [T0, T1 - T0, .., h w - T_last], [h w] when T is empty:
// |T| + 1 entries.  A label >= P belongs to no part.
//
// A CHUNK is kChunk = 1024 consecutive positions k of one image (the table's first_block counts exactly these), worked by ONE wave;
// a block of 4 waves takes 4 consecutive chunks of one image, blockIdx.y is the image and a block beyond its image returns.
// No block waits for another: the order of a list comes from a scan over separate launches,
//   init     area = 0, bbox = (max, max, -1, -1)
//   count    per chunk and part: the number of transitions and the position of the last one -> scratch; area, bbox (integer atomics)
//   lists    one thread per (image, part) walks the image's chunks: scratch becomes (transitions before the chunk, the last
//            transition before the chunk or 0); offsets[i P + p] = the list's length; one sum per block of 256 lists
//   sums     one block scans the (at most 65 281) block sums and writes offsets[n P]
//   offsets  each block scans its 256 lengths behind its sum; bbox becomes (x, y, w, h)
//   write    entry j of a list is T_j - T_(j-1): the transition's rank in its chunk comes from a ballot over the wave, the position
//            of the transition before it from the lower lanes or the chunk's carry; the last chunk adds h w - T_last.
// One read of a label serves all parts: a change of label at k is a transition of the part that ends and of the part that begins.
//
// Reads.  The plane is row-major and a span of k runs down columns, so the 4096 positions of a block lie in `cols` = span / h + (1 or 2)
// neighbouring columns.  The block reads that strip row by row -- consecutive lanes read the `cols` consecutive bytes of a row, then
// the next row -- and stores each byte at its k in an LDS tile (the turn); a strip that would cost more than twice its span in
// reads (a very tall image: at most 3 columns, each a run of consecutive rows) is read position by position instead.  Position k - 1
// of the first chunk element comes from the same tile; at k = 0 it is the byte 255, which is never a part.
#include "common.h"
#include "segment_common.h"

namespace {

using ups_segment::kWords;

constexpr int kWave = 64;
constexpr int kChunk = ups_segment::kChunk;      // 1024 positions: one wave, 16 steps of 64
constexpr int kWaves = 4;                        // chunks per block
constexpr int kBlock = kWave * kWaves;
constexpr int kSpan = kChunk * kWaves;           // positions of a block
constexpr int kMaxP = 255;
constexpr int kNone = 255;                       // the byte before k = 0: no part (P <= 255)
constexpr long long kMaxHW = 1LL << 20;
constexpr int kBig = 0x7fffffff;

// the labels of positions K0 - 1 .. K1 - 1 of the image -> tile[0 .. K1 - K0]; the caller synchronises
__device__ __forceinline__ void load_tile(const uint8_t* __restrict__ img, int h, int w, int K0, int K1, uint8_t* tile) {
    const int tid = threadIdx.x;
    const int span = K1 - K0;
    const int x0 = K0 / h, x1 = (K1 - 1) / h;
    const int cols = x1 - x0 + 1;
    if (tid == 0) {
        int v = kNone;
        if (K0 > 0) {
            const int x = (K0 - 1) / h, y = (K0 - 1) - x * h;
            v = img[(long long)y * w + x];
        }
        tile[0] = (uint8_t)v;
    }
    if ((long long)h * cols <= 2LL * kSpan) {                                // the strip, row by row
        const int cells = h * cols;
        for (int c = tid; c < cells; c += kBlock) {
            const int y = c / cols, x = x0 + (c - y * cols);
            const int k = x * h + y;
            if (k >= K0 && k < K1) tile[k - K0 + 1] = img[(long long)y * w + x];
        }
    } else {                                                                 // position by position
        for (int j = tid; j < span; j += kBlock) {
            const int k = K0 + j;
            const int x = k / h, y = k - x * h;
            tile[j + 1] = img[(long long)y * w + x];
        }
    }
}

__global__ __launch_bounds__(kBlock) void rle_init_kernel(int M, int* __restrict__ area, int* __restrict__ bbox) {
    const int e = (int)blockIdx.x * kBlock + threadIdx.x;
    if (e >= M) return;
    area[e] = 0;
    bbox[4 * e + 0] = kBig;
    bbox[4 * e + 1] = kBig;
    bbox[4 * e + 2] = -1;
    bbox[4 * e + 3] = -1;
}

__global__ __launch_bounds__(kBlock) void rle_count_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ table, int P,
                                                           int* __restrict__ trans, int* __restrict__ last, int* __restrict__ area,
                                                           int* __restrict__ bbox) {
    __shared__ uint8_t tile[kSpan + 16];
    __shared__ int s_cnt[kWaves][256];
    __shared__ int s_last[kWaves][256];
    __shared__ int s_area[256], s_x0[256], s_y0[256], s_x1[256], s_y1[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int hw = h * w;
    const long long K0l = (long long)blockIdx.x * kSpan;
    if (K0l >= hw) return;                                                   // (block-uniform: before any barrier)
    const int K0 = (int)K0l, K1 = min(K0 + kSpan, hw);
    load_tile(labels + off, h, w, K0, K1, tile);
    s_area[tid] = 0;
    s_x0[tid] = kBig;
    s_y0[tid] = kBig;
    s_x1[tid] = -1;
    s_y1[tid] = -1;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) {
        s_cnt[j][tid] = 0;
        s_last[j][tid] = -1;
    }
    __syncthreads();
    const int Kc = K0 + wv * kChunk;                                         // this wave's chunk
    for (int s = 0; s < kChunk / kWave && Kc + s * kWave < hw; ++s) {
        const int k = Kc + s * kWave + lane;
        const bool in = k < hw;
        int a = -1, b = -1;
        if (in) {
            a = tile[k - K0];
            b = tile[k - K0 + 1];
            a = a < P ? a : -1;
            b = b < P ? b : -1;
        }
        if (a != b) {                                                        // (in: outside both are -1)
            if (a >= 0) {
                atomicAdd(&s_cnt[wv][a], 1);
                atomicMax(&s_last[wv][a], k);
            }
            if (b >= 0) {
                atomicAdd(&s_cnt[wv][b], 1);
                atomicMax(&s_last[wv][b], k);
            }
        }
        // area and box.  A wave whose 64 positions are all in the image and all of one part adds once: k_lo .. k_lo + 63 cover the
        // columns x_lo .. x_hi, and all rows between y_lo and y_hi of one column or, over a column's end, the rows 0 and h - 1 too.
        const int b0 = __builtin_amdgcn_readfirstlane(b);
        if (__ballot(in && b == b0) == ~0ull) {
            if (b0 >= 0 && lane == 0) {
                const int k_hi = k + kWave - 1;
                const int xl = k / h, yl = k - xl * h, xh = k_hi / h, yh = k_hi - xh * h;
                atomicAdd(&s_area[b0], kWave);
                atomicMin(&s_x0[b0], xl);
                atomicMax(&s_x1[b0], xh);
                atomicMin(&s_y0[b0], xl == xh ? yl : 0);
                atomicMax(&s_y1[b0], xl == xh ? yh : h - 1);
            }
        } else if (b >= 0) {
            const int x = k / h, y = k - x * h;
            atomicAdd(&s_area[b], 1);
            atomicMin(&s_x0[b], x);
            atomicMax(&s_x1[b], x);
            atomicMin(&s_y0[b], y);
            atomicMax(&s_y1[b], y);
        }
    }
    __syncthreads();
    const int cb = table[img * kWords + 3] + (int)blockIdx.x * kWaves;       // the block's first chunk in the scratch
    for (int j = 0; j < kWaves && K0 + j * kChunk < hw; ++j) {
        if (tid < P) {
            trans[(long long)(cb + j) * P + tid] = s_cnt[j][tid];
            last[(long long)(cb + j) * P + tid] = s_last[j][tid];
        }
    }
    if (tid < P && s_area[tid] > 0) {
        const long long e = (long long)img * P + tid;
        atomicAdd(&area[e], s_area[tid]);
        atomicMin(&bbox[4 * e + 0], s_x0[tid]);
        atomicMin(&bbox[4 * e + 1], s_y0[tid]);
        atomicMax(&bbox[4 * e + 2], s_x1[tid]);
        atomicMax(&bbox[4 * e + 3], s_y1[tid]);
    }
}

// the sum of v over the block (kBlock threads), in every thread
__device__ __forceinline__ long long block_sum(long long v, long long* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if (tid < d) sh[tid] += sh[tid + d];
        __syncthreads();
    }
    const long long r = sh[0];
    __syncthreads();
    return r;
}

// the sum of v over the threads below this one
__device__ __forceinline__ long long block_scan_exclusive(long long v, long long* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const long long t = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const long long r = sh[tid] - v;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kBlock) void rle_lists_kernel(const int* __restrict__ table, int M, int P, int* __restrict__ trans,
                                                           int* __restrict__ last, long long* __restrict__ offsets,
                                                           long long* __restrict__ sums) {
    __shared__ long long sh[kBlock];
    const int e = (int)blockIdx.x * kBlock + threadIdx.x;
    long long len = 0;
    if (e < M) {
        const int img = e / P, p = e - img * P;
        const int hw = table[img * kWords + 1] * table[img * kWords + 2];
        const int cb = table[img * kWords + 3], nc = (hw + kChunk - 1) / kChunk;
        int run = 0, prev = 0;
        for (int c = 0; c < nc; ++c) {
            const long long at = (long long)(cb + c) * P + p;
            const int t = trans[at], l = last[at];
            trans[at] = run;
            last[at] = prev;
            run += t;
            prev = l >= 0 ? l : prev;
        }
        len = (long long)run + 1;
        offsets[e] = len;
    }
    const long long s = block_sum(len, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void rle_sums_kernel(int nb, int M, long long* __restrict__ sums, long long* __restrict__ offsets) {
    __shared__ long long sh[kBlock];
    const int tid = threadIdx.x;
    const int per = (nb + kBlock - 1) / kBlock;
    const int lo = min(tid * per, nb), hi = min(lo + per, nb);
    long long mine = 0;
    for (int j = lo; j < hi; ++j) mine += sums[j];
    long long run = block_scan_exclusive(mine, sh);
    for (int j = lo; j < hi; ++j) {
        const long long v = sums[j];
        sums[j] = run;
        run += v;
    }
    if (tid == kBlock - 1) offsets[M] = run;                                 // (the last thread's end is the total)
}

__global__ __launch_bounds__(kBlock) void rle_offsets_kernel(int M, const long long* __restrict__ sums, long long* __restrict__ offsets,
                                                             const int* __restrict__ area, int* __restrict__ bbox) {
    __shared__ long long sh[kBlock];
    const int e = (int)blockIdx.x * kBlock + threadIdx.x;
    const long long len = e < M ? offsets[e] : 0;
    const long long before = block_scan_exclusive(len, sh);
    if (e >= M) return;
    offsets[e] = sums[blockIdx.x] + before;
    int x0 = 0, y0 = 0, bw = 0, bh = 0;
    if (area[e] > 0) {
        x0 = bbox[4 * e + 0];
        y0 = bbox[4 * e + 1];
        bw = bbox[4 * e + 2] - x0 + 1;
        bh = bbox[4 * e + 3] - y0 + 1;
    }
    bbox[4 * e + 0] = x0;
    bbox[4 * e + 1] = y0;
    bbox[4 * e + 2] = bw;
    bbox[4 * e + 3] = bh;
}

__global__ __launch_bounds__(kBlock) void rle_write_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ table, int P,
                                                           const long long* __restrict__ offsets, const int* __restrict__ trans,
                                                           const int* __restrict__ last, int* __restrict__ counts, long long capacity) {
    __shared__ uint8_t tile[kSpan + 16];
    // (volatile: a lane reads what ANOTHER lane of its wave stored a turn earlier; nothing may be kept in a register across turns)
    __shared__ volatile long long s_at[kWaves][256];                         // where the part's next entry goes
    __shared__ volatile int s_prev[kWaves][256];                             // the position of the part's latest transition, or 0
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int hw = h * w;
    const long long K0l = (long long)blockIdx.x * kSpan;
    if (K0l >= hw) return;                                                   // (block-uniform: before the barrier)
    const int K0 = (int)K0l, K1 = min(K0 + kSpan, hw);
    load_tile(labels + off, h, w, K0, K1, tile);
    const int Kc = K0 + wv * kChunk;
    if (Kc < hw) {
        const long long c = table[img * kWords + 3] + (long long)blockIdx.x * kWaves + wv;
        for (int p = lane; p < P; p += kWave) {
            s_at[wv][p] = offsets[(long long)img * P + p] + trans[c * P + p];
            s_prev[wv][p] = last[c * P + p];
        }
    }
    __syncthreads();                                                         // (the only barrier: from here on a wave is on its own)
    if (Kc >= hw) return;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    for (int s = 0; s < kChunk / kWave && Kc + s * kWave < hw; ++s) {
        const int k_first = Kc + s * kWave;
        const int k = k_first + lane;
        int a = -1, b = -1;
        if (k < hw) {
            a = tile[k - K0];
            b = tile[k - K0 + 1];
            a = a < P ? a : -1;
            b = b < P ? b : -1;
        }
        int e0 = a != b ? a : -1, e1 = a != b ? b : -1;                      // the part that ends here, the part that begins
        unsigned long long todo = __ballot(e0 >= 0 || e1 >= 0);
        while (todo) {                                                       // (wave-uniform) one turn per part with a transition here
            const int src = __ffsll((long long)todo) - 1;
            const int q0 = __shfl(e0, src), q1 = __shfl(e1, src);
            const int p = __builtin_amdgcn_readfirstlane(q0 >= 0 ? q0 : q1);
            const bool mine = e0 == p || e1 == p;
            const unsigned long long mask = __ballot(mine);                  // the part's transitions of this step, ascending by lane
            if (mine) {
                const unsigned long long below = mask & below_me;
                const long long at = s_at[wv][p] + __popcll(below);
                const int prev = below ? k_first + 63 - __clzll((long long)below) : s_prev[wv][p];
                if (at < capacity) counts[at] = k - prev;
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == src) {
                s_at[wv][p] = s_at[wv][p] + __popcll(mask);
                s_prev[wv][p] = k_first + 63 - __clzll((long long)mask);
            }
            __builtin_amdgcn_wave_barrier();
            e0 = e0 == p ? -1 : e0;
            e1 = e1 == p ? -1 : e1;
            todo = __ballot(e0 >= 0 || e1 >= 0);
        }
    }
    if (Kc + kChunk >= hw) {                                                 // the image's last chunk closes every list
        for (int p = lane; p < P; p += kWave) {
            const long long at = s_at[wv][p];
            if (at < capacity) counts[at] = hw - s_prev[wv][p];
        }
    }
}

struct Layout {                                  // what both entries derive from the table: the grids and the scratch's parts
    dim3 grid;
    int M, nb;
    long long chunks;
    long long* sums;
    int* trans;
    int* last;
};

size_t scratch_bytes(long long M, long long chunks, int P) {
    const long long nb = (M + kBlock - 1) / kBlock;
    return (size_t)(nb * 8 + chunks * P * 8);
}

int check_common(const char* fn, const uint8_t* labels, int n, const int32_t* table_host, const int32_t* table, long long total, int P,
                 void* scratch, Layout* lay) {
    UPS_CHECK_ARG(labels && table_host && table && scratch);
    UPS_CHECK_ARG(n >= 1 && n <= 65535);                                     // blockIdx.y is the image
    UPS_CHECK_ARG(P >= 1);
    if (P > kMaxP) {
        ups_set_error("%s: P <= 255 (got P = %d)", fn, P);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG(total >= 1 && total <= 0x7fffffffLL);
    UPS_CHECK_ARG(((uintptr_t)scratch & 7) == 0);
    long long chunks = 0;
    if (const int rc = ups_segment::check_table(table_host, n, total, &chunks)) return rc;
    long long max_hw = 0;
    for (int i = 0; i < n; ++i) {
        const long long hw = (long long)table_host[(long long)i * kWords + 1] * table_host[(long long)i * kWords + 2];
        UPS_CHECK_ARG(hw <= kMaxHW);
        max_hw = hw > max_hw ? hw : max_hw;
    }
    lay->grid = dim3((unsigned)((max_hw + kSpan - 1) / kSpan), (unsigned)n);
    lay->M = n * P;
    lay->nb = (lay->M + kBlock - 1) / kBlock;
    lay->chunks = chunks;
    lay->sums = (long long*)scratch;
    lay->trans = (int*)(lay->sums + lay->nb);
    lay->last = lay->trans + chunks * P;
    return UPS_OK;
}

}  // namespace

extern "C" int32_t ups_segment_rle_chunk(void) { return kChunk; }

// an upper bound that needs no table: an image of h w pixels has ceil(h w / chunk) <= h w / chunk + 1 chunks
extern "C" size_t ups_segment_rle_scratch_bytes(int32_t n, int64_t total, int32_t P) {
    if (n < 1 || total < 1 || P < 1) return 0;
    return scratch_bytes((long long)n * P, total / kChunk + n, P);
}

extern "C" int ups_segment_rle_count(const uint8_t* labels, int32_t n, const int32_t* table_host, const int32_t* table, int64_t total,
                                     int32_t P, int64_t* offsets, int32_t* area, int32_t* bbox, void* scratch, void* stream) {
    UPS_CHECK_ARG(offsets && area && bbox);
    UPS_CHECK_ARG(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)area & 3) == 0 && ((uintptr_t)bbox & 3) == 0);
    Layout lay;
    if (const int rc = check_common("ups_segment_rle_count", labels, n, table_host, table, total, P, scratch, &lay)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 lists((unsigned)lay.nb);
    hipLaunchKernelGGL(rle_init_kernel, lists, dim3(kBlock), 0, s, lay.M, area, bbox);
    hipLaunchKernelGGL(rle_count_kernel, lay.grid, dim3(kBlock), 0, s, labels, table, P, lay.trans, lay.last, area, bbox);
    hipLaunchKernelGGL(rle_lists_kernel, lists, dim3(kBlock), 0, s, table, lay.M, P, lay.trans, lay.last, (long long*)offsets, lay.sums);
    hipLaunchKernelGGL(rle_sums_kernel, dim3(1), dim3(kBlock), 0, s, lay.nb, lay.M, lay.sums, (long long*)offsets);
    hipLaunchKernelGGL(rle_offsets_kernel, lists, dim3(kBlock), 0, s, lay.M, lay.sums, (long long*)offsets, area, bbox);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_segment_rle_write(const uint8_t* labels, int32_t n, const int32_t* table_host, const int32_t* table, int64_t total,
                                     int32_t P, const int64_t* offsets, const void* scratch, int32_t* counts, int64_t capacity,
                                     int64_t n_counts, void* stream) {
    UPS_CHECK_ARG(offsets && counts);
    UPS_CHECK_ARG(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)counts & 3) == 0);
    UPS_CHECK_ARG(n_counts >= 1 && capacity >= n_counts);
    Layout lay;
    if (const int rc = check_common("ups_segment_rle_write", labels, n, table_host, table, total, P, (void*)scratch, &lay)) return rc;
    hipLaunchKernelGGL(rle_write_kernel, lay.grid, dim3(kBlock), 0, (hipStream_t)stream, labels, table, P, (const long long*)offsets,
                       lay.trans, lay.last, counts, (long long)capacity);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
