// Label-free validation metrics (declared in include/upsparts_hip.h): ups_image_metrics -- per-image squared / absolute error sums and
// the SSIM sum of two image batches -- and ups_part_usage -- per-image part areas, mask confidence and entropy.
//
// Both report SUMS; the step to mse / psnr / ssim / part_area / ... is evalutil.reconstruction_from_sums / usage_from_counts on the host.
// All floating-point arithmetic is fp64 on the source values (fp32 and bf16 are exact in fp64), and every floating-point sum has a
// fixed order: a thread adds its items in index order, a block adds its threads with a fixed tree in LDS and writes ONE partial per
// block into caller-owned scratch, and a second launch adds an image's partials in index order (ups_block_tree_sum and
// ups_sum_partials_kernel, common.h).  No floating-point atomics: two launches on the same inputs give the same bits.  The part counts
// are integers (LDS and global integer atomics, as ups_part_confusion).
//
// ups_image_metrics.  One 256-thread block per (image, kTile x kTile tile of the VALID region [H-10, W-10] of the 11 x 11 window).  Per
// channel the block stages the tile with its 10-pixel halo in LDS as the SOURCE floats (42 x 42 values per operand, in two strips of
// 21 rows so that it fits beside the maps), filters the five maps x, y, x^2, y^2, xy along the row into fp64 LDS maps [42][32]
// (53 760 bytes) and then filters those down the column for its 32 x 32 outputs: the separable 11-tap Gaussian whose normalised fp64
// weights are a HOST argument (passed by value), so the host restatement and the device multiply by the same numbers.
// 60 816 bytes of static LDS in all: under the 64 KB default.  Halo cells beyond the image hold 0 and only feed outputs that are masked.
// Error sums: every pixel of the image lies in the staged area of at least one tile; it is counted by the tile that stages it in its
// first kTile rows / columns, or in the halo of the LAST tile row / column.
// Loads are element loads: ld = 3 fp32 rows have no 16-byte alignment, and the three channel passes of a tile hit L2.
//
// ups_part_usage.  One 256-thread block per chunk of kChunk pixels of one image, a thread per pixel (kChunk / 256 rounds).  A pixel
// whose pred is outside [0, P) is counted in `invalid` and never used as an index.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 32;                        // valid (output) pixels per tile edge (ops.IMAGE_METRICS_TILE)
constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kIn = kTile + kHalo;               // 42: staged rows / columns
constexpr int kStrip = kIn / 2;                  // 21 staged rows at a time
constexpr int kMaps = 5;
constexpr int kChunk = 1024;                     // pixels of one ups_part_usage block (ops.PART_USAGE_CHUNK)
static_assert(kIn % 2 == 0, "two strips");
static_assert(kMaps * kIn * kTile * 8 + 2 * kStrip * kIn * 4 <= 65536, "static LDS");
static_assert(kMaps * kIn * kTile >= 3 * kBlock, "the block reduction reuses the maps");

struct Weights { double w[kWin]; };

template <typename T> __device__ __forceinline__ float src_float(const T* p, long long i);
template <> __device__ __forceinline__ float src_float<float>(const float* p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float src_float<bf16>(const bf16* p, long long i) {
    return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(p)[i] << 16);
}

__device__ __forceinline__ double unit(float v) {           // clamp((v + 1) / 2, 0, 1) in fp64
    const double x = ((double)v + 1.0) * 0.5;
    return fmin(fmax(x, 0.0), 1.0);
}

template <typename TA, typename TB>
__global__ __launch_bounds__(kBlock) void image_metrics_kernel(const TA* __restrict__ a, int lda, const TB* __restrict__ b, int ldb,
                                                               int H, int W, int nty, int ntx, Weights wt,
                                                               double* __restrict__ partials) {
    __shared__ double hm[kMaps * kIn * kTile];
    __shared__ float sa[kStrip * kIn], sb[kStrip * kIn];
    const int tid = threadIdx.x;
    const int tiles = nty * ntx;
    const int img = blockIdx.x / tiles, t = blockIdx.x - img * tiles;
    const int ty = t / ntx, tx = t - ty * ntx;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const bool last_y = ty == nty - 1, last_x = tx == ntx - 1;
    const int VH = H - kHalo, VW = W - kHalo;
    const long long base = (long long)img * H * W;
    double sse = 0.0, sae = 0.0, ssim = 0.0;

    for (int c = 0; c < 3; ++c) {
        for (int strip = 0; strip < 2; ++strip) {
            for (int i = tid; i < kStrip * kIn; i += kBlock) {
                const int r = strip * kStrip + i / kIn, col = i % kIn;
                const int gy = y0 + r, gx = x0 + col;
                float va = 0.f, vb = 0.f;
                if (gy < H && gx < W) {
                    const long long px = base + (long long)gy * W + gx;
                    va = src_float<TA>(a, px * lda + c);
                    vb = src_float<TB>(b, px * ldb + c);
                    if ((r < kTile || last_y) && (col < kTile || last_x)) {
                        const double d = unit(va) - unit(vb);
                        sse += d * d;
                        sae += fabs(d);
                    }
                }
                sa[i] = va;
                sb[i] = vb;
            }
            __syncthreads();
            for (int i = tid; i < kStrip * kTile; i += kBlock) {
                const int r = i / kTile, col = i % kTile;
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
                for (int k = 0; k < kWin; ++k) {
                    const double x = unit(sa[r * kIn + col + k]), y = unit(sb[r * kIn + col + k]), w = wt.w[k];
                    m0 += w * x;
                    m1 += w * y;
                    m2 += w * (x * x);
                    m3 += w * (y * y);
                    m4 += w * (x * y);
                }
                const int o = (strip * kStrip + r) * kTile + col;
                hm[o] = m0;
                hm[kIn * kTile + o] = m1;
                hm[2 * kIn * kTile + o] = m2;
                hm[3 * kIn * kTile + o] = m3;
                hm[4 * kIn * kTile + o] = m4;
            }
            __syncthreads();
        }
        for (int i = tid; i < kTile * kTile; i += kBlock) {
            const int r = i / kTile, col = i % kTile;
            if (y0 + r < VH && x0 + col < VW) {
                double m[kMaps] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < kWin; ++k) {
                    const double w = wt.w[k];
                    const int o = (r + k) * kTile + col;
#pragma unroll
                    for (int q = 0; q < kMaps; ++q) m[q] += w * hm[q * kIn * kTile + o];
                }
                const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
                const double mx = m[0], my = m[1];
                const double vx = m[2] - mx * mx, vy = m[3] - my * my, cxy = m[4] - mx * my;
                ssim += ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
            }
        }
        __syncthreads();                 // the next channel overwrites the maps
    }
    double* red = hm;
    red[tid] = sse;
    red[kBlock + tid] = sae;
    red[2 * kBlock + tid] = ssim;
    ups_block_tree_sum<3, kBlock>(red, tid);
    if (tid < 3) partials[(long long)blockIdx.x * 3 + tid] = red[tid * kBlock];
}

__global__ __launch_bounds__(kBlock) void part_usage_kernel(const float* __restrict__ soft, const long long* __restrict__ pred,
                                                            long long HW, int P, int chunks, int* __restrict__ counts,
                                                            int* __restrict__ invalid, double* __restrict__ partials) {
    __shared__ int bins[32];
    __shared__ int bad;
    __shared__ double red[2 * kBlock];
    const int tid = threadIdx.x;
    if (tid < 32) bins[tid] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    const int img = blockIdx.x / chunks;
    const long long at = (long long)(blockIdx.x - img * chunks) * kChunk;
    double conf = 0.0, ent = 0.0;
    int nbad = 0;
    for (int k = 0; k < kChunk / kBlock; ++k) {
        const long long px = at + k * kBlock + tid;
        if (px >= HW) break;
        const long long g = (long long)img * HW + px;
        const long long pv = pred[g];
        if ((unsigned long long)pv < (unsigned long long)P) atomicAdd(&bins[(int)pv], 1);
        else ++nbad;
        const float* s = soft + g * P;
        float mx = s[0];
        double e = 0.0;
        for (int p = 0; p < P; ++p) {
            const float v = s[p];
            mx = fmaxf(mx, v);
            if (v > 0.f) e -= (double)v * log((double)v);
        }
        conf += (double)mx;
        ent += e;
    }
    if (nbad) atomicAdd(&bad, nbad);
    red[tid] = conf;
    red[kBlock + tid] = ent;
    ups_block_tree_sum<2, kBlock>(red, tid);     // (its barriers also order the LDS atomics above before the reads below)
    if (tid < 2) partials[(long long)blockIdx.x * 2 + tid] = red[tid * kBlock];
    if (tid < P) {
        const int v = bins[tid];
        if (v) atomicAdd(&counts[(long long)img * P + tid], v);
    }
    if (tid == 0 && bad) atomicAdd(invalid, bad);
}

// number of tiles per image, or -1 when the block count or the scratch index would leave int
long long metric_tiles(int N, int H, int W, int* nty, int* ntx) {
    *nty = (H - kHalo + kTile - 1) / kTile;
    *ntx = (W - kHalo + kTile - 1) / kTile;
    const long long tiles = (long long)*nty * *ntx;
    return tiles * N <= 0x7fffffffLL / 3 ? tiles : -1;
}

}  // namespace

extern "C" int32_t ups_image_metrics_tile(void) { return kTile; }
extern "C" int32_t ups_part_usage_chunk(void) { return kChunk; }

extern "C" size_t ups_image_metrics_scratch_bytes(int32_t N, int32_t H, int32_t W) {
    int nty, ntx;
    if (N <= 0 || H < kWin || W < kWin) return 0;
    const long long tiles = metric_tiles(N, H, W, &nty, &ntx);
    return tiles < 0 ? 0 : (size_t)tiles * N * 3 * sizeof(double);
}

extern "C" int ups_image_metrics(const void* a, int32_t dtype_a, int32_t lda, const void* b, int32_t dtype_b, int32_t ldb, int32_t N,
                                 int32_t H, int32_t W, const double* weights, double* out, void* scratch, void* stream) {
    UPS_CHECK_ARG(a && b && weights && out && scratch);
    UPS_CHECK_ARG(lda >= 3 && ldb >= 3);
    UPS_CHECK_ARG((dtype_a == UPS_F32 || dtype_a == UPS_BF16) && (dtype_b == UPS_F32 || dtype_b == UPS_BF16));
    UPS_CHECK_ARG(N > 0 && H >= kWin && W >= kWin);
    int nty, ntx;
    const long long tiles = metric_tiles(N, H, W, &nty, &ntx);
    UPS_CHECK_ARG(tiles > 0);            // N * tiles blocks and 3 * N * tiles partials are indexed as int
    const unsigned blocks = (unsigned)(tiles * N);
    Weights wt;
    for (int k = 0; k < kWin; ++k) wt.w[k] = weights[k];
    double* part = reinterpret_cast<double*>(scratch);
    hipStream_t s = (hipStream_t)stream;
#define UPS_IM_LAUNCH(TA, TB)                                                                                             \
    hipLaunchKernelGGL((image_metrics_kernel<TA, TB>), dim3(blocks), dim3(kBlock), 0, s, reinterpret_cast<const TA*>(a), lda, \
                       reinterpret_cast<const TB*>(b), ldb, H, W, nty, ntx, wt, part)
    if (dtype_a == UPS_F32 && dtype_b == UPS_F32) UPS_IM_LAUNCH(float, float);
    else if (dtype_a == UPS_F32) UPS_IM_LAUNCH(float, bf16);
    else if (dtype_b == UPS_F32) UPS_IM_LAUNCH(bf16, float);
    else UPS_IM_LAUNCH(bf16, bf16);
#undef UPS_IM_LAUNCH
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ups_sum_partials_kernel<kBlock>, dim3(ups_cdiv(3LL * N, kBlock)), dim3(kBlock), 0, s, part, (int)tiles, 3, 3 * N,
                       out);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" size_t ups_part_usage_scratch_bytes(int32_t N, int64_t HW) {
    if (N <= 0 || HW <= 0 || HW > 0x7fffffffLL) return 0;
    const long long blocks = (HW + kChunk - 1) / kChunk * N;
    return blocks > 0x7fffffffLL / 2 ? 0 : (size_t)blocks * 2 * sizeof(double);
}

extern "C" int ups_part_usage(const float* soft, const int64_t* pred, int32_t N, int64_t HW, int32_t P, int32_t* counts, int32_t* invalid,
                              double* sharp, void* scratch, void* stream) {
    UPS_CHECK_ARG(soft && pred && counts && invalid && sharp && scratch);
    UPS_CHECK_ARG(N > 0 && HW > 0 && HW <= 0x7fffffffLL && P >= 1);              // a count is at most HW per launch: int32
    if (P > 32) {
        ups_set_error("ups_part_usage: P <= 32 (got P = %d)", P);
        return UPS_E_UNSUPPORTED;
    }
    const long long chunks = (HW + kChunk - 1) / kChunk, blocks = chunks * N;
    UPS_CHECK_ARG(blocks <= 0x7fffffffLL / 2);                                   // blocks and 2 * blocks partials are indexed as int
    UPS_CHECK_ARG((long long)N * P <= 0x7fffffffLL);
    double* part = reinterpret_cast<double*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(part_usage_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, soft, reinterpret_cast<const long long*>(pred),
                       (long long)HW, P, (int)chunks, counts, invalid, part);
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ups_sum_partials_kernel<kBlock>, dim3(ups_cdiv(2LL * N, kBlock)), dim3(kBlock), 0, s, part, (int)chunks, 2, 2 * N,
                       sharp);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
