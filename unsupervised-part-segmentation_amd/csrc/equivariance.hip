// Part equivariance under thin-plate-spline warps (declared in include/upsparts_hip.h): ups_tps_grid -- the source pixel position of
// every output pixel of ups_tps_warp, as a tensor -- and ups_part_equivariance -- per image, the joint histogram of "the part of the
// original's map sampled where the warp took this pixel from" and "the part of the warped image's map at this pixel", and the
// total-variation distance between the two part distributions, over the pixels whose source lies inside the image.
//
// ups_tps_grid restates the position arithmetic of tps_warp_kernel (pointwise.hip) expression for expression: fp32, the compiler's
// default contraction as there (it stands ABOVE the pragma below), phi = d2 * logf(d2 + 1e-6f), px = (x_s + 1) * w * 0.5.  One thread
// per output pixel; T and the control points of the image sit in LDS.
//
// ups_part_equivariance.  The decision and the distance are fp64 on the fp32 source values with contraction off (pragma below): every
// subtraction, multiplication and addition is the IEEE operation, in the order the header states, so tests/equivariance_ref.py's NumPy
// float64 gives the same `la` and the same per-pixel distance; only the order in which the per-pixel distances are added differs.
// One 256-thread block per chunk of kChunk pixels of one image, worked off in rounds of kRound = 128 pixels:
//   1. thread j < 128 reads pixel j's position and pred_b, decides "inside" and leaves the four tap pixels, fx, fy and the label in
//      LDS;
//   2. all 256 threads run over the round's pixel x part plane, element e = pixel * P + part: soft_b is then ONE contiguous run of
//      128 P floats read by consecutive lanes (whole cache lines), and each of the four tap rows of soft_a a run of P consecutive
//      floats read by P consecutive lanes -- no lane strides over a row of its own.  The fp64 sample v and b go to LDS
//      ([128][P | 1]: the odd row stride spreads the rows of phase 3 over the banks);
//   3. thread j < 128 reads pixel j's row of v and b from LDS: NaN check, first maximal part, 0.5 * sum |v - b| with p ascending.
// Histogram: the block keeps the P * P <= 1024 bins in LDS (4 KB) and adds its non-zero bins to `counts` with global integer atomics
// at the end.  Trained masks are piecewise constant, so most lanes of a wave hold the same bin: the wave peels up to kPeel distinct
// bins, one LDS atomic of the lane count each (ballot + popcount), and only what is left adds lane by lane -- noise maps cost what
// plain LDS atomics cost, constant regions one atomic per wave.  (evalparts.hip's run-length form needs consecutive pixels per lane;
// here a lane's pixels are kRound apart, so that phase 2's plane is contiguous.)
// tv: a thread adds its pixels in round order, the block adds its threads with a fixed tree and writes ONE partial into the caller's
// scratch, and a second launch adds an image's partials in index order (ups_block_tree_sum<1> and ups_sum_partials_kernel with K = 1,
// common.h: additions only, nothing for the pragma below to act on).  No floating-point atomics: two calls give the same bits.
// Bounds: a tap index is formed only for an inside pixel (0 <= x0 <= x1 <= w - 1, 0 <= y0 <= y1 <= h - 1, decided in fp64 on the
// finite position); a bin only from 0 <= la < P and a pred_b compared as unsigned 64-bit against P.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kGridMaxK = 32;                    // TPS_MAXK of ups_tps_warp (pointwise.hip)

__global__ __launch_bounds__(kBlock) void tps_grid_kernel(const float* __restrict__ T, const float* __restrict__ coord,
                                                          float* __restrict__ grid, int h, int w, int K) {
    __shared__ float sT[2 * (kGridMaxK + 3)], sC[2 * kGridMaxK];
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * (K + 3); i += kBlock) sT[i] = T[(long long)n * 2 * (K + 3) + i];
    for (int i = threadIdx.x; i < 2 * K; i += kBlock) sC[i] = coord[(long long)n * 2 * K + i];
    __syncthreads();
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= h * w) return;
    const int yy = q / w, xx = q - yy * w;
    const float x = w > 1 ? -1.f + 2.f * (float)xx / (float)(w - 1) : -1.f;
    const float y = h > 1 ? -1.f + 2.f * (float)yy / (float)(h - 1) : -1.f;
    float xs = sT[0] + sT[1] * x + sT[2] * y;
    float ys = sT[K + 3] + sT[K + 4] * x + sT[K + 5] * y;
    for (int i = 0; i < K; ++i) {
        const float dx = x - sC[2 * i], dy = y - sC[2 * i + 1];
        const float d2 = dx * dx + dy * dy;
        const float r = d2 * logf(d2 + 1e-6f);
        xs += sT[3 + i] * r;
        ys += sT[K + 6 + i] * r;
    }
    const float px = (xs + 1.f) * (float)w * 0.5f, py = (ys + 1.f) * (float)h * 0.5f;
    float* o = grid + ((long long)n * h * w + q) * 2;
    o[0] = px;
    o[1] = py;
}

}  // namespace

#pragma clang fp contract(off)

namespace {

constexpr int kRound = 128;                      // pixels per round: two waves own a pixel each in phases 1 and 3
constexpr int kChunk = 1024;                     // pixels of one block (ops.PART_EQUIVARIANCE_CHUNK)
constexpr int kMaxP = 32;
constexpr int kPeel = 4;                         // distinct bins a wave adds with one atomic each
constexpr long long kIntMax = 0x7fffffffLL;
static_assert(kRound % 64 == 0 && kRound <= kBlock && kChunk % kRound == 0, "whole waves per round, whole rounds per chunk");
static_assert(kRound * (kMaxP | 1) * 12 + kRound * 36 + kMaxP * kMaxP * 4 + kBlock * 8 + 16 <= 65536, "LDS");

// every lane of the wave calls; key < 0: nothing to add
__device__ __forceinline__ void wave_add(int* bins, int key) {
    const int lane = threadIdx.x & 63;
    for (int it = 0; it < kPeel; ++it) {
        const unsigned long long pending = __ballot(key >= 0);
        if (!pending) return;
        const int leader = __ffsll((long long)pending) - 1;
        const int k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == k);
        if (key == k) {
            if (lane == leader) atomicAdd(&bins[k], (int)__popcll(same));
            key = -1;
        }
    }
    if (key >= 0) atomicAdd(&bins[key], 1);
}

__global__ __launch_bounds__(kBlock) void part_equivariance_kernel(const float* __restrict__ soft_a, const float* __restrict__ soft_b,
                                                                   const long long* __restrict__ pred_b, const float* __restrict__ grid,
                                                                   int h, int w, int P, int chunks, int* __restrict__ counts,
                                                                   int* __restrict__ invalid, double* __restrict__ partials) {
    extern __shared__ double dyn[];              // v [kRound][S] doubles, then b [kRound][S] floats
    __shared__ int tap[4][kRound];               // pixel index (in the image) of the taps (y0,x0) (y0,x1) (y1,x0) (y1,x1); [0] < 0: not inside
    __shared__ double sfx[kRound], sfy[kRound];
    __shared__ int slb[kRound];                  // pred_b, or -1 when it is outside [0, P)
    __shared__ int bins[kMaxP * kMaxP];
    __shared__ int bad;
    __shared__ double red[kBlock];
    const int tid = threadIdx.x, S = P | 1, nb = P * P;
    double* sv = dyn;
    float* sb = reinterpret_cast<float*>(dyn + kRound * S);
    for (int t = tid; t < nb; t += kBlock) bins[t] = 0;
    if (tid == 0) bad = 0;

    const long long HW = (long long)h * w;
    const long long img = blockIdx.x / chunks;
    const long long at = (long long)(blockIdx.x - img * chunks) * kChunk;
    const long long ibase = img * HW;
    const double xmax = (double)(w - 1), ymax = (double)(h - 1);
    double tsum = 0.0;
    int nbad = 0;
    for (int round = 0; round < kChunk / kRound; ++round) {
        const long long p0 = at + (long long)round * kRound;
        if (p0 >= HW) break;                     // (uniform)
        const int npx = HW - p0 < kRound ? (int)(HW - p0) : kRound;
        __syncthreads();                         // the bins are zero; the round before is done with tap / sv / sb
        if (tid < kRound) {
            int t00 = -1;
            if (tid < npx) {
                const long long g = ibase + p0 + tid;
                const double X = (double)grid[2 * g], Y = (double)grid[2 * g + 1];
                if (X >= 0.0 && X <= xmax && Y >= 0.0 && Y <= ymax) {        // NaN and +-inf fail; -0.0 passes
                    const double x0d = floor(X), y0d = floor(Y);
                    const int x0 = (int)x0d, y0 = (int)y0d;
                    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
                    sfx[tid] = X - x0d;
                    sfy[tid] = Y - y0d;
                    t00 = y0 * w + x0;
                    tap[1][tid] = y0 * w + x1;
                    tap[2][tid] = y1 * w + x0;
                    tap[3][tid] = y1 * w + x1;
                    const long long pv = pred_b[g];
                    slb[tid] = (unsigned long long)pv < (unsigned long long)P ? (int)pv : -1;
                }
            }
            tap[0][tid] = t00;
        }
        __syncthreads();
        const float* arow = soft_a + ibase * P;
        const float* brow = soft_b + (ibase + p0) * P;
        for (int e = tid; e < npx * P; e += kBlock) {
            const int px = e / P, p = e - px * P;
            const int t00 = tap[0][px];
            if (t00 < 0) continue;
            const double a00 = (double)arow[(long long)t00 * P + p], a01 = (double)arow[(long long)tap[1][px] * P + p];
            const double a10 = (double)arow[(long long)tap[2][px] * P + p], a11 = (double)arow[(long long)tap[3][px] * P + p];
            const double fx = sfx[px], fy = sfy[px];
            const double gx = 1.0 - fx, gy = 1.0 - fy;
            const double top = gx * a00 + fx * a01;
            const double bot = gx * a10 + fx * a11;
            sv[px * S + p] = gy * top + fy * bot;
            sb[px * S + p] = brow[e];
        }
        __syncthreads();
        if (tid < kRound) {                      // (whole waves: wave_add is called by every lane)
            int key = -1;
            if (tid < npx && tap[0][tid] >= 0) {
                const int lb = slb[tid];
                bool ok = lb >= 0;
                double best = sv[tid * S], acc = 0.0;
                int la = 0;
                for (int p = 0; p < P; ++p) {
                    const double v = sv[tid * S + p], bb = (double)sb[tid * S + p];
                    if (v != v || bb != bb) ok = false;
                    if (v > best) {
                        best = v;
                        la = p;
                    }
                    acc += fabs(v - bb);
                }
                if (ok) {
                    key = la * P + lb;
                    tsum += 0.5 * acc;
                } else {
                    ++nbad;
                }
            }
            wave_add(bins, key);
        }
    }
    if (nbad) atomicAdd(&bad, nbad);
    red[tid] = tsum;
    ups_block_tree_sum<1, kBlock>(red, tid);     // fixed tree (its barriers also order the LDS atomics before the reads below)
    if (tid == 0) partials[blockIdx.x] = red[0];
    int* out = counts + img * nb;
    for (int t = tid; t < nb; t += kBlock) {
        const int v = bins[t];
        if (v) atomicAdd(&out[t], v);
    }
    if (tid == 0 && bad) atomicAdd(invalid, bad);
}

}  // namespace

extern "C" int ups_tps_grid(const float* T, const float* coord, float* grid, int32_t n, int32_t h, int32_t w, int32_t K, void* stream) {
    UPS_CHECK_ARG(T && coord && grid && n > 0 && h > 0 && w > 0 && K >= 1 && K <= kGridMaxK);
    UPS_CHECK_ARG((long long)h * w <= kIntMax && n <= 65535);                    // a pixel index is an int; n is the grid's y extent
    hipLaunchKernelGGL(tps_grid_kernel, dim3(ups_cdiv((long long)h * w, kBlock), n), dim3(kBlock), 0, (hipStream_t)stream, T, coord, grid,
                       h, w, K);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int32_t ups_part_equivariance_chunk(void) { return kChunk; }

extern "C" size_t ups_part_equivariance_scratch_bytes(int32_t N, int64_t HW) {
    if (N <= 0 || HW <= 0 || HW > kIntMax) return 0;
    const long long blocks = (HW + kChunk - 1) / kChunk * N;
    return blocks > kIntMax ? 0 : (size_t)blocks * sizeof(double);
}

extern "C" int ups_part_equivariance(const float* soft_a, const float* soft_b, const int64_t* pred_b, const float* grid, int32_t N,
                                     int32_t h, int32_t w, int32_t P, int32_t* counts, int32_t* invalid, double* tv, void* scratch,
                                     void* stream) {
    UPS_CHECK_ARG(soft_a && soft_b && pred_b && grid && counts && invalid && tv && scratch);
    UPS_CHECK_ARG(N > 0 && h > 0 && w > 0 && P >= 1);
    const long long HW = (long long)h * w;
    UPS_CHECK_ARG(HW <= kIntMax);                                                // a tap index is an int; a bin counts at most HW: int32
    if (P > kMaxP) {
        ups_set_error("ups_part_equivariance: P <= %d (got P = %d)", kMaxP, P);
        return UPS_E_UNSUPPORTED;
    }
    const long long chunks = (HW + kChunk - 1) / kChunk, blocks = chunks * N;
    UPS_CHECK_ARG(blocks <= kIntMax);
    const int S = P | 1;
    const size_t lds = (size_t)kRound * S * (sizeof(double) + sizeof(float));
    double* part = reinterpret_cast<double*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(part_equivariance_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, s, soft_a, soft_b,
                       reinterpret_cast<const long long*>(pred_b), grid, h, w, P, (int)chunks, counts, invalid, part);
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ups_sum_partials_kernel<kBlock>, dim3(ups_cdiv(N, kBlock)), dim3(kBlock), 0, s, part, (int)chunks, 1, N, tv);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
