// Part-IoU evaluation: the per-image joint histogram of inferred part and ground-truth label (ups_part_confusion; declared in
// include/upsparts_hip.h).
//
//     counts[i][p][g] += #{pixels k of image i : pred[i][k] == p and lut[gt[i][k]] == g}          (lut == NULL: identity)
//
// Everything the protocol of eval_01.py:229-383 reports (best remapping, pooled and per-image IoU, the label means, `overall`) is a
// function of this [N, P, G] table of integers (evalutil.evaluate_from_counts).
//
// The kernel TAKES the arg-max map; it does not recompute an arg-max from the logits.  out_parts_hard is "first maximal index of the
// fp32 soft-max" (ups_part_softmax_fwd): two different logits whose soft-max values round to the same float tie there and would
// not tie on the logits, so a fused arg-max + confusion kernel would not be bit-equal to what the evaluation reports.  There is no
// fused form.
//
// Form: an image is split into chunks of kChunk = kBlock * kPerLane pixels, one 256-thread block per chunk (grid = N * chunks per
// image, so a batch of 2B small maps still fills the machine).  The block keeps the P * G <= 1024 bins in LDS (4 KB: occupancy is
// bounded by waves, not by LDS) and adds its non-zero bins to `counts` with global integer atomics at the end -- integer sums:
// the result depends neither on the launch geometry nor on the order in which blocks finish.
// Contention: real masks are piecewise constant, so neighbouring pixels hit the same bin almost always and an LDS atomic per pixel
// would serialise a wave on one address.  Every lane therefore owns kPerLane CONSECUTIVE pixels and carries a (key, run length) pair
// in registers; LDS sees one atomic per run, i.e. per key change -- one per lane for a constant region.
// Loads: a lane's 8 pred values are four 16-byte loads and its 8 labels two dword loads when the image's rows of both tensors are so
// aligned and the lane's run is whole; otherwise (odd HW, offset pointers, the tail of an image) element loads.  The choice is per
// lane and changes no result.
// Bounds: a key is formed only from 0 <= pred < P (compared as unsigned 64-bit: negative and huge values fail) and a mapped label
// < G; any other pixel is counted in `invalid` and touches neither LDS nor `counts`.
#include "common.h"

namespace {

constexpr int kBlock = 256;                      // threads per block
constexpr int kPerLane = 8;                      // consecutive pixels of one lane
constexpr int kChunk = kBlock * kPerLane;        // pixels of one block: 2048 (tests/test_gpu_parteval.py states it)
constexpr int kMaxBins = 32 * 32;

struct Run {                                     // the lane's current run: `len` pixels of bin `key` not yet in LDS (key < 0: none)
    int key, len;
};

__device__ __forceinline__ void flush(int* bins, const Run& r) {
    if (r.key >= 0) atomicAdd(&bins[r.key], r.len);
}

// one pixel: extends the run, or flushes it and starts the next one.  Returns 1 for a pixel that is counted nowhere.
template <bool LUT>
__device__ __forceinline__ int pixel(long long pv, unsigned gv, const uint8_t* slut, int P, int G, int* bins, Run& r) {
    const unsigned lab = LUT ? (unsigned)slut[gv] : gv;
    if ((unsigned long long)pv >= (unsigned long long)P || lab >= (unsigned)G) return 1;
    const int key = (int)pv * G + (int)lab;      // < P * G <= kMaxBins
    if (key == r.key) {
        ++r.len;
    } else {
        flush(bins, r);
        r.key = key;
        r.len = 1;
    }
    return 0;
}

template <bool LUT>
__global__ __launch_bounds__(kBlock) void part_confusion_kernel(const long long* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                const uint8_t* __restrict__ lut, long long HW, int P, int G,
                                                                int chunks, int* __restrict__ counts, int* __restrict__ invalid) {
    __shared__ int bins[kMaxBins];
    __shared__ int bad;
    __shared__ uint8_t slut[256];
    const int tid = threadIdx.x, nb = P * G;
    for (int t = tid; t < nb; t += kBlock) bins[t] = 0;
    if (tid == 0) bad = 0;
    if (LUT) slut[tid] = lut[tid];               // kBlock == 256 == the table
    __syncthreads();

    const long long img = blockIdx.x / chunks;
    const long long at = (long long)(blockIdx.x - img * chunks) * kChunk + (long long)tid * kPerLane;     // first pixel of this lane
    const long long* p = pred + img * HW + at;
    const uint8_t* g = gt + img * HW + at;
    const long long left = HW - at;
    Run r = {-1, 0};
    int nbad = 0;
    if (left >= kPerLane && (((uintptr_t)p & 15) | ((uintptr_t)g & 3)) == 0) {
        long long pv[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; k += 2) {
            const longlong2 v = *reinterpret_cast<const longlong2*>(p + k);
            pv[k] = v.x;
            pv[k + 1] = v.y;
        }
        unsigned gw[kPerLane / 4];
#pragma unroll
        for (int k = 0; k < kPerLane / 4; ++k) gw[k] = reinterpret_cast<const unsigned*>(g)[k];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) nbad += pixel<LUT>(pv[k], (gw[k >> 2] >> (8 * (k & 3))) & 255u, slut, P, G, bins, r);
    } else {
        const int n = left < kPerLane ? (left > 0 ? (int)left : 0) : kPerLane;
        for (int k = 0; k < n; ++k) nbad += pixel<LUT>(p[k], g[k], slut, P, G, bins, r);
    }
    flush(bins, r);
    if (nbad) atomicAdd(&bad, nbad);
    __syncthreads();

    int* out = counts + img * nb;
    for (int t = tid; t < nb; t += kBlock) {
        const int v = bins[t];
        if (v) atomicAdd(&out[t], v);
    }
    if (tid == 0 && bad) atomicAdd(invalid, bad);
}

}  // namespace

extern "C" int ups_part_confusion(const int64_t* pred, const uint8_t* gt, const uint8_t* lut, int32_t N, int64_t HW, int32_t P, int32_t G,
                                  int32_t* counts, int32_t* invalid, void* stream) {
    UPS_CHECK_ARG(pred && gt && counts && invalid);
    UPS_CHECK_ARG(N > 0 && HW > 0 && HW <= 0x7fffffffLL);                       // a bin counts at most HW pixels per launch: int32
    if (P < 1 || P > 32 || G < 1 || G > 32) {
        ups_set_error("ups_part_confusion: 1 <= P <= 32 and 1 <= G <= 32 (got P = %d, G = %d)", P, G);
        return UPS_E_UNSUPPORTED;
    }
    const long long chunks = (HW + kChunk - 1) / kChunk, blocks = chunks * N;
    UPS_CHECK_ARG(blocks <= 0x7fffffffLL);
    const long long* p = reinterpret_cast<const long long*>(pred);
    if (lut) hipLaunchKernelGGL(part_confusion_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, p, gt, lut,
                                (long long)HW, P, G, (int)chunks, counts, invalid);
    else hipLaunchKernelGGL(part_confusion_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, p, gt, lut,
                            (long long)HW, P, G, (int)chunks, counts, invalid);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
