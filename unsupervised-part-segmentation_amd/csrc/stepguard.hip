// The guarded optimizer step: a device-side record per optimizer key of what this step's gradient is like (ups_step_guard: squared
// norm, clip scale, non-finite count, skip decision and the run's counters), written by ups_grad_guard and read by ups_adam_guarded
// without the host; and the state update that keeps the old state when a statistic is not finite.  Definitions: include/upsparts_hip.h;
// restated in NumPy float64 with equal bits by tests/stepguard_ref.py.
#include <math.h>

#include "common.h"
#include "optim.h"

static_assert(sizeof(ups_step_guard) == 64, "ups_step_guard is a 64-byte record (lib.StepGuard mirrors it)");

namespace {

constexpr int kBlock = 256;             // threads of a block
constexpr int kSlots = 1024;            // accumulators of a chunk: element e of the chunk goes to slot e % kSlots
constexpr int kRows = 8;                // a slot takes its kRows elements in ascending order
constexpr int kChunk = kSlots * kRows;  // elements per partial (32 KB of gradient)
constexpr int kDefaultBlocks = 2048;    // 8 blocks per CU on 256 CUs
constexpr long long kMaxChunks = 1ll << 28;

__device__ __forceinline__ void take(float x, double& a, int& nf) {
    const double d = (double)x;
    a += d * d;             // (the square of an fp32 value is exact in fp64: fused or not, one rounding)
    nf += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// the fixed tree over 256 values held in LDS, by wave 0: (t[l] + t[l+128]) + (t[l+64] + t[l+192]), then strides 32 .. 1.  Lane 0 holds
// the sum; the same values as `for s = 128, 64, .., 1: t[i] += t[i + s] (i < s)`
__device__ __forceinline__ double tree256(const double* t, int lane) {
    double u = (t[lane] + t[lane + 128]) + (t[lane + 64] + t[lane + 192]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u += __shfl_down(u, o, 64);
    return u;
}

// One partial and one count per chunk of kChunk elements, whatever the grid and the alignment of g.  Element e of a chunk belongs to slot
// e % kSlots; a slot adds its elements' squares in ascending e from 0.0; the slots are folded (s[i] + s[i+256]) + (s[i+512] + s[i+768])
// and the 256 results go through tree256.  A thread owns four consecutive slots, placed so that its 16-byte loads are aligned: with h
// elements in front of the first aligned one, thread t's row r starts at chunk element 1024 r + 4 t + h - 4 (h > 0: thread 0's first row
// begins before the chunk and it takes a ninth row; the elements of such a ragged row are loaded one by one, as is a chunk's tail).
__global__ __launch_bounds__(kBlock) void grad_stats_kernel(const float* __restrict__ g, long long count, long long nchunks,
                                                           double* __restrict__ partial, int* __restrict__ nfpart) {
    __shared__ double slot[kSlots];
    __shared__ double fold[kBlock];
    __shared__ int nfw[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int h = (int)((4u - (unsigned)(((unsigned long long)g >> 2) & 3ull)) & 3u);
    const int d0 = 4 * tid + h - (h ? 4 : 0);                   // -3 .. 1023
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long base = c * kChunk;
        const int n = (int)(count - base < kChunk ? count - base : kChunk);
        const float* gc = g + base;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        int nf = 0;
        if (n == kChunk && d0 >= 0) {                           // whole rows: every load in flight before the first use
            float4 v[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) v[r] = *reinterpret_cast<const float4*>(gc + d0 + r * kSlots);
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                take(v[r].x, a[0], nf); take(v[r].y, a[1], nf); take(v[r].z, a[2], nf); take(v[r].w, a[3], nf);
            }
        } else {
            for (int r = 0; r <= kRows; ++r) {
                const int e = d0 + r * kSlots;
                if (e >= n) break;
                if (e >= 0 && e + 3 < n) {
                    const float4 v = *reinterpret_cast<const float4*>(gc + e);
                    take(v.x, a[0], nf); take(v.y, a[1], nf); take(v.z, a[2], nf); take(v.w, a[3], nf);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k >= 0 && e + k < n) take(gc[e + k], a[k], nf);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) slot[(d0 + k) & (kSlots - 1)] = a[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
        if (lane == 0) nfw[wid] = nf;
        __syncthreads();
        fold[tid] = (slot[tid] + slot[tid + 256]) + (slot[tid + 512] + slot[tid + 768]);
        if (tid == kBlock - 1) nfpart[c] = (nfw[0] + nfw[1]) + (nfw[2] + nfw[3]);
        __syncthreads();
        if (wid == 0) {
            const double u = tree256(fold, lane);
            if (lane == 0) partial[c] = u;
        }
        // (the next chunk's writes: slot and nfw were last read before the second barrier; fold is written after the next first barrier,
        // which wave 0 reaches only once it has read it)
    }
}

// One block: thread i adds partial[i], partial[i + 256], ... in ascending order from 0.0, tree256 over the 256 sums; the record.
__global__ __launch_bounds__(kBlock) void grad_guard_finalize_kernel(const double* __restrict__ partial, const int* __restrict__ nfpart,
                                                                    long long nchunks, double grad_scale, double clip_norm,
                                                                    int skip_nonfinite, ups_step_guard* __restrict__ rec) {
    __shared__ double fold[kBlock];
    __shared__ long long nfw[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double s = 0.0;
    long long nf = 0;
    for (long long j = tid; j < nchunks; j += kBlock) {
        s += partial[j];
        nf += nfpart[j];
    }
    fold[tid] = s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if (lane == 0) nfw[wid] = nf;
    __syncthreads();
    if (wid != 0) return;
    const double sumsq = tree256(fold, lane);
    if (lane != 0) return;
    const long long nonfinite = (nfw[0] + nfw[1]) + (nfw[2] + nfw[3]);
    const double norm = sqrt(sumsq) * grad_scale;
    float scale = 1.f;
    if (clip_norm > 0.0) {
        const double den = (norm > clip_norm || norm != norm) ? norm : clip_norm;      // max(norm, clip_norm); a NaN norm stays NaN
        scale = (float)(clip_norm / den);
    }
    const int skip = skip_nonfinite && nonfinite > 0;
    rec->sumsq = sumsq;
    rec->norm = norm;
    rec->scale = scale;
    rec->skip = skip;
    rec->nonfinite = nonfinite;
    if (skip) {
        rec->skipped_total += 1;
        rec->consecutive += 1;
    } else {
        rec->consecutive = 0;
        if (scale < 1.f) rec->clipped_total += 1;
    }
}

__global__ void state_update_guarded_kernel(const float* __restrict__ stats, const float* __restrict__ old, float* __restrict__ out,
                                            float decay, float gain, int up_loa, float loa_lr, float loa_target, int up_lor,
                                            float lor_lr, float lor_target, float lor_min, float lor_max,
                                            long long* __restrict__ skipped) {
    const int i = threadIdx.x;
    if (i >= 9) return;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) bad |= (__float_as_uint(stats[k]) & 0x7f800000u) == 0x7f800000u;
    const float o = old[i];
    out[i] = bad ? o : ups_state_value(i, stats, o, decay, gain, up_loa, loa_lr, loa_target, up_lor, lor_lr, lor_target, lor_min, lor_max);
    if (i == 0) {
        if (bad) {
            skipped[0] += 1;
            skipped[1] += 1;
        } else {
            skipped[1] = 0;
        }
    }
}

inline long long chunks_of(int64_t count) { return (count + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int32_t ups_step_guard_bytes(void) { return (int32_t)sizeof(ups_step_guard); }
extern "C" int32_t ups_grad_guard_chunk(void) { return kChunk; }

// nchunks doubles, then nchunks int32 (padded to 8 bytes); never 0, so that a caller can always allocate it
extern "C" size_t ups_grad_guard_scratch_bytes(int64_t count) {
    if (count < 0 || chunks_of(count) > kMaxChunks) return 0;
    const long long nc = chunks_of(count);
    return (size_t)(nc * 8 + ((nc * 4 + 7) / 8) * 8 + 16);
}

extern "C" int ups_grad_guard(const float* g, int64_t count, double grad_scale, double clip_norm, int32_t skip_nonfinite, void* scratch,
                              ups_step_guard* rec, int32_t max_blocks, void* stream) {
    UPS_CHECK_ARG(rec && scratch && count >= 0 && (g || count == 0) && max_blocks >= 0);
    UPS_CHECK_ARG(((unsigned long long)g & 3ull) == 0 && ((unsigned long long)scratch & 7ull) == 0 && ((unsigned long long)rec & 7ull) == 0);
    UPS_CHECK_ARG(clip_norm >= 0.0 && grad_scale == grad_scale);        // (a NaN clip_norm fails the comparison)
    const long long nc = chunks_of(count);
    UPS_CHECK_ARG(nc <= kMaxChunks);
    double* partial = reinterpret_cast<double*>(scratch);
    int* nfpart = reinterpret_cast<int*>(partial + nc);
    hipStream_t s = (hipStream_t)stream;
    if (nc > 0) {
        const long long cap = max_blocks > 0 ? max_blocks : kDefaultBlocks;
        hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)(nc < cap ? nc : cap)), dim3(kBlock), 0, s, g, (long long)count, nc, partial,
                           nfpart);
        UPS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)partial, (const int*)nfpart, nc, grad_scale,
                       clip_norm, (int)(skip_nonfinite != 0), rec);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_adam_guarded(float* p, const float* g, float* m, float* v, int64_t count, float lr_t, const float* lr_t_dev, float beta1,
                                float beta2, float eps, float grad_scale, const ups_step_guard* rec, void* stream) {
    UPS_CHECK_ARG(p && g && m && v && rec && count >= 0);
    if (count == 0) return UPS_OK;
    hipLaunchKernelGGL(adam_kernel<true>, dim3(ups_adam_grid(count)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)count, lr_t,
                       lr_t_dev, beta1, beta2, eps, grad_scale, rec);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_state_update_guarded(const float* stats, const float* old_state, float* new_state, float decay, float gain,
                                        int32_t update_loa, float loa_lr, float loa_target, int32_t update_lor, float lor_lr,
                                        float lor_target, float lor_min, float lor_max, int64_t* skipped, void* stream) {
    UPS_CHECK_ARG(stats && old_state && new_state && skipped && lor_min <= lor_max);
    hipLaunchKernelGGL(state_update_guarded_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, old_state, new_state, decay, gain,
                       update_loa, loa_lr, loa_target, update_lor, lor_lr, lor_target, lor_min, lor_max,
                       reinterpret_cast<long long*>(skipped));
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
