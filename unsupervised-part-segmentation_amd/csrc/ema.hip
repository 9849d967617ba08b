// Weight EMA: the shadow buckets of all optimizer keys updated in the step without the host (ups_ema_update: one one-block launch that
// turns each key's update count and skip flag into its 1 - decay, one streaming launch over every key's bucket), and the in-place exchange
// of shadows and weights (ups_ema_swap).  Definitions: include/upsparts_hip.h; restated in NumPy with equal bits by tests/ema_ref.py.
#include "common.h"

static_assert(sizeof(ups_ema_item) == 32, "ups_ema_item is a 32-byte record (lib.EmaItem mirrors it)");

namespace {

constexpr int kBlock = 256;                     // threads of a block
constexpr int kVecs = 4;                        // 16-byte pieces of the shadow a thread takes per chunk, kBlock pieces apart
constexpr int kChunkVecs = kBlock * kVecs;      // pieces per chunk: 16 KB of shadow, 16 KB of weights
constexpr int kDefaultBlocks = 2048;            // 8 blocks per CU on 256 CUs

// the items by value in the kernel arguments (the bucket pointers never change: a captured graph bakes them in), and where each item's
// chunks begin in the grid's chunk numbering: item k owns chunks [first[k], first[k + 1])
struct EmaArgs {
    ups_ema_item it[UPS_EMA_MAX_ITEMS];
    long long first[UPS_EMA_MAX_ITEMS + 1];
    int n;
};

// elements in front of the first 16-byte aligned one of a 4-byte aligned bucket
__host__ __device__ inline int ema_head(const float* p, long long count) {
    const int h = (int)((4u - (unsigned)(((unsigned long long)p >> 2) & 3ull)) & 3u);
    return count < h ? (int)count : h;
}
// an item's chunks: its aligned 16-byte pieces in chunks of kChunkVecs; chunk 0 also takes the single elements in front of and behind them
inline long long ema_chunks(const ups_ema_item& it) {
    if (it.count <= 0) return 0;
    const long long nvec = (it.count - ema_head(it.shadow, it.count)) >> 2;
    const long long nc = (nvec + kChunkVecs - 1) / kChunkVecs;
    return nc > 0 ? nc : 1;
}

// s - (s - w) * omd, three fp32 operations of one rounding each
__device__ __forceinline__ float ema1(float s, float w, float omd) {
#pragma clang fp contract(off)
    const float t = s - w;
    const float u = t * omd;
    return s - u;
}

// four floats at a 4-byte aligned address: the widest accesses that alignment permits
__device__ __forceinline__ f32x4 ld4u(const float* p) {
    f32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void st4u(float* p, const f32x4& v) { __builtin_memcpy(p, &v, 16); }

template <bool SWAP>
__device__ __forceinline__ void ema_one(float* s, float* w, float omd) {
    const float a = *s, b = *w;
    if constexpr (SWAP) {
        *s = b;
        *w = a;
    } else {
        *s = ema1(a, b, omd);
    }
}
template <bool SWAP>
__device__ __forceinline__ f32x4 ema_vec(const f32x4& a, const f32x4& b, float omd) {
    if constexpr (SWAP) return b;
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = ema1(a[e], b[e], omd);
    return r;
}

// (a) one thread per item: this update's 1 - decay in fp64, the count advanced -- or 0 and the count kept when the key's step was skipped
__global__ void ema_prepare_kernel(const EmaArgs a, double decay, int warmup, long long* __restrict__ n_updates, float* __restrict__ omd) {
    const int k = threadIdx.x;
    if (k >= a.n) return;
    const ups_step_guard* rec = a.it[k].rec;
    if (rec && rec->skip != 0) {
        omd[k] = 0.f;
        return;
    }
    const long long n = n_updates[k];
    double d = decay;
    if (warmup) {
        const double r = (1.0 + (double)n) / (10.0 + (double)n);      // TF's num_updates rule
        d = d < r ? d : r;
    }
    omd[k] = (float)(1.0 - d);
    n_updates[k] = n + 1;
}

// (b) one block per (item, chunk), striding over the chunks when the grid is capped.  The 16-byte pieces are laid on the SHADOW (read
// and written: 8 of the 12 bytes per element); the weights take 16-byte loads when they are misaligned alike, and the widest loads their
// alignment permits otherwise.  Every load of a chunk is in flight before the first store.
template <bool SWAP>
__global__ __launch_bounds__(kBlock) void ema_stream_kernel(const EmaArgs a, const float* omd) {
    const int tid = threadIdx.x;
    const long long total = a.first[a.n];
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        int k = 0;
        while (c >= a.first[k + 1]) ++k;        // (an item without chunks has first[k + 1] == first[k] and is passed over)
        const ups_ema_item it = a.it[k];
        float f = 0.f;
        if constexpr (!SWAP) {
            if (it.rec && it.rec->skip != 0) continue;      // a skipped key: the shadow keeps its bits and is not written
            f = omd[k];
        }
        const long long cc = c - a.first[k];
        const int head = ema_head(it.shadow, it.count);
        float* s = it.shadow + head;
        float* w = it.weights + head;
        const long long body = it.count - head, nvec = body >> 2;
        const int tail = (int)(body & 3);
        if (cc == 0) {          // the single elements: in front of the pieces (wave 0) and behind them (wave 1)
            if (tid < head) ema_one<SWAP>(it.shadow + tid, it.weights + tid, f);
            else if (tid >= 64 && tid < 64 + tail) ema_one<SWAP>(s + 4 * nvec + (tid - 64), w + 4 * nvec + (tid - 64), f);
        }
        const long long v0 = cc * kChunkVecs + tid;
        const bool w16 = ((unsigned long long)w & 15ull) == 0;
        f32x4 sv[kVecs], wv[kVecs];
        if (w16 && cc * kChunkVecs + kChunkVecs <= nvec) {      // a whole chunk, both sides aligned
#pragma unroll
            for (int j = 0; j < kVecs; ++j) {
                sv[j] = *reinterpret_cast<const f32x4*>(s + 4 * (v0 + j * kBlock));
                wv[j] = *reinterpret_cast<const f32x4*>(w + 4 * (v0 + j * kBlock));
            }
#pragma unroll
            for (int j = 0; j < kVecs; ++j) {
                *reinterpret_cast<f32x4*>(s + 4 * (v0 + j * kBlock)) = ema_vec<SWAP>(sv[j], wv[j], f);
                if constexpr (SWAP) *reinterpret_cast<f32x4*>(w + 4 * (v0 + j * kBlock)) = sv[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < kVecs; ++j) {
                const long long v = v0 + j * kBlock;
                if (v < nvec) {
                    sv[j] = *reinterpret_cast<const f32x4*>(s + 4 * v);
                    wv[j] = w16 ? *reinterpret_cast<const f32x4*>(w + 4 * v) : ld4u(w + 4 * v);
                }
            }
#pragma unroll
            for (int j = 0; j < kVecs; ++j) {
                const long long v = v0 + j * kBlock;
                if (v < nvec) {
                    *reinterpret_cast<f32x4*>(s + 4 * v) = ema_vec<SWAP>(sv[j], wv[j], f);
                    if constexpr (SWAP) {
                        if (w16) *reinterpret_cast<f32x4*>(w + 4 * v) = sv[j];
                        else st4u(w + 4 * v, sv[j]);
                    }
                }
            }
        }
    }
}

// the checks both entries share, and the chunk numbering
int ema_args(const ups_ema_item* items, int32_t n_items, int32_t max_blocks, EmaArgs* a) {
    UPS_CHECK_ARG(n_items >= 0 && n_items <= UPS_EMA_MAX_ITEMS && (items || n_items == 0) && max_blocks >= 0);
    a->n = n_items;
    a->first[0] = 0;
    for (int k = 0; k < UPS_EMA_MAX_ITEMS; ++k) {
        if (k < n_items) {
            const ups_ema_item& it = items[k];
            UPS_CHECK_ARG(it.count >= 0 && ((it.shadow && it.weights) || it.count == 0));
            UPS_CHECK_ARG(((unsigned long long)it.shadow & 3ull) == 0 && ((unsigned long long)it.weights & 3ull) == 0 &&
                          ((unsigned long long)it.rec & 7ull) == 0);
            a->it[k] = it;
            a->first[k + 1] = a->first[k] + ema_chunks(it);
        } else {
            a->it[k] = ups_ema_item{nullptr, nullptr, 0, nullptr};
            a->first[k + 1] = a->first[k];
        }
    }
    return UPS_OK;
}

inline unsigned ema_grid(long long total, int32_t max_blocks) {
    const long long cap = max_blocks > 0 ? max_blocks : kDefaultBlocks;
    return (unsigned)(total < cap ? total : cap);
}

}  // namespace

extern "C" int32_t ups_ema_item_bytes(void) { return (int32_t)sizeof(ups_ema_item); }

extern "C" int ups_ema_update(const ups_ema_item* items, int32_t n_items, double decay, int32_t warmup, int64_t* n_updates, float* omd,
                              int32_t max_blocks, void* stream) {
    EmaArgs a;
    const int rc = ema_args(items, n_items, max_blocks, &a);
    if (rc != UPS_OK) return rc;
    UPS_CHECK_ARG(n_updates && omd && ((unsigned long long)n_updates & 7ull) == 0 && ((unsigned long long)omd & 3ull) == 0);
    UPS_CHECK_ARG(decay >= 0.0 && decay < 1.0);        // (a NaN decay fails both comparisons)
    if (n_items == 0) return UPS_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(64), 0, s, a, decay, (int)(warmup != 0), reinterpret_cast<long long*>(n_updates),
                       omd);
    UPS_LAUNCH_CHECK();
    const long long total = a.first[n_items];
    if (total > 0) {
        hipLaunchKernelGGL(ema_stream_kernel<false>, dim3(ema_grid(total, max_blocks)), dim3(kBlock), 0, s, a, (const float*)omd);
        UPS_LAUNCH_CHECK();
    }
    return UPS_OK;
}

extern "C" int ups_ema_swap(const ups_ema_item* items, int32_t n_items, int32_t max_blocks, void* stream) {
    EmaArgs a;
    const int rc = ema_args(items, n_items, max_blocks, &a);
    if (rc != UPS_OK) return rc;
    const long long total = a.first[a.n];
    if (n_items == 0 || total == 0) return UPS_OK;
    hipLaunchKernelGGL(ema_stream_kernel<true>, dim3(ema_grid(total, max_blocks)), dim3(kBlock), 0, (hipStream_t)stream, a,
                       (const float*)nullptr);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
