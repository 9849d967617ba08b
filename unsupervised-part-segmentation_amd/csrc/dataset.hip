// Device-resident training data: the batch views gathered from a uint8 image store (ups_gather_views; declared in
// include/upsparts_hip.h).
//
// The store is [n_images, S, S, 3] uint8 -- every image of the csv decoded and resized ONCE (data.build_u8_store) -- and a step's
// batch is described by a plan [B, 3] int32: source image of view0, source image of view1, flip bits (bit 0 horizontal, bit 1
// vertical; one draw flips both views).  The kernel writes what StochasticPairs.get_example + batches() would have stacked on the host:
//
//     view0[b][y][x][c] = target[b][y][x][c] = lut(images[plan[b][0]][fv ? S-1-y : y][fh ? S-1-x : x][c])
//     view1[b][y][x][c] =                      lut(images[plan[b][1]][ same source pixel ][c])
//     lut(u) = float(u) / 127.5f - 1.0f          (channels are never reversed)
//
// lut is the host's `np.float32(u) / 127.5 - 1.0`: one correctly rounded fp32 division (hipcc's default for `/`; the library is built
// without fast-math) and one fp32 subtraction, contraction off -- equal to NumPy bit for bit over all 256 bytes
// (tests/test_gpu_devdata.py).
//
// Form: pure streaming, no LDS, no atomics.  S % 4 == 0 (and 4- / 16-byte aligned buffers): a lane owns FOUR consecutive output
// pixels of a row -- 12 source bytes = three dword loads, 12 floats = three float4 stores, per view; a horizontally flipped run
// starts at source pixel S-4-x (dword aligned under the same condition) and its four pixels are taken in reverse.  Otherwise one
// lane per pixel, byte loads and scalar stores.  The launcher chooses.  `target` is stored from the registers of view0.
//
// The host validates every plan index before the copy (data.device_batches); a plan that reaches the kernel with an index outside
// [0, n_images) nevertheless reads nothing out of bounds: that item is written as NaN.
#include "common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float lut(unsigned u) { return (float)u / 127.5f - 1.0f; }

struct Item {                    // one batch item's plan, decoded
    long long i0, i1;            // source images (0 when out of range: `ok` then selects NaN)
    bool ok0, ok1, fh, fv;
};

__device__ __forceinline__ Item read_item(const int32_t* __restrict__ plan, int b, long long n_images) {
    const int p0 = plan[3 * b], p1 = plan[3 * b + 1], fl = plan[3 * b + 2];
    Item it;
    it.ok0 = p0 >= 0 && (long long)p0 < n_images;
    it.ok1 = p1 >= 0 && (long long)p1 < n_images;
    it.i0 = it.ok0 ? p0 : 0;
    it.i1 = it.ok1 ? p1 : 0;
    it.fh = (fl & 1) != 0;
    it.fv = (fl & 2) != 0;
    return it;
}

// four pixels of one view: src -> 12 bytes at a dword-aligned address, dst -> 12 floats at a 16-byte aligned address
__device__ __forceinline__ void run4(const uint8_t* __restrict__ src, bool fh, bool ok, float* __restrict__ dst, float* __restrict__ dst2) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
    // the four RGB pixels as 24-bit values, in source order
    uint32_t p0 = w0 & 0xffffffu, p1 = (w0 >> 24) | ((w1 & 0xffffu) << 8), p2 = (w1 >> 16) | ((w2 & 0xffu) << 16), p3 = w2 >> 8;
    if (fh) {
        uint32_t t = p0; p0 = p3; p3 = t;
        t = p1; p1 = p2; p2 = t;
    }
    const uint32_t px[4] = {p0, p1, p2, p3};
    const float nan = __uint_as_float(0x7fc00000u);
    float f[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) f[3 * k + c] = ok ? lut((px[k] >> (8 * c)) & 255u) : nan;
    float4* d = reinterpret_cast<float4*>(dst);
    d[0] = make_float4(f[0], f[1], f[2], f[3]);
    d[1] = make_float4(f[4], f[5], f[6], f[7]);
    d[2] = make_float4(f[8], f[9], f[10], f[11]);
    if (dst2) {
        float4* e = reinterpret_cast<float4*>(dst2);
        e[0] = make_float4(f[0], f[1], f[2], f[3]);
        e[1] = make_float4(f[4], f[5], f[6], f[7]);
        e[2] = make_float4(f[8], f[9], f[10], f[11]);
    }
}

// S % 4 == 0: thread t owns output pixels [4 xg, 4 xg + 4) of row y of item b, t = (b * S + y) * (S / 4) + xg
__global__ __launch_bounds__(256) void gather_views_x4(const uint8_t* __restrict__ images, long long n_images, const int32_t* __restrict__ plan,
                                                       long long groups, int S, float* __restrict__ view0, float* __restrict__ view1,
                                                       float* __restrict__ target) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= groups) return;
    const int S4 = S >> 2;
    const long long row = t / S4;                   // b * S + y
    const int x = (int)(t - row * S4) << 2;
    const int b = (int)(row / S), y = (int)(row - (long long)b * S);
    const Item it = read_item(plan, b, n_images);
    const int ys = it.fv ? S - 1 - y : y, xs = it.fh ? S - 4 - x : x;
    const long long so = ((long long)ys * S + xs) * 3, img = (long long)S * S * 3;
    const long long o = (row * S + x) * 3;
    run4(images + it.i0 * img + so, it.fh, it.ok0, view0 + o, target ? target + o : nullptr);
    run4(images + it.i1 * img + so, it.fh, it.ok1, view1 + o, nullptr);
}

// any S: thread t owns output pixel t = (b * S + y) * S + x
__global__ __launch_bounds__(256) void gather_views_x1(const uint8_t* __restrict__ images, long long n_images, const int32_t* __restrict__ plan,
                                                       long long pixels, int S, float* __restrict__ view0, float* __restrict__ view1,
                                                       float* __restrict__ target) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pixels) return;
    const long long row = t / S;
    const int x = (int)(t - row * S);
    const int b = (int)(row / S), y = (int)(row - (long long)b * S);
    const Item it = read_item(plan, b, n_images);
    const int ys = it.fv ? S - 1 - y : y, xs = it.fh ? S - 1 - x : x;
    const long long so = ((long long)ys * S + xs) * 3, img = (long long)S * S * 3;
    const uint8_t* s0 = images + it.i0 * img + so;
    const uint8_t* s1 = images + it.i1 * img + so;
    const float nan = __uint_as_float(0x7fc00000u);
    const long long o = t * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = it.ok0 ? lut(s0[c]) : nan;
        view0[o + c] = a;
        if (target) target[o + c] = a;
        view1[o + c] = it.ok1 ? lut(s1[c]) : nan;
    }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int ups_gather_views(const uint8_t* images, int64_t n_images, const int32_t* plan, int32_t B, int32_t S, float* view0,
                                float* view1, float* target, void* stream) {
    UPS_CHECK_ARG(images && plan && view0 && view1);
    UPS_CHECK_ARG(B > 0 && S > 0 && n_images > 0);
    const long long pixels = (long long)B * S * S;
    UPS_CHECK_ARG(pixels * 3 <= 0x7fffffffLL);                                  // (a batch, not the store: the store is indexed in 64 bits)
    UPS_CHECK_ARG(n_images <= 0x7fffffffLL);                                    // plan entries are int32
    const bool x4 = S % 4 == 0 && aligned_to(images, 4) && aligned_to(view0, 16) && aligned_to(view1, 16) && (!target || aligned_to(target, 16));
    const long long threads = x4 ? pixels / 4 : pixels;
    const long long blocks = (threads + 255) / 256;
    UPS_CHECK_ARG(blocks <= 0x7fffffffLL);
    if (x4) hipLaunchKernelGGL(gather_views_x4, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, images, (long long)n_images, plan,
                               threads, S, view0, view1, target);
    else hipLaunchKernelGGL(gather_views_x1, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, images, (long long)n_images, plan,
                            threads, S, view0, view1, target);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
