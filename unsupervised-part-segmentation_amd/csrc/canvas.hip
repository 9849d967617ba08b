// Training image logs: the img_ops of M:968-1053 rendered as uint8 canvases (ups_canvas_*; declared in include/upsparts_hip.h).
//
// Every kernel writes bytes straight into a caller-owned canvas [rows*H, cols*W, C] (C = 3 RGB, C = 1 gray).  The canvas is taken
// as one flat byte array: thread t owns the RUN of bytes [16 t, 16 t + 16) and writes it with one 16-byte store (the last run of a
// canvas whose size is no multiple of 16 falls back to byte stores).  A run walks its pixels in canvas order -- 5 or 6 pixels of an
// RGB canvas, 16 of a gray one -- and asks a pixel functor for each; the functor maps the canvas position back through the tiling
// to (image, y, x), reads its sources and returns the packed bytes.  Nothing is staged: masks and views are read once per use and
// the bytes are written once (the kernels are bound by their stores; the sources of neighbouring runs share cache lines).
//
// Arithmetic: sources are fp32 / bf16 values; every DECISION -- the truncation of the quantisation, the comparison with a level or
// an edge threshold, the half-to-even rounding of the colour index -- is taken on fp64 arithmetic over those values, in the
// operation order of tests/imglog_ref.py, with contraction off.  The canvases therefore equal the fp64 restatement byte for byte;
// the fp32 graph of the reference can differ only where a value lies within an fp32 rounding of a decision boundary.
//
//   quantisation (edflow save_image, re-derived, UNVERIFIED): byte = (uint8) clamp((v + 1) * 127.5, 0, 255), truncating.  Value 0
//   (a blank tile, a masked-out pixel) is byte 127; images the reference leaves in [0,1] go through the same rule and come out
//   between gray (127) and white (255).
//   tiling (tf_batch_to_canvas, re-derived, UNVERIFIED): row-major, tile n at (n / cols, n % cols); tiles n >= N are blank.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RUN = 16;                 // bytes per thread: one 16-byte store
constexpr unsigned BLANK = 127u;        // quantise(0)
constexpr unsigned BLANK3 = BLANK | (BLANK << 8) | (BLANK << 16);
constexpr int MAX_SETS = 8;             // level / ratio thresholds of ups_canvas_first_item

__device__ __forceinline__ unsigned quantise(double v) {
    double q = (v + 1.0) * 127.5;
    q = !(q >= 0.0) ? 0.0 : (q > 255.0 ? 255.0 : q);    // (NaN -> 0: the conversion below never sees one)
    return (unsigned)(int)q;
}

template <typename T> __device__ __forceinline__ float ld_val(const T* p, long long i) { return (float)p[i]; }

// ---- the run: 16 bytes of a [.., Wc, C] canvas starting at byte 16 * run
template <int C, typename F>
__device__ __forceinline__ void canvas_run(uint8_t* __restrict__ canvas, long long run, long long total, int Wc, const F& f) {
    const long long b0 = run * RUN;
    if (b0 >= total) return;
    long long px = b0 / C;
    int c = (int)(b0 - px * C);
    long long Y = px / Wc;
    int X = (int)(px - Y * Wc);
    const int n = total - b0 >= RUN ? RUN : (int)(total - b0);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    unsigned pix = f(Y, X);
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
        if (i < n) {
            w[i >> 2] |= ((pix >> (8 * c)) & 255u) << (8 * (i & 3));
            if (++c == C) {
                c = 0;
                if (++X == Wc) { X = 0; ++Y; }
                if (i + 1 < n) pix = f(Y, X);
            }
        }
    }
    if (n == RUN) {
        *reinterpret_cast<uint4*>(canvas + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int i = 0; i < n; ++i) canvas[b0 + i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
    }
}

template <int C, typename F>
__global__ __launch_bounds__(256) void canvas_kernel(uint8_t* __restrict__ canvas, long long total, int Wc, F f) {
    canvas_run<C>(canvas, (long long)blockIdx.x * 256 + threadIdx.x, total, Wc, f);
}

// ---- pixel functors.  Each returns r | g << 8 | b << 16 (gray: the byte) of canvas pixel (Y, X).
template <typename T> struct ImagesPx {          // [N,H,W,ld] in [-1,1] -> tiles
    const T* img; int N, H, W, ld, cols;
    __device__ unsigned operator()(long long Y, int X) const {
        const int tr = (int)(Y / H), y = (int)(Y - (long long)tr * H), tc = X / W, x = X - tc * W;
        const long long n = (long long)tr * cols + tc;
        if (n >= N) return BLANK3;
        const long long o = ((n * H + y) * W + x) * ld;
        return quantise(ld_val(img, o)) | (quantise(ld_val(img, o + 1)) << 8) | (quantise(ld_val(img, o + 2)) << 16);
    }
};

// part index of a pixel's mask: MODE 0 arg-max (lowest index wins ties, tf.argmax), 1 the mask is one-hot already (first non-zero
// entry; -1 when there is none: the reference's sum of hot * colour is then 0), 2 the sign-packed hard bits (lowest set bit)
template <int MODE> __device__ __forceinline__ int part_of(const float* __restrict__ mask, const uint32_t* __restrict__ bits, long long pixel, int P) {
    if (MODE == 2) {
        const uint32_t b = bits[pixel];
        return b ? __ffs((int)b) - 1 : -1;
    }
    const float* m = mask + pixel * P;
    if (MODE == 1) {
        for (int p = 0; p < P; ++p)
            if (m[p] != 0.f) return p;
        return -1;
    }
    int best = 0;
    float bv = m[0];
    for (int p = 1; p < P; ++p) {
        const float v = m[p];
        if (v > bv) { bv = v; best = p; }
    }
    return best;
}

template <int MODE> struct MaskRgbPx {           // [N,H,W,P] -> colour of the pixel's part -> tiles
    const float* mask; const uint32_t* bits; const uint8_t* colors; int N, H, W, P, cols;
    __device__ unsigned operator()(long long Y, int X) const {
        const int tr = (int)(Y / H), y = (int)(Y - (long long)tr * H), tc = X / W, x = X - tc * W;
        const long long n = (long long)tr * cols + tc;
        if (n >= N) return BLANK3;
        const int p = part_of<MODE>(mask, bits, (n * H + y) * W + x, P);
        if (p < 0) return BLANK3;
        return (unsigned)colors[3 * p] | ((unsigned)colors[3 * p + 1] << 8) | ((unsigned)colors[3 * p + 2] << 16);
    }
};

// M:990-1006: for part p the grid (cols=None: g x g, g = ceil(sqrt(2B))) of hard0[b][..][p] * view0[b] (b < B) followed by
// hard1[b][..][p] * view1[b]; the P grids in 5 columns
template <typename T, bool BITS> struct AssignedPx {
    const float* hard0; const float* hard1; const uint32_t* bits0; const uint32_t* bits1; const T* view0; const T* view1;
    int B, H, W, P, ld, g, ocols;
    __device__ unsigned operator()(long long Y, int X) const {
        const int gh = g * H, gw = g * W;
        const int pr = (int)(Y / gh), yy = (int)(Y - (long long)pr * gh), pc = X / gw, xx = X - pc * gw;
        const int p = pr * ocols + pc;
        if (p >= P) return BLANK3;
        const int ir = yy / H, y = yy - ir * H, ic = xx / W, x = xx - ic * W;
        const int i = ir * g + ic;
        if (i >= 2 * B) return BLANK3;
        const bool second = i >= B;
        const long long pixel = ((long long)(second ? i - B : i) * H + y) * W + x;
        double mk;
        if (BITS) mk = (((second ? bits1 : bits0)[pixel] >> p) & 1u) ? 1.0 : 0.0;
        else mk = (double)(second ? hard1 : hard0)[pixel * P + p];
        const T* v = (second ? view1 : view0);
        const long long o = pixel * ld;
        return quantise(mk * (double)ld_val(v, o)) | (quantise(mk * (double)ld_val(v, o + 1)) << 8) | (quantise(mk * (double)ld_val(v, o + 2)) << 16);
    }
};

// ---- first item of the batch (M:986-988, 1009-1032): four gray / RGB canvases from m = m0_sample[0] and the hard mask of image 0
struct LevelsPx {                                // [P*H, nl*W]: row p, column k: m[..p] > level[k]   (M:1012-1017)
    const float* m; int H, W, P; float lev[MAX_SETS];
    __device__ unsigned operator()(long long Y, int X) const {
        const int p = (int)(Y / H), y = (int)(Y - (long long)p * H), k = X / W, x = X - k * W;
        return m[((long long)y * W + x) * P + p] > lev[k] ? 255u : BLANK;
    }
};

struct EdgesPx {                                 // [P*H, nr*W]: row p, column k: |grad m[..p]|^2 > ratio[k]   (M:1021-1029, N:1366-1404)
    const float* m; int H, W, P; float ratio[MAX_SETS];
    __device__ unsigned operator()(long long Y, int X) const {
        const int p = (int)(Y / H), y = (int)(Y - (long long)p * H), k = X / W, x = X - k * W;
        // N:1366-1374: the 3x3 filters hold 0.5 * [0, 0.5, -0.5] along x (resp. y): 0.25 * (m[y][x] - m[y][x+1]), zero beyond the edge
        const double a = (double)m[((long long)y * W + x) * P + p];
        const double r = x + 1 < W ? (double)m[((long long)y * W + x + 1) * P + p] : 0.0;
        const double d = y + 1 < H ? (double)m[((long long)(y + 1) * W + x) * P + p] : 0.0;
        const double gx = 0.25 * (a - r), gy = 0.25 * (a - d);
        const double g = gx * gx + gy * gy;
        return g > (double)ratio[k] ? 255u : BLANK;
    }
};

struct HeatPx {                                  // p_heatmap (M:1031-1032, N:2051-2062): viridis[rint(255 m)], P tiles, cols=None
    const float* m; const uint8_t* table; int H, W, P, g;
    __device__ unsigned operator()(long long Y, int X) const {
        const int tr = (int)(Y / H), y = (int)(Y - (long long)tr * H), tc = X / W, x = X - tc * W;
        const int p = tr * g + tc;
        if (p >= P) return BLANK3;
        double v = rint((double)m[((long long)y * W + x) * P + p] * 255.0);       // half to even (tf.round)
        v = v >= 0.0 ? (v > 255.0 ? 255.0 : v) : 0.0;                              // (NaN -> 0)
        const int i = 3 * (int)v;
        return (unsigned)table[i] | ((unsigned)table[i + 1] << 8) | ((unsigned)table[i + 2] << 16);
    }
};

template <bool BITS> struct MasksPx {            // masks (M:986-988): hard[0][..][p] as P gray tiles, cols=None
    const float* hard; const uint32_t* bits; int H, W, P, g;
    __device__ unsigned operator()(long long Y, int X) const {
        const int tr = (int)(Y / H), y = (int)(Y - (long long)tr * H), tc = X / W, x = X - tc * W;
        const int p = tr * g + tc;
        if (p >= P) return BLANK;
        const long long pixel = (long long)y * W + x;
        if (BITS) return ((bits[pixel] >> p) & 1u) ? 255u : BLANK;
        return quantise((double)hard[pixel * P + p]);
    }
};

struct FirstItemArgs {
    uint8_t *levels, *edges, *heat, *masks;
    long long t_levels, t_edges, t_heat, t_masks;        // bytes of each canvas
    long long r_levels, r_edges, r_heat;                 // runs of the first three (the fourth takes the rest)
    int w_levels, w_edges, w_tiles;                      // canvas widths in pixels
};

template <bool BITS>
__global__ __launch_bounds__(256) void first_item_kernel(FirstItemArgs a, LevelsPx lv, EdgesPx ed, HeatPx ht, MasksPx<BITS> mk) {
    long long run = (long long)blockIdx.x * 256 + threadIdx.x;
    if (run < a.r_levels) { canvas_run<1>(a.levels, run, a.t_levels, a.w_levels, lv); return; }
    run -= a.r_levels;
    if (run < a.r_edges) { canvas_run<1>(a.edges, run, a.t_edges, a.w_edges, ed); return; }
    run -= a.r_edges;
    if (run < a.r_heat) { canvas_run<3>(a.heat, run, a.t_heat, a.w_tiles, ht); return; }
    run -= a.r_heat;
    canvas_run<1>(a.masks, run, a.t_masks, a.w_tiles, mk);
}

inline long long runs_of(long long bytes) { return (bytes + RUN - 1) / RUN; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline int grid_side(int n) { int g = 1; while ((long long)g * g < n) ++g; return g; }      // ceil(sqrt(n))

template <int C, typename F> int launch_canvas(uint8_t* canvas, long long total, int Wc, const F& f, void* stream) {
    const long long blocks = (runs_of(total) + 255) / 256;
    UPS_CHECK_ARG(blocks >= 1 && blocks <= 0x7fffffffLL);
    hipLaunchKernelGGL((canvas_kernel<C, F>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, canvas, total, Wc, f);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

}  // namespace

extern "C" int ups_canvas_grid_side(int32_t n) { return n < 1 ? 0 : grid_side(n); }

extern "C" int ups_canvas_images(const void* img, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t ld, int32_t rows, int32_t cols,
                                 uint8_t* canvas, void* stream) {
    UPS_CHECK_ARG(img && canvas && aligned16(canvas));
    UPS_CHECK_ARG(dtype == UPS_F32 || dtype == UPS_BF16);
    UPS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && ld >= 3 && rows >= 1 && cols >= 1 && (long long)rows * cols >= N);
    UPS_CHECK_ARG((long long)cols * W <= 0x7fffffffLL);
    const long long total = (long long)rows * H * cols * W * 3;
    if (dtype == UPS_F32) return launch_canvas<3>(canvas, total, cols * W, ImagesPx<float>{(const float*)img, N, H, W, ld, cols}, stream);
    return launch_canvas<3>(canvas, total, cols * W, ImagesPx<bf16>{(const bf16*)img, N, H, W, ld, cols}, stream);
}

extern "C" int ups_canvas_mask_rgb(const float* mask, const uint32_t* bits, int32_t one_hot, const uint8_t* colors, int32_t N, int32_t H,
                                   int32_t W, int32_t P, int32_t rows, int32_t cols, uint8_t* canvas, void* stream) {
    UPS_CHECK_ARG((mask != nullptr) != (bits != nullptr));
    UPS_CHECK_ARG(colors && canvas && aligned16(canvas));
    UPS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && P >= 1 && rows >= 1 && cols >= 1 && (long long)rows * cols >= N);
    UPS_CHECK_ARG(!bits || P <= 32);
    UPS_CHECK_ARG((long long)cols * W <= 0x7fffffffLL);
    const long long total = (long long)rows * H * cols * W * 3;
    if (bits) return launch_canvas<3>(canvas, total, cols * W, MaskRgbPx<2>{nullptr, bits, colors, N, H, W, P, cols}, stream);
    if (one_hot) return launch_canvas<3>(canvas, total, cols * W, MaskRgbPx<1>{mask, nullptr, colors, N, H, W, P, cols}, stream);
    return launch_canvas<3>(canvas, total, cols * W, MaskRgbPx<0>{mask, nullptr, colors, N, H, W, P, cols}, stream);
}

extern "C" int ups_canvas_assigned_parts(const float* hard0, const float* hard1, const uint32_t* bits0, const uint32_t* bits1,
                                         const void* view0, const void* view1, int32_t dtype, int32_t ld, int32_t B, int32_t H, int32_t W,
                                         int32_t P, uint8_t* canvas, void* stream) {
    const bool by_bits = bits0 != nullptr;
    UPS_CHECK_ARG(by_bits ? (bits1 && !hard0 && !hard1) : (hard0 && hard1 && !bits1));
    UPS_CHECK_ARG(view0 && view1 && canvas && aligned16(canvas));
    UPS_CHECK_ARG(dtype == UPS_F32 || dtype == UPS_BF16);
    UPS_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && P >= 1 && ld >= 3 && (!by_bits || P <= 32));
    const int g = grid_side(2 * B), ocols = 5, orows = (P + ocols - 1) / ocols;
    UPS_CHECK_ARG((long long)ocols * g * W <= 0x7fffffffLL && (long long)g * H <= 0x7fffffffLL);
    const int Wc = ocols * g * W;
    const long long total = (long long)orows * g * H * Wc * 3;
    const float *h0 = hard0, *h1 = hard1;
    if (dtype == UPS_F32) {
        const float *v0 = (const float*)view0, *v1 = (const float*)view1;
        if (by_bits) return launch_canvas<3>(canvas, total, Wc, AssignedPx<float, true>{h0, h1, bits0, bits1, v0, v1, B, H, W, P, ld, g, ocols}, stream);
        return launch_canvas<3>(canvas, total, Wc, AssignedPx<float, false>{h0, h1, bits0, bits1, v0, v1, B, H, W, P, ld, g, ocols}, stream);
    }
    const bf16 *v0 = (const bf16*)view0, *v1 = (const bf16*)view1;
    if (by_bits) return launch_canvas<3>(canvas, total, Wc, AssignedPx<bf16, true>{h0, h1, bits0, bits1, v0, v1, B, H, W, P, ld, g, ocols}, stream);
    return launch_canvas<3>(canvas, total, Wc, AssignedPx<bf16, false>{h0, h1, bits0, bits1, v0, v1, B, H, W, P, ld, g, ocols}, stream);
}

extern "C" int ups_canvas_first_item(const float* m, const float* hard, const uint32_t* bits, int32_t H, int32_t W, int32_t P,
                                     const float* levels, int32_t n_levels, const float* ratios, int32_t n_ratios, const uint8_t* table,
                                     uint8_t* c_levels, uint8_t* c_edges, uint8_t* c_heat, uint8_t* c_masks, void* stream) {
    UPS_CHECK_ARG(m && table && levels && ratios && (hard != nullptr) != (bits != nullptr));
    UPS_CHECK_ARG(c_levels && c_edges && c_heat && c_masks);
    UPS_CHECK_ARG(aligned16(c_levels) && aligned16(c_edges) && aligned16(c_heat) && aligned16(c_masks));
    UPS_CHECK_ARG(H >= 1 && W >= 1 && P >= 1 && (!bits || P <= 32));
    UPS_CHECK_ARG(n_levels >= 1 && n_levels <= MAX_SETS && n_ratios >= 1 && n_ratios <= MAX_SETS);
    const int g = grid_side(P);
    UPS_CHECK_ARG((long long)MAX_SETS * W <= 0x7fffffffLL && (long long)g * W <= 0x7fffffffLL);
    FirstItemArgs a;
    a.levels = c_levels; a.edges = c_edges; a.heat = c_heat; a.masks = c_masks;
    a.w_levels = n_levels * W; a.w_edges = n_ratios * W; a.w_tiles = g * W;
    a.t_levels = (long long)P * H * a.w_levels;
    a.t_edges = (long long)P * H * a.w_edges;
    a.t_heat = (long long)g * H * a.w_tiles * 3;
    a.t_masks = (long long)g * H * a.w_tiles;
    a.r_levels = runs_of(a.t_levels); a.r_edges = runs_of(a.t_edges); a.r_heat = runs_of(a.t_heat);
    const long long blocks = (a.r_levels + a.r_edges + a.r_heat + runs_of(a.t_masks) + 255) / 256;
    UPS_CHECK_ARG(blocks <= 0x7fffffffLL);
    LevelsPx lv{m, H, W, P, {}};
    EdgesPx ed{m, H, W, P, {}};
    for (int i = 0; i < n_levels; ++i) lv.lev[i] = levels[i];
    for (int i = 0; i < n_ratios; ++i) ed.ratio[i] = ratios[i];
    HeatPx ht{m, table, H, W, P, g};
    if (bits) hipLaunchKernelGGL(first_item_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, lv, ed, ht,
                                 MasksPx<true>{nullptr, bits, H, W, P, g});
    else hipLaunchKernelGGL(first_item_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, lv, ed, ht,
                            MasksPx<false>{hard, nullptr, H, W, P, g});
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
