// Device-side appearance and shape augmentation of the device-resident training data (ups_augment_views, ups_augment_field,
// ups_augment_record_words; declared in include/upsparts_hip.h).
//
// The host draws the realisations of AugmentedPair2's two pipelines (augment.draw_appearance / draw_shape, in the host iterator's
// order) and writes one fixed-size record per OUTPUT image (data.fill_aug_plan); the kernels here execute the records on the uint8
// store of dataset.hip.  An output image's value chain is the host path's (augment.py):
//
//     store byte (plan flips) -> T_in -> appearance ops -> T_mid (only when both pipelines are on) -> shape ops -> v * 2 / 255 - 1
//
// T_in[u] = _to_u8(float32(u) / 127.5 - 1) and T_mid[v] = _to_u8(_from_u8(v)) are the host's truncating uint8 round trips, built by the
// host with augment.py's own expressions and passed in as two 256-byte tables.
//
// Three passes, all images of a batch in one launch each, one lane per pixel, through two uint8 scratch buffers [n,S,S,3] (a 256 x 256
// image does not fit twice in LDS, and the 3 x 3 filters and the warps read neighbours that other blocks produce):
//     pass 1   gather + T_in + 3 x 3 filter + colour chain (bc / rgb / hsv, gray, perm)     -> scratch a
//     pass 2   T_mid + hflip + affine warp                                                  -> scratch b
//     pass 3   grid or elastic warp, v * 2 / 255 - 1                                        -> float32 outputs
// A pass in which an image has no op copies it through.  The record is read block-uniformly (blockIdx.y is the image).  Every warp
// computes its source coordinates in fp32, clamps them to [0, S-1] (a NaN coordinate goes to 0), floors, interpolates
// a + (b - a) * fx along x on both rows and then along y in the same form, and rounds with rintf and a clip: a uint8 rounding after each
// warp, as on the host.  The whole file is compiled with contraction off and hipcc's correctly rounded `/`, so tests/devaug_ref.py's
// float32 NumPy restatement gives the same bits.
//
// The elastic displacement fields come from ups_augment_field: a separable Gaussian (sigma 50, radius 200; the 401 fp32 weights are the
// host's), scipy's `reflect` border repeated as often as the radius needs, axis 0 first, the accumulator starting at 0 and adding
// taps 0 .. 400 in order.
//
// An image whose source index, elastic index or any op code is out of range is written as NaN (and as zero bytes in the scratch); nothing
// is read out of bounds.
#include "common.h"

#pragma clang fp contract(off)

namespace {

// record layout (int32 words; floats are stored by bit pattern).  data.py REC_* mirror these.
constexpr int REC_WORDS = 272;
constexpr int R_SRC = 0, R_FLIP = 1, R_MID = 2, R_FILTER = 3, R_COLOR = 4 /* 3 kinds */, R_CPAR = 7 /* 3 x 3 ints */, R_GRAY = 16, R_PERM = 17,
              R_PIDX = 18 /* 3 */, R_HFLIP = 21, R_AFFINE = 22, R_WARP = 23, R_FIELD = 24, R_AMAT = 32 /* 6 floats */, R_EMAT = 38 /* 6 */,
              R_JY = 44 /* 16 */, R_JX = 60 /* 16 */, R_BC = 76 /* 3 x 256 bytes */;
constexpr int FILTER_MEDIAN = 1, FILTER_BOX = 2, COLOR_BC = 1, COLOR_RGB = 2, COLOR_HSV = 3, WARP_GRID = 1, WARP_ELASTIC = 2;
constexpr int RADIUS = 200, TAPS = 2 * RADIUS + 1;

__device__ __forceinline__ bool flag01(int v) { return v == 0 || v == 1; }

// every index and op code of a record in range?  (block-uniform: all lanes of a block read the same record)
__device__ __forceinline__ bool rec_ok(const int32_t* __restrict__ r, long long n_images, int n_fields) {
    bool ok = r[R_SRC] >= 0 && (long long)r[R_SRC] < n_images;
    ok = ok && (r[R_FLIP] & ~3) == 0 && flag01(r[R_MID]) && r[R_FILTER] >= 0 && r[R_FILTER] <= FILTER_BOX;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && r[R_COLOR + k] >= 0 && r[R_COLOR + k] <= COLOR_HSV && r[R_PIDX + k] >= 0 && r[R_PIDX + k] <= 2;
    ok = ok && flag01(r[R_GRAY]) && flag01(r[R_PERM]) && flag01(r[R_HFLIP]) && flag01(r[R_AFFINE]);
    ok = ok && r[R_WARP] >= 0 && r[R_WARP] <= WARP_ELASTIC;
    ok = ok && (r[R_WARP] != WARP_ELASTIC || (r[R_FIELD] >= 0 && r[R_FIELD] < n_fields));
    return ok;
}

__device__ __forceinline__ float recf(const int32_t* __restrict__ r, int w) { return __int_as_float(r[w]); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clip255(int v) { return clampi(v, 0, 255); }
__device__ __forceinline__ int round_clip(float v) { return (int)fminf(fmaxf(rintf(v), 0.f), 255.f); }      // (v is finite here)

__device__ __forceinline__ void sort2(int& a, int& b) { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }
__device__ __forceinline__ int median9(int* p) {
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]); sort2(p[0], p[1]); sort2(p[3], p[4]); sort2(p[6], p[7]);
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]); sort2(p[0], p[3]); sort2(p[5], p[8]); sort2(p[4], p[7]);
    sort2(p[3], p[6]); sort2(p[1], p[4]); sort2(p[2], p[5]); sort2(p[4], p[7]); sort2(p[4], p[2]); sort2(p[6], p[4]);
    sort2(p[4], p[2]);
    return p[4];
}

// augment._hue_sat_val, operation for operation in fp32
__device__ __forceinline__ void hue_sat_val(int* px, int dh, int ds, int dv) {
    const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
    const float v = fmaxf(fmaxf(r, g), b), d = v - fminf(fminf(r, g), b);
    const float s = v > 0.f ? d / fmaxf(v, 1e-12f) * 255.0f : 0.f;
    const float dd = fmaxf(d, 1e-12f);
    float h = (v == r ? (g - b) / dd : (v == g ? 2.0f + (b - r) / dd : 4.0f + (r - g) / dd)) * 60.0f;
    h = d > 0.f ? h : 0.f;
    h = (h < 0.f ? h + 360.0f : h) / 2.0f;
    int hi = (int)rintf(h);                              // 0 .. 180
    hi = hi >= 180 ? hi - 180 : hi;                      // rint(h) % 180
    int H = (hi + dh) % 180;
    H = H < 0 ? H + 180 : H;                             // NumPy's non-negative remainder
    const int S_ = clip255((int)rintf(s) + ds), V_ = clip255((int)v + dv);
    const float hh = (float)H * 2.0f / 60.0f, ss = (float)S_ / 255.0f, vv = (float)V_;
    const float fl = floorf(hh), f = hh - fl;
    const int i = (int)fl % 6;
    const float p = vv * (1.0f - ss), q = vv * (1.0f - ss * f), t = vv * (1.0f - ss * (1.0f - f));
    const float R = i == 0 || i == 5 ? vv : (i == 1 ? q : (i == 4 ? t : p));
    const float G = i == 0 ? t : (i == 1 || i == 2 ? vv : (i == 3 ? q : p));
    const float B = i <= 1 ? p : (i == 2 ? t : (i == 5 ? q : vv));
    px[0] = round_clip(R); px[1] = round_clip(G); px[2] = round_clip(B);
}

// ---------------------------------------------------------------------------------------------------------------- pass 1
__global__ __launch_bounds__(256) void aug_appearance(const uint8_t* __restrict__ images, long long n_images, const int32_t* __restrict__ recs,
                                                      const uint8_t* __restrict__ luts, int n_fields, int S, uint8_t* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const long long n = blockIdx.y;
    const int32_t* __restrict__ r = recs + n * REC_WORDS;
    const long long o = (n * S * S + pix) * 3;
    if (!rec_ok(r, n_images, n_fields)) {
        out[o] = 0; out[o + 1] = 0; out[o + 2] = 0;
        return;
    }
    const int y = pix / S, x = pix - y * S;
    const bool fh = (r[R_FLIP] & 1) != 0, fv = (r[R_FLIP] & 2) != 0;
    const uint8_t* __restrict__ img = images + (long long)r[R_SRC] * S * S * 3;
    const uint8_t* __restrict__ t_in = luts;
    auto load = [&](int yy, int xx, int* p) {            // (yy, xx) inside the image
        const int ys = fv ? S - 1 - yy : yy, xs = fh ? S - 1 - xx : xx;
        const uint8_t* q = img + ((long long)ys * S + xs) * 3;
        p[0] = t_in[q[0]]; p[1] = t_in[q[1]]; p[2] = t_in[q[2]];
    };
    int px[3];
    const int filter = r[R_FILTER];
    if (filter == 0) {
        load(y, x, px);
    } else {
        int nb[3][9];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                int yy = y + dy, xx = x + dx;
                if (filter == FILTER_BOX) {              // reflect-101: -1 -> 1, S -> S - 2
                    yy = yy < 0 ? -yy : (yy >= S ? 2 * S - 2 - yy : yy);
                    xx = xx < 0 ? -xx : (xx >= S ? 2 * S - 2 - xx : xx);
                }
                int p[3];
                load(clampi(yy, 0, S - 1), clampi(xx, 0, S - 1), p);        // (median: edge replication)
                const int k = (dy + 1) * 3 + dx + 1;
                nb[0][k] = p[0]; nb[1][k] = p[1]; nb[2][k] = p[2];
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (filter == FILTER_MEDIAN) {
                px[c] = median9(nb[c]);
            } else {
                int sum = 0;
#pragma unroll
                for (int k = 0; k < 9; ++k) sum += nb[c][k];
                px[c] = (2 * sum + 9) / 18;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int kind = r[R_COLOR + k];
        if (kind == COLOR_BC) {
            const uint8_t* __restrict__ tab = reinterpret_cast<const uint8_t*>(r + R_BC) + 256 * k;
            px[0] = tab[px[0]]; px[1] = tab[px[1]]; px[2] = tab[px[2]];
        } else if (kind == COLOR_RGB) {
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = clip255(px[c] + clampi(r[R_CPAR + 3 * k + c], -255, 255));
        } else if (kind == COLOR_HSV) {
            hue_sat_val(px, clampi(r[R_CPAR + 3 * k], -32000, 32000), clampi(r[R_CPAR + 3 * k + 1], -32000, 32000),
                        clampi(r[R_CPAR + 3 * k + 2], -32000, 32000));
        }
    }
    if (r[R_GRAY]) {
        const int g = round_clip(((float)px[0] * 0.299f + (float)px[1] * 0.587f) + (float)px[2] * 0.114f);
        px[0] = g; px[1] = g; px[2] = g;
    }
    if (r[R_PERM]) {
        const int q[3] = {px[0], px[1], px[2]};
        const int i0 = r[R_PIDX], i1 = r[R_PIDX + 1], i2 = r[R_PIDX + 2];
        px[0] = i0 == 0 ? q[0] : (i0 == 1 ? q[1] : q[2]);
        px[1] = i1 == 0 ? q[0] : (i1 == 1 ? q[1] : q[2]);
        px[2] = i2 == 0 ? q[0] : (i2 == 1 ? q[1] : q[2]);
    }
    out[o] = (uint8_t)px[0]; out[o + 1] = (uint8_t)px[1]; out[o + 2] = (uint8_t)px[2];
}

// ---------------------------------------------------------------------------------------------------------------- the warps
struct Tap {                     // a clamped bilinear footprint along one axis
    int i0, i1;
    float f;
};
__device__ __forceinline__ Tap tap(float c, int size) {
    const float hi = (float)(size - 1);
    const float cc = !(c >= 0.f) ? 0.f : (c > hi ? hi : c);          // NaN -> 0
    const float fl = floorf(cc);
    Tap t;
    t.i0 = (int)fl;
    t.i1 = min(t.i0 + 1, size - 1);
    t.f = cc - fl;
    return t;
}
__device__ __forceinline__ float lerp2(float a00, float a01, float a10, float a11, float fx, float fy) {
    const float top = a00 + (a01 - a00) * fx, bot = a10 + (a11 - a10) * fx;
    return top + (bot - top) * fy;
}
// bilinear read of a 4 x 4 float table of the record at (cy, cx)
__device__ __forceinline__ float grid_read(const int32_t* __restrict__ r, int base, float cy, float cx) {
    const Tap ty = tap(cy, 4), tx = tap(cx, 4);
    return lerp2(recf(r, base + 4 * ty.i0 + tx.i0), recf(r, base + 4 * ty.i0 + tx.i1), recf(r, base + 4 * ty.i1 + tx.i0),
                 recf(r, base + 4 * ty.i1 + tx.i1), tx.f, ty.f);
}

// pass 2: T_mid + hflip + affine warp, uint8 -> uint8
__global__ __launch_bounds__(256) void aug_affine(const uint8_t* __restrict__ in, long long n_images, const int32_t* __restrict__ recs,
                                                  const uint8_t* __restrict__ luts, int n_fields, int S, uint8_t* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const long long n = blockIdx.y;
    const int32_t* __restrict__ r = recs + n * REC_WORDS;
    const long long o = (n * S * S + pix) * 3;
    if (!rec_ok(r, n_images, n_fields)) {
        out[o] = 0; out[o + 1] = 0; out[o + 2] = 0;
        return;
    }
    const int y = pix / S, x = pix - y * S;
    const uint8_t* __restrict__ img = in + n * S * S * 3;
    const uint8_t* __restrict__ t_mid = luts + 256;
    const bool mid = r[R_MID] != 0, hf = r[R_HFLIP] != 0;
    auto load = [&](int yy, int xx, int c) -> int {
        const int v = img[((long long)yy * S + (hf ? S - 1 - xx : xx)) * 3 + c];
        return mid ? t_mid[v] : v;
    };
    if (!r[R_AFFINE]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[o + c] = (uint8_t)load(y, x, c);
        return;
    }
    const float fx = (float)x, fy = (float)y;
    const float ys = (recf(r, R_AMAT + 3) * fx + recf(r, R_AMAT + 4) * fy) + recf(r, R_AMAT + 5);
    const float xs = (recf(r, R_AMAT + 0) * fx + recf(r, R_AMAT + 1) * fy) + recf(r, R_AMAT + 2);
    const Tap ty = tap(ys, S), tx = tap(xs, S);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[o + c] = (uint8_t)round_clip(lerp2((float)load(ty.i0, tx.i0, c), (float)load(ty.i0, tx.i1, c), (float)load(ty.i1, tx.i0, c),
                                               (float)load(ty.i1, tx.i1, c), tx.f, ty.f));
}

// pass 3: grid or elastic warp, uint8 -> float32 views.  Image n of the batch is role n / B (0 view0, 1 view1, 2 target), item n % B.
__global__ __launch_bounds__(256) void aug_warp_out(const uint8_t* __restrict__ in, long long n_images, const int32_t* __restrict__ recs,
                                                    const float* __restrict__ field, int n_fields, int B, int S, float* __restrict__ view0,
                                                    float* __restrict__ view1, float* __restrict__ target) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const long long n = blockIdx.y;
    const int role = (int)(n / B);
    const long long b = n - (long long)role * B;
    float* __restrict__ dst = (role == 0 ? view0 : (role == 1 ? view1 : target)) + (b * S * S + pix) * 3;
    const int32_t* __restrict__ r = recs + n * REC_WORDS;
    if (!rec_ok(r, n_images, n_fields)) {
        const float nan = __uint_as_float(0x7fc00000u);
        dst[0] = nan; dst[1] = nan; dst[2] = nan;
        return;
    }
    const int y = pix / S, x = pix - y * S;
    const uint8_t* __restrict__ img = in + n * S * S * 3;
    const int warp = r[R_WARP];
    int px[3];
    if (warp == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = img[(long long)pix * 3 + c];
    } else {
        const float fx = (float)x, fy = (float)y;
        float ys, xs;
        if (warp == WARP_GRID) {
            const float den = (float)max(S - 1, 1);
            const float cy = (fy * 3.0f) / den, cx = (fx * 3.0f) / den;
            ys = fy + grid_read(r, R_JY, cy, cx);
            xs = fx + grid_read(r, R_JX, cy, cx);
        } else {
            const float* __restrict__ fld = field + (long long)r[R_FIELD] * 2 * S * S;        // [2][S][S]: dx, dy
            ys = ((recf(r, R_EMAT + 3) * fx + recf(r, R_EMAT + 4) * fy) + recf(r, R_EMAT + 5)) + fld[(long long)S * S + pix];
            xs = ((recf(r, R_EMAT + 0) * fx + recf(r, R_EMAT + 1) * fy) + recf(r, R_EMAT + 2)) + fld[pix];
        }
        const Tap ty = tap(ys, S), tx = tap(xs, S);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a00 = (float)img[((long long)ty.i0 * S + tx.i0) * 3 + c], a01 = (float)img[((long long)ty.i0 * S + tx.i1) * 3 + c];
            const float a10 = (float)img[((long long)ty.i1 * S + tx.i0) * 3 + c], a11 = (float)img[((long long)ty.i1 * S + tx.i1) * 3 + c];
            px[c] = round_clip(lerp2(a00, a01, a10, a11, tx.f, ty.f));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (float)px[c] * 2.0f / 255.0f - 1.0f;
}

// ---------------------------------------------------------------------------------------------------------------- the field
// one axis of the separable Gaussian over planes [n_planes][S][S]: out[p][y][x] = sum_k w[k] * in[p][reflect(y + k - 200)][x] (AXIS 0)
template <int AXIS>
__global__ __launch_bounds__(256) void aug_gauss(const float* __restrict__ in, const float* __restrict__ w, int S, float* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const long long plane = (long long)blockIdx.y * S * S;
    const int y = pix / S, x = pix - y * S;
    const int pos = AXIS == 0 ? y : x, period = 2 * S;
    int m = (pos - RADIUS) % period;                     // scipy `reflect`: d c b a | a b c d | d c b a, period 2 S
    m = m < 0 ? m + period : m;
    float acc = 0.f;
    for (int k = 0; k < TAPS; ++k) {
        const int i = m < S ? m : period - 1 - m;
        acc = acc + w[k] * in[plane + (AXIS == 0 ? (long long)i * S + x : (long long)y * S + i)];
        m = m + 1 == period ? 0 : m + 1;
    }
    out[plane + pix] = acc;
}

}  // namespace

extern "C" int32_t ups_augment_record_words(void) { return REC_WORDS; }

extern "C" int ups_augment_field(const float* noise, const float* weights, int32_t n_fields, int32_t S, float* tmp, float* field, void* stream) {
    UPS_CHECK_ARG(noise && weights && tmp && field);
    UPS_CHECK_ARG(n_fields > 0 && S > 0);
    UPS_CHECK_ARG((long long)S * S <= 0x3fffffffLL && 2LL * n_fields <= 65535);
    const dim3 grid((unsigned)(((long long)S * S + 255) / 256), (unsigned)(2 * n_fields));
    hipLaunchKernelGGL(aug_gauss<0>, grid, dim3(256), 0, (hipStream_t)stream, noise, weights, S, tmp);
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(aug_gauss<1>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)tmp, weights, S, field);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_augment_views(const uint8_t* images, int64_t n_images, const int32_t* records, const uint8_t* luts, const float* field,
                                 int32_t n_fields, int32_t B, int32_t S, uint8_t* scratch_a, uint8_t* scratch_b, float* view0, float* view1,
                                 float* target, int32_t passes, void* stream) {
    UPS_CHECK_ARG(images && records && luts && scratch_a && scratch_b && view0 && view1);
    UPS_CHECK_ARG(B > 0 && S > 0 && n_images > 0 && n_fields >= 0);
    UPS_CHECK_ARG(n_fields == 0 || field);
    UPS_CHECK_ARG(passes > 0 && passes <= 7);
    UPS_CHECK_ARG((long long)S * S <= 0x3fffffffLL && 3LL * B <= 65535);
    UPS_CHECK_ARG(n_images <= 0x7fffffffLL);                                    // record entries are int32
    const int n = (target ? 3 : 2) * B;
    const dim3 grid((unsigned)(((long long)S * S + 255) / 256), (unsigned)n);
    hipStream_t s = (hipStream_t)stream;
    if (passes & 1) {
        hipLaunchKernelGGL(aug_appearance, grid, dim3(256), 0, s, images, (long long)n_images, records, luts, n_fields, S, scratch_a);
        UPS_LAUNCH_CHECK();
    }
    if (passes & 2) {
        hipLaunchKernelGGL(aug_affine, grid, dim3(256), 0, s, (const uint8_t*)scratch_a, (long long)n_images, records, luts, n_fields, S, scratch_b);
        UPS_LAUNCH_CHECK();
    }
    if (passes & 4) {
        hipLaunchKernelGGL(aug_warp_out, grid, dim3(256), 0, s, (const uint8_t*)scratch_b, (long long)n_images, records, field, n_fields, B, S,
                           view0, view1, target);
        UPS_LAUNCH_CHECK();
    }
    return UPS_OK;
}
