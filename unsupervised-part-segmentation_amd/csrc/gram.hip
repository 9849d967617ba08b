// Gram-matrix (style) terms of the perceptual loss (edflow VGG19Features(default_gram=gram_weight), UNVERIFIED):
//     term = w * mean_{b,i,j} |G(F_t)[b,i,j] - G(F_g)[b,i,j]|,   G(F)[b] = F[b]^T F[b] / (4 h w),   F = act(feature) as [n, h*w, c]
// The kernels work on the UNNORMALISED D_b = F_g[b]^T F_g[b] - F_t[b]^T F_t[b]; the caller owns the 1 / (4 h w) and the mean.
//
// Forward (ups_gram_l1_fwd): ONE fp32 accumulator per 32x32 tile of D, the GEMM of [F_g; F_t]^T with [F_g; -F_t] along K = 2 h w
// (G itself never exists).  Only tiles on or above the diagonal are computed (pair p -> (ti <= tj)); their sign matrix is mirrored
// and off-diagonal tiles count twice, so S is exactly symmetric and the MFMA work is halved.  Inside a diagonal tile only i <= j is
// read.  Split K: block (s, p, b) sums the k-steps of split s into an fp32 partial tile; with more than one split a second kernel
// adds the partials in split order (no atomics: the loss and S are bit-reproducible).  The epilogue writes S = sign(D) as int8 into
// [n][cp][cp] (cp = c rounded up to 32; pad entries 0) and one sum of |D| per (b, p) that ups_sum_scale reduces.
// Fragments: v_mfma_f32_32x32x16_bf16 (bf16) or the exact-fp32 v_mfma_f32_32x32x2_f32 (fp32 parity mode); both have the same C/D
// map (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  A[i][k] = F[k][c0 + i] is a column of the NHWC map: each
// lane gathers its k values one row apart (32 lanes read 64 contiguous bytes of a row); F_t enters with its sign flipped (exact).
//
// Backward (ups_gram_l1_bwd): gb[b] += coef * act'(y) * (F_g[b] S_b), coef = scale * scale_dev[0]: the [h w, c] x [c, c] GEMM with S as
// an exact +-1 / 0 operand.  A[m][k] = F[m][k] is row-major (16-byte loads), B[k][j] = S[k][j] = S[j][k] (S symmetric: 8 contiguous
// bytes).  It ACCUMULATES into gb (the L1 term's gradient, written just before); channels [c, ld) are not touched.
#include "common.h"

namespace {

constexpr int GT = 32;                  // tile edge (both MFMA shapes are 32 x 32)
constexpr int GRAM_TARGET_BLOCKS = 2048;
constexpr int GRAM_MIN_STEPS = 16;      // k-steps per split at the least (4 per wave)
constexpr int GRAM_MAX_SPLITS = 64;

template <typename T> struct GramK;
template <> struct GramK<float> { static constexpr int KS = 2; };     // rows of K per v_mfma_f32_32x32x2_f32
template <> struct GramK<bf16> { static constexpr int KS = 16; };     // rows of K per v_mfma_f32_32x32x16_bf16

struct GramPlan { int tiles, pairs, splits, spb, cp; long long steps; };

GramPlan gram_plan(int n, long long hw, int c, int dtype) {
    GramPlan p;
    p.tiles = ups_cdiv(c, GT);
    p.cp = p.tiles * GT;
    p.pairs = p.tiles * (p.tiles + 1) / 2;
    const int ks = dtype == UPS_F32 ? GramK<float>::KS : GramK<bf16>::KS;
    p.steps = (hw + ks - 1) / ks;
    long long want = ((long long)GRAM_TARGET_BLOCKS + (long long)n * p.pairs - 1) / ((long long)n * p.pairs);
    long long most = (p.steps + GRAM_MIN_STEPS - 1) / GRAM_MIN_STEPS;
    long long s = want < most ? want : most;
    if (s > GRAM_MAX_SPLITS) s = GRAM_MAX_SPLITS;
    if (s < 1) s = 1;
    p.spb = (int)((p.steps + s - 1) / s);
    p.splits = (int)((p.steps + p.spb - 1) / p.spb);
    return p;
}

__device__ inline void pair_tiles(int p, int tiles, int& ti, int& tj) {
    ti = 0;
    while (p >= tiles - ti) { p -= tiles - ti; ++ti; }
    tj = ti + p;
}

// act on a bf16 bit pattern (relu / leaky-relu with slope 0, as the L1 term applies them): exact
__device__ inline unsigned short gram_bits(unsigned short u, int act) { return act != UPS_ACT_NONE && (u & 0x8000u) ? 0 : u; }
__device__ inline float gram_act(float x, int act) { return act != UPS_ACT_NONE ? (x > 0.f ? x : 0.f) : x; }

// one operand fragment of D's tile at channel c0, rows [k, k + KS) of image map F (rows >= hw and channels >= c read as zero);
// neg() flips the sign of every element (exact)
template <typename T> struct GramFrag;
template <> struct GramFrag<bf16> {
    typedef bf16x8 V;
    __device__ static inline V ld(const bf16* F, long long hw, int c, int ld, int c0, long long k, int lane, int act) {
        const int ch = c0 + (lane & 31);
        const long long r0 = k + 8 * (lane >> 5);
        union { V v; unsigned short s[8]; } u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned short x = 0;
            if (ch < c && r0 + j < hw) x = gram_bits(((const unsigned short*)F)[(r0 + j) * ld + ch], act);
            u.s[j] = x;
        }
        return u.v;
    }
    __device__ static inline V neg(V v) {
        union { V v; unsigned short s[8]; } u;
        u.v = v;
#pragma unroll
        for (int j = 0; j < 8; ++j) u.s[j] ^= 0x8000u;
        return u.v;
    }
    __device__ static inline f32x16 mfma(V a, V b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); }
};
template <> struct GramFrag<float> {
    typedef float V;
    __device__ static inline V ld(const float* F, long long hw, int c, int ld, int c0, long long k, int lane, int act) {
        const int ch = c0 + (lane & 31);
        const long long r = k + (lane >> 5);
        return (ch < c && r < hw) ? gram_act(F[r * ld + ch], act) : 0.f;
    }
    __device__ static inline V neg(V v) { return -v; }
    __device__ static inline f32x16 mfma(V a, V b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }
};

// the (b, p) tile's epilogue for element e = 32 i + j of the tile: S (mirrored) and the weighted |D| (0 below a diagonal tile's diagonal)
__device__ inline float gram_epilogue(float v, int e, int ti, int tj, int cp, signed char* __restrict__ S) {
    const int i = e >> 5, j = e & 31;
    if (ti == tj && i > j) return 0.f;
    const int ci = ti * GT + i, cj = tj * GT + j;
    const signed char sg = v > 0.f ? 1 : (v < 0.f ? -1 : 0);
    S[(long long)ci * cp + cj] = sg;
    S[(long long)cj * cp + ci] = sg;
    return (ci == cj ? 1.f : 2.f) * fabsf(v);
}

// grid (splits, pairs, n), 256 threads: 4 waves take k-steps w, w + 4, ... of the split; their tiles are added in wave order
template <typename T>
__global__ __launch_bounds__(256) void gram_fwd_kernel(const T* __restrict__ ft, const T* __restrict__ fg, long long hw, int c, int ld,
                                                        int act, int tiles, int spb, long long steps, int cp,
                                                        float* __restrict__ partial, signed char* __restrict__ sign,
                                                        float* __restrict__ ws) {
    typedef GramFrag<T> FR;
    constexpr int KS = GramK<T>::KS;
    __shared__ float red[4][GT * GT];
    __shared__ float red4[4];
    const int s = blockIdx.x, p = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int ti, tj;
    pair_tiles(p, tiles, ti, tj);
    const T* Fg = fg + (long long)b * hw * ld;
    const T* Ft = ft + (long long)b * hw * ld;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const long long st_end = (long long)(s + 1) * spb < steps ? (long long)(s + 1) * spb : steps;
    for (long long st = (long long)s * spb + w; st < st_end; st += 4) {
        const long long k = st * KS;
        const typename FR::V ag = FR::ld(Fg, hw, c, ld, ti * GT, k, lane, act), at = FR::ld(Ft, hw, c, ld, ti * GT, k, lane, act);
        // same channels: the B fragments of a diagonal tile are its A fragments (before F_t's sign flip)
        const typename FR::V bg = ti == tj ? ag : FR::ld(Fg, hw, c, ld, tj * GT, k, lane, act);
        const typename FR::V bt = ti == tj ? at : FR::ld(Ft, hw, c, ld, tj * GT, k, lane, act);
        acc = FR::mfma(ag, bg, acc);
        acc = FR::mfma(FR::neg(at), bt, acc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[w][((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * GT + (lane & 31)] = acc[r];
    __syncthreads();
    const long long tile = (long long)b * gridDim.y + p;
    signed char* S = sign + (long long)b * cp * cp;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = threadIdx.x + 256 * q;
        const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        if (gridDim.x == 1) sum += gram_epilogue(v, e, ti, tj, cp, S);
        else ws[(tile * gridDim.x + s) * (GT * GT) + e] = v;
    }
    if (gridDim.x == 1) {
        sum = block_sum_256(sum, red4);
        if (threadIdx.x == 0) partial[tile] = sum;
    }
}

// split-K finish: grid (pairs, n); the partial tiles of one (b, p) are added in split order
__global__ __launch_bounds__(256) void gram_fwd_reduce_kernel(const float* __restrict__ ws, int splits, int tiles, int cp,
                                                               float* __restrict__ partial, signed char* __restrict__ sign) {
    __shared__ float red4[4];
    const int p = blockIdx.x, b = blockIdx.y;
    int ti, tj;
    pair_tiles(p, tiles, ti, tj);
    const long long tile = (long long)b * gridDim.x + p;
    const float* src = ws + tile * splits * (GT * GT);
    signed char* S = sign + (long long)b * cp * cp;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = threadIdx.x + 256 * q;
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += src[s * (GT * GT) + e];
        sum += gram_epilogue(v, e, ti, tj, cp, S);
    }
    sum = block_sum_256(sum, red4);
    if (threadIdx.x == 0) partial[tile] = sum;
}

// ---- backward operands: A = F rows (act applied), B[k][j] = S[j][k] as an exact +-1 / 0 value
template <typename T> struct GramBwd;
template <> struct GramBwd<bf16> {
    typedef bf16x8 V;
    static constexpr int KS = 16;
    __device__ static inline V lda(const bf16* F, long long hw, int c, int ld, long long m0, int k0, int lane, int act) {
        const long long m = m0 + (lane & 31);
        const int k = k0 + 8 * (lane >> 5);
        union { V v; uint4 q; unsigned short s[8]; } u;
        u.q = make_uint4(0, 0, 0, 0);
        if (m < hw && k < c) {          // k and ld are multiples of 8: the chunk lies inside the row
            u.q = *(const uint4*)(F + m * ld + k);
#pragma unroll
            for (int j = 0; j < 8; ++j) u.s[j] = k + j < c ? gram_bits(u.s[j], act) : (unsigned short)0;
        }
        return u.v;
    }
    __device__ static inline V ldb(const signed char* S, int cp, int n0, int k0, int lane) {
        const uint2 q = *(const uint2*)(S + (long long)(n0 + (lane & 31)) * cp + k0 + 8 * (lane >> 5));
        const signed char* sb = (const signed char*)&q;
        union { V v; unsigned short s[8]; } u;
#pragma unroll
        for (int j = 0; j < 8; ++j) u.s[j] = sb[j] > 0 ? 0x3F80u : (sb[j] < 0 ? 0xBF80u : 0u);
        return u.v;
    }
    __device__ static inline f32x16 mfma(V a, V b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); }
};
template <> struct GramBwd<float> {
    typedef float V;
    static constexpr int KS = 2;
    __device__ static inline V lda(const float* F, long long hw, int c, int ld, long long m0, int k0, int lane, int act) {
        const long long m = m0 + (lane & 31);
        const int k = k0 + (lane >> 5);
        return (m < hw && k < c) ? gram_act(F[m * ld + k], act) : 0.f;
    }
    __device__ static inline V ldb(const signed char* S, int cp, int n0, int k0, int lane) {
        return (float)S[(long long)(n0 + (lane & 31)) * cp + k0 + (lane >> 5)];
    }
    __device__ static inline f32x16 mfma(V a, V b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }
};

// grid (ceil(hw / 128), cp / 32, n), 256 threads: wave w owns rows [128 x + 32 w, +32) x channels [32 y, +32) of image z
template <typename T>
__global__ __launch_bounds__(256) void gram_bwd_kernel(const T* __restrict__ fg, const signed char* __restrict__ sign, T* __restrict__ gb,
                                                        long long hw, int c, int ld, int act, int cp,
                                                        const float* __restrict__ scale_dev, float scale) {
    typedef GramBwd<T> BW;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.z, n0 = blockIdx.y * GT;
    const long long m0 = (long long)blockIdx.x * 128 + 32 * w;
    if (m0 >= hw) return;
    const T* F = fg + (long long)b * hw * ld;
    const signed char* S = sign + (long long)b * cp * cp;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < c; k0 += BW::KS)
        acc = BW::mfma(BW::lda(F, hw, c, ld, m0, k0, lane, act), BW::ldb(S, cp, n0, k0, lane), acc);
    const float coef = scale * (scale_dev ? scale_dev[0] : 1.f);
    const int ch = n0 + (lane & 31);
    if (ch >= c) return;
    T* G = gb + (long long)b * hw * ld;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long m = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < hw) {
            const long long o = m * ld + ch;
            const float y = ld_as_float<T>(F + o);
            st_from_float<T>(G + o, ld_as_float<T>(G + o) + coef * ups_dact(y, act, 0.f) * acc[r]);
        }
    }
}

}  // namespace

extern "C" int ups_gram_plan(int32_t n, int64_t hw, int32_t c, int32_t dtype, int64_t* out) {
    UPS_CHECK_ARG(out && n >= 1 && hw >= 1 && c >= 1 && (dtype == UPS_F32 || dtype == UPS_BF16));
    const GramPlan p = gram_plan(n, hw, c, dtype);
    out[0] = p.splits;
    out[1] = (int64_t)n * p.pairs;
    out[2] = p.splits > 1 ? (int64_t)n * p.pairs * p.splits * GT * GT : 0;
    out[3] = (int64_t)n * p.cp * p.cp;
    return UPS_OK;
}

extern "C" int ups_gram_l1_fwd(const void* a, const void* b, int32_t dtype, int32_t n, int64_t hw, int32_t c, int32_t ld, int32_t act,
                               float* partial, void* sign, float* workspace, void* stream) {
    UPS_CHECK_ARG(a && b && partial && sign && n >= 1 && hw >= 1 && c >= 1 && ld % 8 == 0 && c <= ld);
    UPS_CHECK_ARG(act == UPS_ACT_NONE || act == UPS_ACT_RELU || act == UPS_ACT_LRELU);
    UPS_CHECK_ARG(dtype == UPS_F32 || dtype == UPS_BF16);
    const GramPlan p = gram_plan(n, hw, c, dtype);
    UPS_CHECK_ARG(p.splits == 1 || workspace);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(p.splits, p.pairs, n);
    signed char* S = (signed char*)sign;
    if (dtype == UPS_F32)
        hipLaunchKernelGGL(gram_fwd_kernel<float>, grid, dim3(256), 0, s, (const float*)a, (const float*)b, (long long)hw, c, ld, act,
                           p.tiles, p.spb, p.steps, p.cp, partial, S, workspace);
    else
        hipLaunchKernelGGL(gram_fwd_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)a, (const bf16*)b, (long long)hw, c, ld, act,
                           p.tiles, p.spb, p.steps, p.cp, partial, S, workspace);
    UPS_LAUNCH_CHECK();
    if (p.splits > 1) {
        hipLaunchKernelGGL(gram_fwd_reduce_kernel, dim3(p.pairs, n), dim3(256), 0, s, (const float*)workspace, p.splits, p.tiles, p.cp,
                           partial, S);
        UPS_LAUNCH_CHECK();
    }
    return UPS_OK;
}

extern "C" int ups_gram_l1_bwd(const void* b, const void* sign, void* gb, int32_t dtype, int32_t n, int64_t hw, int32_t c, int32_t ld,
                               int32_t act, const float* scale_dev, float scale, void* stream) {
    UPS_CHECK_ARG(b && sign && gb && n >= 1 && hw >= 1 && c >= 1 && ld % 8 == 0 && c <= ld);
    UPS_CHECK_ARG(act == UPS_ACT_NONE || act == UPS_ACT_RELU || act == UPS_ACT_LRELU);
    UPS_CHECK_ARG(dtype == UPS_F32 || dtype == UPS_BF16);
    const int cp = ups_cdiv(c, GT) * GT;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ups_cdiv(hw, 128), cp / GT, n);
    if (dtype == UPS_F32)
        hipLaunchKernelGGL(gram_bwd_kernel<float>, grid, dim3(256), 0, s, (const float*)b, (const signed char*)sign, (float*)gb,
                           (long long)hw, c, ld, act, cp, scale_dev, scale);
    else
        hipLaunchKernelGGL(gram_bwd_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)b, (const signed char*)sign, (bf16*)gb,
                           (long long)hw, c, ld, act, cp, scale_dev, scale);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
