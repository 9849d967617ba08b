// Weight-normalised transposed convolution of `upsample(x, nf, "conv_transposed")` (N:818-822, deconv2d N:938-1039):
//     y[n, 2i+ky, 2j+kx, o] += sum_c x[n, i, j, c] * W[ky, kx, o, c],   W = g * V / max(||V_o||, 1e-6)  (l2_normalize over kh, kw, in)
// with TF 'SAME' geometry for stride 2 on an even size (pad 0 before, 1 after: taps landing on row / column 2H are dropped), plus b
// and, in CoordConv scopes, the two coordinate channels of x (add_coordinates at the input's resolution) as an affine epilogue.
//
// The four output parity classes hold 4 + 2 + 2 + 1 = 9 non-zero tap products per input pixel:
//     (even, even): W[0,0] x[i,j] + W[0,2] x[i,j-1] + W[2,0] x[i-1,j] + W[2,2] x[i-1,j-1]
//     (even, odd):  W[0,1] x[i,j] + W[2,1] x[i-1,j]          (odd, even): W[1,0] x[i,j] + W[1,2] x[i,j-1]          (odd, odd): W[1,1] x[i,j]
// deconv_fwd_kernel computes all four for a tile of input pixels in one launch: the input row pair (i-1, i) of the tile and its
// one-pixel left halo are staged in LDS once, the 9 tap GEMMs run on v_mfma_f32_16x16x32_{bf16,f16} (fp32 accumulation), and the
// 2 x 2 output pixels of every input pixel go back through LDS so that the block stores two whole output row segments with
// 16-byte writes.  The depth-to-space input-gradient form of the stride-2 convolution (one stride-1 3x3 over 4 C channels,
// ops.conv_dgrad) was not used for this forward: it runs 36 tap slots per input pixel of which only these 9 are non-zero.
//
// The rest of the layer reuses the convolution engine (the deconvolution is the input gradient of a stride-2 3x3 convolution with
// forward weights W): dx is a stride-2 forward convolution of dy with W, dW[.., :C] a stride-2 weight gradient with the roles of the
// two tensors swapped.  The small kernels here make W (ups_deconv_prep), reduce db and the coordinate rows of dW
// (ups_deconv_bias_coord_grad) and take dW back through the normalisation (ups_deconv_wn_bwd).
#include "common.h"

namespace {

constexpr float WN_EPS = 1e-12f;       // tf.nn.l2_normalize epsilon: x * rsqrt(max(sum x^2, eps))

// ---- block-wide sum of a float (256 threads)
__device__ __forceinline__ float block_sum256(float v, float* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// per output filter o: inv_norm[o] and the fp32 W[t][o][c] = g[o] * V[t][o][c] * inv_norm[o]   (V [9][nf][cin_v], TF [kh,kw,out,in])
__global__ __launch_bounds__(256) void deconv_norm_kernel(const float* __restrict__ V, const float* __restrict__ g, int nf, int cin_v,
                                                          float* __restrict__ w32, float* __restrict__ inv_norm) {
    __shared__ float red[4];
    const int o = blockIdx.x;
    float ss = 0.f;
    for (int e = threadIdx.x; e < 9 * cin_v; e += 256) {
        const int t = e / cin_v, c = e - t * cin_v;
        const float v = V[((long long)t * nf + o) * cin_v + c];
        ss = __fmaf_rn(v, v, ss);
    }
    ss = block_sum256(ss, red);
    const float inv = rsqrtf(fmaxf(ss, WN_EPS));
    const float s = g[o] * inv;
    for (int e = threadIdx.x; e < 9 * cin_v; e += 256) {
        const int t = e / cin_v, c = e - t * cin_v;
        const long long i = ((long long)t * nf + o) * cin_v + c;
        w32[i] = V[i] * s;
    }
    if (threadIdx.x == 0) inv_norm[o] = inv;
}

template <typename T> __device__ __forceinline__ T cvt_w(float v) { return (T)v; }

// forward operand, blocked-K as ups_weight_prep's w_fwd: wf[t][kc][o][BK] = W[t][o][kc*BK + j] (c < ci_log, else 0)
template <typename T>
__global__ void deconv_wfwd_kernel(const float* __restrict__ w32, int nf, int cin_v, int ci_log, int kc_n, T* __restrict__ wf) {
    constexpr int BK = 64 / (int)sizeof(T);
    const long long total = 9ll * kc_n * nf * BK;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e % BK);
        long long r = e / BK;
        const int o = (int)(r % nf); r /= nf;
        const int kc = (int)(r % kc_n);
        const int t = (int)(r / kc_n);
        const int c = kc * BK + j;
        wf[e] = cvt_w<T>(c < ci_log ? w32[((long long)t * nf + o) * cin_v + c] : 0.f);
    }
}

// input-gradient operand (a stride-2 forward convolution of dy with W: reduction over o, output channels c):
// wd[t][ko][c][BK] = W[t][ko*BK + j][c] (o < nf, else 0)
template <typename T>
__global__ void deconv_wdx_kernel(const float* __restrict__ w32, int nf, int cin_v, int ci_log, int ko_n, T* __restrict__ wd) {
    constexpr int BK = 64 / (int)sizeof(T);
    const long long total = 9ll * ko_n * ci_log * BK;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e % BK);
        long long r = e / BK;
        const int c = (int)(r % ci_log); r /= ci_log;
        const int ko = (int)(r % ko_n);
        const int t = (int)(r / ko_n);
        const int o = ko * BK + j;
        wd[e] = cvt_w<T>(o < nf ? w32[((long long)t * nf + o) * cin_v + c] : 0.f);
    }
}

// The parity classes' taps, r-major: rows of class py (ky, source row offset), columns likewise.
__device__ __forceinline__ int cls_n(int p) { return p ? 1 : 2; }
__device__ __forceinline__ int cls_k(int p, int a) { return p ? 1 : (a ? 2 : 0); }
__device__ __forceinline__ int cls_d(int p, int a) { return (p == 0 && a == 1) ? -1 : 0; }

// CoordConv table of class cls = 2 py + px in the layout of ups_conv_desc.coord_tab: [64 masks][3][nf], mask = ym * 8 + xm with bit a
// of ym set when the class's row tap a reads inside the image (likewise xm): value k0 + j kj + i ki at lattice point (i, j).
// Channel ci_log of x's coordinates is -1 + ax * column, channel ci_log + 1 is -1 + ay * row (add_coordinates, N:2123-2154).
__global__ void deconv_ctab_kernel(const float* __restrict__ w32, int nf, int cin_v, int ci_log, float ax, float ay,
                                   float* __restrict__ ctab) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y, cls = blockIdx.z;
    if (o >= nf) return;
    const int py = cls >> 1, px = cls & 1, ym = m >> 3, xm = m & 7;
    float k0 = 0.f, kj = 0.f, ki = 0.f;
    for (int a = 0; a < cls_n(py); ++a) {
        if (!((ym >> a) & 1)) continue;
        for (int b = 0; b < cls_n(px); ++b) {
            if (!((xm >> b) & 1)) continue;
            const int t = cls_k(py, a) * 3 + cls_k(px, b);
            const float vx = w32[((long long)t * nf + o) * cin_v + ci_log];
            const float vy = w32[((long long)t * nf + o) * cin_v + ci_log + 1];
            k0 = __fmaf_rn(__fmaf_rn(ax, (float)cls_d(px, b), -1.f), vx, k0);
            k0 = __fmaf_rn(__fmaf_rn(ay, (float)cls_d(py, a), -1.f), vy, k0);
            kj = __fmaf_rn(ax, vx, kj);
            ki = __fmaf_rn(ay, vy, ki);
        }
    }
    float* tb = ctab + ((long long)cls * 64 + m) * 3 * nf + o;
    tb[0] = k0; tb[nf] = kj; tb[2 * nf] = ki;
}

// ------------------------------------------------------------------------------------------------ one-launch forward
typedef __attribute__((ext_vector_type(8))) short s16x8;

template <typename T> __device__ __forceinline__ f32x4 mfma16(const s16x8& a, const s16x8& b, const f32x4& c);
template <> __device__ __forceinline__ f32x4 mfma16<bf16>(const s16x8& a, const s16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mfma16<f16>(const s16x8& a, const s16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

struct DeconvK {
    const void* x; const void* wf; const float* bias; const float* ctab; void* y;
    int n, h, w, ci, ldi, kc_n, nf, ldo, sub;     // sub: 16-pixel sub-tiles per block (tile = 16 sub input pixels of one row)
    int xp, yp;                                   // LDS pitches (elements) of a staged input pixel / output pixel
};

// grid (w / (16 sub), h, n), 256 threads.  LDS: xs[2][16 sub + 1][xp] (rows i-1, i; column 0 = j0 - 1), ys[2][32 sub][yp].
template <typename T>
__global__ __launch_bounds__(256) void deconv_fwd_kernel(const DeconvK p) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tw = 16 * p.sub, cols = tw + 1;
    T* xs = (T*)smem;
    T* ys = xs + 2 * cols * p.xp;
    const int j0 = blockIdx.x * tw, i = blockIdx.y, img = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const T* __restrict__ x = (const T*)p.x;

    // ---- stage rows i-1 and i, columns j0-1 .. j0+tw-1, channels [0, 32 kc_n) (zero outside the image / past ci)
    const int kch = p.kc_n * 4;              // 16-byte chunks per staged pixel
    for (int e = tid; e < 2 * cols * kch; e += 256) {
        const int ch = e % kch, q = e / kch;
        const int col = q % cols, row = q / cols;
        const int gi = i - 1 + row, gj = j0 - 1 + col;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (gi >= 0 && gj >= 0 && ch * 8 < p.ci)
            v = *(const uint4*)(x + (((long long)img * p.h + gi) * p.w + gj) * p.ldi + ch * 8);
        *(uint4*)(xs + (row * cols + col) * p.xp + ch * 8) = v;
    }
    __syncthreads();

    // ---- work items (sub-tile, 16-channel tile of the output) over the four waves
    const int nt_n = (p.nf + 15) >> 4;
    const int r16 = lane & 15, kq = (lane >> 4) * 8;
    const T* __restrict__ wf = (const T*)p.wf;
    for (int item = wv; item < p.sub * nt_n; item += 4) {
        const int st = item % p.sub, nt = item / p.sub;
        const int o = nt * 16 + r16;
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int pc = 1 + st * 16 + r16;          // staged column of input pixel j0 + 16 st + r16
        for (int kc = 0; kc < p.kc_n; ++kc) {
            const int k = kc * 32 + kq;
            const s16x8 a_ij = *(const s16x8*)(xs + (cols + pc) * p.xp + k);        // x[i, j]
            const s16x8 a_ijm = *(const s16x8*)(xs + (cols + pc - 1) * p.xp + k);   // x[i, j-1]
            const s16x8 a_imj = *(const s16x8*)(xs + pc * p.xp + k);                // x[i-1, j]
            const s16x8 a_imjm = *(const s16x8*)(xs + (pc - 1) * p.xp + k);         // x[i-1, j-1]
            s16x8 b[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                b[t] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
                if (o < p.nf) b[t] = *(const s16x8*)(wf + (((long long)t * p.kc_n + kc) * p.nf + o) * 32 + kq);
            }
            acc[0] = mfma16<T>(a_ij, b[0], acc[0]);      // (even, even)
            acc[0] = mfma16<T>(a_ijm, b[2], acc[0]);
            acc[0] = mfma16<T>(a_imj, b[6], acc[0]);
            acc[0] = mfma16<T>(a_imjm, b[8], acc[0]);
            acc[1] = mfma16<T>(a_ij, b[1], acc[1]);      // (even, odd)
            acc[1] = mfma16<T>(a_imj, b[7], acc[1]);
            acc[2] = mfma16<T>(a_ij, b[3], acc[2]);      // (odd, even)
            acc[2] = mfma16<T>(a_ijm, b[5], acc[2]);
            acc[3] = mfma16<T>(a_ij, b[4], acc[3]);      // (odd, odd)
        }
        // ---- epilogue into LDS: bias + CoordConv terms; lane holds column o, pixels 4 (lane >> 4) + r of the sub-tile
        if (o < p.nf) {
            const float bo = p.bias ? p.bias[o] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int py = c >> 1, px = c & 1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pl = st * 16 + (lane >> 4) * 4 + r;       // input pixel of the tile
                    const int j = j0 + pl;
                    float v = acc[c][r] + bo;
                    if (p.ctab) {
                        const int ym = py ? 1 : (1 | ((i > 0) << 1));
                        const int xm = px ? 1 : (1 | ((j > 0) << 1));
                        const float* tb = p.ctab + ((long long)c * 64 + ym * 8 + xm) * 3 * p.nf + o;
                        v += tb[0] + (float)j * tb[p.nf] + (float)i * tb[2 * p.nf];
                    }
                    T tv;
                    st_from_float<T>(&tv, v);
                    ys[(py * 2 * tw + 2 * pl + px) * p.yp + o] = tv;
                }
            }
        }
    }
    __syncthreads();

    // ---- two output row segments [2i + py][2 j0, 2 j0 + 2 tw) x ldo channels, 16 bytes per store (pad channels written as zero)
    T* __restrict__ y = (T*)p.y;
    const int och = p.ldo >> 3;
    const int wo = 2 * p.w;
    for (int e = tid; e < 2 * 2 * tw * och; e += 256) {
        const int ch = e % och, q = e / och;
        const int oc = q % (2 * tw), py = q / (2 * tw);
        uint4 v = *(const uint4*)(ys + (py * 2 * tw + oc) * p.yp + ch * 8);
        if (ch * 8 + 8 > p.nf) {
            unsigned short* h = (unsigned short*)&v;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (ch * 8 + k >= p.nf) h[k] = 0;
        }
        *(uint4*)(y + (((long long)img * 2 * p.h + 2 * i + py) * wo + 2 * j0 + oc) * p.ldo + ch * 8) = v;
    }
}

// ------------------------------------------------------------------------------------------------ backward reductions
// Partial sums of dy over one row set: per channel o, s[0] = sum dy (db), s[1 + 2 t + q] = sum over the input lattice points (i, j)
// that tap t = 3 ky + kx maps to output (2i + ky, 2j + kx) < (2H, 2W) of dy * coord_q, coord_0 = -1 + ax j, coord_1 = -1 + ay i.
// grid (ceil(nf / 64), splits); block 64 x 4: lane = channel, wave = output-column phase.  part [splits][19][nf].
template <typename T>
__global__ __launch_bounds__(256) void deconv_bgrad_kernel(const T* __restrict__ dy, int n, int h, int w, int nf, int ldo, int coords,
                                                           float ax, float ay, float* __restrict__ part) {
    __shared__ float red[4][19][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = blockIdx.x * 64 + lane;
    const int ho = 2 * h, wo = 2 * w, nrows = n * ho;
    float s[19];
#pragma unroll
    for (int k = 0; k < 19; ++k) s[k] = 0.f;
    if (o < nf) {
        for (int rr = blockIdx.y; rr < nrows; rr += gridDim.y) {
            const int Y = rr % ho;
            // row taps: Y = 2 i + ky
            const int ky_a = Y & 1, i_a = Y >> 1;                 // ky 0 or 1
            const bool has_b = !(Y & 1) && Y >= 2;                // ky 2 from row i = Y / 2 - 1
            const float yy_a = -1.f + ay * (float)i_a, yy_b = -1.f + ay * (float)(i_a - 1);
            for (int X = wv; X < wo; X += 4) {
                const float v = ld_as_float<T>(dy + ((long long)rr * wo + X) * ldo + o);
                s[0] += v;
                if (!coords) continue;
                const int kx_a = X & 1, j_a = X >> 1;
                const bool hasx_b = !(X & 1) && X >= 2;
                const float xx_a = -1.f + ax * (float)j_a, xx_b = -1.f + ax * (float)(j_a - 1);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (u == 1 && !has_b) continue;
                    const int ky = u ? 2 : ky_a;
                    const float yy = u ? yy_b : yy_a;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (q == 1 && !hasx_b) continue;
                        const int kx = q ? 2 : kx_a;
                        const float xx = q ? xx_b : xx_a;
                        const int t = ky * 3 + kx;
                        // (t is not a compile-time index here: select through a small unrolled switch)
#pragma unroll
                        for (int tt = 0; tt < 9; ++tt)
                            if (tt == t) { s[1 + 2 * tt] += v * xx; s[2 + 2 * tt] += v * yy; }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 19; ++k) red[wv][k][lane] = s[k];
    __syncthreads();
    if (wv == 0 && o < nf) {
#pragma unroll
        for (int k = 0; k < 19; ++k)
            part[((long long)blockIdx.y * 19 + k) * nf + o] = ((red[0][k][lane] + red[1][k][lane]) + red[2][k][lane]) + red[3][k][lane];
    }
}

// fixed-order sum of the partials: db[o] and dwc[t][o][q] (the two coordinate columns of dW)
__global__ void deconv_bgrad_final(const float* __restrict__ part, int splits, int nf, int coords, float* __restrict__ db,
                                   float* __restrict__ dwc) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (o >= nf || (k > 0 && !coords)) return;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += part[((long long)sp * 19 + k) * nf + o];
    if (k == 0) db[o] = s;
    else dwc[((long long)((k - 1) >> 1) * nf + o) * 2 + ((k - 1) & 1)] = s;
}

// dW -> (dV, dg) through W = g V / ||V||, one block per output filter:
//     dg = <Vhat, dW>,  dV = (g / ||V||) (dW - Vhat dg)   (no projection term where the norm is clamped at the epsilon)
// dW comes in two pieces: dwx [9][nf][ci_log] (the weight-gradient kernel) and dwc [9][nf][2] (coordinate columns, or NULL)
__global__ __launch_bounds__(256) void deconv_wn_bwd_kernel(const float* __restrict__ V, const float* __restrict__ g, const float* __restrict__ dwx,
                                                            const float* __restrict__ dwc, int nf, int cin_v, int ci_log,
                                                            float* __restrict__ dV, float* __restrict__ dg) {
    __shared__ float red[4];
    const int o = blockIdx.x;
    float ss = 0.f, dot = 0.f;
    for (int e = threadIdx.x; e < 9 * cin_v; e += 256) {
        const int t = e / cin_v, c = e - t * cin_v;
        const float v = V[((long long)t * nf + o) * cin_v + c];
        const float d = c < ci_log ? dwx[((long long)t * nf + o) * ci_log + c] : dwc[((long long)t * nf + o) * 2 + (c - ci_log)];
        ss = __fmaf_rn(v, v, ss);
        dot = __fmaf_rn(v, d, dot);
    }
    ss = block_sum256(ss, red);
    dot = block_sum256(dot, red);
    const float inv = rsqrtf(fmaxf(ss, WN_EPS));
    const float dgo = dot * inv;
    const float s = g[o] * inv;
    const float proj = ss >= WN_EPS ? dgo * inv : 0.f;        // Vhat * dg = V * (inv * dg)
    for (int e = threadIdx.x; e < 9 * cin_v; e += 256) {
        const int t = e / cin_v, c = e - t * cin_v;
        const long long iv = ((long long)t * nf + o) * cin_v + c;
        const float d = c < ci_log ? dwx[((long long)t * nf + o) * ci_log + c] : dwc[((long long)t * nf + o) * 2 + (c - ci_log)];
        dV[iv] = s * (d - V[iv] * proj);
    }
    if (threadIdx.x == 0) dg[o] = dgo;
}

}  // namespace

extern "C" int ups_deconv_prep(const float* V, const float* g, int32_t nf, int32_t cin_v, int32_t ci_log, int32_t fwd_dtype, void* w_fwd,
                               int32_t dx_dtype, void* w_dx, float* w32, float* inv_norm, float* ctab, int32_t hi, int32_t wi,
                               void* stream) {
    UPS_CHECK_ARG(V && g && w32 && inv_norm && nf > 0 && ci_log > 0 && (cin_v == ci_log || cin_v == ci_log + 2));
    UPS_CHECK_ARG(!ctab || cin_v == ci_log + 2);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(deconv_norm_kernel, dim3(nf), dim3(256), 0, s, V, g, nf, cin_v, w32, inv_norm);
    if (w_fwd) {
        UPS_CHECK_ARG(fwd_dtype == UPS_F32 || fwd_dtype == UPS_BF16 || fwd_dtype == UPS_F16);
        const int bk = fwd_dtype == UPS_F32 ? 16 : 32;
        const int kc_n = ups_cdiv((ci_log + 7) / 8 * 8, bk);
        const int blocks = std::min(ups_cdiv(9ll * kc_n * nf * bk, 256), 4096);
        if (fwd_dtype == UPS_F32) hipLaunchKernelGGL(deconv_wfwd_kernel<float>, dim3(blocks), dim3(256), 0, s, w32, nf, cin_v, ci_log, kc_n, (float*)w_fwd);
        else if (fwd_dtype == UPS_BF16) hipLaunchKernelGGL(deconv_wfwd_kernel<bf16>, dim3(blocks), dim3(256), 0, s, w32, nf, cin_v, ci_log, kc_n, (bf16*)w_fwd);
        else hipLaunchKernelGGL(deconv_wfwd_kernel<f16>, dim3(blocks), dim3(256), 0, s, w32, nf, cin_v, ci_log, kc_n, (f16*)w_fwd);
    }
    if (w_dx) {
        UPS_CHECK_ARG(dx_dtype == UPS_F32 || dx_dtype == UPS_BF16);
        const int bk = dx_dtype == UPS_F32 ? 16 : 32;
        const int ko_n = ups_cdiv((nf + 7) / 8 * 8, bk);
        const int blocks = std::min(ups_cdiv(9ll * ko_n * ci_log * bk, 256), 4096);
        if (dx_dtype == UPS_F32) hipLaunchKernelGGL(deconv_wdx_kernel<float>, dim3(blocks), dim3(256), 0, s, w32, nf, cin_v, ci_log, ko_n, (float*)w_dx);
        else hipLaunchKernelGGL(deconv_wdx_kernel<bf16>, dim3(blocks), dim3(256), 0, s, w32, nf, cin_v, ci_log, ko_n, (bf16*)w_dx);
    }
    if (ctab) {
        const float ax = 2.f / (float)std::max(1, hi - 1), ay = 2.f / (float)std::max(1, wi - 1);
        hipLaunchKernelGGL(deconv_ctab_kernel, dim3(ups_cdiv(nf, 64), 64, 4), dim3(64), 0, s, w32, nf, cin_v, ci_log, ax, ay, ctab);
    }
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_deconv3x3_s2_fwd(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ci, int32_t ldi,
                                    const void* w_fwd, const float* bias, const float* ctab, int32_t nf, int32_t ldo, void* y,
                                    void* stream) {
    UPS_CHECK_ARG(x && w_fwd && y && n > 0 && h > 0 && w > 0 && nf > 0);
    UPS_CHECK_ARG(ci > 0 && ci % 8 == 0 && ci <= ldi && ldi % 8 == 0 && ldo % 8 == 0 && ldo >= nf);
    UPS_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)w_fwd & 15) == 0);
    if ((dtype != UPS_BF16 && dtype != UPS_F16) || w % 16 != 0 || ci > 256 || nf > 256) {
        ups_set_error("ups_deconv3x3_s2_fwd: 16-bit tensors, width a multiple of 16, at most 256 input / output channels");
        return UPS_E_UNSUPPORTED;
    }
    DeconvK k;
    k.x = x; k.wf = w_fwd; k.bias = bias; k.ctab = ctab; k.y = y;
    k.n = n; k.h = h; k.w = w; k.ci = ci; k.ldi = ldi; k.kc_n = ups_cdiv(ci, 32); k.nf = nf; k.ldo = ldo;
    k.xp = k.kc_n * 32 + 8;       // +16 bytes: consecutive pixels' fragment reads start on different banks
    k.yp = ldo + 8;
    auto lds = [&](int sub) { return (size_t)2 * (16 * sub + 1) * k.xp * 2 + (size_t)2 * 32 * sub * k.yp * 2; };
    k.sub = 1;
    for (int sub : {4, 2}) {
        if (w % (16 * sub) == 0 && lds(sub) <= 64 * 1024) { k.sub = sub; break; }
    }
    const size_t bytes = lds(k.sub);
    if (bytes > 64 * 1024) {
        ups_set_error("ups_deconv3x3_s2_fwd: tile does not fit in LDS");
        return UPS_E_UNSUPPORTED;
    }
    const dim3 grid(w / (16 * k.sub), h, n);
    const int rc = dtype == UPS_BF16 ? ups_launch_lds<deconv_fwd_kernel<bf16>>("deconv_fwd_kernel", 64 * 1024, grid, dim3(256), bytes, (hipStream_t)stream, k)
                                     : ups_launch_lds<deconv_fwd_kernel<f16>>("deconv_fwd_kernel", 64 * 1024, grid, dim3(256), bytes, (hipStream_t)stream, k);
    if (rc != UPS_OK) return rc;
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_deconv_bias_coord_grad(const void* dy, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t nf, int32_t ldo,
                                          int32_t coords, float* db, float* dwc, float* part, int32_t splits, void* stream) {
    UPS_CHECK_ARG(dy && db && part && n > 0 && h > 0 && w > 0 && nf > 0 && ldo >= nf && splits >= 1 && splits <= 1024);
    UPS_CHECK_ARG(!coords || dwc);
    UPS_CHECK_ARG(dtype == UPS_F32 || dtype == UPS_BF16);
    const float ax = 2.f / (float)std::max(1, h - 1), ay = 2.f / (float)std::max(1, w - 1);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ups_cdiv(nf, 64), splits);
    if (dtype == UPS_F32) hipLaunchKernelGGL(deconv_bgrad_kernel<float>, grid, dim3(256), 0, s, (const float*)dy, n, h, w, nf, ldo, coords, ax, ay, part);
    else hipLaunchKernelGGL(deconv_bgrad_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)dy, n, h, w, nf, ldo, coords, ax, ay, part);
    hipLaunchKernelGGL(deconv_bgrad_final, dim3(ups_cdiv(nf, 64), 19), dim3(64), 0, s, part, splits, nf, coords, db, dwc);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_deconv_wn_bwd(const float* V, const float* g, const float* dwx, const float* dwc, int32_t nf, int32_t cin_v,
                                 int32_t ci_log, float* dV, float* dg, void* stream) {
    UPS_CHECK_ARG(V && g && dwx && dV && dg && nf > 0 && ci_log > 0 && (cin_v == ci_log || (cin_v == ci_log + 2 && dwc)));
    hipLaunchKernelGGL(deconv_wn_bwd_kernel, dim3(nf), dim3(256), 0, (hipStream_t)stream, V, g, dwx, dwc, nf, cin_v, ci_log, dV, dg);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
