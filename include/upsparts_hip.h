/* upsparts_hip.h -- C ABI of libupsparts_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the part-discovery training hot path of
 * CompVis/unsupervised-part-segmentation.  The reference has NO FFI of its own
 * (it is TensorFlow-1.14 graph code); every entry point below replaces the stock
 * TF op(s) that the cited reference lines execute.  Citations are relative to
 * /root/reference:  M = cub/code/SB_model48i/model.py,  N = cub/code/nn.py.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *     (caller-owned, no hidden allocation) unless a parameter says "host";
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 = ok, negative = UPS_E_* (no exceptions cross the ABI);
 *   - activations are NHWC, element type UPS_F32, UPS_BF16 or (forward tensors only) UPS_F16, with a physical
 *     channel count that is a multiple of 8 (16-byte rows); accumulation is fp32;
 *   - thread-compatible: one stream per concurrent caller.
 */
#ifndef UPSPARTS_HIP_H
#define UPSPARTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ups_conv_desc grew by out_act / res_act, ups_wgrad_desc by in_f16, UPS_F16 was added (round 3) -- a stale library
 * built against the older structs ignores those fields silently, so the loader also compares ups_struct_sizes().
 * 3: ups_wgrad_desc grew by dout_f8 / dout_f8_scale / in_f8_scale / in_f8_amax (the fp8 weight gradient, round 5).
 * 5: ups_gather_views was added (device-resident training data): a binding that expects it refuses an older library by number.
 * 6: ups_part_confusion was added (part-IoU evaluation on the device). */
#define UPS_ABI_VERSION 6

/* UPS_F16 (IEEE half): element type of FORWARD tensors of precision-critical scopes (the mask decoder): ups_conv_igemm,
 * ups_weight_prep(_batch), ups_bilinear2x_fwd, ups_convert / ups_pad_convert accept it; gradients are never fp16 (range): the
 * input-gradient call of such a layer is a plain UPS_BF16 call (`dact` only has its sign read, which is the same bit in both
 * 16-bit formats), its weight-gradient call sets ups_wgrad_desc.in_f16. */
enum { UPS_F32 = 0, UPS_BF16 = 1, UPS_F16 = 2 };
/* UPS_ACT_ELU (tf.nn.elu, N:757-758; no shipped yaml uses it): accepted by the pointwise entry points only (ups_elu_fwd / _bwd,
 * ups_act_mean_*); the convolution descriptors take NONE / LRELU / RELU -- a scope with `activation: elu` materialises act(x). */
enum { UPS_ACT_NONE = 0, UPS_ACT_LRELU = 1, UPS_ACT_RELU = 2, UPS_ACT_ELU = 3 };
enum { UPS_OK = 0, UPS_E_ARG = -1, UPS_E_UNSUPPORTED = -2, UPS_E_LAUNCH = -3 };

int ups_abi_version(void);
/* sizeof of the descriptor structs AS THE LIBRARY WAS COMPILED: out[0] ups_conv_desc, [1] ups_wgrad_desc, [2] ups_prior_desc,
 * [3] ups_prep_item.  A binding compares them with its own struct sizes at load time. */
void ups_struct_sizes(int64_t out[4]);
/* human readable description of the last error on this thread (host string) */
const char* ups_last_error(void);

/* ---------------------------------------------------------------- convolution engine
 * Implicit-GEMM gather convolution on MFMA (bf16 32x32x16 / exact-f32 32x32x2).
 * One kernel serves tf.nn.conv2d forward (N:617-664, nin N:811-813, downsample
 * N:816-817) and its input gradient (dgrad), for stride 1 and 2 with TF 'SAME'
 * padding, by describing the op as
 *     out[img, i*out_sy+out_oy, j*out_sx+out_ox, c] =
 *         epi( sum_t sum_k in[img, i*in_sy+tap_dy[t], j*in_sx+tap_dx[t], k] * w[tap_w[t]][c][k] )
 * over the lattice i<ho, j<wo.  Out-of-range source pixels read as zero.
 * epi:  v = acc + bias[c] + coord_affine(c) ; v *= act'(dact[pix][c]) ; v += res[pix][c].
 */
typedef struct {
    int32_t dtype;            /* UPS_F32 / UPS_BF16: element type of in, w, res, dact and (unless out_f32) out */
    int32_t n, hi, wi;        /* input tensor [n, hi, wi, ldi] */
    int32_t ci;               /* reduction channels per tap (multiple of 8, <= ldi) */
    int32_t ldi;              /* physical input channels */
    int32_t ho, wo;           /* lattice points per image */
    int32_t co;               /* logical output channels = rows of each weight slice */
    int32_t co_fill;          /* channels [co, co_fill) of out are written as zero (>= co) */
    int32_t ldo;              /* physical channels of out */
    int32_t out_h, out_w;     /* physical output spatial size */
    int32_t out_sy, out_sx, out_oy, out_ox;
    int32_t in_sy, in_sx;
    int32_t ntaps, kh, kw;    /* taps are r-major (t = r*kw + s) when coord_tab is used */
    int32_t tap_dy[9], tap_dx[9], tap_w[9];
    int32_t act_in;           /* UPS_ACT_* applied to `in` while it is staged (fused lrelu/relu-on-load) */
    float   act_slope;        /* leaky slope (0.2: N:755-756) */
    int32_t out_f32;          /* 1: out is float regardless of dtype */
    int32_t dact_kind;        /* UPS_ACT_* of the activation whose derivative multiplies the result (dgrad) */
    int32_t ldr, ldd;         /* physical channels of res / dact */
    const void*  in;
    const void*  w;           /* blocked-K weights [n_slices][ceil(ci/BK)][co][BK], BK = 64 bytes / sizeof(dtype)
                                 (32 bf16 / 16 f32), zero padded in K: produced by ups_weight_prep */
    void*        out;
    const float* bias;        /* [co] or NULL */
    const float* coord_tab;   /* [64][3][co] affine CoordConv table (ups_coord_table) or NULL */
    const void*  res;         /* residual, same pixel lattice as out, or NULL */
    const void*  dact;        /* pre-activation tensor for dact_kind, same lattice as out, or NULL */
    float*       workspace;   /* optional fp32 scratch for the deterministic split-K path of small-M problems (few tiles,
                               * long K loops); NULL or too small = no split */
    size_t       workspace_bytes;
    /* Part-masked input (mask_parts + apply_partwise, M:176-187, N:81-113) fused into the load, so that the
     * [P*B,H,W,C] part tensor never exists (3x3 / stride-1 patch kernels, bf16, 16-aligned images; else UPS_E_UNSUPPORTED):
     * `n` = P*mask_batch logical images in part-major order (image p*mask_batch + b); `in` is the UNMASKED view tensor
     * [mask_batch, hi, wi, ldi]; pixel (b,y,x) of part image p reads as in[b,y,x,:] if bit p of mask_bits[b,y,x] is set, else 0. */
    const uint32_t* mask_bits;   /* [mask_batch, hi, wi] hard-mask bit sets (ups_part_softmax_fwd) or NULL */
    int32_t      mask_batch;
    /* Input gradient of such a convolution reduced straight to the hard mask (the dgrad call of the same layer): instead
     * of out[p*B+b][y][x][c] the kernel writes mask_grad[b][y][x][p] = sum_c out * mask_view[b][y][x][c] (M:185 backward). */
    float*       mask_grad;      /* [mask_batch, out_h, out_w, n / mask_batch] fp32 or NULL (`out` may then be NULL) */
    const float* mask_view;      /* [mask_batch, out_h, out_w, co] fp32 view tensor, required with mask_grad */
    /* fp8 forward (BASELINE config #5: e4m3 MFMA operands, fp32 accumulate, bf16 tensors; 3x3 / stride-1 patch kernels,
     * dtype UPS_BF16, 16-aligned images, ci % 64 == 0, no mask; else UPS_E_UNSUPPORTED).  f8_deq != NULL selects it:
     * `w` then holds e4m3 weights [9][ci/64][co][64] scaled per output channel (ups_weight_prep_f8), f8_deq[c] = 1 / that
     * scale; the staged activations are multiplied by *f8_scale before the conversion (device scalar, delayed scaling) and
     * max |act(in)| of this launch is collected into the 64 slots of f8_amax (atomic max of non-negative float bits). */
    const float* f8_deq;         /* [co] or NULL */
    const float* f8_scale;       /* device scalar */
    float*       f8_amax;        /* [64] */
    int32_t      f8_e5m2;        /* 1: `in` is a gradient -- staged as e5m2 (the input-gradient call of an fp8 layer; `w` from
                                  * ups_weight_prep_f8 with transpose = 1), 0: e4m3 */
    /* fp8 copies handed from layer to layer.  Producer side (any bf16 patch-kernel call with the staged epilogue): out_f8_amax != NULL
     * records max |act(out)| (act = out_f8_act, the consumer's activation-on-load) into its 64 slots; with out_f8 != NULL the epilogue also
     * writes e4m3 (out_f8_e5m2: e5m2) of act(out) * *out_f8_scale to out_f8 [n, out_h, out_w, ldo] bytes, next to the bf16 tensor.
     * Consumer side: in_f8 != NULL (with f8_deq) = that byte tensor [n, hi, wi, ldi]; it is staged as it is (f8_scale = the scale it was
     * written with, act_in is not applied again, f8_amax unused) with the bf16 kernel's register budget (two blocks per CU). */
    const void*  in_f8;
    void*        out_f8;
    const float* out_f8_scale;
    float*       out_f8_amax;
    int32_t      out_f8_act, out_f8_e5m2;
    /* Depth-to-space output (input gradient of a 3x3 / stride-2 convolution as ONE stride-1 convolution over the gradient
     * lattice, N:811-817 backward): d2s = C > 0 (power of two, >= 8) declares co = 4 C GEMM channels ordered (py, px, c); channel c of
     * class (py, px) at lattice pixel (y, x) is written to out[n][2y + py][2x + px][c] of a [n, out_h = 2 ho, out_w = 2 wo, ldo]
     * tensor; res / dact are read on that lattice.  `w` = ups_weight_prep_d2s.  bf16 patch kernel only (else UPS_E_UNSUPPORTED). */
    int32_t      d2s;
    /* Post-activation storage.  A 16-bit (or fp32) tensor whose only convolution consumer applies an activation on load may be
     * STORED as act(x) instead of x: the consumer then stages it untouched (act_in = UPS_ACT_NONE: the halo patch can arrive by
     * LDS-DMA, no staging registers, no VALU), its weight gradient reads the operand as it is, its input gradient still takes
     * the sign for act' from it (sign(act(x)) = sign(x)).
     *   out_act  activation applied to the finished value (after bias, CoordConv, act', residual) before it is stored;
     *   res_act  `res` holds act(x) of a leaky-ReLU (slope > 0): it is inverted (r > 0 ? r : r / slope) before it is added --
     *            the residual stream x + conv(act(x)) of N:1042-1056 with x stored as act(x).  UPS_ACT_LRELU or UPS_ACT_NONE.
     * Gradients are always with respect to the pre-activation values: nothing changes in the backward calls. */
    int32_t      out_act, res_act;
    /* Bit-packed activation signs (ABI 4).  An input-gradient launch needs ONE bit of every element of the layer's forward input --
     * the sign, for act' -- and used to re-read the whole 16-bit tensor for it (`dact`).
     *   sign_out   forward call, 16-bit `out` [n, out_h, out_w, ldo] with ldo % 8 == 0, plain (unstrided, no d2s) output: also
     *              write bits[n][out_h][out_w][ldo / 8] bytes, bit e of byte j = (out[..., 8 j + e] > 0) of the STORED value
     *              (with out_act: of act(value), which has the value's sign).  BEST EFFORT: written by the kernels that have the
     *              output tile in hand (the 16-bit patch kernel); a launch that went to another kernel leaves the buffer untouched
     *              (a pass over `out` would cost the read the bits save) -- ups_conv_sign_out_written() tells, ups_sign_pack packs.
     *   dact_bits  backward call with `dact`: the same bytes for the tensor `dact` points to ([n, out_h, out_w, ldd / 8]); kernels
     *              that can (the 16-bit patch kernel) read them INSTEAD of `dact`, the others ignore them.  `dact` stays mandatory. */
    void*        sign_out;
    const void*  dact_bits;
} ups_conv_desc;

int ups_conv_igemm(const ups_conv_desc* d, void* stream);
/* 1 when the calling thread's last ups_conv_igemm call wrote its ups_conv_desc.sign_out buffer, else 0 */
int ups_conv_sign_out_written(void);

/* Weights of the depth-to-space input gradient of a 3x3 / stride-2 'SAME' convolution with forward variable V [3][3][cin_v][co]:
 * w[t9][k][(py*2+px)*C + c][32] (blocked-K over the co gradient channels, bf16), t9 = (dy+1)*3 + (dx+1) the 3x3 neighbourhood of
 * the gradient lattice, C = ci_log rounded up to a power of two (>= 8), = V[r][s][c][k-chunk] where tap (r, s) reaches class (py, px)
 * from lattice offset (dy, dx) -- r = py + pad_y - 2 dy, s likewise -- and zero elsewhere. */
int ups_weight_prep_d2s(const float* src, int32_t cin_v, int32_t ci_log, int32_t co, int32_t pad_y, int32_t pad_x, int32_t C,
                        void* w, void* stream);

/* e4m3 weights for the fp8 forward: w_f8[tap][k][c][64] = e4m3(V[tap][64 k + j][c] * 448 / amax_c), zero padded in K,
 * deq[c] = amax_c / 448 with amax_c = max |V[:, :ci_log, c]| (the CoordConv rows ci_log.. stay fp32 in ups_coord_table).
 * transpose = 1: the input-gradient operand -- rows = input channels, K = output channels: w_f8[tap][k][ci][64] =
 * e4m3(V[tap][ci][64 k + j] * 448 / amax_ci), deq[ci] = amax_ci / 448.
 * src is the HWIO fp32 variable [ntaps][cin_v][co] (N:644-652). */
int ups_weight_prep_f8(const float* src, int32_t ntaps, int32_t cin_v, int32_t ci_log, int32_t co, int32_t transpose,
                       void* w_f8, float* deq, void* stream);

/* Weight gradient  dV[tap][ci][co] = sum_pix act(in)[src(pix,tap)][ci] * dout[pix][co]
 * (gradient of N:661-663 w.r.t. V), split-K over pixels into fp32 slabs + deterministic reduce.
 * grad layout is the TF variable layout HWIO with `cin_v` input channels (cin_v = ci_log (+2 CoordConv)). */
typedef struct {
    int32_t dtype;
    int32_t n, hi, wi, ci, ldi;       /* forward input, ci = channels to differentiate (multiple of 8) */
    int32_t ci_log;                   /* rows actually stored (logical input channels) */
    int32_t cin_v;                    /* input-channel extent of grad (>= ci_log) */
    int32_t ho, wo, co, ldo;          /* dout tensor [n, ho, wo, ldo], co logical */
    int32_t in_sy, in_sx;
    int32_t ntaps;
    int32_t tap_dy[9], tap_dx[9], tap_w[9];
    int32_t act_in; float act_slope;
    int32_t splitk;                   /* from ups_conv_wgrad_plan */
    const void* in; const void* dout;
    float* grad;                      /* [kh*kw][cin_v][co] fp32 */
    float* grad_bias;                 /* [co] fp32 or NULL: sum_pix dout, reduced from the same dout tiles */
    float* workspace;                 /* bytes from ups_conv_wgrad_plan */
    const uint32_t* mask_bits;        /* part-masked input, same meaning as in the conv descriptor; bf16 3x3 / stride-1 patch kernel only; or NULL */
    int32_t mask_batch;
    int32_t in_f16;                   /* dtype UPS_BF16 only: `in` holds fp16 (the forward tensor of a UPS_F16 layer); it is converted to
                                       * bf16 (after the activation) while it is staged -- dout stays bf16 */
    /* fp8 weight gradient (ABI 3; BASELINE config #5): dout_f8 != NULL selects it for the wide 3x3 / stride-1 layers (ci % 64 == 0,
     * co % 128 == 0, 16-aligned images, forward tap order): e5m2(dout * *dout_f8_scale) as its producer wrote it, [n, ho, wo, ldo]
     * bytes -- the copy the layer's input-gradient launch reads (ups_conv_desc.in_f8) --, `in` quantised to e4m3 with
     * *in_f8_scale while it is staged (max |act(in)| recorded into the 64 slots of in_f8_amax for the next step's scale, or NULL),
     * block-scaled K = 128 MFMA, fp32 accumulation; other shapes ignore these fields and run the bf16 kernels on `dout`. */
    const void*  dout_f8;
    const float* dout_f8_scale;
    const float* in_f8_scale;
    float*       in_f8_amax;
} ups_wgrad_desc;

int ups_conv_wgrad_plan(const ups_wgrad_desc* d, int32_t* splitk, size_t* workspace_bytes);
int ups_conv_wgrad(const ups_wgrad_desc* d, void* stream);

/* fp32 HWIO master weights -> dtype copies in the blocked-K layout [tap][k-chunk][row][BK] (BK = 64 bytes):
 * w_fwd rows = co, K = ci_pad; w_dgrad rows = dgrad_rows, K = dgrad_k.
 * src [ntaps][cin_v][co]; only input channels < ci_log are copied (CoordConv rows are handled by
 * ups_coord_table); rows/cols beyond the logical extent are zero.  Either dst may be NULL. */
int ups_weight_prep(const float* src, int32_t ntaps, int32_t cin_v, int32_t ci_log, int32_t co,
                    int32_t dtype, void* w_fwd, int32_t ci_pad,
                    void* w_dgrad, int32_t dgrad_rows, int32_t dgrad_k, void* stream);

/* Batched form: one launch converts every convolution of a sub-network after its optimizer step (weights in both
 * layouts + the CoordConv table).  `items` is a DEVICE array of n_items descriptors, `block_prefix` a DEVICE array of
 * n_items+1 cumulative 256-thread block counts (ups_prep_item_blocks gives the per-item count). */
typedef struct {
    const float* src;         /* fp32 HWIO variable V [ntaps][cin_v][co] */
    void*  w_fwd;             /* [ntaps][ceil(ci_pad/BK)][co][BK] or NULL */
    void*  w_dgrad;           /* [ntaps][ceil(dgrad_k/BK)][dgrad_rows][BK] or NULL */
    float* ctab;              /* [64][3][co] or NULL (no CoordConv) */
    int32_t ntaps, cin_v, ci_log, co, ci_pad, dgrad_rows, dgrad_k;
    int32_t kh, kw, in_sy, in_sx;
    int32_t dy[3], dx[3];
    float ax, ay;
} ups_prep_item;
int64_t ups_prep_item_blocks(const ups_prep_item* item_host, int32_t dtype);
/* Host constants of the batched launch: 256-element chunks converted per thread block (a unit of four chunks must lie inside one
 * block), and the item count up to which the prefix is searched in LDS (beyond it: in global memory). */
int32_t ups_prep_chunks_per_block(void);
int32_t ups_prep_lds_items(void);
int ups_weight_prep_batch(const ups_prep_item* items, const int64_t* block_prefix, int32_t n_items, int64_t total_blocks,
                          int32_t dtype, void* stream);

/* CoordConv (N:2123-2154) folded into an affine epilogue: tab[cls][0..2][c] with
 * cls = ymask*8 + xmask (valid-tap bitmasks of the output pixel);
 * contribution = tab[cls][0][c] + j*tab[cls][1][c] + i*tab[cls][2][c].
 * V is the fp32 HWIO variable with ci_log+2 input channels; ax = 2/max(1,H-1), ay = 2/max(1,W-1). */
int ups_coord_table(const float* V, int32_t kh, int32_t kw, int32_t ci_log, int32_t co,
                    const int32_t* tap_dy, const int32_t* tap_dx, int32_t in_sy, int32_t in_sx,
                    float ax, float ay, float* tab, void* stream);
/* gsum[pix][c] = sum_n dout[n][pix][c] (fp32); dout is UPS_F32 or UPS_BF16 (gradients are never fp16: UPS_F16 is refused) */
int ups_batch_sum(const void* dout, int32_t dtype, int32_t n, int64_t pix, int32_t co, int32_t ldo,
                  float* gsum, void* stream);
/* gradient of the two CoordConv rows of V (and optionally the bias) from gsum [ho*wo][co];
 * `scratch` holds (2*kh+1)*wo*co floats (separable two-stage reduction: rows first -- two planes per tap row and one for the
 * bias --, then columns); grad_bias [co] or NULL */
int ups_coord_wgrad(const float* gsum, int32_t hi, int32_t wi, int32_t ho, int32_t wo, int32_t co,
                    int32_t kh, int32_t kw, const int32_t* tap_dy, const int32_t* tap_dx,
                    int32_t in_sy, int32_t in_sx, float ax, float ay,
                    int32_t ci_log, float* gradV, float* grad_bias, float* scratch, void* stream);
/* grad_bias[c] = sum_rows dout[row][c]; dout is UPS_F32 or UPS_BF16 (UPS_F16 is refused); workspace >= 1024*co floats */
int ups_col_sum(const void* dout, int32_t dtype, int64_t rows, int32_t co, int32_t ldo,
                float* out, float* workspace, void* stream);

/* ---------------------------------------------------------------- weight-normalised transposed convolution
 * upsample(x, nf, "conv_transposed") = deconv2d(x, nf, stride 2), 3x3, TF 'SAME' (N:818-822, 938-1039):
 *     y[n, 2i+ky, 2j+kx, o] = b[o] + sum_c x~[n, i, j, c] * W[ky][kx][o][c],   W = g[o] * V / max(||V_o||, 1e-6)
 * (taps landing on row / column 2H are dropped; x~ = x plus the two CoordConv channels in CoordConv scopes).  V [3,3,nf,cin_v] is
 * the TF transpose layout [kh, kw, out, in], cin_v = ci_log (+2 with coordinates).
 *
 * ups_deconv_prep: once per weight version, from V and g: inv_norm [nf], the fp32 W [3,3,nf,cin_v] (w32), and optionally
 *   w_fwd  forward operand [9][ceil(round8(ci_log)/BK)][nf][BK] of fwd_dtype (F32 / BF16 / F16; BK = 64 bytes / element) -- the
 *          `w` of ups_deconv3x3_s2_fwd and of the per-class ups_conv_igemm launches (tap_w = 3 ky + kx);
 *   w_dx   input-gradient operand [9][ceil(round8(nf)/BK)][ci_log][BK] of dx_dtype (F32 / BF16): the `w` of the stride-2 forward
 *          convolution dx = conv2d(dy, W[.., :ci_log]) (ups_conv_igemm, taps (r, s) = (ky, kx));
 *   ctab   CoordConv tables [4 classes 2 py + px][64][3][nf] in the ups_conv_desc.coord_tab layout of the class launches, whose taps are
 *          r-major over the class's rows (py = 0: ky 0 / 2 from input rows i / i-1; py = 1: ky 1 from row i) and columns; hi x wi
 *          is the INPUT size (add_coordinates runs at the input's resolution). */
int ups_deconv_prep(const float* V, const float* g, int32_t nf, int32_t cin_v, int32_t ci_log, int32_t fwd_dtype, void* w_fwd,
                    int32_t dx_dtype, void* w_dx, float* w32, float* inv_norm, float* ctab, int32_t hi, int32_t wi, void* stream);
/* One-launch forward on the 16-bit MFMA: x [n,h,w,ldi] (BF16 or F16), ci = round8(ci_log) channels reduced, y [n,2h,2w,ldo] with
 * channels [nf, ldo) written as zero; bias [nf] (or NULL), ctab = ups_deconv_prep's tables (or NULL).  UPS_E_UNSUPPORTED (nothing
 * launched) unless w % 16 == 0, ci <= 256 and nf <= 256: the caller then runs the four per-class ups_conv_igemm launches. */
int ups_deconv3x3_s2_fwd(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ci, int32_t ldi, const void* w_fwd,
                         const float* bias, const float* ctab, int32_t nf, int32_t ldo, void* y, void* stream);
/* From dy [n,2h,2w,ldo] (F32 / BF16): db[o] = sum dy and, with coords, dwc [9][nf][2] = the gradient of W's two coordinate columns
 * (sum over the lattice points a tap reaches of dy * coordinate).  part: splits * 19 * nf floats of scratch (deterministic). */
int ups_deconv_bias_coord_grad(const void* dy, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t nf, int32_t ldo, int32_t coords,
                               float* db, float* dwc, float* part, int32_t splits, void* stream);
/* dW -> dV [3,3,nf,cin_v], dg [nf] through the normalisation: dg = <Vhat_o, dW_o>, dV = (g / ||V_o||) (dW_o - Vhat_o dg_o).
 * dW arrives as dwx [9][nf][ci_log] (columns of x) and dwc [9][nf][2] (coordinate columns; NULL when cin_v == ci_log). */
int ups_deconv_wn_bwd(const float* V, const float* g, const float* dwx, const float* dwc, int32_t nf, int32_t cin_v, int32_t ci_log,
                      float* dV, float* dg, void* stream);

/* ---------------------------------------------------------------- resampling / pooling
 * Legacy TF-1 bilinear x2 (N:834-847, tf.image.resize_images BILINEAR, no half-pixel centres). */
int ups_bilinear2x_fwd(const void* x, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, void* stream);
int ups_bilinear2x_bwd(const void* gy, void* gx, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, void* stream);
/* The other up-sampling methods of nn.upsample (N:820-849).  "subpixel" = a convolution to 4 C channels (ups_conv_igemm) followed by
 * tf.depth_to_space(x, 2): y[b, 2i+di, 2j+dj, c] = x[b, i, j, (2 di + dj) C + c]; x is [n,h,w,ldx] (4 C logical channels), y is
 * [n,2h,2w,ldy] (C logical channels, pad channels written as zero).  bwd != 0: src = the gradient w.r.t. y, dst = w.r.t. x.
 * "nearest_neighbor": y[b, 2i+di, 2j+dj, :] = x[b, i, j, :]; bwd != 0: src = gradient [n,2h,2w,c], dst [n,h,w,c] = the sum of the four. */
int ups_depth_to_space(const void* src, void* dst, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t C, int32_t ldx, int32_t ldy,
                       int32_t bwd, void* stream);
int ups_nearest2x(const void* src, void* dst, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t bwd, void* stream);
/* The ho x wo window of x [n,h,w,c] whose corner (oy, ox) = yx_dev[0..1] is read ON THE DEVICE (int32; clamped to the image):
 * the random 224x224 window of edflow VGG19Features(original_scale=True).make_loss_op as `perceptual_input: resize256_crop224`
 * reads it (M:610-618; UNVERIFIED), one window per step for the whole batch.  bwd: gx [n,h,w,c] = gy inside the window, 0
 * elsewhere.  16-bit dtypes are copied as raw bits (UPS_BF16 and UPS_F16 alike). */
int ups_crop_fwd(const void* x, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo,
                 const int32_t* yx_dev, void* stream);
int ups_crop_bwd(const void* gy, void* gx, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo,
                 const int32_t* yx_dev, void* stream);
/* y = act(bilinear x2 of x): the up-sampled tensor in post-activation storage (ups_conv_desc.out_act) for a consuming residual block */
int ups_bilinear2x_fwd_act(const void* x, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t act, float slope,
                           void* stream);
/* ... the same, also writing the sign bits of the stored values (ups_conv_desc.sign_out layout: [n][2h][2w][c / 8] bytes);
 * 16-bit dtypes. */
int ups_bilinear2x_fwd_bits(const void* x, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t act, float slope,
                            void* sign_bits, void* stream);
/* bits[i] = sign byte of the 8 elements x[8 i .. 8 i + 7] (16-bit dtype), chunks = elements / 8 */
int ups_sign_pack(const void* x, int32_t dtype, int64_t chunks, void* sign_bits, void* stream);
/* The same (bf16) with an fp8 copy of the result for a consuming fp8 convolution (ups_conv_desc.in_f8): max |act(y)| goes to
 * amax[64]; with y_f8 != NULL also e4m3 (e5m2 != 0: e5m2) of act(y) * *scale, one byte per element, laid out like y. */
int ups_bilinear2x_fwd_f8(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, void* y_f8, const float* scale,
                          float* amax, int32_t act, float slope, int32_t e5m2, void* stream);
int ups_bilinear2x_bwd_f8(const void* gy, void* gx, int32_t n, int32_t h, int32_t w, int32_t c, void* gx_f8, const float* scale,
                          float* amax, int32_t e5m2, void* stream);
/* activate + global spatial mean (M:50-51): y[n][c] = mean_hw act(x) */
/* y = elu(x) = x > 0 ? x : exp(x) - 1 (nn.py:747-758 `activate(x, "elu")`), gx = gy * (x > 0 ? 1 : exp(x)); n elements of dtype
 * UPS_F32 / UPS_BF16 / UPS_F16 (n a multiple of 8). */
int ups_elu_fwd(const void* x, void* y, int32_t dtype, int64_t n, void* stream);
int ups_elu_bwd(const void* x, const void* gy, void* gx, int32_t dtype, int64_t n, void* stream);
int ups_act_mean_fwd(const void* x, void* y, int32_t dtype, int32_t n, int32_t hw, int32_t c, int32_t act, float slope, void* stream);
int ups_act_mean_bwd(const void* x, const void* gy, void* gx, int32_t dtype, int32_t n, int32_t hw, int32_t c, int32_t act, float slope, void* stream);
/* 2x2/2 max pool on pre-activations (Keras VGG19 block*_pool); bwd routes to the first maximal element */
int ups_maxpool2_fwd(const void* x, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, void* stream);
/* bf16 form that also hands the pooled tensor to an fp8 convolution (Keras VGG19 pools in front of block{2..5}_conv1; edflow
 * VGG19Features, external): max |act(y)| into amax[64]; with y_f8 != NULL the e4m3 bytes of act(y) * *scale next to y. */
int ups_maxpool2_fwd_f8(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, void* y_f8, const float* scale,
                        float* amax, int32_t act, float slope, void* stream);
int ups_maxpool2_bwd(const void* x, const void* gy, void* gx, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, void* stream);
/* copy `c` channels between tensors with different physical widths / offsets (concat for N:1049-1051) */
int ups_copy_channels(const void* src, int32_t lds, void* dst, int32_t ldd, int32_t dtype, int64_t rows, int32_t c, void* stream);
/* dst[row][0..c) += src[row][0..c) */
int ups_add_channels(const void* src, int32_t lds, void* dst, int32_t ldd, int32_t dtype, int64_t rows, int32_t c, void* stream);

/* ---------------------------------------------------------------- perceptual loss pieces (M:607-619, edflow VGG19Features)
 * [-1,1] RGB fp32 [n,h,w,3] or dtype [n,h,w,ldx] -> BGR*255 - mean, dtype [n,h,w,8] (channels 3..7 zero) */
int ups_vgg_preprocess_fwd(const void* x, int32_t x_is_f32, int32_t ldx, void* y, int32_t dtype, int64_t pixels, void* stream);
int ups_vgg_preprocess_bwd(const void* gy, void* gx, int32_t dtype, int32_t ldgx, int64_t pixels, void* stream);
/* partial[block] = sum |act(a) - act(b)| ; loss = scale * sum(partial) is finished by ups_sum_scale */
int ups_l1_fwd(const void* a, const void* b, int32_t dtype, int64_t rows, int32_t c, int32_t ld, int32_t act,
               float* partial, int32_t nblocks, void* stream);
/* gb[row][c] = -scale * sign(act(a)-act(b)) * act'(b), pad channels zero (gradient w.r.t. the 2nd operand) */
int ups_l1_bwd(const void* a, const void* b, void* gb, int32_t dtype, int64_t rows, int32_t c, int32_t ld, int32_t act,
               const float* scale_dev, float scale, void* stream);
/* out[0] (+)= scale * sum(partial[0..n)) */
int ups_sum_scale(const float* partial, int32_t n, float scale, float* out, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------- Gram-matrix terms of the perceptual loss (csrc/gram.hip)
 * edflow VGG19Features(default_gram=w) (UNVERIFIED): term = w * mean_{b,i,j} |G(F_t)[b] - G(F_g)[b]|, G(F)[b] = F[b]^T F[b] / (4 h w),
 * F = act(map) as [n, h w, c] (c logical channels of an [n, h, w, ld] map, F32 or BF16; act NONE, RELU or LRELU with slope 0).
 * The kernels see the unnormalised D_b = F_g[b]^T F_g[b] - F_t[b]^T F_t[b]; the caller applies 1 / (4 h w) and the mean over n c c.
 *
 * ups_gram_plan: out[0] = K splits, out[1] = partial floats (n * tile pairs), out[2] = workspace floats (0 without a split),
 *   out[3] = sign bytes (n * cp * cp, cp = c rounded up to 32).
 * ups_gram_l1_fwd: a = target, b = generated; partial[b, pair] = sum over the pair's 32x32 tile of |D| (off-diagonal tiles twice),
 *   finished by ups_sum_scale; sign [n][cp][cp] int8 = sign(D) (symmetric, 0 outside [c, c]) for the backward.  Deterministic.
 * ups_gram_l1_bwd: gb[b] += scale * scale_dev[0] * act'(b) * (act(b)[b] S_b) on channels [0, c) (ACCUMULATES into the L1 term's
 *   gradient; channels [c, ld) untouched); scale_dev may be NULL. */
int ups_gram_plan(int32_t n, int64_t hw, int32_t c, int32_t dtype, int64_t* out);
int ups_gram_l1_fwd(const void* a, const void* b, int32_t dtype, int32_t n, int64_t hw, int32_t c, int32_t ld, int32_t act,
                    float* partial, void* sign, float* workspace, void* stream);
int ups_gram_l1_bwd(const void* b, const void* sign, void* gb, int32_t dtype, int32_t n, int64_t hw, int32_t c, int32_t ld,
                    int32_t act, const float* scale_dev, float scale, void* stream);

/* ---------------------------------------------------------------- part path
 * l = mean + eps (N:1427-1433); m = softmax_P(l) (N:58-62); hard = (m == max_P m) (N:134-136);
 * argmax = first maximal index (M:447,470); hard_bits[pixel] = bit set of the hard mask (bit p = hard[pixel][p], P <= 32:
 * the compact form the part-masked convolution reads).  eps, hard, argmax, hard_bits may be NULL.  All fp32, [pixels][P]. */
int ups_part_softmax_fwd(const float* mean, const float* eps, float* l, float* m, float* hard, int64_t* argmax,
                         uint32_t* hard_bits, int64_t pixels, int32_t P, void* stream);
/* The same plus, from the same pass, the spatial soft-max moments of gamma * hard (the one-hot map has them in closed form from
 * per-part integer sums of the hard pixels' coordinates): stats [n][P][8] as ups_spatial_moments(hard, gamma, no rectangle) writes
 * them (M:437-440: the input of the rectangle centres).  mean is [n,h,w,P]; h*w must be a multiple of the kernel's pixel tile
 * = ups_part_softmax_moments_tile(P) (else UPS_E_ARG: call ups_part_softmax_fwd + ups_spatial_moments); scratch:
 * ups_part_softmax_moments_ints(n*h*w, P) int32. */
int32_t ups_part_softmax_moments_tile(int32_t P);
size_t ups_part_softmax_moments_ints(int64_t pixels, int32_t P);
int ups_part_softmax_moments_fwd(const float* mean, const float* eps, float* l, float* m, float* hard, int64_t* argmax,
                                 uint32_t* hard_bits, int32_t n, int32_t h, int32_t w, int32_t P, float gamma, float* stats,
                                 int32_t* scratch, void* stream);
/* spatial soft-max moments (N:65-71, N:1541-1587) of gamma*x per (n,p) over H*W, optionally masked by
 * (1 - rect) with integer rectangle centres `rect_c` [n*P][2] (y,x) and half sizes:
 * stats[n][p] = {max, Z, sum e*k, sum e*k*gy, sum e*k*gx, sum e*k*(gy^2+gx^2), sum e*k*gy^2, 0},  e = exp(gamma*x - max) */
int ups_spatial_moments(const float* x, int32_t n, int32_t h, int32_t w, int32_t P, float gamma,
                        const int32_t* rect_c, int32_t half_h, int32_t half_w, float* stats, void* stream);
/* The same pass also sums x * log(P * x + 1e-20) over the whole map -- categorical_kl of view 1's soft map (M:21-25, 659-665), the
 * only other prior term of that view, which therefore needs no pass of its own: kl_sums16[0] = the sum (slots 1..15 zeroed: the
 * layout of ups_prior_desc.sums). */
int ups_spatial_moments_kl(const float* x, int32_t n, int32_t h, int32_t w, int32_t P, float gamma,
                           const int32_t* rect_c, int32_t half_h, int32_t half_w, float* stats, float* kl_sums16, void* stream);
/* `stats` must hold n*P*8 floats of result followed by scratch; total = ups_spatial_moments_floats(n, P). */
size_t ups_spatial_moments_floats(int32_t n, int32_t P);
/* px[n*P][2] = (row, column) centre of the rectangle tfutils.draw_rect paints for int32(mu*h/2 + h/2) (M:441,459;
   truncation) from the un-masked stats.  xy_order != 0: the helper reads the (y, x) pair as (x, y) -- row centre from mu_x,
   column centre from mu_y (the reading the reference's step-0 patch_loss supports; oracle/ref_model.py draw_rect) */
int ups_moments_to_px(const float* stats, int32_t count, int32_t h, int32_t xy_order, int32_t* px, void* stream);
/* tfutils.draw_rect (external; semantics inferred): out [n,h,w,P] fp32 */
int ups_draw_rect(const int32_t* px, int32_t n, int32_t h, int32_t w, int32_t P, int32_t half_h, int32_t half_w,
                  float* out, void* stream);
/* mask_parts + apply_partwise transpose (M:176-187, N:97-103): out[(p*B+b)][y][x][0..8) = view[b][y][x][c]*hard[b][y][x][p] */
int ups_mask_parts_fwd(const float* view, const float* hard, void* out, int32_t dtype, int32_t B, int64_t hw, int32_t P, void* stream);
/* g_hard[b][pix][p] = sum_c g_out[(p*B+b)][pix][c] * view[b][pix][c] */
int ups_mask_parts_bwd(const float* view, const void* g_out, float* g_hard, int32_t dtype, int32_t B, int64_t hw, int32_t P, void* stream);
/* unpool_features + concat (M:225-249, 482-484): out[b][pix][f] = sum_p hard*feat[b][p][f]; out[..][F+p] = hard; pad zero */
int ups_unpool_fwd(const float* hard, const float* feat, void* out, int32_t dtype, int32_t B, int64_t hw, int32_t P, int32_t F, int32_t ldo, void* stream);
/* mixed unpool (appearance transfer; inference only, no backward): hard [n,hw,P], feat [m,P,F] fp32, pose_idx [K], app_idx [K*P]
 * int32 DEVICE arrays with 0 <= pose_idx < n, 0 <= app_idx < m (the caller validates them: the kernel does not), out [K,hw,ldo]:
 *   out[k][pix][f] = sum_p hard[pose_idx[k]][pix][p] * feat[app_idx[k*P+p]][p][f];  out[k][pix][F+p] = hard[pose_idx[k]][pix][p];
 *   channels [F+P, ldo) zero.  Bit-identical to ups_unpool_fwd on explicitly gathered inputs.  K >= 1, ldo % 8 == 0, ldo >= F+P,
 *   F % 8 == 0, feat and out 16-byte aligned (the feature rows are gathered with 16-byte loads): UPS_E_ARG otherwise. */
int ups_unpool_mix_fwd(const float* hard, const float* feat, const int32_t* pose_idx, const int32_t* app_idx, void* out, int32_t dtype,
                       int32_t K, int32_t n, int32_t m, int64_t hw, int32_t P, int32_t F, int32_t ldo, void* stream);
/* g_hard[b][pix][p] = sum_f g[..f]*feat[b][p][f] + g[..F+p];  g_feat_partial[blk][b][p][f] partial sums (blocks_per_image each) */
int ups_unpool_bwd(const float* hard, const float* feat, const void* g, float* g_hard, float* g_feat,
                   int32_t dtype, int32_t B, int64_t hw, int32_t P, int32_t F, int32_t ldo, void* stream);
/* `g_feat` must hold B*P*F floats of result followed by scratch; total = ups_unpool_bwd_floats(B,P,F). */
size_t ups_unpool_bwd_floats(int32_t B, int32_t P, int32_t F);
/* The route ups_unpool_bwd takes for these arguments (host code only; ups_unpool_bwd itself launches from it): out[0] form (0: the
 * generic kernel, 1: the matrix-core kernel -- bf16, F = 64, P in 10 / 16 / 20 / 25 with ldo = round8(64 + P), hw % 128 == 0,
 * aligned16 and UPS_UNPOOL_MFMA not 0, read at every call), out[1] blocks per image, out[2] tiles per block, out[3] pixels per
 * tile, out[4] pixels per block, out[5] bytes of dynamic LDS.  aligned16: hard, g and g_hard are all 16-byte aligned.
 * B, hw, P >= 1, 8 <= F <= 64, F % 8 == 0, P <= 64, ldo % 8 == 0, ldo >= F + P (and g itself 16-byte aligned in ups_unpool_bwd):
 * UPS_E_ARG otherwise. */
int ups_unpool_bwd_plan(int32_t dtype, int32_t B, int64_t hw, int32_t P, int32_t F, int32_t ldo, int32_t aligned16, int64_t* out);

/* ---------------------------------------------------------------- training image logs (M:968-1053), csrc/canvas.hip
 * uint8 canvases of the reference's img_ops.  Every entry writes a caller-owned canvas [rows*H, cols*W, C] (C = 3 RGB, 1 gray;
 * 16-byte aligned) completely -- blank tiles included -- with 16-byte stores, one run of 16 bytes per thread.
 *   quantisation (edflow save_image, re-derived, UNVERIFIED): byte = (uint8) clamp((v + 1) * 127.5, 0, 255), truncating; value 0
 *     (blank tiles, masked-out pixels) is byte 127, and maps the reference leaves in [0,1] come out between 127 and 255;
 *   tiling (tf_batch_to_canvas, re-derived, UNVERIFIED): tile n at row n / cols, column n % cols; tiles n >= N are blank;
 *   every decision (truncation, thresholds, half-to-even rounding) is taken in fp64 on the fp32 / bf16 source values.
 * Sources are NHWC; images are UPS_F32 or UPS_BF16 with `ld` physical channels (ld >= 3: the first three are R, G, B), masks are
 * fp32 [..][P] or the sign-packed hard bits of ups_part_softmax_fwd (uint32 per pixel, P <= 32).  UPS_E_ARG on anything else. */
/* ceil(sqrt(n)): the side of the square grid tf_batch_to_canvas(cols=None) lays n tiles out in */
int ups_canvas_grid_side(int32_t n);
/* img [N,H,W,ld] in [-1,1] -> canvas [rows*H, cols*W, 3]; rows * cols >= N */
int ups_canvas_images(const void* img, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t ld, int32_t rows, int32_t cols,
                      uint8_t* canvas, void* stream);
/* mask2rgb (N:2067-2089) -> canvas [rows*H, cols*W, 3]: colors[3 p ..] (uint8 [P,3], DEVICE, already quantised by the host) of the
 * pixel's part.  Exactly one of mask [N,H,W,P] fp32 / bits [N,H,W] is given.  mask, one_hot = 0: arg-max over P, the lowest index
 * wins ties (tf.argmax); one_hot = 1 (make_hot=False): the mask is one-hot already, the first non-zero entry names the part;
 * bits: the lowest set bit.  A pixel without a part (all-zero one-hot / bits) is value 0, byte 127. */
int ups_canvas_mask_rgb(const float* mask, const uint32_t* bits, int32_t one_hot, const uint8_t* colors, int32_t N, int32_t H, int32_t W,
                        int32_t P, int32_t rows, int32_t cols, uint8_t* canvas, void* stream);
/* assigned_parts (M:990-1006) in one launch: for part p the g x g grid (g = ups_canvas_grid_side(2B)) of the 2B images
 * hard0[b][..][p] * view0[b] (b < B), then hard1[b][..][p] * view1[b]; the P grids in 5 columns ->
 * canvas [ceil(P/5)*g*H, 5*g*W, 3].  Masks: hard0 / hard1 [B,H,W,P] fp32, or bits0 / bits1 [B,H,W] (the other pair NULL);
 * views [B,H,W,ld] of `dtype`. */
int ups_canvas_assigned_parts(const float* hard0, const float* hard1, const uint32_t* bits0, const uint32_t* bits1, const void* view0,
                              const void* view1, int32_t dtype, int32_t ld, int32_t B, int32_t H, int32_t W, int32_t P, uint8_t* canvas,
                              void* stream);
/* The four canvases of batch item 0 (M:986-988, 1009-1032) in one launch, from m [H,W,P] fp32 (m0_sample[0]) and the hard mask of
 * the same image (hard [H,W,P] fp32 or bits [H,W], the other NULL); gp = ups_canvas_grid_side(P):
 *   c_levels [P*H, n_levels*W, 1]  row p, column k: m[..][p] > levels[k]                                   (M:1009-1017)
 *   c_edges  [P*H, n_ratios*W, 1]  row p, column k: gx^2 + gy^2 > ratios[k], gx = (m[y][x] - m[y][x+1]) / 4, gy likewise along y,
 *                                  zero beyond the border: edge_set(m, 1, r) (N:1401-1404) on the stencil of N:1366-1390
 *   c_heat   [gp*H, gp*W, 3]       p_heatmap: table[rint(255 m)] (half to even, clamped to 0..255), P tiles (N:2051-2062)
 *   c_masks  [gp*H, gp*W, 1]       masks: the hard mask, P tiles
 * levels / ratios: HOST arrays of at most 8 floats; table: uint8 [256,3] DEVICE, already quantised by the host (viridis). */
int ups_canvas_first_item(const float* m, const float* hard, const uint32_t* bits, int32_t H, int32_t W, int32_t P, const float* levels,
                          int32_t n_levels, const float* ratios, int32_t n_ratios, const uint8_t* table, uint8_t* c_levels,
                          uint8_t* c_edges, uint8_t* c_heat, uint8_t* c_masks, void* stream);

/* ---------------------------------------------------------------- device-resident training data (csrc/dataset.hip)
 * The batch views of eddata's StochasticPairs / AugmentedPair2 (cub/code/data/data.py:157-175) gathered from a uint8 image store that
 * stays in device memory, instead of decoded, flipped, normalised and stacked on the host every step.
 *   images [n_images, S, S, 3] uint8 (every image already resized to S x S);  plan [B, 3] int32, DEVICE: source image of view0, source
 *   image of view1, flip bits (bit 0 horizontal, bit 1 vertical: one draw flips both views);  view0, view1, target [B, S, S, 3] fp32.
 *     view0[b][y][x][c] = target[b][y][x][c] = lut(images[plan[b][0]][fv ? S-1-y : y][fh ? S-1-x : x][c])
 *     view1[b][y][x][c] =                      lut(images[plan[b][1]][the same source pixel][c])
 *     lut(u) = float(u) / 127.5f - 1.0f in fp32, two correctly rounded operations: NumPy's `np.float32(u) / 127.5 - 1.0` bit for bit.
 * Channels are never reversed.  target may be NULL (StochasticPairs has no view0_target); it is stored from view0's registers.
 * UPS_E_ARG, nothing launched: B <= 0, S <= 0, n_images <= 0, a NULL required pointer, B * S * S * 3 > 2^31 - 1.  The caller
 * validates the plan's indices (it wrote them); an index outside [0, n_images) reads nothing and writes that item as NaN.
 * S % 4 == 0 with a 4-byte aligned store and 16-byte aligned outputs runs four pixels per lane (dword loads, float4 stores); any other
 * shape or alignment one pixel per lane.  No scratch, no atomics: the same plan gives the same bits. */
int ups_gather_views(const uint8_t* images, int64_t n_images, const int32_t* plan, int32_t B, int32_t S, float* view0, float* view1,
                     float* target, void* stream);

/* ---------------------------------------------------------------- device-side augmentation of the training data (csrc/augment.hip)
 * AugmentedPair2's appearance and shape pipelines (cub/code/data/data.py:57-154, restated in augment.py) executed on the uint8 store of
 * ups_gather_views from realisations the HOST has drawn (augment.draw_appearance / draw_shape): one record of
 * ups_augment_record_words() int32 words per output image (layout: the R_* constants of csrc/augment.hip = data.REC_*).  Added without
 * a new UPS_ABI_VERSION: no struct changed, and a binding that expects these symbols fails to load an older library by name.
 *   images  [n_images, S, S, 3] uint8;   records [n, words] int32, DEVICE, n = 3 B (target given) or 2 B: image r * B + b is role r
 *   (0 view0, 1 view1, 2 target) of item b;   luts [2, 256] uint8, DEVICE: T_in, T_mid (the host's truncating uint8 round trips);
 *   field [n_fields, 2, S, S] fp32 from ups_augment_field (dx, dy), may be NULL when n_fields == 0;
 *   scratch_a, scratch_b [n, S, S, 3] uint8 (caller-owned, overwritten);   view0, view1, target [B, S, S, 3] fp32, target may be NULL.
 * value chain: store byte (plan flips) -> T_in -> filter, three colour ops, gray, perm -> T_mid (records with the `mid` flag) ->
 * hflip, affine warp -> grid or elastic warp -> v * 2 / 255 - 1.  Every warp: fp32 source coordinates, clamped to [0, S-1], floored,
 * a + (b - a) * f along x then y, rintf and clip to uint8.  Bit-equal to tests/devaug_ref.py's float32 NumPy restatement.
 * passes: bit 0 pass 1 (-> scratch_a), bit 1 pass 2 (scratch_a -> scratch_b), bit 2 pass 3 (scratch_b -> views); 7 runs all (the
 * single passes exist for timing).  UPS_E_ARG, nothing launched: B <= 0, S <= 0, n_images <= 0, n_fields < 0, a NULL required pointer,
 * passes outside 1..7, 3 B > 65535.  A record with a source image, field index or op code out of range reads nothing and gives a NaN image. */
int32_t ups_augment_record_words(void);
int ups_augment_views(const uint8_t* images, int64_t n_images, const int32_t* records, const uint8_t* luts, const float* field,
                      int32_t n_fields, int32_t B, int32_t S, uint8_t* scratch_a, uint8_t* scratch_b, float* view0, float* view1,
                      float* target, int32_t passes, void* stream);
/* The elastic displacement fields: noise [n_fields, 2, S, S] fp32 -> field, through tmp of the same size.  Separable Gaussian of 401
 * taps (weights: DEVICE, fp32, sigma 50 / radius 200, normalised in float64 on the host), scipy `reflect` border repeated as often as the
 * radius needs, axis 0 first, the accumulator starting at 0 and adding taps 0 .. 400 in order, contraction off.
 * UPS_E_ARG: n_fields <= 0, S <= 0, a NULL pointer, 2 n_fields > 65535. */
int ups_augment_field(const float* noise, const float* weights, int32_t n_fields, int32_t S, float* tmp, float* field, void* stream);

/* ---------------------------------------------------------------- part-IoU evaluation (csrc/evalparts.hip)
 * The per-image joint histogram of inferred part and ground-truth label: the sufficient statistic of the protocol of
 * eval_01.py:229-383 (evalutil.evaluate_from_counts).
 * counts[i][p][g] += #{pixels k of image i : pred[i][k] == p and lut[gt[i][k]] == g}      (lut == NULL: identity)
 * pred   [N, HW] int64   arg-max map of ups_part_softmax_fwd (8-byte aligned; 16-byte loads where the address allows)
 * gt     [N, HW] uint8   ground-truth labels as stored (any alignment)
 * lut    [256]   uint8   DEVICE, raw label -> evaluated label (the reference's dp_remap_dict), or NULL
 * counts [N, P, G] int32, caller-zeroed or holding earlier launches' counts: the kernel only adds
 * invalid [1] int32: += number of pixels with pred outside [0,P) or mapped label >= G; such pixels touch no count
 * 1 <= P <= 32, 1 <= G <= 32, else UPS_E_UNSUPPORTED.  UPS_E_ARG: a NULL required pointer, N <= 0, HW <= 0, HW > 2^31 - 1.
 * Integer atomics only: the result does not depend on launch geometry or on the order in which blocks finish.
 * The kernel takes the arg-max map and never recomputes it from logits: out_parts_hard is the first maximal index of the fp32
 * soft-max, where two different logits can round to a tie that they would not have as logits -- a fused arg-max + confusion form
 * would not be bit-equal to the host evaluation, so there is none. */
int ups_part_confusion(const int64_t* pred, const uint8_t* gt, const uint8_t* lut, int32_t N, int64_t HW, int32_t P, int32_t G,
                       int32_t* counts, int32_t* invalid, void* stream);

/* ---------------------------------------------------------------- label-free validation metrics (csrc/valmetrics.hip)
 * Added without a new UPS_ABI_VERSION, as the ups_augment_* entries: no struct changed, and a binding that expects these symbols fails
 * to load an older library by name.  The reference has no validation: the definitions here are the specification.
 *
 * ups_image_metrics: per-image error sums and SSIM sum of two image batches.
 *   a, b   [N, H, W, ld] NHWC, each with its own dtype (UPS_F32 | UPS_BF16) and its own ld >= 3; channels 0..2 are R, G, B, the rest
 *          is never read.  No alignment beyond the element's is assumed (ld = 3 fp32 rows are not 16-byte aligned).
 *   weights  HOST array of the 11 normalised fp64 weights of the separable Gaussian window (sigma 1.5 in Wang et al. 2004; the
 *          caller's numbers are used as they are, so a host restatement multiplies by the same values)
 *   out    double [N, 3] = (sse, sae, ssim_sum) per image, written completely
 *   scratch  ups_image_metrics_scratch_bytes(N, H, W) bytes, 8-byte aligned, caller-owned, overwritten
 * All arithmetic is fp64 on the source values: x = clamp((v + 1) / 2, 0, 1); sse = sum (x - y)^2, sae = sum |x - y| over the 3 H W
 * values; SSIM per channel over the VALID region (H - 10) x (W - 10), no padding: mu = sum w x, var_x = sum w x^2 - mu_x^2,
 * cov = sum w x y - mu_x mu_y (no unbiased correction), C1 = 0.01^2, C2 = 0.03^2,
 *   map = (2 mu_x mu_y + C1) (2 cov + C2) / ((mu_x^2 + mu_y^2 + C1) (var_x + var_y + C2)),   ssim_sum = sum of map over the valid
 * pixels and the three channels.  No floating-point atomics: one partial per block in `scratch`, added in index order by a second
 * launch -- two calls on the same inputs give the same bits.
 * UPS_E_ARG, nothing launched: a NULL pointer, ld < 3, another dtype, N <= 0, H < 11 or W < 11, or 3 * N * tiles > 2^31 - 1 with
 * tiles = ceil((H-10) / T) * ceil((W-10) / T), T = ups_image_metrics_tile() (then ups_image_metrics_scratch_bytes returns 0). */
int32_t ups_image_metrics_tile(void);
size_t ups_image_metrics_scratch_bytes(int32_t N, int32_t H, int32_t W);
int ups_image_metrics(const void* a, int32_t dtype_a, int32_t lda, const void* b, int32_t dtype_b, int32_t ldb, int32_t N, int32_t H,
                      int32_t W, const double* weights, double* out, void* scratch, void* stream);
/* ups_part_usage: per-image part areas and mask sharpness.
 *   soft   [N, HW, P] fp32  the soft-max of ups_part_softmax_fwd (out_parts_soft);   pred [N, HW] int64  its arg-max map
 *   counts [N, P] int32, caller-zeroed or holding earlier launches' counts: += #{pixels k of image i : pred[i][k] == p}
 *   invalid [1] int32: += number of pixels with pred outside [0, P); such a value is never used as an index
 *   sharp  double [N, 2] = (sum_k max_p soft, sum_k -sum_p s ln s with 0 ln 0 = 0), fp64, natural log, written completely
 *   scratch  ups_part_usage_scratch_bytes(N, HW) bytes, 8-byte aligned, caller-owned, overwritten
 * Integer atomics for the counts; `sharp` by per-block partials added in index order (same bits on every call).  One block per
 * chunk of ups_part_usage_chunk() pixels.  P > 32: UPS_E_UNSUPPORTED (the caller counts on the host).  UPS_E_ARG: a NULL pointer,
 * N <= 0, P < 1, HW <= 0, HW > 2^31 - 1, 2 * N * chunks > 2^31 - 1. */
int32_t ups_part_usage_chunk(void);
size_t ups_part_usage_scratch_bytes(int32_t N, int64_t HW);
int ups_part_usage(const float* soft, const int64_t* pred, int32_t N, int64_t HW, int32_t P, int32_t* counts, int32_t* invalid,
                   double* sharp, void* scratch, void* stream);

/* ---------------------------------------------------------------- segmentation export (csrc/segexport.hip)
 * Added without a new UPS_ABI_VERSION, as the ups_augment_* entries: no struct changed, and a binding that expects these symbols fails
 * to load an older library by name.  The reference never renders a part map above the model's resolution: the definitions here are
 * the specification (tests/segexport_ref.py restates them in NumPy float64, and the bytes are equal).
 *
 * ups_segment_render: one launch renders n images, image i at its own size h_i x w_i, from the soft-max maps.
 *   soft   [n, S, S, P] fp32, contiguous, finite: out_parts_soft (ups_part_softmax_fwd)
 *   table_host / table  [n, ups_segment_table_words() = 4] int32 rows (pixel_offset, h, w, first_block): the SAME numbers on the host
 *          (read by the launcher's checks) and on the device (read by the kernel).  pixel_offset: where image i starts in every packed
 *          plane, a multiple of 16, ascending, images not overlapping; first_block: the sum over the images before i of
 *          ceil(h * w / ups_segment_chunk())
 *   total  pixels of each packed plane: every pixel_offset + h * w <= total <= 2^31 - 1
 *   src    uint8 [total, 3] packed RGB source images at the output sizes, or NULL;   colors  uint8 [P, 3] (required with overlay)
 *   labels uint8 [total], overlay uint8 [total, 3], confidence uint8 [total]: each may be NULL (skipped); only the h * w pixels of
 *          each image are written, the alignment gaps between images keep their bytes
 *   counts int32 [n, P] or NULL, caller-zeroed or holding earlier launches' counts: += #{pixels of image i with label p}
 * For output pixel (y, x):  sy = ((y + 0.5) * S) / h - 0.5 clamped to [0, S-1], y0 = floor(sy), y1 = min(y0 + 1, S-1), fy = sy - y0
 * (x alike);  v_p = (1-fy) ((1-fx) a00 + fx a01) + fy ((1-fx) a10 + fx a11) in fp64 on the fp32 values, no contraction;
 * label = first p with maximal v_p;  confidence = clamp(floor(v_label * 255 + 0.5), 0, 255);
 * overlay_c = clamp(floor(alpha * colors[label][c] + (1 - alpha) * src_c + 0.5), 0, 255), or colors[label][c] when src is NULL.
 * The same formula shrinks (h < S) without antialiasing; at h = w = S the label is the first maximal index of soft itself.
 * Integer atomics only (an LDS histogram per block, one global add per block and part).
 * UPS_E_UNSUPPORTED: P > 255.  UPS_E_ARG, nothing launched: P < 1, n < 1, S < 1, S * S * P >= 2^29, a NULL soft or table, all four outputs NULL, overlay
 * without colors, alpha outside [0, 1], h or w < 1, a pixel_offset that is negative, no multiple of 16, not ascending or past total, a
 * first_block that is not the prefix sum, a plane, src or counts pointer that is not 4-byte aligned. */
int32_t ups_segment_chunk(void);
int32_t ups_segment_table_words(void);
int ups_segment_render(const float* soft, int32_t n, int32_t S, int32_t P, const int32_t* table_host, const int32_t* table,
                       int64_t total, const uint8_t* src, const uint8_t* colors, double alpha, uint8_t* labels, uint8_t* overlay,
                       uint8_t* confidence, int32_t* counts, void* stream);

/* Edge-aware refinement of the export: joint bilateral upsampling guided by the photograph (Kopf et al. 2007).  Added by name, without
 * a new UPS_ABI_VERSION, as the entries above.  The definitions are DESIGN.md section 8's; tests/segrefine_ref.py restates them in
 * NumPy with equal bytes.  Two launches per pass of n images, tables and planes as for ups_segment_render (the same table checks):
 * ups_segment_guide: guide uint8 [n, S, S, 3], the low-resolution photograph.  Tap t of an axis of extent e covers the source indices
 *   [a, b), a = (t e) / S, b = max(a + 1, ((t + 1) e) / S) (integer division; never empty, also when e < S), and
 *   guide[i, ty, tx, c] = (2 sum + cnt) / (2 cnt) over the cnt source pixels of the tap's rows x columns: integer arithmetic only.
 * ups_segment_render_guided: ups_segment_render with the four bilinear taps replaced by the (2R+2)^2 window ty = y0 + j, tx = x0 + k,
 *   j, k = -R .. R+1 (j outer, ascending; y0, fy, x0, fx as above; a tap outside [0, S-1] is SKIPPED, not repeated):
 *     wy = 1 - |fy - j| / (R + 1), wx alike;  d1 = sum_c |src[y, x, c] - guide[ty, tx, c]| (0 .. 765);  w = (wy wx) range_w[d1];
 *     den += w;  num_p += w soft[ty, tx, p]   (fp64 from 0.0, every operation rounded once, each num_p its own chain in tap order)
 *     label = first p of maximal num_p;  confidence = clamp(floor((num_label / den) * 255 + 0.5), 0, 255);  overlay, counts as above.
 *   src (packed, at the output sizes), guide (of ups_segment_guide on the same src) and range_w are REQUIRED;  0 <= R <= 3.
 *   range_w: 766 doubles ON THE DEVICE, 8-byte aligned, built by the host: max(exp(-(d/3)^2 / (2 sigma^2)), 2^-64) for d = 0 .. 765,
 *   sigma in uint8 levels of mean absolute channel difference.  The floor keeps den > 0; the kernel evaluates no transcendental.
 * Integer atomics only.  Status codes as ups_segment_render's (UPS_E_UNSUPPORTED: P > 255); also UPS_E_ARG for a NULL src, guide or
 * range_w, R outside 0 .. 3, n * S > 2^31 - 1 (the guide's grid) and a range_w that is not 8-byte aligned. */
int ups_segment_guide(const uint8_t* src, int32_t n, int32_t S, const int32_t* table_host, const int32_t* table, int64_t total,
                      uint8_t* guide, void* stream);
int ups_segment_render_guided(const float* soft, int32_t n, int32_t S, int32_t P, const int32_t* table_host, const int32_t* table,
                              int64_t total, const uint8_t* src, const uint8_t* guide, const double* range_w, int32_t R,
                              const uint8_t* colors, double alpha, uint8_t* labels, uint8_t* overlay, uint8_t* confidence,
                              int32_t* counts, void* stream);

/* ---------------------------------------------------------------- part coherence (csrc/components.hip)
 * Connected components of integer label maps, their sizes, per-part statistics and one round of speck clean-up.  Added by name,
 * without a new UPS_ABI_VERSION, as the entries above.  Everything is integer arithmetic; these definitions are the specification
 * (DESIGN.md section 8 "Part coherence"; tests/components_ref.py restates them twice in NumPy and the device results are equal).
 *
 * Images and tables.  A launch covers n <= 65535 images, image i of its own size (h_i, w_i), 1 <= h w <= 2^20, packed into planes of
 *   `total` elements by the table of ups_segment_render (table_host / table, 4 words per image, the same checks).
 * Labels.  `labels` is uint8 [total] (label_bytes = 1) or int64 [total] (label_bytes = 8).  A pixel is VALID if 0 <= label < P,
 *   1 <= P <= 255.  An invalid pixel belongs to no component and is never a neighbour.
 * Adjacency.  conn = 4: pixels that share an edge; conn = 8: an edge or a corner.  Always inside one image: x = w - 1 is not adjacent
 *   to x = 0 of the next row, and no pixel of image i is adjacent to one of image i + 1.
 * Components.  Two valid pixels of equal label are in one component if a chain of adjacent pixels of that label joins them.
 *   comp int32 [total]: the smallest in-image index y w + x of the pixel's component; -1 at an invalid pixel; the alignment gaps are
 *   not written.  A function of the map alone: two launches give the same bytes.
 *   err int32 [1]: |= 1 when a label-chasing loop reached its bound (h w steps of a find, 2 h w retries of a union): a bug, never
 *   expected.  The caller reads it when it next synchronises.  scratch: ups_label_components_scratch_bytes(total) = 0 bytes (comp is the
 *   union-find's parent array); may be NULL.
 * Sizes and statistics (ups_label_component_stats; comp is ups_label_components' of the same labels).
 *   area int32 [total]: the pixel count of the pixel's component, 0 at an invalid pixel.
 *   stats int32 [n, P, 4], ADDED to (caller-zeroed or accumulating): [0] += the pixels of part p, [1] += its components,
 *   [2] = max(itself, the area of its largest component), [3] += its components with area < small (small >= 0).
 *   invalid int32 [1] += the invalid pixels.  scratch: ups_label_component_stats_scratch_bytes(total) = 4 total bytes, 4-byte aligned.
 * Clean-up, one round (ups_label_components_clean; comp and area as above), threshold min_area >= 1.
 *   A component is SMALL if area < min_area.  For a small component c of part p, votes[q] counts the ordered pairs (pixel k of c, one
 *   of k's FOUR edge neighbours k' inside the image -- whatever conn was) with k' valid, the component of k' not small and
 *   label[k'] = q.  If the largest vote is positive every pixel of c takes the first q of maximal vote; otherwise c keeps its label.
 *   All decisions are taken from the input map.  out (the width of labels; out == labels is allowed) equals the input everywhere
 *   else, invalid values included; the gaps are not written.  changed int32 [1] += the pixels whose label changed.
 *   src, colors, overlay, confidence, counts: each may be NULL.  A relabelled pixel's overlay is blended anew from src with
 *   ups_segment_render's blend (colors alone when src is NULL; colors is required with overlay), its confidence byte becomes 0, and
 *   counts[i, old] -= 1, counts[i, new] += 1.
 *   scratch: ups_label_components_clean_scratch_bytes(total) = 12 total bytes, independent of P: one vote counter and a running
 *   (best vote, best q) pair per element, one pass per part.
 * UPS_E_UNSUPPORTED: P > 255.  UPS_E_ARG, nothing launched: a NULL required pointer, label_bytes not 1 or 8, n outside 1 .. 65535,
 * P < 1, conn not 4 or 8, small < 0, min_area < 1, h w > 2^20, a table ups_segment_render refuses, overlay without colors, alpha
 * outside [0, 1], int64 labels or out that are not 8-byte aligned. */
int32_t ups_components_tile(void);
size_t ups_label_components_scratch_bytes(int64_t total);
size_t ups_label_component_stats_scratch_bytes(int64_t total);
size_t ups_label_components_clean_scratch_bytes(int64_t total);
int ups_label_components(const void* labels, int32_t label_bytes, int32_t n, const int32_t* table_host, const int32_t* table,
                         int64_t total, int32_t P, int32_t conn, int32_t* comp, int32_t* err, void* scratch, void* stream);
int ups_label_component_stats(const void* labels, int32_t label_bytes, const int32_t* comp, int32_t n, const int32_t* table_host,
                              const int32_t* table, int64_t total, int32_t P, int32_t small, int32_t* area, int32_t* stats,
                              int32_t* invalid, void* scratch, void* stream);
int ups_label_components_clean(const void* labels, int32_t label_bytes, const int32_t* comp, const int32_t* area, int32_t n,
                               const int32_t* table_host, const int32_t* table, int64_t total, int32_t P, int32_t min_area, void* out,
                               int32_t* changed, const uint8_t* src, const uint8_t* colors, double alpha, uint8_t* overlay,
                               uint8_t* confidence, int32_t* counts, void* scratch, void* stream);

/* ---------------------------------------------------------------- run-length annotations (csrc/segrle.hip)
 * COCO run-length encoding of the label planes of the segmentation export, for every image and part at once.  Added by name, without
 * a new UPS_ABI_VERSION, as the entries above.  Integer arithmetic only; these definitions are the specification (DESIGN.md section 8
 * "Run-length annotations"; tests/segrle_ref.py restates them twice and the device results are equal).
 *
 * Inputs.  Planes, images and the table are ups_segment_render's (the same checks), with the limits of the components kernels:
 *   n <= 65535 images, 1 <= h w <= 2^20 each, labels uint8 [total], 1 <= P <= 255.  A pixel with label >= P belongs to no part.
 *   The alignment gaps between images are never read.
 * Mask and order.  For image i (h x w at pixel offset off_i) and part p, in COCO's column-major order:
 *   m[k] = (labels[off_i + y w + x] == p),  k = x h + y,  0 <= k < h w.
 * Transitions.  T = the ascending positions k with m[k] != m[k-1], taking m[-1] = 0 (never the previous image's last pixel).
 * Counts.  [T0, T1 - T0, .., h w - T_last], and [h w] when T is empty: COCO's uncompressed counts, alternating runs that begin with
 *   a run of zeros (0 when m[0] = 1); |T| + 1 entries whose sum is h w.
 * Outputs.
 *   offsets int64 [n P + 1]   the exclusive prefix sum of the lists' lengths in (image, part) order; offsets[n P] is the total
 *   counts  int32 [offsets[n P]]  the lists, concatenated in (image, part) order
 *   area    int32 [n, P]      the pixels of the part: WRITTEN, not added (equal to ups_segment_render's counts)
 *   bbox    int32 [n, P, 4]   (x_min, y_min, x_max - x_min + 1, y_max - y_min + 1); (0, 0, 0, 0) for a part without a pixel
 *   Functions of the label plane alone: two launches give the same bytes.
 * Two calls.  ups_segment_rle_count writes offsets, area and bbox and leaves per-chunk write positions in `scratch`
 *   (ups_segment_rle_scratch_bytes(n, total, P) bytes, 8-byte aligned; a chunk is ups_segment_rle_chunk() = 1024 positions k).  The
 *   caller reads the one int64 offsets[n P], allocates counts, and calls ups_segment_rle_write with the SAME labels, table, offsets
 *   and scratch: n_counts is the offsets[n P] it read, capacity the int32 elements it allocated.  No block waits for another block:
 *   positions come from a scan over separate launches, never from the order in which atomics land (area and bbox alone use integer
 *   atomics).  The write kernel stores nothing at or beyond `capacity`, whatever offsets holds.
 * UPS_E_UNSUPPORTED: P > 255.  UPS_E_ARG, nothing launched: a NULL required pointer, n outside 1 .. 65535, P < 1, h w > 2^20, a table
 * ups_segment_render refuses, offsets or scratch not 8-byte aligned, counts, area or bbox not 4-byte aligned, n_counts < 1 or
 * capacity < n_counts. */
int32_t ups_segment_rle_chunk(void);
size_t ups_segment_rle_scratch_bytes(int32_t n, int64_t total, int32_t P);
int ups_segment_rle_count(const uint8_t* labels, int32_t n, const int32_t* table_host, const int32_t* table, int64_t total, int32_t P,
                          int64_t* offsets, int32_t* area, int32_t* bbox, void* scratch, void* stream);
int ups_segment_rle_write(const uint8_t* labels, int32_t n, const int32_t* table_host, const int32_t* table, int64_t total, int32_t P,
                          const int64_t* offsets, const void* scratch, int32_t* counts, int64_t capacity, int64_t n_counts,
                          void* stream);

/* ---------------------------------------------------------------- part-appearance index (csrc/partindex.hip)
 * Nearest neighbours and k-means on a bank of per-part appearance codes (TrainModel.encode_parts): what deepfashion/code/eval/eval_02's
 * make_clusters does off-line with scikit-learn.  Restated in NumPy float64 by tests/partindex_ref.py with equal bits.
 *   bank      feat [N, P, A] fp32, finite (no alignment beyond the element's is assumed); valid [N, P] uint8: an entry with valid == 0
 *             (an absent part: it has a code, but no meaning) is never a query, a neighbour or a cluster member
 *   distance  d(x, y) = sum_{a = 0 .. A-1} (double(x_a) - double(y_a))^2: fp64, accumulated in ascending a from 0.0, every
 *             subtraction, multiplication and addition rounded once (no contraction), so a loop over a in NumPy gives the same bits.
 *             There is NO matrix-core form |x|^2 + |y|^2 - 2 x.y: it is not bit-equal to any restatement and it cancels for close
 *             codes.  No distance matrix is written.
 * ups_part_knn: for a valid query (q, p) the K items g with gvalid[g, p] (and g != q when exclude_same_index) that are smallest in
 *   the total order (d, g) -- distance, then gallery index -- in that order: idx [Nq, P, K] int32, dist [Nq, P, K] double.  Slots
 *   beyond the number of eligible items, and every slot of an invalid query, are -1 / +inf.  Both outputs are written completely.
 * ups_part_kmeans_step: cent [P, k, A] double.  label [N, P] int32 = the FIRST j with minimal d(feat[n, p], cent[p, j]), -1 where
 *   invalid; mind [N, P] double = that distance, +inf where invalid (both written completely).  prev_label [N, P] or NULL: changed [1]
 *   int32 (required with prev_label) += #{label != prev_label}.  counts [P, k] int32 += the members (integer atomics: caller-zeroed),
 *   sums [P, k, A] double = the members' codes, converted to double and added, inertia [P] double = sum of mind over the valid items
 *   (both written).  Floating-point sums use no atomics: one partial per block of ups_part_kmeans_chunk() items (members in index
 *   order) in `scratch` (ups_part_kmeans_scratch_bytes, overwritten before it is read), added in block order by a second launch:
 *   two calls give the same bits.  counts, sums and inertia may be NULL together (assignment only; scratch may then be NULL too).
 *   The new centroid, sums / counts in fp64 with an empty cluster keeping its own, is the caller's.
 * ups_part_knn_tile(): queries per block = gallery items per staged tile;  ups_part_kmeans_chunk(): items per block.
 * UPS_E_UNSUPPORTED: K > 32, k > 64, A > 512.  UPS_E_ARG, nothing launched: a NULL required pointer, Nq, Ng, N, P, A, K or k < 1,
 * Nq P A, Ng P A, Nq P K, N P A, P k A or the scratch index past 2^31 - 1, counts / sums / inertia given only in part, sums without
 * scratch, prev_label without changed.  ups_part_kmeans_scratch_bytes returns 0 for sizes the step refuses. */
int32_t ups_part_knn_tile(void);
int32_t ups_part_kmeans_chunk(void);
int ups_part_knn(const float* q, const uint8_t* qvalid, int32_t Nq, const float* g, const uint8_t* gvalid, int32_t Ng, int32_t P,
                 int32_t A, int32_t K, int32_t exclude_same_index, int32_t* idx, double* dist, void* stream);
size_t ups_part_kmeans_scratch_bytes(int32_t N, int32_t P, int32_t A, int32_t k);
int ups_part_kmeans_step(const float* feat, const uint8_t* valid, int32_t N, int32_t P, int32_t A, const double* cent, int32_t k,
                         const int32_t* prev_label, int32_t* label, double* mind, int32_t* counts, double* sums, double* inertia,
                         int32_t* changed, void* scratch, void* stream);

/* ---------------------------------------------------------------- landmark regression evaluation (csrc/landmarks.hip)
 * Part centres, a per-keypoint ridge fit from the centres to annotated keypoints, and its predictions: the evaluation the part-discovery
 * papers report on CUB and PennAction.  The reference does not have it: the definitions here are this project's own (DESIGN.md
 * section 8; tests/landmarks_ref.py restates all four entries in NumPy float64, and the bits are equal).  Added by name, without a new
 * UPS_ABI_VERSION, as the entries above.  Everything is fp64 with every multiplication, addition, division and square root rounded
 * once (no contraction), no floating-point atomics, every order of summation fixed: two calls give the same bits.
 * ups_part_moments: mass and centre of every part of every image.
 *   soft   [N, h, w, P] fp32  out_parts_soft;   pred [N, h, w] int64, its arg-max map, or NULL (hard and invalid are then not touched)
 *   mass   [N, P] double = sum over the pixels of s = double(soft);   centre [N, P, 2] double = (sum s u_x / mass, sum s u_y / mass) with
 *          u_x = double(2x + 1 - w) / double(w), u_y = double(2y + 1 - h) / double(h): pixel centres on [-1, 1], each product rounded
 *   valid  [N, P] uint8 = mass is finite, > 0 and >= min_mass; where it is 0 the centre is (0, 0).  mass, centre, valid: written completely
 *   hard   [N, P, 3] int32, caller-zeroed or holding earlier launches' sums: += (count, sum (2x + 1 - w), sum (2y + 1 - h)) over the
 *          pixels with pred == p (integer atomics);  invalid [1] int32 += pixels with pred outside [0, P), which touch no sum
 *   scratch  ups_part_moments_scratch_bytes(N, h, w, P) bytes, 8-byte aligned, caller-owned, overwritten before it is read
 *   The float sums: one partial per block of ups_part_moments_chunk() consecutive pixels of one image (pixels past the end are zeros).
 *   With Pp = the power of two >= P and G = chunk / Pp, group g adds its pixels g Pp .. g Pp + Pp - 1 in ascending order from 0.0,
 *   then t[g] += t[g + s] for s = G/2, G/4 .. 1.  A second launch adds the partials in block order from 0.0 and divides.
 *   UPS_E_UNSUPPORTED: P > 32.  UPS_E_ARG, nothing launched: a NULL soft, mass, centre, valid or scratch, pred without hard and
 *   invalid, N, h, w or P < 1, a NaN min_mass, h w > 2^20 or h w max(h, w) > 2^31 - 1 (the integer sums of one image stay in int32),
 *   3 P N chunks > 2^31 - 1.  ups_part_moments_scratch_bytes returns 0 for sizes the entry refuses.
 * ups_landmark_gram: the normal equations per keypoint.  f_n = (feat[n, 0 .. D-2], 1): the kernel appends the constant itself.
 *   feat [N, D-1] double;  target [N, K, 2] double;  vis [N, K] uint8 (a target with vis == 0 is never read: it may hold anything)
 *   G [K, D, D] = sum_{n: vis[n, k]} f_a f_b (the full matrix; symmetric in bits), R [K, D, 2] = sum f_a target[n, k, c], cnt [K] int32 =
 *   the visible items: all written completely.  Within a block of ups_landmark_chunk() items the sum runs over ascending n from 0.0 and
 *   SKIPS the invisible items; the block partials go to scratch (ups_landmark_gram_scratch_bytes(N, D, K)) and a second launch adds them
 *   in block order from 0.0.
 * ups_landmark_solve: W [K, D, 2] double, written completely: (G_k + lambda diag(1, .., 1, 0)) W_k = R_k, the bias row not penalised
 *   (A[a][a] = G[a][a] + lambda, a < D - 1: one rounded addition).  Cholesky by columns j = 0 .. D-1:
 *     L[j][j] = sqrt(A[j][j] - sum_{m<j} L[j][m] L[j][m]);  L[i][j] = (A[i][j] - sum_{m<j} L[i][m] L[j][m]) / L[j][j], i > j
 *   each a subtraction chain in ascending m that starts from A's element, each product rounded; then per coordinate c
 *     y[i] = (R[i][c] - sum_{m<i} L[i][m] y[m]) / L[i][i]   (chain in ascending m),   i ascending
 *     W[i][c] = (y[i] - sum_{m>i} L[m][i] W[m][c]) / L[i][i]   (chain in DESCENDING m from D-1),   i descending.
 *   A keypoint with cnt <= 0, or with a pivot A[j][j] - sum that is not positive or not finite, gets W_k = 0 and adds 1 to the DEVICE
 *   counter *n_singular (int32, the caller's; never reset here), as ups_tps_solve does.  One block per keypoint, one launch.
 * ups_landmark_predict: pred [N, K, 2] = sum_a f_a W[k, a, c], over ascending a from 0.0, each product rounded (the last is 1 W).
 *   target, vis and d2 are given together or all NULL: d2 [N, K] = dx dx + dy dy with d = pred - target where vis, -1 where not.
 *   Both outputs are written completely.  The square root, the means and the PCK counts are the host's.
 * D <= 65 and K <= 32, else UPS_E_UNSUPPORTED (gram, solve, predict).  UPS_E_ARG, nothing launched: a NULL required pointer (feat may
 * be NULL at D = 1), N, D or K < 1, lambda negative or not finite, target / vis / d2 given only in part, 2 N K, N D or the scratch
 * index past 2^31 - 1.  ups_landmark_gram_scratch_bytes returns 0 for sizes the entry refuses. */
int32_t ups_part_moments_chunk(void);
size_t ups_part_moments_scratch_bytes(int32_t N, int32_t h, int32_t w, int32_t P);
int ups_part_moments(const float* soft, const int64_t* pred, int32_t N, int32_t h, int32_t w, int32_t P, double min_mass, double* mass,
                     double* centre, uint8_t* valid, int32_t* hard, int32_t* invalid, void* scratch, void* stream);
int32_t ups_landmark_chunk(void);
size_t ups_landmark_gram_scratch_bytes(int32_t N, int32_t D, int32_t K);
int ups_landmark_gram(const double* feat, const double* target, const uint8_t* vis, int32_t N, int32_t D, int32_t K, double* G, double* R,
                      int32_t* cnt, void* scratch, void* stream);
int ups_landmark_solve(const double* G, const double* R, const int32_t* cnt, int32_t D, int32_t K, double lambda, double* W,
                       int32_t* n_singular, void* stream);
int ups_landmark_predict(const double* feat, const double* W, int32_t N, int32_t D, int32_t K, const double* target, const uint8_t* vis,
                         double* pred, double* d2, void* stream);

/* ---------------------------------------------------------------- mask priors (M:652-797), fused
 * One pass over l/m per view producing the partial sums, one fused backward producing dl.
 * See csrc/priors.hip for the slot layout of `sums`. */
typedef struct {
    int32_t n, h, w, P;
    int32_t view;                 /* 0: KL + entropy + mumford-shah + area + patch + gmrf ; 1: KL + variance */
    int32_t entropy_ce;           /* 0: entropy_func "entropy", 1: "cross_entropy" (M:671-680) */
    float gamma;
    int32_t half_h, half_w;
    float ms_alpha, ms_lambda;    /* 1.0, 1e-2 hard-coded at M:744-746 */
    float w_kl, w_entropy, w_ms, w_area, w_patch, w_gmrf, w_var;  /* schedule weights at this step */
    const float* l;               /* mean + eps */
    const float* l_mean;          /* view 0 only (gmrf) */
    const float* m;               /* softmax(l) */
    const float* hard;
    const int32_t* px;            /* rectangle centres [n*P][2] */
    float* per_np;                /* [n][P][8] per-(image,part) sums */
    float* sums;                  /* [16] global sums (zeroed by the call) */
    const float* g_hard;          /* upstream gradient w.r.t. the STE hard mask or NULL (bwd) */
    float* dl;                    /* d total / d l_mean (bwd); l = l_mean + eps, so the gmrf term is fused in */
    int32_t variant;              /* 0: cub/pennaction SB_model48i; 1: deepfashion SB_model48c (DF:719-776): no rectangles
                                   * (px may be NULL), view 0 adds w_ms_logits * mean_b sum min(ms_alpha * g(l_mean), ms_lambda)
                                   * (deepfashion/code/nn.py:1388-1391,1451-1455; its sum is returned in sums[2], the patch slot),
                                   * view 1 variance = sum_p (S00^2 + S11^2) of the renormalised, un-masked spatial soft-max */
    float w_ms_logits;
    float* dl_rec;                /* optional (bwd): d(reconstruction loss alone)/d l, i.e. the result of a second call with every
                                   * weight zero -- the encoder_0 key sees this one, decoder_visualize sees `dl` */
} ups_prior_desc;
/* `sums` must hold 16 floats of result followed by scratch; total = ups_prior_sums_floats(n, P). */
size_t ups_prior_sums_floats(int32_t n, int32_t P);
int ups_prior_fwd(const ups_prior_desc* d, void* stream);
int ups_prior_bwd(const ups_prior_desc* d, void* stream);

/* ---------------------------------------------------------------- noise (tf.random_normal of the sampling ops, N:1187, 1431)
 * out[i] ~ N(0, 1), i < n: Philox4x32-10 keyed by `seed`, counter = offset + i / 4, Box-Muller.  A pure function of (seed, offset,
 * i); the caller advances offset by ceil(n / 4) per call. */
int ups_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* ---------------------------------------------------------------- MI critic head (M:159-173 last line, 524-536, 800-834, 855)
 * h_pi, h_al [2B][ld] (K logical channels): the two 512-d embeddings of discriminator_model; rows [0,B) are the joint pairs,
 * [B,2B) the marginal pairs.  logits[i] = <h_pi[i], h_al[i]>; out4 = {0.5 (mean softplus(-joint) + mean softplus(marg)),
 * accuracy ((#joint > 0) + (#marg < 0)) / 2B, mean joint logit (logit_constraint(real=False)), 0}.  Single block: fixed
 * reduction order.  bwd: g_loss / g_mim are DEVICE scalars (NULL = 0), the upstream gradients of out4[0] / out4[2];
 * g_h_pi = dlogit * h_al, g_h_al = dlogit * h_pi (either may be NULL). */
int ups_critic_head_fwd(const void* h_pi, const void* h_al, int32_t dtype, int32_t B, int32_t K, int32_t ld, float* logits,
                        float* out4, void* stream);
int ups_critic_head_bwd(const void* h_pi, const void* h_al, const float* logits, const float* g_loss, const float* g_mim,
                        int32_t dtype, int32_t B, int32_t K, int32_t ld, void* g_h_pi, void* g_h_al, void* stream);

/* ---------------------------------------------------------------- state update (M:28-35, 829-834, 861-866, 890-909, 921-930)
 * stats[6] = {mean joint logit of critic 0 (mim), of critic 1 (independent mim), accuracy 0, accuracy 1, loss_dis0, loss_dis1}
 * (batch means, already averaged over the ranks); old_state / new_state [9] = {avg_acc0, avg_acc1, avg_acc_error, avg_loss_dis0,
 * avg_loss_dis1, avg_mim, avg_independent_mim, loa, lor}.  EMAs: new = decay * old + gain * value (value of avg_acc_error =
 * acc1 - acc0); loa' = max(loa + loa_lr (mim - loa_target), 0) when update_loa, lor' = clip(lor + lor_lr (ind - lor_target),
 * lor_min, lor_max) when update_lor, else copied.  One launch, every product and sum rounded on its own. */
int ups_state_update(const float* stats, const float* old_state, float* new_state, float decay, float gain,
                     int32_t update_loa, float loa_lr, float loa_target, int32_t update_lor, float lor_lr,
                     float lor_target, float lor_min, float lor_max, void* stream);

/* ---------------------------------------------------------------- the critics' towers as grouped launches (M:159-173, round 5)
 * discriminator_model is two towers of nin -> (L - 2) x residual_block(k = 1) -> nin on [M = 2B, 512] rows; the three critics of a
 * step are six such towers.  ups_towers_fwd runs layer l of EVERY tower in one launch (L launches), ups_towers_bwd the input
 * gradients likewise (L - 1 launches, + 1 where a tower's first input wants its gradient) and EVERY weight / bias gradient of every
 * tower and layer in one more -- instead of T * L generic convolution calls (each a split-K GEMM + epilogue launch) per direction.
 * UPS_BF16 only, leaky-ReLU, post-activation storage as ups_conv_desc.out_act / res_act describe it: acts[t * L + l] holds
 * lrelu(x) for l < L - 1 (the next layer activates its input) and the plain value for the last layer; a residual layer adds the x it
 * recovers from its stored input.  Requirements (else UPS_E_ARG): k % 32 == 0, n % 128 == 0, square residual layers, T <= 8, L <= 6.
 *   layers  [T * L], tower-major.  w_fwd / w_dgrad: ups_weight_prep's blocked-K copies of the 1x1 kernel; bias [n] or NULL;
 *           grad_w [k][n] (HWIO of a 1x1 kernel) / grad_b [n]: OVERWRITTEN by ups_towers_bwd(want_wgrad = 1); grad_w NULL skips the layer
 *   x0, ld0 [T]: the towers' inputs [M][ld0] (plain values);  acts [T * L]: outputs [M][n] of every layer (caller-owned)
 *   g_out   [T]: gradients w.r.t. the towers' outputs [M][n_last]; a NULL entry leaves that tower out of the call
 *   g_ws    [T * L]: scratch [M][n] per layer (entry l receives the gradient w.r.t. layer l's output; the last entry is unused)
 *   g_x0, ldg0 [T] or NULL: where a tower's input gradient [M][ldg0] is wanted (k of its first layer % 128 == 0) */
typedef struct ups_tower_layer {
    const void*  w_fwd;
    const void*  w_dgrad;
    const float* bias;
    float*       grad_w;
    float*       grad_b;
    int32_t      k, n;
} ups_tower_layer;
int ups_towers_fwd(const ups_tower_layer* layers, int32_t T, int32_t L, const void* const* x0, const int32_t* ld0,
                   void* const* acts, int32_t M, float slope, void* stream);
int ups_towers_bwd(const ups_tower_layer* layers, int32_t T, int32_t L, const void* const* x0, const int32_t* ld0,
                   const void* const* acts, const void* const* g_out, void* const* g_ws, void* const* g_x0,
                   const int32_t* ldg0, int32_t want_wgrad, int32_t M, float slope, void* stream);

/* ---------------------------------------------------------------- full-covariance latent (N:1134-1208, util.py:878-995)
 * params [B][dim + dim(dim+1)/2] fp32.  samples[s][b][i] = mean + L (level[s]*eps[s][b]) ; kl_rows[b][i]. */
/* `level` is a HOST array of S noise levels (S <= 12).  kl_rows may be NULL. */
int ups_latent_fwd(const float* params, const float* eps, const float* level, int32_t S, int32_t B, int32_t dim,
                   float* samples, float* kl_rows, void* stream);
/* g_params = J^T g_samples + gk * d(sum_i kl_rows[b][i])/d params, gk = g_kl_scale * (g_kl_dev ? *g_kl_dev : 1) */
int ups_latent_bwd(const float* params, const float* eps, const float* level, const float* g_samples,
                   const float* g_kl_dev, float g_kl_scale,
                   int32_t S, int32_t B, int32_t dim, float* g_params, void* stream);

/* ---------------------------------------------------------------- optimizer (tf.train.AdamOptimizer, Appendix A.12)
 * p -= lr_t * m / (sqrt(v) + eps) over a flat fp32 buffer; lr_t computed by the caller. */
int ups_adam(float* p, const float* g, float* m, float* v, int64_t count, float lr_t, float beta1, float beta2, float eps,
             float grad_scale, void* stream);
/* same update with the step size read from a device scalar (a captured HIP graph of the step is replayed with new values) */
int ups_adam_dev(float* p, const float* g, float* m, float* v, int64_t count, const float* lr_t_dev, float beta1, float beta2,
                 float eps, float grad_scale, void* stream);

/* ---------------------------------------------------------------- guarded optimizer step (csrc/stepguard.hip)
 * What an optimizer key's gradient is like THIS step, decided and recorded on the device so that Adam can act on it without the host
 * (and a captured HIP graph replays the decision afresh).  Added without a new UPS_ABI_VERSION, as the ups_augment_* entries were: no
 * existing struct changed, and a binding that expects these symbols refuses an older library by name.
 *
 * ups_step_guard: 64 bytes, caller-owned DEVICE memory, 8-byte aligned, zeroed once by the caller; one per optimizer key.  The first five
 * fields are rewritten by every ups_grad_guard, the other three accumulate over its calls.
 *
 * ups_grad_guard(g, count, grad_scale, clip_norm, skip_nonfinite, scratch, rec, max_blocks, stream): two launches.
 *   (a) one fp64 partial and one int32 count per chunk of C = ups_grad_guard_chunk() elements of the flat fp32 bucket g (chunk c covers
 *       elements [c C, min(count, (c + 1) C)); element e of the chunk belongs to slot e % 1024).  A slot adds (double)x * (double)x of its
 *       elements in ascending e, from 0.0; the 1024 slots are folded f[i] = (s[i] + s[i+256]) + (s[i+512] + s[i+768]), i < 256, and the
 *       256 values reduced by the tree `for d = 128, 64, .., 1: f[i] += f[i + d] (i < d)`; the partial is f[0].  The count is the number
 *       of elements whose exponent bits are all ones (NaN, +inf, -inf).  16-byte loads wherever four consecutive elements of a row are
 *       16-byte aligned, single elements in front of and behind them: the values above do not depend on the alignment of g (4 bytes
 *       suffice), on the grid or on max_blocks (0: the default grid; n > 0: at most n blocks, each striding over the chunks).
 *   (b) one block: t[i] = partial[i] + partial[i + 256] + ... (ascending, from 0.0), i < 256, the same tree over t -> sumsq; the counts
 *       are added as integers -> nonfinite.  Then
 *         norm  = sqrt(sumsq) * grad_scale                                  (fp64; grad_scale = 1 / world: the rank-averaged gradient)
 *         scale = clip_norm > 0 ? (float)(clip_norm / max(norm, clip_norm)) : 1     (tf.clip_by_global_norm; a NaN norm gives NaN)
 *         skip  = skip_nonfinite && nonfinite > 0
 *         skip: skipped_total += 1, consecutive += 1;  else: consecutive = 0, and clipped_total += 1 when scale < 1.
 *       With skip_nonfinite == 0 a non-finite gradient gives what the formulas give (an infinite norm: scale 0; a NaN norm: scale NaN
 *       when clipping, else 1).  count == 0: sumsq = norm = 0, scale = 1, skip = 0.
 *   No floating-point atomics: two calls give the same bits.  scratch: ups_grad_guard_scratch_bytes(count) bytes (never 0 for a count
 *   the entry accepts), 8-byte aligned, caller-owned, overwritten.  UPS_E_ARG, nothing launched: a NULL rec or scratch, a NULL g with
 *   count > 0, count < 0 or past 2^28 chunks, g not 4-byte aligned, scratch or rec not 8-byte aligned, clip_norm negative or NaN, a NaN
 *   grad_scale, max_blocks < 0.
 *
 * ups_adam_guarded: ups_adam / ups_adam_dev (lr_t_dev NULL: the step size is lr_t, else *lr_t_dev) with the gradient
 *   gg = (g[i] * grad_scale) * rec->scale; when rec->skip is set the whole grid returns without touching p, m, v.  Both fields are read
 *   from device memory when the kernel runs.  One kernel body with ups_adam: {scale 1, skip 0} gives ups_adam's bits.
 *
 * ups_state_update_guarded: ups_state_update, except that when any of the six stats is non-finite new_state gets old_state's bits and
 *   skipped[0] (total) and skipped[1] (consecutive) advance; otherwise ups_state_update's bits and skipped[1] = 0.  skipped: int64 [2],
 *   DEVICE, zeroed once by the caller. */
typedef struct ups_step_guard {
    double sumsq;            /* this step: sum of squares of the bucket */
    double norm;             /*            sqrt(sumsq) * grad_scale */
    float scale;             /*            the clip factor Adam multiplies the gradient by */
    int32_t skip;            /*            1: Adam leaves p, m, v alone */
    int64_t nonfinite;       /*            elements that are NaN or +-inf */
    int64_t skipped_total;   /* cumulative: steps skipped */
    int64_t clipped_total;   /*             steps taken with scale < 1 */
    int32_t consecutive;     /*             skipped steps in a row up to and including this one */
    int32_t reserved[3];
} ups_step_guard;
int32_t ups_step_guard_bytes(void);
int32_t ups_grad_guard_chunk(void);
size_t ups_grad_guard_scratch_bytes(int64_t count);
int ups_grad_guard(const float* g, int64_t count, double grad_scale, double clip_norm, int32_t skip_nonfinite, void* scratch,
                   ups_step_guard* rec, int32_t max_blocks, void* stream);
int ups_adam_guarded(float* p, const float* g, float* m, float* v, int64_t count, float lr_t, const float* lr_t_dev, float beta1,
                     float beta2, float eps, float grad_scale, const ups_step_guard* rec, void* stream);
int ups_state_update_guarded(const float* stats, const float* old_state, float* new_state, float decay, float gain,
                             int32_t update_loa, float loa_lr, float loa_target, int32_t update_lor, float lor_lr,
                             float lor_target, float lor_min, float lor_max, int64_t* skipped, void* stream);

/* ---------------------------------------------------------------- weight EMA (csrc/ema.hip)
 * Shadow weights: an exponential moving average of every optimizer key's flat fp32 bucket, kept on the device and updated in the step
 * without the host.  The reference has no weight EMA: these definitions are the project's own (the decay warm-up is the `num_updates`
 * rule of tf.train.ExponentialMovingAverage).  Added without a new UPS_ABI_VERSION, as the ups_augment_* entries were.
 *
 * ups_ema_item: one key.  `items` is a HOST array of at most UPS_EMA_MAX_ITEMS; the entries copy it into their kernels' arguments, so
 * a captured graph bakes the bucket pointers in.  shadow and weights: count floats each, DEVICE, 4-byte aligned (any misalignment
 * against 16 bytes, the two sides alike or not), not overlapping.  rec: the key's ups_step_guard, or NULL for a key that is never
 * skipped.
 *
 * ups_ema_update(items, n_items, decay, warmup, n_updates, omd, max_blocks, stream): two launches for all items together.
 *   (a) one thread per item k.  rec != NULL and rec->skip != 0 (read from device memory when the kernel runs: a graph replay decides
 *       afresh): omd[k] = 0 and n_updates[k] stays.  Otherwise, in fp64, with n = n_updates[k]:
 *         d = warmup ? min(decay, (1.0 + n) / (10.0 + n)) : decay;   omd[k] = (float)(1.0 - d);   n_updates[k] = n + 1.
 *   (b) every element of every item whose skip is not set, in fp32 with one rounding per operation (no contraction):
 *         t = s - w;  u = t * omd[k];  s = s - u.
 *       A skipped item's shadow is not written.  A non-finite w gives what the formula gives (which NaN a NaN result is, is the
 *       hardware's choice).  One grid over (item, chunk of 4096 elements); 16-byte accesses on the shadow wherever it is 16-byte
 *       aligned, on the weights where they are misaligned like the shadow (else the widest their alignment permits), single elements
 *       in front of and behind; the result does not depend on the alignment, on the grid or on max_blocks (0: the default grid; n > 0:
 *       at most n blocks, each striding over the chunks).
 *   n_updates: int64 [n_items], DEVICE, zeroed once by the caller.  omd: float [n_items], DEVICE scratch, overwritten.
 * ups_ema_swap(items, n_items, max_blocks, stream): shadow and weights of every item exchange their bits in place, one launch, no
 *   temporary buffer (rec is not read).
 * UPS_E_ARG, nothing launched: n_items < 0 or > UPS_EMA_MAX_ITEMS, NULL items with n_items > 0, a NULL bucket with count > 0,
 * count < 0, a bucket not 4-byte aligned (a rec not 8-byte aligned), max_blocks < 0; for ups_ema_update also a NULL n_updates or omd
 * and a decay that is NaN or outside [0, 1).  n_items == 0: UPS_OK, nothing launched. */
#define UPS_EMA_MAX_ITEMS 16
typedef struct ups_ema_item {
    float* shadow;                 /* flat fp32 bucket, DEVICE */
    float* weights;                /* the key's ParamBank "p" bucket */
    int64_t count;
    const ups_step_guard* rec;     /* NULL: never skipped */
} ups_ema_item;
int32_t ups_ema_item_bytes(void);
int ups_ema_update(const ups_ema_item* items, int32_t n_items, double decay, int32_t warmup, int64_t* n_updates, float* omd,
                   int32_t max_blocks, void* stream);
int ups_ema_swap(const ups_ema_item* items, int32_t n_items, int32_t max_blocks, void* stream);

/* ---------------------------------------------------------------- thin-plate-spline augmentation (M:282-311)
 * Replaces eddata.utils.tps.ThinPlateSpline (un-vendored; "adapted from CompVis/unsupervised-disentangling", Y:188):
 * out[n][y][x][:] = bilinear sample of img[n] at (x_s, y_s) = T[n] @ [1, x, y, phi(|(x,y) - coord[n][i]|^2)...],
 * phi(d2) = d2 log(d2 + 1e-6), (x, y) on linspace(-1, 1); `_interpolate` convention: pixel = (coord + 1) * size / 2,
 * clamped corner indices.  img / out fp32 [n,h,w,c]; T fp32 [n][2][K+3]; coord fp32 [n][K][2] (x, y); K <= 32.
 * Semantics re-derived from the published algorithm: UNVERIFIED (parity unpinned). */
int ups_tps_warp(const float* img, const float* T, const float* coord, float* out, int32_t n, int32_t h, int32_t w,
                 int32_t c, int32_t K, void* stream);

/* ---------------------------------------------------------------- thin-plate-spline parameters and solve (csrc/tps.hip)
 * Added without a new UPS_ABI_VERSION, as the ups_augment_* entries: no struct changed, and a binding that expects these symbols fails
 * to load an older library by name.
 * ups_tps_solve: T [n][2][K+3] fp32 of coord / vector [n][K][2] fp32 (x, y): the system ups_tps_warp's T solves, f(c_i) = c_i + v_i with
 *   the affine side conditions, built in fp64 from the fp32 inputs (phi(d2) = d2 log(d2 + 1e-6)), solved in fp64 by Gaussian elimination
 *   with partial pivoting (largest |a| at or below the diagonal, ties to the lowest row), rounded to fp32 once.  One wave per sample, one
 *   launch, no host check: a sample whose pivot is exactly 0 (coincident control points) or whose solution is not finite gets the
 *   identity transform T[0] = (0,1,0,0...), T[1] = (0,0,1,0...) and adds 1 to the DEVICE counter *n_singular (int32, the caller's; it is
 *   never reset here).  Two launches give the same bits.
 * ups_tps_params: coord, vector and T of n samples from uniforms [n][4K+7] fp32 in [0,1) (layout of tps.tps_parameters: 2K control-point
 *   jitters, 2K TPS vectors, offset, offset_2, the two scales, the rotation) and base_points [K][2] DOUBLE, device: ranges, scale about
 *   `offset`, rotation about `offset_2`, cos / sin all in fp64; coord is rounded to fp32 once, vector = fp32(target - double(coord)), and
 *   the solve of ups_tps_solve runs on those two rounded outputs in the same launch.
 * UPS_E_UNSUPPORTED: K < 3 (no unique affine part) or K > 32.  UPS_E_ARG, nothing launched: a NULL pointer, n < 1.
 * Semantics re-derived from the published algorithm: UNVERIFIED (parity unpinned), as ups_tps_warp. */
int ups_tps_solve(const float* coord, const float* vector, float* T, int32_t* n_singular, int32_t n, int32_t K, void* stream);
int ups_tps_params(const float* uniforms, const double* base_points, int32_t K, double scal, double tps_scal, double rot_scal,
                   double off_scal, double scal_var, double augm_scal, float* coord, float* vector, float* T, int32_t* n_singular,
                   int32_t n, void* stream);

/* ---------------------------------------------------------------- part equivariance under TPS warps (csrc/equivariance.hip)
 * Added without a new UPS_ABI_VERSION, as the ups_augment_* entries: no struct changed, and a binding that expects these symbols fails
 * to load an older library by name.  The reference has no validation: the definitions here are the specification (DESIGN.md section 8;
 * tests/equivariance_ref.py restates them in NumPy float64).
 *
 * ups_tps_grid: grid [n][h][w][2] fp32 = (px, py), the source PIXEL position ups_tps_warp samples for every output pixel, before its
 *   corner clamp: the same fp32 arithmetic (phi(d2) = d2 logf(d2 + 1e-6f), px = (x_s + 1) * w * 0.5, py = (y_s + 1) * h * 0.5).
 *   T fp32 [n][2][K+3], coord fp32 [n][K][2].  UPS_E_ARG, nothing launched: a NULL pointer, n, h or w < 1, K outside 1..32,
 *   h * w > 2^31 - 1, n > 65535.
 *
 * ups_part_equivariance: do the parts of a warped image sit where the warp carried the parts of the original?
 *   soft_a, soft_b [N, h, w, P] fp32  the soft-max maps of the originals and of the warped images (out_parts_soft)
 *   pred_b [N, h, w] int64   the arg-max map of the warped images as segment_soft returned it: taken, not recomputed, for the reason
 *          ups_part_confusion gives
 *   grid   [N, h, w, 2] fp32 (px, py) per pixel of the warped image (ups_tps_grid)
 *   Pixel (y, x) of image i is INSIDE iff px and py are finite and 0 <= px <= w - 1, 0 <= py <= h - 1.  A pixel that is not inside
 *   touches nothing.  For an inside pixel, in fp64, every operation rounded once (no contraction):
 *     X = (double)px, x0 = floor(X), fx = X - x0, x1 = min(x0 + 1, w - 1); Y, y0, fy, y1 likewise
 *     top_p = (1 - fx) * a[y0][x0][p] + fx * a[y0][x1][p];   bot_p the same on row y1;   v_p = (1 - fy) * top_p + fy * bot_p
 *     la = the first maximal p of v;   lb = pred_b
 *   If some v_p or soft_b value of the pixel is NaN, or lb is outside [0, P): *invalid += 1 and the pixel touches nothing else.
 *   Otherwise counts[i][la][lb] += 1 and t = 0.5 * sum_p |v_p - (double)b_p| (p ascending from 0.0): the total variation between
 *   the two part distributions at the pixel.
 *   counts [N, P, P] int32, caller-zeroed or holding earlier launches' counts: the kernel only adds (integer atomics)
 *   invalid [1] int32
 *   tv     double [N], written completely: the sum of t over image i's counted pixels, from per-block partials (one per chunk of
 *          ups_part_equivariance_chunk() pixels) added in index order by a second launch; no floating-point atomics: two calls give
 *          the same bits
 *   scratch  ups_part_equivariance_scratch_bytes(N, h * w) bytes, 8-byte aligned, caller-owned, overwritten
 * P > 32: UPS_E_UNSUPPORTED (evalutil.equivariance_host computes the same on the host).  UPS_E_ARG, nothing launched: a NULL pointer,
 * N, h, w or P < 1, h * w > 2^31 - 1, N * chunks > 2^31 - 1 (then ups_part_equivariance_scratch_bytes returns 0). */
int ups_tps_grid(const float* T, const float* coord, float* grid, int32_t n, int32_t h, int32_t w, int32_t K, void* stream);
int32_t ups_part_equivariance_chunk(void);
size_t ups_part_equivariance_scratch_bytes(int32_t N, int64_t HW);
int ups_part_equivariance(const float* soft_a, const float* soft_b, const int64_t* pred_b, const float* grid, int32_t N, int32_t h,
                          int32_t w, int32_t P, int32_t* counts, int32_t* invalid, double* tv, void* scratch, void* stream);

/* ---------------------------------------------------------------- Gaussian renderers (N:1639-1702, N:1976-2021)
 * tf_hm: P_xy [B][K][2], stddev [B][K][2] on the integer pixel grid (x,y order) -> heat [B,h,w,K] */
int ups_gauss_hm(const float* pts, const float* stddev, float* out, int32_t B, int32_t h, int32_t w, int32_t K, void* stream);
/* tf_hm3: mu [B][K][2] (y,x in [-1,1]), L [B][K][2][2] -> density [B,h,w,K] */
int ups_gauss_hm3(const float* mu, const float* L, float* out, int32_t B, int32_t h, int32_t w, int32_t K, void* stream);

/* ---------------------------------------------------------------- misc
 * dtype conversion of a flat buffer (fp32 <-> bf16, fp32 <-> fp16, fp16 -> bf16) */
int ups_convert(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t count, void* stream);
/* dst[row][0..c) = src[row][0..c) (fp32 -> dtype), dst[row][c..ldd) = 0 */
int ups_pad_convert(const float* src, int32_t c, void* dst, int32_t dtype, int32_t ldd, int64_t rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UPSPARTS_HIP_H */
