// Mask priors of Trainer.make_loss_ops (cub/code/SB_model48i/model.py:652-797) fused into one streaming
// pass per view (forward sums) and one fused backward that emits d(loss)/d(logits) directly.
//
//  view 0 : categorical KL (model.py:21-25,659-665), entropy / cross-entropy (model.py:667-681),
//           Mumford-Shah + area (model.py:744-769, nn.py:1366-1398), patch (model.py:771-783),
//           improper GMRF on the noise-free logits (nn.py:1444-1451)
//  view 1 : categorical KL, variance (model.py:683-719; moments from ups_spatial_moments)
//
// Forward: GP = pow2 >= P adjacent lanes own the parts of one pixel (part reductions = shuffles), consecutive lane groups
// own consecutive pixels.  Backward: a block stages a tile of consecutive pixels of every map it reads in LDS (16-byte
// accesses, tile.h; the maps with finite-difference stencils come with the rows above and below), ONE THREAD OWNS ONE
// PIXEL and walks its P parts in LDS (odd pixel pitch: conflict-free, no cross-lane traffic -- the lane-per-part form spent
// 24 ds_bpermute per 4 pixels on the six part reductions), and the result tiles go back out the same way.
//
// sums[16] (written by the forward finalize):
//   0 sum m*log(P*m+1e-20)   1 sum_pix CE/entropy   2 sum hard*(1-rect)   3 sum 0.5*(dy^2+dx^2)
//   4 sum_np R^2   5 sum_np S^2   6 sum_np Rsmooth^2   7 sum_np Rcontour^2
// per_np (view 0) [n][P][8]: 0 S = sum m, 1 R = sum r, 2 Rsmooth, 3 Rcontour
// per_np (view 1) = stats of ups_spatial_moments: 0 max, 1 Z, 2 S0, 3 Sy, 4 Sx, 5 Q
#include <stdlib.h>
#include <initializer_list>

#include "common.h"
#include "tile.h"

namespace {

constexpr int NSLAB = 64;     // row slabs per image in the forward pass (n x NSLAB blocks: 4 096 at B = 64, two tiles each at 128x128)

struct PriorK {
    int n, h, w, P, view, entropy_ce, half_h, half_w, variant;
    float gamma, ms_alpha, ms_lambda, w_kl, w_entropy, w_ms, w_area, w_patch, w_gmrf, w_var, w_msl;
    const float* l; const float* l_mean; const float* m; const float* hard; const int* px;
    float* per_np; float* sums; const float* g_hard; float* dl; float* ws; float* dl_rec;
};

// Logical block index for a 1-D grid whose consecutive logical blocks share halo rows: hardware block b runs on XCD b % 8, so
// logical = (b % 8) * (total / 8) + b / 8 puts a run of consecutive logical blocks on ONE XCD (its L2 then serves the rows that
// neighbouring tiles re-read; with the identity order every halo row came from HBM / Infinity Cache once per XCD that needed it).
__device__ __forceinline__ int xcd_logical_block() {
    const int total = gridDim.x, b = blockIdx.x;
    return (total & 7) == 0 ? (b & 7) * (total >> 3) + (b >> 3) : b;
}

template <int GP>
__device__ inline float gsum(float v) {
#pragma unroll
    for (int o = GP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GP);
    return v;
}
template <int GP>
__device__ inline float gmax(float v) {
#pragma unroll
    for (int o = GP / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, GP));
    return v;
}

__device__ inline float mval(const float* m, long long img_base, int y, int x, int h, int w, int P, int c) {
    return ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) ? m[(img_base + (long long)y * w + x) * P + c] : 0.f;
}

// value of a staged map at the pixel `dq` pixels after staged pixel hp (0 outside the image: SAME-padded differences)
__device__ inline float tval(const float* t, int PP, int hp, int dq, int c, int y, int x, int h, int w) {
    return ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) ? t[(hp + dq) * PP + c] : 0.f;
}

// ws layout: glob_partial[n][NSLAB][4], then np_partial[n][NSLAB][P][4]
// One block = one slab of rows of one image, walked in tiles of tpx (<= 256) pixels.  Per tile: stage m (+ the row below) and,
// for view 0, l_mean (same), l and hard; phase 1: one thread per pixel walks its parts (log-soft-max, entropy / CE, patch,
// GMRF and the Mumford-Shah term r, which it leaves in the hard slot with the sign marking the contour branch); phase 2:
// threads = (part, sub-lane) sum the columns of the staged tile into the per-part accumulators S, R, Rsmooth, Rcontour.
// PC / LW: the part count and log2 of the image width as compile-time constants for the common shapes (0 / -1: run-time values).
// (__logf / __expf / __fdividef: the hardware's log2 / exp2 / rcp, ~1e-7 relative -- two orders below the 1e-3 parity bar; the
// libm forms are 15-20 VALU instructions each.)
// These launches are VALU-bound (SQ counters, profiles/round4_pmc_part_kernels.txt: the vector ALU busy 60-80 % of the CU-busy
// cycles): the item index -> (pixel, part) and pixel -> (row, column) divisions by run-time values were a third of the instructions.
template <int PC, int LW>
__global__ __launch_bounds__(256, 3) void prior_fwd_kernel(const PriorK p, int rows_per_slab, int tpx) {
    extern __shared__ __attribute__((aligned(16))) float ts[];
    const int P = PC > 0 ? PC : p.P, PP = tile_pitch(P);
    const int W = LW >= 0 ? (1 << (LW >= 0 ? LW : 0)) : p.w;
    const int halo = p.view == 0 ? W + 1 : 0;
    float* tm = ts;
    float* tlm = tm + (size_t)(tpx + halo) * PP;
    float* tl = tlm + (p.view == 0 ? (size_t)(tpx + halo) * PP : 0);
    float* th = tl + (p.view == 0 ? (size_t)tpx * PP : 0);
    float* scratch = th + (p.view == 0 ? (size_t)tpx * PP : 0);      // red_np[NS][P][4], red4[4]
    const int NS = 256 / P;                                           // sub-lanes per part in phase 2
    float* red4 = scratch + (size_t)NS * P * 4;
    int* cpx = (int*)(red4 + 4);                                      // rectangle centres of this image [P][2]
    float* pst = (float*)(cpx + 2 * P);                               // per-pixel log-sum-exp of the tile [tpx]
    const int lb = xcd_logical_block();
    const int n = lb / NSLAB, slab = lb - n * NSLAB;
    if (p.view == 0 && p.px)
        for (int i = threadIdx.x; i < 2 * P; i += 256) cpx[i] = p.px[(long long)n * P * 2 + i];
    const int y0 = slab * rows_per_slab, y1 = max(y0, min(p.h, y0 + rows_per_slab));
    const int hw = p.h * W;
    const long long img = (long long)n * hw;
    float kl = 0.f, ent = 0.f, patch = 0.f, gmrf = 0.f;
    float S = 0.f, R = 0.f, Rs = 0.f, Rc = 0.f;
    const int c2 = threadIdx.x % P, s2 = threadIdx.x / P;            // phase-2 role
    const int q0 = y0 * W, q1 = y1 * W;
    // software pipeline over the slab's tiles: all maps of a tile are requested at once (one HBM round trip, tile.h) and the NEXT
    // tile's pieces are in flight while the current one is computed
    TileReq<3> rm, rlm;         // (P <= 11 at 128-wide images: everything in one round trip; larger P: the rest synchronously)
    TileReq<2> rl, rh;
    auto request = [&](int t0) {
        const int cnt = min(tpx, q1 - t0), cnt_h = min(cnt + halo, hw - t0);
        tile_request(rm, p.m + (img + t0) * P, cnt_h, P);
        if (p.view == 0) {
            tile_request(rlm, p.l_mean + (img + t0) * P, cnt_h, P);
            tile_request(rl, p.l + (img + t0) * P, cnt, P);
            tile_request(rh, p.hard + (img + t0) * P, cnt, P);
        }
    };
    if (q0 < q1) request(q0);
    for (int t0 = q0; t0 < q1; t0 += tpx) {
        const int cnt = min(tpx, q1 - t0);
        const int cnt_h = min(cnt + halo, hw - t0);
        __syncthreads();
        tile_commit(rm, p.m + (img + t0) * P, cnt_h, P, PP, tm);
        if (p.view == 0) {
            tile_commit(rlm, p.l_mean + (img + t0) * P, cnt_h, P, PP, tlm);
            tile_commit(rl, p.l + (img + t0) * P, cnt, P, PP, tl);
            tile_commit(rh, p.hard + (img + t0) * P, cnt, P, PP, th);
        }
        if (t0 + tpx < q1) request(t0 + tpx);
        __syncthreads();
        // element-wise work on ITEMS (pixel, part) over all 256 threads; only the log-sum-exp stays per pixel (see prior_bwd_kernel)
        if (p.view == 0) {
            for (int px = threadIdx.x; px < cnt; px += 256) {
                const float* lrow = tl + px * PP;
                float mx = -INFINITY;
                for (int c = 0; c < P; ++c) mx = fmaxf(mx, lrow[c]);
                float se = 0.f;
                for (int c = 0; c < P; ++c) se += __expf(lrow[c] - mx);
                pst[px] = mx + __logf(se);
            }
            __syncthreads();
        }
        // (items over all 256 threads -- exactly cnt * P / 256 each; the (part, pixel lane) form of the backward kernel measured
        // 19 % slower here: 250 busy threads with 5 or 6 pixels each)
        const int items = cnt * P;
        for (int it = threadIdx.x; it < items; it += 256) {
            const int px = it / P, c = it - px * P;
            const float* tmc = tm + px * PP + c;
            const float mc = tmc[0];
            kl += mc * __logf((float)P * mc + 1e-20f);
            if (p.view == 0) {
                const int q = t0 + px;
                const int yy = q / W, xx = q - yy * W;
                const bool vr = xx + 1 < W, vd = yy + 1 < p.h;
                const float sl = tl[px * PP + c] - pst[px];
                const float hv = th[px * PP + c];
                ent += -(p.entropy_ce ? hv : mc) * sl;
                const float* tlc = tlm + px * PP + c;
                const float lm = tlc[0];
                const float lr = vr ? tlc[PP] : 0.f, ld = vd ? tlc[W * PP] : 0.f;
                if (p.variant == 0) {
                    const bool in_rect = abs(yy - cpx[2 * c]) <= p.half_h && abs(xx - cpx[2 * c + 1]) <= p.half_w;
                    patch += hv * (in_rect ? 0.f : 1.f);
                } else {
                    // SB_model48c: Mumford-Shah on the noise-free logits, min(alpha * g, lambda) summed (patch slot)
                    const float gw = 0.25f * (lm - lr), gh = 0.25f * (lm - ld);
                    patch += fminf(p.ms_alpha * (gw * gw + gh * gh), p.ms_lambda);
                }
                if (vd) { const float d = ld - lm; gmrf += 0.5f * d * d; }
                if (vr) { const float d = lr - lm; gmrf += 0.5f * d * d; }
                const float mr = vr ? tmc[PP] : 0.f, md = vd ? tmc[W * PP] : 0.f;
                const float gw = 0.25f * (mc - mr), gh = 0.25f * (mc - md);
                const float g = p.ms_alpha * (gw * gw + gh * gh);
                const float r = fminf(g, p.ms_lambda);
                th[px * PP + c] = (g < p.ms_lambda) ? r : -r;            // sign = contour branch (r = lambda > 0 there)
            }
        }
        if (p.view == 0) {
            __syncthreads();
            if (s2 < NS) {
                for (int px = s2; px < cnt; px += NS) {
                    S += tm[px * PP + c2];
                    const float r = th[px * PP + c2];
                    const float ar = fabsf(r);
                    R += ar;
                    if (__float_as_uint(r) >> 31) Rc += ar; else Rs += ar;
                }
            }
        }
    }
    // per-(n,p) partials
    __syncthreads();
    if (s2 < NS) {
        float* d = scratch + ((size_t)s2 * P + c2) * 4;
        d[0] = S; d[1] = R; d[2] = Rs; d[3] = Rc;
    }
    __syncthreads();
    float* np_partial = p.ws + (long long)p.n * NSLAB * 4;
    if (threadIdx.x < P) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < NS; ++q)
            for (int k = 0; k < 4; ++k) o[k] += scratch[((size_t)q * P + threadIdx.x) * 4 + k];
        float* d = np_partial + (((long long)n * NSLAB + slab) * P + threadIdx.x) * 4;
        for (int k = 0; k < 4; ++k) d[k] = o[k];
    }
    float v;
    float* gp = p.ws + ((long long)n * NSLAB + slab) * 4;
    v = block_sum_256(kl, red4);   if (threadIdx.x == 0) gp[0] = v;
    v = block_sum_256(ent, red4);  if (threadIdx.x == 0) gp[1] = v;
    v = block_sum_256(patch, red4); if (threadIdx.x == 0) gp[2] = v;
    v = block_sum_256(gmrf, red4); if (threadIdx.x == 0) gp[3] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 5: the view-0 forward sums for the headline shape class as a PIXEL-PER-LANE kernel (north_star's ">= 50 % of the HBM roof" on
// this row, asked four times).  What held prior_fwd_kernel at a quarter of the roof was instruction count, not bytes: ~500 VALU per
// thread and tile to convert the [pixel][P] rows into an odd-pitch LDS image (a division by P per 16-byte piece, four ds_write per
// piece) and ~175 instructions per (pixel, part) item where the arithmetic needs ~35 (tools/asm_loops.py).  Here
//   * a tile is 256 consecutive pixels (whole rows: W | 256) and EVERY map of it is copied LINEARLY into LDS by LDS-DMA (1 KiB per
//     wave instruction, no registers, no VALU): a P-float pixel pitch with P even is conflict-free for ds_read_b64 at one pixel per
//     lane (P/2 * px mod 32 hits every bank pair once for P/2 odd; P = 10: 5 px mod 32);
//   * one thread owns one pixel with its P parts unrolled in registers; the right neighbour is pixel + 1 of the same image, the lower
//     neighbour pixel + W: in the same tile or in the first rows of the NEXT tile, which the ring already holds (no halo copies);
//   * per-part sums (S, R, Rsmooth, Rcontour) and the four pixel sums are carried in registers over the block's tiles and reduced
//     once per block (shuffles + one LDS exchange), written into the first slab record of the block's slab group (the others zero),
//     so the finalize kernels and the workspace layout are unchanged;
//   * rings: (m, l_mean) four slots -- tiles i, i+1 are read while i+2, i+3 are in flight -- and (l, hard) three slots; the pieces of
//     tile i+2's (l, hard) and tile i+3's (m, l_mean) are issued in iteration i, so every byte has one to two tile times of cover.
// Instances: P = 10, W = 128 / 256 (the CUB / PennAction benchmark shapes); everything else keeps prior_fwd_kernel.
template <int P, int LW, int VAR>
__global__ __launch_bounds__(256) void prior_fwd_px_kernel(const PriorK p, const int tiles_per_block, const int slabs_per_block) {
    static_assert(P % 2 == 0 && ((P / 2) & 1) == 1, "conflict-free ds_read_b64 needs P / 2 odd");
    constexpr int W = 1 << LW;
    static_assert(W <= 256 && 256 % W == 0, "a tile is a whole number of rows");
    constexpr int TB = 256 * P * 4;                 // bytes of one map of one tile
    constexpr int PCS = TB / 1024;                  // 1 KiB DMA pieces per map and tile (= P)
    static_assert(TB % 1024 == 0 && (2 * PCS) % 4 == 0, "piece counts");
    constexpr int PW = 2 * PCS / 4;                 // pieces per wave and map pair
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* ML = smem;                       // 4 slots x (m, l_mean)
    unsigned char* LH = smem + 4 * 2 * TB;          // 3 slots x (l, hard)
    float* red = (float*)(smem + 7 * 2 * TB);       // [4 waves][4 + 4 P]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hw = p.h * W, tiles_img = hw >> 8;
    const int bpi = tiles_img / tiles_per_block;
    const int n = blockIdx.x / bpi, bi = blockIdx.x - n * bpi;
    const int t_begin = bi * tiles_per_block, t_end = t_begin + tiles_per_block;       // tiles of this image
    const long long img = (long long)n * hw;
    const unsigned smem_lds = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned char* gm = (const unsigned char*)(p.m + img * P);
    const unsigned char* glm = (const unsigned char*)(p.l_mean + img * P);
    const unsigned char* gl = (const unsigned char*)(p.l + img * P);
    const unsigned char* gh = (const unsigned char*)(p.hard + img * P);
    const unsigned voff = (unsigned)lane * 16u;

    // pieces of a map pair: piece q = wid + 4 k of 2 * PCS (first map then second), into ring slot `slot`
    auto issue_pair = [&](const unsigned char* a, const unsigned char* b, int tile, unsigned lds_base) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            const int q = wid + 4 * k;
            const unsigned char* src = (q < PCS ? a : b) + (long long)tile * TB + (q < PCS ? q : q - PCS) * 1024;
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)q * 1024u);
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                         :: "s"(dst), "v"(voff), "s"(src) : "memory", "m0");
        }
    };
    auto issue_ml = [&](int t) __attribute__((always_inline)) { issue_pair(gm, glm, t, smem_lds + (unsigned)(((t - t_begin) & 3) * 2 * TB)); };
    auto issue_lh = [&](int t) __attribute__((always_inline)) { issue_pair(gl, gh, t, smem_lds + (unsigned)(4 * 2 * TB + ((t - t_begin) % 3) * 2 * TB)); };
    // tiles whose (m, l_mean) are needed: t_begin .. min(t_end, tiles_img - 1) (the tile below the block's last one, if the image has one)
    const int ml_last = min(t_end, tiles_img - 1);

    // rectangle centres of this image (uniform: scalar loads)
    int cy[P], cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        cy[c] = (VAR == 0 && p.px) ? p.px[((long long)n * P + c) * 2] : 0;
        cx[c] = (VAR == 0 && p.px) ? p.px[((long long)n * P + c) * 2 + 1] : 0;
    }
    float kl = 0.f, ent = 0.f, patch = 0.f, gmrf = 0.f;
    float S[P], R[P], Rs[P], Rc[P];
#pragma unroll
    for (int c = 0; c < P; ++c) S[c] = R[c] = Rs[c] = Rc[c] = 0.f;

    // prologue: (m, l_mean) of tiles t_begin, +1, +2 and (l, hard) of t_begin, +1 -- in the order the loop issues them
    issue_ml(t_begin); issue_lh(t_begin);
    if (t_begin + 1 <= ml_last) issue_ml(t_begin + 1);
    if (t_begin + 1 < t_end) issue_lh(t_begin + 1);
    if (t_begin + 2 <= ml_last) issue_ml(t_begin + 2);

    for (int t = t_begin; t < t_end; ++t) {
        // landed from here on: (m, l_mean) of t and t + 1, (l, hard) of t.  Younger, allowed in flight: (l, hard) of t + 1 and
        // (m, l_mean) of t + 2 -- PW pieces per wave each, where they exist
        const int young = (t + 1 < t_end ? PW : 0) + (t + 2 <= ml_last ? PW : 0);
        if (young == 2 * PW) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PW) : "memory");
        else if (young == PW) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                 // every wave's pieces are in; every wave is done with tile t - 1's slots
        if (t + 2 < t_end) issue_lh(t + 2);           // slot (t + 2) % 3 = (t - 1) % 3: free
        if (t + 3 <= ml_last) issue_ml(t + 3);        // slot (t + 3) & 3 = (t - 1) & 3: free

        const int s4 = (t - t_begin) & 3, s3 = (t - t_begin) % 3;
        const float* tm = (const float*)(ML + s4 * 2 * TB);
        const float* tlm = tm + 256 * P;
        const float* tmn = (const float*)(ML + ((s4 + 1) & 3) * 2 * TB);       // the tile below
        const float* tlmn = tmn + 256 * P;
        const float* tl = (const float*)(LH + s3 * 2 * TB);
        const float* th = tl + 256 * P;
        const int q = (t << 8) + tid;                  // pixel of the image
        const int yy = q >> LW, xx = q & (W - 1);
        const bool vr = xx + 1 < W, vd = yy + 1 < p.h;
        const int qd = tid + W;                        // lower neighbour: this tile or the next one
        const float* md_p = qd < 256 ? tm + qd * P : tmn + (qd - 256) * P;
        const float* lmd_p = qd < 256 ? tlm + qd * P : tlmn + (qd - 256) * P;
        float m[P], mr[P], md[P], lm[P], lr[P], ld[P], l[P], hv[P];
        auto ld_row = [&](const float* src, float (&dst)[P]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < P; c += 2) { const float2 v = *(const float2*)(src + c); dst[c] = v.x; dst[c + 1] = v.y; }
        };
        ld_row(tm + tid * P, m); ld_row(tlm + tid * P, lm); ld_row(tl + tid * P, l); ld_row(th + tid * P, hv);
        ld_row(tm + (tid + 1) * P, mr); ld_row(tlm + (tid + 1) * P, lr);      // (tid = 255: x = W - 1, the values are dropped)
        ld_row(md_p, md); ld_row(lmd_p, ld);
        float mx = l[0];
#pragma unroll
        for (int c = 1; c < P; ++c) mx = fmaxf(mx, l[c]);
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < P; ++c) se += __expf(l[c] - mx);
        const float lse = mx + ups_log_fast(se);
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const float mc = m[c];
            kl += mc * ups_log_fast((float)P * mc + 1e-20f);
            ent += -(p.entropy_ce ? hv[c] : mc) * (l[c] - lse);
            const float lmc = lm[c];
            const float lrc = vr ? lr[c] : 0.f, ldc = vd ? ld[c] : 0.f;
            if (VAR == 0) {
                const bool in_rect = abs(yy - cy[c]) <= p.half_h && abs(xx - cx[c]) <= p.half_w;
                patch += in_rect ? 0.f : hv[c];
            } else {
                const float gw = 0.25f * (lmc - lrc), gh = 0.25f * (lmc - ldc);
                patch += fminf(p.ms_alpha * (gw * gw + gh * gh), p.ms_lambda);
            }
            if (vd) { const float d = ldc - lmc; gmrf += 0.5f * d * d; }
            if (vr) { const float d = lrc - lmc; gmrf += 0.5f * d * d; }
            const float mrc = vr ? mr[c] : 0.f, mdc = vd ? md[c] : 0.f;
            const float gw = 0.25f * (mc - mrc), gh = 0.25f * (mc - mdc);
            const float g = p.ms_alpha * (gw * gw + gh * gh);
            const float r = fminf(g, p.ms_lambda);
            S[c] += mc; R[c] += r;
            if (g < p.ms_lambda) Rs[c] += r; else Rc[c] += r;
        }
    }
    // ---- block reduction: wave sums by shuffles, the four waves through LDS, one record per block
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    kl = wave_sum_full(kl); ent = wave_sum_full(ent); patch = wave_sum_full(patch); gmrf = wave_sum_full(gmrf);
#pragma unroll
    for (int c = 0; c < P; ++c) { S[c] = wave_sum_full(S[c]); R[c] = wave_sum_full(R[c]); Rs[c] = wave_sum_full(Rs[c]); Rc[c] = wave_sum_full(Rc[c]); }
    if (lane == 0) {
        float* d = red + wid * (4 + 4 * P);
        d[0] = kl; d[1] = ent; d[2] = patch; d[3] = gmrf;
#pragma unroll
        for (int c = 0; c < P; ++c) { d[4 + 4 * c] = S[c]; d[5 + 4 * c] = R[c]; d[6 + 4 * c] = Rs[c]; d[7 + 4 * c] = Rc[c]; }
    }
    __syncthreads();
    // workspace: glob_partial[n][NSLAB][4], np_partial[n][NSLAB][P][4]; this block owns slabs [bi * slabs_per_block, + slabs_per_block)
    float* gpart = p.ws + ((long long)n * NSLAB + (long long)bi * slabs_per_block) * 4;
    float* npart = p.ws + (long long)p.n * NSLAB * 4 + ((long long)n * NSLAB + (long long)bi * slabs_per_block) * P * 4;
    for (int i = tid; i < slabs_per_block * 4; i += 256)
        gpart[i] = i < 4 ? red[i] + red[(4 + 4 * P) + i] + red[2 * (4 + 4 * P) + i] + red[3 * (4 + 4 * P) + i] : 0.f;
    for (int i = tid; i < slabs_per_block * P * 4; i += 256)
        npart[i] = i < 4 * P ? red[4 + i] + red[(4 + 4 * P) + 4 + i] + red[2 * (4 + 4 * P) + 4 + i] + red[3 * (4 + 4 * P) + 4 + i] : 0.f;
}

// Two short stages instead of one single-block pass (which walked n * NSLAB * (1 + P) partial records serially per thread: 16 us
// behind a 120 us forward pass).  Stage 1, one block per image: the image's slab partials -> per_np[n][P][8] and the image's eight
// sums (4 pixel sums, 4 sums of squares over its parts), every reduction in a fixed order.  Stage 2, one block: the images.
__global__ __launch_bounds__(256) void prior_finalize_img_kernel(const PriorK p) {
    __shared__ float red4[4];
    const int n = blockIdx.x;
    const float* gpart = p.ws + (long long)n * NSLAB * 4;
    const float* np_partial = p.ws + (long long)p.n * NSLAB * 4 + (long long)n * NSLAB * p.P * 4;
    float* img_part = p.ws + (long long)p.n * NSLAB * 4 + (long long)p.n * NSLAB * p.P * 4 + (long long)n * 8;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < NSLAB; i += 256)
        for (int k = 0; k < 4; ++k) a[k] += gpart[i * 4 + k];
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.view == 0) {
        // wave per part: lanes over the slabs
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int c = wv; c < p.P; c += 4) {
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            for (int s = lane; s < NSLAB; s += 64)
                for (int k = 0; k < 4; ++k) o[k] += np_partial[((long long)s * p.P + c) * 4 + k];
            for (int k = 0; k < 4; ++k) o[k] = wave_sum(o[k]);
            if (lane == 0) {
                float* d = p.per_np + ((long long)n * p.P + c) * 8;
                d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3]; d[4] = d[5] = d[6] = d[7] = 0.f;
                sq[0] += o[1] * o[1]; sq[1] += o[0] * o[0]; sq[2] += o[2] * o[2]; sq[3] += o[3] * o[3];
            }
        }
    }
    for (int k = 0; k < 4; ++k) {
        const float v = block_sum_256(a[k], red4);
        if (threadIdx.x == 0) img_part[k] = v;
    }
    for (int k = 0; k < 4; ++k) {
        const float v = block_sum_256(sq[k], red4);
        if (threadIdx.x == 0) img_part[4 + k] = v;
    }
}

// Finalize of the pixel-per-lane forward: a block of prior_fwd_px_kernel leaves ONE record per slab group, so an image has only
// `bpi` non-zero records and the whole reduction -- per_np[n][P][8], the four pixel sums and the four sums of squares over (n, part) --
// is a few thousand floats: one block, one launch (the two-stage pair of the slab kernel costs 10 us behind a 38 us forward).
// (round 6, late: 1 024 threads = four record groups x 256 (image, part) items: a wave reads 64 CONSECUTIVE 16-byte pieces of one
// record row -- eight cache lines per instruction -- with a group's eight loads independent of each other, and the four groups meet in
// LDS.  One thread per item walking 32 records in a chain kept 16 KB in flight: 53 us behind a 95 us forward at P = 25, B = 64; four
// adjacent lanes per item touched 64 lines per instruction: 27 us)
__global__ __launch_bounds__(1024) void prior_finalize_px_kernel(const PriorK p, const int bpi, const int spb) {
    constexpr int RS = 4;
    __shared__ float4 part[RS][256];
    __shared__ float red[4][8];
    const float4* gpart = (const float4*)p.ws;
    const float4* npart = (const float4*)(p.ws + (long long)p.n * NSLAB * 4);
    const int tid = threadIdx.x, rs = tid >> 8, ti = tid & 255;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int items = p.n * p.P;
    // pass 0: the four pixel sums (items = images, one piece per record); pass 1: the per-part sums (items = (image, part))
    for (int pass = 0; pass < 2; ++pass) {
        const int cnt = pass == 0 ? p.n : items;
        for (int i0 = 0; i0 < cnt; i0 += 256) {
            const int it = i0 + ti;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (it < cnt) {
                const int n = pass == 0 ? it : it / p.P, c = pass == 0 ? 0 : it - n * p.P;
                const float4* src = pass == 0 ? gpart + (long long)n * NSLAB : npart + (long long)n * NSLAB * p.P + c;
                const long long step = pass == 0 ? (long long)spb : (long long)spb * p.P;
#pragma unroll 8
                for (int b = rs; b < bpi; b += RS) {
                    const float4 q = src[b * step];
                    o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
                }
            }
            __syncthreads();                       // (the previous chunk's partials have been read)
            part[rs][ti] = o;
            __syncthreads();
            if (rs == 0 && it < cnt) {
                const float4 q1 = part[1][ti], q2 = part[2][ti], q3 = part[3][ti];
                o.x = (o.x + q1.x) + (q2.x + q3.x); o.y = (o.y + q1.y) + (q2.y + q3.y);
                o.z = (o.z + q1.z) + (q2.z + q3.z); o.w = (o.w + q1.w) + (q2.w + q3.w);
                if (pass == 0) { a[0] += o.x; a[1] += o.y; a[2] += o.z; a[3] += o.w; }
                else {
                    float4* d = (float4*)(p.per_np + (long long)it * 8);
                    d[0] = o; d[1] = make_float4(0.f, 0.f, 0.f, 0.f);
                    a[4] += o.y * o.y; a[5] += o.x * o.x; a[6] += o.z * o.z; a[7] += o.w * o.w;
                }
            }
        }
    }
    if (rs == 0) {          // (waves 0 .. 3 hold the sums)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = a[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            a[k] = v;
        }
        if ((tid & 63) == 0)
            for (int k = 0; k < 8; ++k) red[tid >> 6][k] = a[k];
    }
    __syncthreads();
    if (tid < 16) p.sums[tid] = tid < 8 ? (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]) : 0.f;
}

__global__ __launch_bounds__(256) void prior_finalize_kernel(const PriorK p) {
    __shared__ float red4[4];
    const float* img_part = p.ws + (long long)p.n * NSLAB * 4 + (long long)p.n * NSLAB * p.P * 4;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < p.n; i += 256)
        for (int k = 0; k < 8; ++k) a[k] += img_part[(long long)i * 8 + k];
    for (int k = 0; k < 8; ++k) {
        const float v = block_sum_256(a[k], red4);
        if (threadIdx.x == 0) p.sums[k] = v;
    }
    if (threadIdx.x == 0) for (int k = 8; k < 16; ++k) p.sums[k] = 0.f;
}

// One block = one tile of tpx (<= 256) consecutive pixels of image blockIdx.y.  LDS: m and (view 0) l_mean with w pixels of
// halo on either side, l / hard / g_hard own pixels only, the per-part constants of the image; the result tiles dl (in the l
// slot) and dl_rec (in the g_hard slot) go back out with 16-byte stores.
template <int PC, int LW>
__global__ __launch_bounds__(256) void prior_bwd_kernel(const PriorK p, int tpx) {
    extern __shared__ __attribute__((aligned(16))) float ts[];
    const int P = PC > 0 ? PC : p.P, PP = tile_pitch(P);
    const int W = LW >= 0 ? (1 << (LW >= 0 ? LW : 0)) : p.w;
    const int hw = p.h * W;
    const int tiles = (hw + tpx - 1) / tpx;
    const int lb = xcd_logical_block();
    const int n = lb / tiles;
    const int t0 = (lb - n * tiles) * tpx;
    const int cnt = min(tpx, hw - t0);
    const int halo = p.view == 0 ? W : 0;
    const int lo = max(0, t0 - halo), hi = min(hw, t0 + cnt + halo);
    const int off = t0 - lo;                       // tile pixel px sits at staged pixel px + off of the halo maps
    float* tm = ts;
    float* tlm = tm + (size_t)(tpx + 2 * halo) * PP;
    float* tl = tlm + (p.view == 0 ? (size_t)(tpx + 2 * halo) * PP : 0);      // l (view 0) -> direct term -> dl
    float* th = tl + (size_t)tpx * PP;                                          // hard (view 0) -> gm
    float* tg = th + (size_t)tpx * PP;                                          // g_hard -> dl_rec
    float* cst = tg + (size_t)tpx * PP;                                         // [P][8]: per-part constants of this image
    const long long img = (long long)n * hw;
    {   // every map's pieces are requested before any of them is waited for: one HBM round trip per block instead of five
        TileReq<4> rm, rlm;
        TileReq<2> rl, rh, rg;
        tile_request(rm, p.m + (img + lo) * P, hi - lo, P);
        if (p.view == 0) {
            tile_request(rlm, p.l_mean + (img + lo) * P, hi - lo, P);
            tile_request(rl, p.l + (img + t0) * P, cnt, P);
            tile_request(rh, p.hard + (img + t0) * P, cnt, P);
        }
        if (p.g_hard) tile_request(rg, p.g_hard + (img + t0) * P, cnt, P);
        tile_commit(rm, p.m + (img + lo) * P, hi - lo, P, PP, tm);
        if (p.view == 0) {
            tile_commit(rlm, p.l_mean + (img + lo) * P, hi - lo, P, PP, tlm);
            tile_commit(rl, p.l + (img + t0) * P, cnt, P, PP, tl);
            tile_commit(rh, p.hard + (img + t0) * P, cnt, P, PP, th);
        }
        if (p.g_hard) tile_commit(rg, p.g_hard + (img + t0) * P, cnt, P, PP, tg);
    }
    for (int c = threadIdx.x; c < P; c += 256) {
        float* k = cst + c * 8;
        const float* np = p.per_np + ((long long)n * P + c) * 8;
        k[0] = p.px ? (float)p.px[((long long)n * P + c) * 2] : 0.f;
        k[1] = p.px ? (float)p.px[((long long)n * P + c) * 2 + 1] : 0.f;
        if (p.view == 0) { k[2] = np[0]; k[3] = np[1]; }
        else {
            const float Z = np[1];
            k[2] = np[0]; k[3] = Z; k[4] = np[3] / Z; k[5] = np[4] / Z; k[6] = np[5] / Z; k[7] = np[6] / Z;
        }
    }
    __syncthreads();
    const long long npix_total = (long long)p.n * hw;
    const float inv_pix = 1.f / (float)npix_total, inv_n = 1.f / (float)p.n;
    const float a8 = p.ms_alpha * 0.125f, a16 = p.ms_alpha * 0.0625f;
    const float sy = p.h > 1 ? 2.f / (float)(p.h - 1) : 0.f, sx = W > 1 ? 2.f / (float)(W - 1) : 0.f;
    // Compute in four short phases (round 4).  The per-pixel form (one thread walks the P parts of its pixel: a serial chain of
    // ~150 dependent instructions per part with half the block idle at 128-pixel tiles) bounded the launch, not its bytes: the
    // element-wise work now runs on ITEMS (pixel, part) spread over all 256 threads (independent items per thread), only the
    // per-pixel reductions (log-sum-exp, the soft-max Jacobian's dot products) stay per pixel.
    float* pst = cst + P * 8;                                   // [tpx][4]: lse, qs, labsum | dot, dot_r
    const int items = cnt * P;
    const int NS = 256 / P;                                     // pixel lanes of the (part, pixel lane) phases
    const int s2 = threadIdx.x / P, c2 = threadIdx.x - s2 * P;
    const int dyy = NS / W, dxx = NS - dyy * W;                 // pixel step NS in (row, column) form
    if (p.view == 0) {
        for (int px = threadIdx.x; px < cnt; px += 256) {       // A: per-pixel log-sum-exp, sum m * log-soft-max, sum of labels
            const float* mrow = tm + (px + off) * PP;
            const float* lrow = tl + px * PP;
            const float* hrow = th + px * PP;
            float mx = -INFINITY;
            for (int c = 0; c < P; ++c) mx = fmaxf(mx, lrow[c]);
            float se = 0.f;
            for (int c = 0; c < P; ++c) se += __expf(lrow[c] - mx);
            const float lse = mx + __logf(se);
            float qs = 0.f, labsum = 0.f;
            for (int c = 0; c < P; ++c) { qs += mrow[c] * (lrow[c] - lse); labsum += hrow[c]; }
            pst[px * 4] = lse; pst[px * 4 + 1] = qs; pst[px * 4 + 2] = labsum;
        }
        __syncthreads();
        // B: d loss / d m (-> hard slot) and the direct term (-> l slot).  Thread = (part c, pixel lane): the part is FIXED per thread
        // (its constants sit in registers, no item -> (pixel, part) division), the pixel coordinates advance incrementally, and the
        // validity of the stencil neighbours is four flags per pixel instead of two range tests per tap.
        if (s2 < NS) {
            const float* kc = cst + c2 * 8;
            const int rcy = (int)kc[0], rcx = (int)kc[1];
            const float kS = kc[2], kR = kc[3];
            int yy = (t0 + s2) / W, xx = (t0 + s2) - yy * W;
            for (int px = s2; px < cnt; px += NS) {
                const int c = c2;
                const int hp = px + off;
                const bool vr = xx + 1 < W, vd = yy + 1 < p.h, vl = xx > 0, vu = yy > 0;
                const float* tmc = tm + hp * PP + c;
                const float mc = tmc[0];
                const float lse = pst[px * 4], qs = pst[px * 4 + 1], labsum = pst[px * 4 + 2];
                const float sl = tl[px * PP + c] - lse;
                const float hv = th[px * PP + c];
                const float gh = p.g_hard ? tg[px * PP + c] : 0.f;
                const float pm = (float)P * mc;
                float gm = p.w_kl * inv_pix * (__logf(pm + 1e-20f) + __fdividef(pm, pm + 1e-20f)) + gh;
                float direct = p.w_entropy * inv_pix * (-mc * (sl - qs));
                if (p.entropy_ce) direct += p.w_entropy * inv_pix * (-(hv - mc * labsum));
                if (p.variant == 0) {      // patch (STE)
                    const bool in_rect = abs(yy - rcy) <= p.half_h && abs(xx - rcx) <= p.half_w;
                    gm += p.w_patch * inv_n * (in_rect ? 0.f : 1.f);
                }
                // area + mumford-shah (cells: own, left neighbour's -- its right value is me --, upper neighbour's -- its down value is me)
                gm += p.w_area * inv_n * 2.f * kS;
                const float m_r = vr ? tmc[PP] : 0.f;
                const float m_d = vd ? tmc[W * PP] : 0.f;
                float dR = 0.f;
                {
                    const float g = a16 * ((mc - m_r) * (mc - m_r) + (mc - m_d) * (mc - m_d));
                    if (g <= p.ms_lambda) dR += a8 * ((mc - m_r) + (mc - m_d));
                }
                if (vl) {
                    const float m_l = tmc[-PP];
                    const float m_ld = vd ? tmc[(W - 1) * PP] : 0.f;
                    const float g = a16 * ((m_l - mc) * (m_l - mc) + (m_l - m_ld) * (m_l - m_ld));
                    if (g <= p.ms_lambda) dR -= a8 * (m_l - mc);
                }
                if (vu) {
                    const float m_u = tmc[-W * PP];
                    const float m_ur = vr ? tmc[(1 - W) * PP] : 0.f;
                    const float g = a16 * ((m_u - m_ur) * (m_u - m_ur) + (m_u - mc) * (m_u - mc));
                    if (g <= p.ms_lambda) dR -= a8 * (m_u - mc);
                }
                gm += p.w_ms * inv_n * 2.f * kR * dR;
                // gmrf on the noise-free logits (same tensor path: l = l_mean + eps)
                const float* tlc = tlm + hp * PP + c;
                const float lm = tlc[0];
                if (p.variant == 1) {
                    // SB_model48c: d/d l_mean of sum min(alpha * g(l_mean), lambda): the stencil above applied to the logits
                    const float l_r = vr ? tlc[PP] : 0.f;
                    const float l_d = vd ? tlc[W * PP] : 0.f;
                    float dL = 0.f;
                    {
                        const float g = a16 * ((lm - l_r) * (lm - l_r) + (lm - l_d) * (lm - l_d));
                        if (g <= p.ms_lambda) dL += a8 * ((lm - l_r) + (lm - l_d));
                    }
                    if (vl) {
                        const float l_l = tlc[-PP];
                        const float l_ld = vd ? tlc[(W - 1) * PP] : 0.f;
                        const float g = a16 * ((l_l - lm) * (l_l - lm) + (l_l - l_ld) * (l_l - l_ld));
                        if (g <= p.ms_lambda) dL -= a8 * (l_l - lm);
                    }
                    if (vu) {
                        const float l_u = tlc[-W * PP];
                        const float l_ur = vr ? tlc[(1 - W) * PP] : 0.f;
                        const float g = a16 * ((l_u - l_ur) * (l_u - l_ur) + (l_u - lm) * (l_u - lm));
                        if (g <= p.ms_lambda) dL -= a8 * (l_u - lm);
                    }
                    direct += p.w_msl * inv_n * dL;
                }
                float gg = 0.f;
                if (vu) gg += lm - tlc[-W * PP];
                if (vd) gg -= tlc[W * PP] - lm;
                if (vl) gg += lm - tlc[-PP];
                if (vr) gg -= tlc[PP] - lm;
                direct += p.w_gmrf * inv_n * gg;
                th[px * PP + c] = gm; tl[px * PP + c] = direct;
                xx += dxx; yy += dyy;
                if (xx >= W) { xx -= W; ++yy; }
            }
        }
    } else {
        if (s2 < NS) {                                          // B (view 1): d loss / d m -> l slot; thread = (part, pixel lane)
            const float* kc = cst + c2 * 8;
            const int rcy = (int)kc[0], rcx = (int)kc[1];
            const float kmax = kc[2], rZ = __fdividef(1.f, kc[3]), muy = kc[4], mux = kc[5], k6 = kc[6], k7 = kc[7];
            // SB_model48c variance (DF:750-776): v_np = S00^2 + S11^2 of c = softmax_hw(gamma*m) (no rectangle, renormalised),
            // S00 = Qy/Z - muy^2, S11 = Qx/Z - mux^2;  SB_model48i: v_np = Q/Z - muy^2 - mux^2 over softmax_hw(gamma*m) * (1-rect)
            const float Qyn = k7, Qxn = k6 - k7;
            const float S00 = Qyn - muy * muy, S11 = Qxn - mux * mux;
            const float T = k6 - 2.f * muy * muy - 2.f * mux * mux;
            const float wv = p.w_var * inv_n * p.gamma * rZ;
            int yy = (t0 + s2) / W, xx = (t0 + s2) - yy * W;
            for (int px = s2; px < cnt; px += NS) {
                const float gy = -1.f + sy * (float)yy, gx = -1.f + sx * (float)xx;
                const float mc = tm[(px + off) * PP + c2];
                const float gh = p.g_hard ? tg[px * PP + c2] : 0.f;
                const float pm = (float)P * mc;
                float gm = p.w_kl * inv_pix * (__logf(pm + 1e-20f) + __fdividef(pm, pm + 1e-20f)) + gh;
                const float sq = __expf(p.gamma * mc - kmax);
                if (p.variant == 1) {
                    const float ay = gy * gy - 2.f * muy * gy - (Qyn - 2.f * muy * muy);
                    const float ax = gx * gx - 2.f * mux * gx - (Qxn - 2.f * mux * mux);
                    gm += wv * sq * 2.f * (S00 * ay + S11 * ax);
                } else {
                    const float kk = (abs(yy - rcy) <= p.half_h && abs(xx - rcx) <= p.half_w) ? 0.f : 1.f;
                    const float a = gy * gy + gx * gx - 2.f * muy * gy - 2.f * mux * gx;
                    gm += wv * sq * (a * kk - T);
                }
                tl[px * PP + c2] = gm;
                xx += dxx; yy += dyy;
                if (xx >= W) { xx -= W; ++yy; }
            }
        }
    }
    __syncthreads();
    const float* gms = p.view == 0 ? th : tl;                   // where phase B left d loss / d m
    for (int px = threadIdx.x; px < cnt; px += 256) {           // C: the soft-max Jacobian's dot products per pixel
        const float* mrow = tm + (px + off) * PP;
        float dot = 0.f, dot_r = 0.f;
        for (int c = 0; c < P; ++c) {
            const float mc = mrow[c];
            dot += mc * gms[px * PP + c];
            if (p.g_hard) dot_r += mc * tg[px * PP + c];
        }
        pst[px * 4] = dot; pst[px * 4 + 1] = dot_r;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < items; it += 256) {         // D: dl (l slot) and the reconstruction-only dl_rec (g_hard slot)
        const int px = it / P, c = it - px * P;
        const float mc = tm[(px + off) * PP + c];
        const float gh = p.g_hard ? tg[px * PP + c] : 0.f;
        const float gm = gms[px * PP + c];
        const float direct = p.view == 0 ? tl[px * PP + c] : 0.f;
        tl[px * PP + c] = mc * (gm - pst[px * 4]) + direct;
        tg[px * PP + c] = mc * (gh - pst[px * 4 + 1]);
    }
    __syncthreads();
    tile_store_f32(p.dl + (img + t0) * P, cnt, P, PP, tl);
    if (p.dl_rec) tile_store_f32(p.dl_rec + (img + t0) * P, cnt, P, PP, tg);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 5: the VIEW-1 backward (KL + variance terms through the soft-max Jacobian; inputs m and g_hard, outputs dl and dl_rec) in the
// pixel-per-lane form of prior_fwd_px_kernel: linear LDS-DMA tiles of 256 pixels (two slots), one thread = one pixel with its P
// parts and the image's per-part constants in registers, the two result rows written back into a linear LDS tile (ds_write_b64 at
// a 40-byte pitch is conflict-free like the reads) and stored with 16-byte accesses.  Two blocks per CU cover each other's waits.
template <int P, int LW, int VAR>
__global__ __launch_bounds__(256, 2) void prior_bwd1_px_kernel(const PriorK p, const int tiles_per_block) {
    static_assert(P % 2 == 0 && ((P / 2) & 1) == 1, "conflict-free 8-byte LDS accesses need P / 2 odd");
    constexpr int W = 1 << LW;
    constexpr int TB = 256 * P * 4, PCS = TB / 1024, PW = 2 * PCS / 4;
    static_assert(TB % 1024 == 0 && (2 * PCS) % 4 == 0 && (2 * TB / 16) % 256 == 0, "piece counts");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* IN = smem;                        // 2 slots x (m, g_hard)
    unsigned char* OUT = smem + 2 * 2 * TB;          // (dl, dl_rec)
    float* cst = (float*)(smem + 3 * 2 * TB);        // [P][8]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hw = p.h * W, tiles_img = hw >> 8;
    const int bpi = tiles_img / tiles_per_block;
    const int n = blockIdx.x / bpi, bi = blockIdx.x - n * bpi;
    const int t_begin = bi * tiles_per_block, t_end = t_begin + tiles_per_block;
    const long long img = (long long)n * hw;
    const unsigned smem_lds = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned char* gm_ = (const unsigned char*)(p.m + img * P);
    const unsigned char* gg_ = (const unsigned char*)(p.g_hard + img * P);
    const unsigned voff = (unsigned)lane * 16u;
    auto issue = [&](int t) __attribute__((always_inline)) {
        const unsigned base = smem_lds + (unsigned)(((t - t_begin) & 1) * 2 * TB);
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            const int q = wid + 4 * k;
            const unsigned char* src = (q < PCS ? gm_ : gg_) + (long long)t * TB + (q < PCS ? q : q - PCS) * 1024;
            const unsigned dst = __builtin_amdgcn_readfirstlane(base + (unsigned)q * 1024u);
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                         :: "s"(dst), "v"(voff), "s"(src) : "memory", "m0");
        }
    };
    issue(t_begin);
    // the image's per-part constants (as prior_bwd_kernel): rectangle centre, max / Z / means / second moments of the spatial soft-max
    for (int c = tid; c < P; c += 256) {
        float* k = cst + c * 8;
        const float* np = p.per_np + ((long long)n * P + c) * 8;
        const float Z = np[1];
        k[0] = p.px ? (float)p.px[((long long)n * P + c) * 2] : 0.f;
        k[1] = p.px ? (float)p.px[((long long)n * P + c) * 2 + 1] : 0.f;
        k[2] = np[0]; k[3] = Z; k[4] = np[3] / Z; k[5] = np[4] / Z; k[6] = np[5] / Z; k[7] = np[6] / Z;
    }
    __syncthreads();
    const float inv_pix = 1.f / (float)((long long)p.n * hw), inv_n = 1.f / (float)p.n;
    const float sy = p.h > 1 ? 2.f / (float)(p.h - 1) : 0.f, sx = W > 1 ? 2.f / (float)(W - 1) : 0.f;
    const float wkl = p.w_kl * inv_pix;
    int rcy[P], rcx[P];
    float kmax[P], wv[P], muy2[P], mux2[P], ca[P], cb[P], cc[P];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        const float* k = cst + c * 8;
        rcy[c] = (int)k[0]; rcx[c] = (int)k[1];
        kmax[c] = k[2];
        const float rZ = __fdividef(1.f, k[3]), muy = k[4], mux = k[5], k6 = k[6], k7 = k[7];
        wv[c] = p.w_var * inv_n * p.gamma * rZ;
        muy2[c] = 2.f * muy; mux2[c] = 2.f * mux;
        if (VAR == 1) {     // SB_model48c: v = S00^2 + S11^2 of the renormalised spatial soft-max (DF:750-776)
            const float Qyn = k7, Qxn = k6 - k7;
            ca[c] = Qyn - 2.f * muy * muy; cb[c] = Qxn - 2.f * mux * mux;          // subtracted from ay / ax
            cc[c] = Qyn - muy * muy;                                                // S00; S11 is recomputed from cb below
            wv[c] *= 2.f;
        } else {            // SB_model48i: v = Q / Z - muy^2 - mux^2 over softmax_hw(gamma m) * (1 - rect)
            ca[c] = k6 - 2.f * muy * muy - 2.f * mux * mux;                         // T
            cb[c] = 0.f; cc[c] = 0.f;
        }
    }
    float s11[P];
#pragma unroll
    for (int c = 0; c < P; ++c) s11[c] = VAR == 1 ? (cst[c * 8 + 6] - cst[c * 8 + 7]) - 0.25f * mux2[c] * mux2[c] : 0.f;

    for (int t = t_begin; t < t_end; ++t) {
        if (t + 1 < t_end) { issue(t + 1); asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PW) : "memory"); }
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const float* tm = (const float*)(IN + ((t - t_begin) & 1) * 2 * TB);
        const float* tg = tm + 256 * P;
        const int q = (t << 8) + tid;
        const int yy = q >> LW, xx = q & (W - 1);
        const float gy = -1.f + sy * (float)yy, gx = -1.f + sx * (float)xx;
        const float gq = gy * gy + gx * gx;
        float m[P], gh[P], gmv[P];
#pragma unroll
        for (int c = 0; c < P; c += 2) {
            const float2 a = *(const float2*)(tm + tid * P + c), b = *(const float2*)(tg + tid * P + c);
            m[c] = a.x; m[c + 1] = a.y; gh[c] = b.x; gh[c + 1] = b.y;
        }
        float dot = 0.f, dot_r = 0.f;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const float mc = m[c];
            const float pm = (float)P * mc;
            float g = wkl * (ups_log_fast(pm + 1e-20f) + __fdividef(pm, pm + 1e-20f)) + gh[c];
            const float sq = __expf(p.gamma * mc - kmax[c]);
            if (VAR == 1) {
                const float ay = gy * gy - muy2[c] * gy - ca[c];
                const float ax = gx * gx - mux2[c] * gx - cb[c];
                g += wv[c] * sq * (cc[c] * ay + s11[c] * ax);
            } else {
                const float kk = (abs(yy - rcy[c]) <= p.half_h && abs(xx - rcx[c]) <= p.half_w) ? 0.f : 1.f;
                const float a = gq - muy2[c] * gy - mux2[c] * gx;
                g += wv[c] * sq * (a * kk - ca[c]);
            }
            gmv[c] = g;
            dot += mc * g; dot_r += mc * gh[c];
        }
        float* to = (float*)OUT;
#pragma unroll
        for (int c = 0; c < P; c += 2) {
            *(float2*)(to + tid * P + c) = make_float2(m[c] * (gmv[c] - dot), m[c + 1] * (gmv[c + 1] - dot));
            *(float2*)(to + 256 * P + tid * P + c) = make_float2(m[c] * (gh[c] - dot_r), m[c + 1] * (gh[c + 1] - dot_r));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float4* d0 = (float4*)(p.dl + (img + ((long long)t << 8)) * P);
        float4* d1 = (float4*)(p.dl_rec + (img + ((long long)t << 8)) * P);
        const float4* o4 = (const float4*)OUT;
#pragma unroll
        for (int k = 0; k < 2 * TB / 16 / 256; ++k) {      // 2 * 640 16-byte pieces over 256 threads
            const int j = tid + 256 * k;
            if (j < TB / 16) d0[j] = o4[j]; else d1[j - TB / 16] = o4[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 5: the VIEW-0 backward (KL, entropy, patch / Mumford-Shah on the logits, area, Mumford-Shah, GMRF through the soft-max
// Jacobian; seven maps of traffic: m, l_mean, l, hard, g_hard in, dl, dl_rec out) pixel-per-lane.  The stencils reach one row up and
// one row down, so the (m, l_mean) ring holds the tiles t - 1, t, t + 1 with t + 2 in flight (four slots); (l, hard, g_hard) of a
// tile arrive one tile ahead (two slots) and the tile's results overwrite its own l / g_hard rows (thread-private) before they
// leave LINEARLY with 16-byte stores.  140 KB of LDS: one block per CU, so nothing may idle: the wait at the top of a tile is
// COUNTED -- vmcnt(STORES) lets the previous tile's stores stay in flight (gfx9 retires vector memory operations of one wave in
// issue order, loads and stores alike; the compiler's own waits rely on the same) -- and a slot is re-filled as soon as the stores'
// LDS reads are over (the barrier), not when the stores are acknowledged.
template <int P, int LW, int VAR>
__global__ __launch_bounds__(256, 1) void prior_bwd0_px_kernel(const PriorK p, const int tiles_per_block) {
    static_assert(P % 2 == 0 && ((P / 2) & 1) == 1, "conflict-free 8-byte LDS accesses need P / 2 odd");
    constexpr int W = 1 << LW;
    static_assert(W <= 256 && 256 % W == 0, "a tile is a whole number of rows");
    constexpr int TB = 256 * P * 4, PCS = TB / 1024;
    constexpr int STORES = 2 * TB / 16 / 256;          // 16-byte stores per thread and tile (dl + dl_rec)
    static_assert(TB % 1024 == 0 && (2 * TB / 16) % 256 == 0 && (TB / 16) % 64 == 0, "piece counts");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* ML = smem;                          // 4 slots x (m, l_mean)
    unsigned char* LHG = smem + 4 * 2 * TB;            // 2 slots x (l, hard, g_hard)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hw = p.h * W, tiles_img = hw >> 8;
    const int bpi = tiles_img / tiles_per_block;
    const int n = blockIdx.x / bpi, bi = blockIdx.x - n * bpi;
    const int t_begin = bi * tiles_per_block, t_end = t_begin + tiles_per_block;
    const int ml_first = max(t_begin - 1, 0), ml_last = min(t_end, tiles_img - 1);
    const long long img = (long long)n * hw;
    const unsigned smem_lds = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned char* g_m = (const unsigned char*)(p.m + img * P);
    const unsigned char* g_lm = (const unsigned char*)(p.l_mean + img * P);
    const unsigned char* g_l = (const unsigned char*)(p.l + img * P);
    const unsigned char* g_h = (const unsigned char*)(p.hard + img * P);
    const unsigned char* g_g = (const unsigned char*)(p.g_hard + img * P);
    const unsigned voff = (unsigned)lane * 16u;
    // (m, l_mean) of tile t: slot (t - t_begin + 1) & 3, 2 * PCS pieces over the four waves
    auto issue_ml = [&](int t) __attribute__((always_inline)) {
        const unsigned base = smem_lds + (unsigned)(((t - t_begin + 1) & 3) * 2 * TB);
#pragma unroll
        for (int k = 0; k < 2 * PCS / 4; ++k) {
            const int q = wid + 4 * k;
            const unsigned char* src = (q < PCS ? g_m : g_lm) + (long long)t * TB + (q < PCS ? q : q - PCS) * 1024;
            const unsigned dst = __builtin_amdgcn_readfirstlane(base + (unsigned)q * 1024u);
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(dst), "v"(voff), "s"(src) : "memory", "m0");
        }
    };
    // (l, hard, g_hard) of tile t: slot (t - t_begin) & 1, 3 * PCS pieces: wave w takes pieces w, w + 4, ...
    auto issue_lhg = [&](int t) __attribute__((always_inline)) {
        const unsigned base = smem_lds + (unsigned)(4 * 2 * TB + ((t - t_begin) & 1) * 3 * TB);
#pragma unroll
        for (int k = 0; k < (3 * PCS + 3) / 4; ++k) {
            const int q = wid + 4 * k;
            if (q < 3 * PCS) {
                const int mp = q < PCS ? 0 : (q < 2 * PCS ? 1 : 2);
                const unsigned char* src = (mp == 0 ? g_l : (mp == 1 ? g_h : g_g)) + (long long)t * TB + (q - mp * PCS) * 1024;
                const unsigned dst = __builtin_amdgcn_readfirstlane(base + (unsigned)q * 1024u);
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(dst), "v"(voff), "s"(src) : "memory", "m0");
            }
        }
    };
    if (ml_first < t_begin) issue_ml(ml_first);
    issue_ml(t_begin); issue_lhg(t_begin);
    if (t_begin + 1 <= ml_last) issue_ml(t_begin + 1);

    // the image's per-part constants (uniform): rectangle centre, S and R of the forward pass
    int rcy[P], rcx[P];
    float kS[P], kR[P];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        rcy[c] = (VAR == 0 && p.px) ? p.px[((long long)n * P + c) * 2] : 0;
        rcx[c] = (VAR == 0 && p.px) ? p.px[((long long)n * P + c) * 2 + 1] : 0;
        kS[c] = p.per_np[((long long)n * P + c) * 8];
        kR[c] = p.per_np[((long long)n * P + c) * 8 + 1];
    }
    const float inv_pix = 1.f / (float)((long long)p.n * hw), inv_n = 1.f / (float)p.n;
    const float a8 = p.ms_alpha * 0.125f, a16 = p.ms_alpha * 0.0625f;
    const float wkl = p.w_kl * inv_pix, went = p.w_entropy * inv_pix;
    const float wpatch = p.w_patch * inv_n, warea2 = p.w_area * inv_n * 2.f, wms2 = p.w_ms * inv_n * 2.f;
    const float wmsl = p.w_msl * inv_n, wgmrf = p.w_gmrf * inv_n;

    for (int t = t_begin; t < t_end; ++t) {
        // landed from here on: (m, l_mean) of t - 1, t, t + 1 and (l, hard, g_hard) of t -- all issued before the previous tile's stores
        if (t == t_begin) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(STORES) : "memory");
        __builtin_amdgcn_s_barrier();                 // every wave's pieces are in; every wave has read tile t - 1's results out of LDS
        if (t + 2 <= ml_last) issue_ml(t + 2);        // slot of tile t - 2: free
        if (t + 1 < t_end) issue_lhg(t + 1);          // slot of tile t - 1: free

        const int s4 = (t - t_begin + 1) & 3;
        const float* tm = (const float*)(ML + s4 * 2 * TB);
        const float* tmu = (const float*)(ML + ((s4 + 3) & 3) * 2 * TB);       // the tile above
        const float* tmd = (const float*)(ML + ((s4 + 1) & 3) * 2 * TB);       // the tile below
        float* tl = (float*)(LHG + ((t - t_begin) & 1) * 3 * TB);
        const float* th = tl + 256 * P;
        float* tg = tl + 2 * 256 * P;
        const int q = (t << 8) + tid;
        const int yy = q >> LW, xx = q & (W - 1);
        const bool vr = xx + 1 < W, vd = yy + 1 < p.h, vl = xx > 0, vu = yy > 0;
        // neighbour rows: pixel index within the tile, or in the tile above / below (m at +0, l_mean at +256 * P floats)
        const int iu = tid - W, id = tid + W;
        const float* pu = iu >= 0 ? tm + iu * P : tmu + (iu + 256) * P;          // up
        const float* pur = iu + 1 >= 0 ? tm + (iu + 1) * P : tmu + (iu + 257) * P;   // up-right
        const float* pd = id < 256 ? tm + id * P : tmd + (id - 256) * P;         // down
        const float* pld = id - 1 < 256 ? tm + (id - 1) * P : tmd + (id - 257) * P;  // left-down
        const float* po = tm + tid * P;
        auto ld_row = [&](const float* src, float (&dst)[P]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < P; c += 2) { const float2 v = *(const float2*)(src + c); dst[c] = v.x; dst[c + 1] = v.y; }
        };
        float m[P], l[P], hv[P], gh[P];
        ld_row(po, m); ld_row(tl + tid * P, l); ld_row(th + tid * P, hv); ld_row(tg + tid * P, gh);
        float mx = l[0];
#pragma unroll
        for (int c = 1; c < P; ++c) mx = fmaxf(mx, l[c]);
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < P; ++c) se += __expf(l[c] - mx);
        const float lse = mx + ups_log_fast(se);
        float qs = 0.f, labsum = 0.f;
#pragma unroll
        for (int c = 0; c < P; ++c) { qs += m[c] * (l[c] - lse); labsum += hv[c]; }
        float gm[P], direct[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const float mc = m[c];
            const float pm = (float)P * mc;
            float g = wkl * (ups_log_fast(pm + 1e-20f) + __fdividef(pm, pm + 1e-20f)) + gh[c];
            float dr = went * (-mc * ((l[c] - lse) - qs));
            if (p.entropy_ce) dr += went * (-(hv[c] - mc * labsum));
            if (VAR == 0) {
                const bool in_rect = abs(yy - rcy[c]) <= p.half_h && abs(xx - rcx[c]) <= p.half_w;
                g += in_rect ? 0.f : wpatch;
            }
            g += warea2 * kS[c];
            gm[c] = g; direct[c] = dr;
        }
        {   // Mumford-Shah on the soft masks: own cell, the left neighbour's cell (its right value is me), the upper neighbour's
            float mr[P], md[P], ml[P], mld[P], mu[P], mur[P];
            ld_row(po + P, mr); ld_row(pd, md); ld_row(po - P, ml); ld_row(pld, mld); ld_row(pu, mu); ld_row(pur, mur);
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const float mc = m[c];
                const float m_r = vr ? mr[c] : 0.f, m_d = vd ? md[c] : 0.f;
                float dR = 0.f;
                {
                    const float g = a16 * ((mc - m_r) * (mc - m_r) + (mc - m_d) * (mc - m_d));
                    if (g <= p.ms_lambda) dR += a8 * ((mc - m_r) + (mc - m_d));
                }
                if (vl) {
                    const float m_l = ml[c], m_ld = vd ? mld[c] : 0.f;
                    const float g = a16 * ((m_l - mc) * (m_l - mc) + (m_l - m_ld) * (m_l - m_ld));
                    if (g <= p.ms_lambda) dR -= a8 * (m_l - mc);
                }
                if (vu) {
                    const float m_u = mu[c], m_ur = vr ? mur[c] : 0.f;
                    const float g = a16 * ((m_u - m_ur) * (m_u - m_ur) + (m_u - mc) * (m_u - mc));
                    if (g <= p.ms_lambda) dR -= a8 * (m_u - mc);
                }
                gm[c] += wms2 * kR[c] * dR;
            }
        }
        {   // the noise-free logits: GMRF, and (SB_model48c) the Mumford-Shah stencil on them
            constexpr int LMO = 256 * P;
            float lm[P], lr[P], ld[P], ll[P], lu[P];
            ld_row(po + LMO, lm); ld_row(po + LMO + P, lr); ld_row(pd + LMO, ld); ld_row(po + LMO - P, ll); ld_row(pu + LMO, lu);
            if (VAR == 1) {
                float lld[P], lur[P];
                ld_row(pld + LMO, lld); ld_row(pur + LMO, lur);
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    const float lmc = lm[c];
                    const float l_r = vr ? lr[c] : 0.f, l_d = vd ? ld[c] : 0.f;
                    float dL = 0.f;
                    {
                        const float g = a16 * ((lmc - l_r) * (lmc - l_r) + (lmc - l_d) * (lmc - l_d));
                        if (g <= p.ms_lambda) dL += a8 * ((lmc - l_r) + (lmc - l_d));
                    }
                    if (vl) {
                        const float l_l = ll[c], l_ld = vd ? lld[c] : 0.f;
                        const float g = a16 * ((l_l - lmc) * (l_l - lmc) + (l_l - l_ld) * (l_l - l_ld));
                        if (g <= p.ms_lambda) dL -= a8 * (l_l - lmc);
                    }
                    if (vu) {
                        const float l_u = lu[c], l_ur = vr ? lur[c] : 0.f;
                        const float g = a16 * ((l_u - l_ur) * (l_u - l_ur) + (l_u - lmc) * (l_u - lmc));
                        if (g <= p.ms_lambda) dL -= a8 * (l_u - lmc);
                    }
                    direct[c] += wmsl * dL;
                }
            }
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const float lmc = lm[c];
                float gg = 0.f;
                if (vu) gg += lmc - lu[c];
                if (vd) gg -= ld[c] - lmc;
                if (vl) gg += lmc - ll[c];
                if (vr) gg -= lr[c] - lmc;
                direct[c] += wgmrf * gg;
            }
        }
        float dot = 0.f, dot_r = 0.f;
#pragma unroll
        for (int c = 0; c < P; ++c) { dot += m[c] * gm[c]; dot_r += m[c] * gh[c]; }
#pragma unroll
        for (int c = 0; c < P; c += 2) {
            *(float2*)(tl + tid * P + c) = make_float2(m[c] * (gm[c] - dot) + direct[c], m[c + 1] * (gm[c + 1] - dot) + direct[c + 1]);
            *(float2*)(tg + tid * P + c) = make_float2(m[c] * (gh[c] - dot_r), m[c + 1] * (gh[c + 1] - dot_r));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float4* d0 = (float4*)(p.dl + (img + ((long long)t << 8)) * P);
        float4* d1 = (float4*)(p.dl_rec + (img + ((long long)t << 8)) * P);
        const float4* o0 = (const float4*)tl;
        const float4* o1 = (const float4*)tg;
#pragma unroll
        for (int k = 0; k < STORES; ++k) {          // exactly STORES store instructions per wave (the counted wait above)
            const int j = tid + 256 * k;
            const bool first = j < TB / 16;          // (wave-uniform: TB / 16 is a multiple of 64)
            const float4 v = first ? o0[j] : o1[j - TB / 16];
            float4* dst = first ? d0 + j : d1 + (j - TB / 16);
            *dst = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 6: the prior passes for the part counts the pixel-per-lane RINGS cannot hold (P = 16 / 20 / 25: BASELINE configs #3 / #5 and
// every shipped yaml).  A tile-row of the four maps is 16-25 KB per map at 256 columns; seven slot pairs of them do not fit 160 KB of
// LDS, and the staged kernels above pay for that with a two-row halo around a one-row tile (3x the reads of m and l_mean, one HBM
// round trip per block: prior_bwd at 256x256, P = 20 ran at 0.06 of the HBM roof, 1.27 ms of config #5's step --
// profiles/round6_hbm_kernels.txt).  These forms keep NOTHING in LDS: every row comes straight from global memory (the neighbours' rows
// are the neighbouring lanes' / the next rows' own loads: served by L1 / the XCD's L2, blocks of one image run on one XCD in row order),
// every wait is the compiler's own: no inline-asm loads, no counted waits -- correct by construction.  The first form of the round
// (one thread per pixel, rows in chunks of four or five parts) reached 0.24-0.58 of the roof: 4-6 rows of P floats per thread are
// 224-350 registers -- one or two waves per SIMD -- and a 16-byte load per lane at a 4 P byte stride touches 20-50 cache lines per wave
// instruction.  It is replaced by the chunk-per-lane form below.
template <int P> struct PChunk { static constexpr int N = (P % 4 == 0) ? 4 : ((P % 5 == 0) ? 5 : (P % 2 == 0 ? 2 : 1)); };
template <int N>
__device__ __forceinline__ void ldg_chunk(const float* __restrict__ src, float (&dst)[N]) {
    if constexpr (N == 4) { const float4 v = *(const float4*)src; dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
    else if constexpr (N == 2) { const float2 v = *(const float2*)src; dst[0] = v.x; dst[1] = v.y; }
    else {
#pragma unroll
        for (int e = 0; e < N; ++e) dst[e] = src[e];
    }
}
template <int N>
__device__ __forceinline__ void stg_chunk(float* __restrict__ dst, const float (&v)[N]) {
    if constexpr (N == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else if constexpr (N == 2) *(float2*)dst = make_float2(v[0], v[1]);
    else {
#pragma unroll
        for (int e = 0; e < N; ++e) dst[e] = v[e];
    }
}
// ---------------------------------------------------------------------------------------------------------------------------
// Chunk-per-lane forms (round 6, late).  A lane owns ONE chunk of CH parts of one pixel (P / CH lanes per pixel, 12 or 16 pixels per wave): every wave
// load is 1 KiB of consecutive bytes, a lane's state is a handful of CH-wide arrays, and the per-pixel sums over the parts (soft-max
// normaliser, the two Jacobian dot products) are NCH-term shuffle sums taken in the same order by every lane of the pixel.
template <int P> struct Cpl {
    static constexpr int CH = PChunk<P>::N, NCH = P / CH;       // 4 x 4 (P = 16), 5 x 4 (P = 20), 5 x 5 (P = 25)
    static constexpr int PXW = 64 / NCH, PXB = 4 * PXW;          // pixels per wave / block: 16 / 64, 12 / 48
    static_assert(CH * NCH == P && CH >= 4, "chunks");
};
template <int NCH> __device__ __forceinline__ float cpl_sum(float v, int gb) {
    float s = __shfl(v, gb, 64);
#pragma unroll
    for (int k = 1; k < NCH; ++k) s += __shfl(v, gb + k, 64);
    return s;
}
template <int NCH> __device__ __forceinline__ float cpl_max(float v, int gb) {
    float s = __shfl(v, gb, 64);
#pragma unroll
    for (int k = 1; k < NCH; ++k) s = fmaxf(s, __shfl(v, gb + k, 64));
    return s;
}

// The view-1 backward chunk-per-lane (no stencil: the two Jacobian dot products are the only cross-lane terms).
template <int P, int LW, int VAR>
__global__ __launch_bounds__(256) void prior_bwd1_cpl_kernel(const PriorK p, const int bpi) {
    typedef Cpl<P> C;
    constexpr int W = 1 << LW, CH = C::CH, NCH = C::NCH;
    __shared__ float cst[P][10];       // rcy, rcx, kmax, wv, muy2, mux2, ca, cb, cc, s11
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int hw = p.h * W;
    const int lb = xcd_logical_block();
    const int n = lb / bpi, bi = lb - n * bpi;
    const float inv_pix = 1.f / (float)((long long)p.n * hw), inv_n = 1.f / (float)p.n;
    if (tid < P) {
        const float* np = p.per_np + ((long long)n * P + tid) * 8;
        const float Z = np[1], muy = np[3] / Z, mux = np[4] / Z, k6 = np[5] / Z, k7 = np[6] / Z;
        float* k = cst[tid];
        k[0] = p.px ? (float)p.px[((long long)n * P + tid) * 2] : 0.f;
        k[1] = p.px ? (float)p.px[((long long)n * P + tid) * 2 + 1] : 0.f;
        k[2] = np[0];
        float wv = p.w_var * inv_n * p.gamma * __fdividef(1.f, Z);
        k[4] = 2.f * muy; k[5] = 2.f * mux;
        if (VAR == 1) {
            const float Qyn = k7, Qxn = k6 - k7;
            k[6] = Qyn - 2.f * muy * muy; k[7] = Qxn - 2.f * mux * mux; k[8] = Qyn - muy * muy;
            k[9] = (k6 - k7) - mux * mux;
            wv *= 2.f;
        } else {
            k[6] = k6 - 2.f * muy * muy - 2.f * mux * mux; k[7] = 0.f; k[8] = 0.f; k[9] = 0.f;
        }
        k[3] = wv;
    }
    __syncthreads();
    const float sy = p.h > 1 ? 2.f / (float)(p.h - 1) : 0.f, sx = W > 1 ? 2.f / (float)(W - 1) : 0.f;
    const float wkl = p.w_kl * inv_pix;
    const int pl_raw = lane / NCH, ci = lane - pl_raw * NCH;
    const int pl = min(pl_raw, C::PXW - 1), gb = pl * NCH;
    const int q_raw = bi * C::PXB + wid * C::PXW + pl;
    const bool act = pl_raw < C::PXW && q_raw < hw;
    const int q = min(q_raw, hw - 1);
    const int c0 = ci * CH;
    const int yy = q >> LW, xx = q & (W - 1);
    const float gy = -1.f + sy * (float)yy, gx = -1.f + sx * (float)xx;
    const float gq = gy * gy + gx * gx;
    const long long o0 = ((long long)n * hw + q) * P + c0;
    float m[CH], gh[CH], gmv[CH];
    ldg_chunk<CH>(p.m + o0, m); ldg_chunk<CH>(p.g_hard + o0, gh);
    float dot = 0.f, dot_r = 0.f;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
        const float* k = cst[c0 + e];
        const float mc = m[e];
        const float pm = (float)P * mc;
        float g = wkl * (ups_log_fast(pm + 1e-20f) + __fdividef(pm, pm + 1e-20f)) + gh[e];
        const float sq = __expf(p.gamma * mc - k[2]);
        if (VAR == 1) {
            const float ay = gy * gy - k[4] * gy - k[6];
            const float ax = gx * gx - k[5] * gx - k[7];
            g += k[3] * sq * (k[8] * ay + k[9] * ax);
        } else {
            const float kk = (abs(yy - (int)k[0]) <= p.half_h && abs(xx - (int)k[1]) <= p.half_w) ? 0.f : 1.f;
            const float a = gq - k[4] * gy - k[5] * gx;
            g += k[3] * sq * (a * kk - k[6]);
        }
        gmv[e] = g;
        dot += mc * g; dot_r += mc * gh[e];
    }
    dot = cpl_sum<NCH>(dot, gb); dot_r = cpl_sum<NCH>(dot_r, gb);
    float a[CH], b[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { a[e] = m[e] * (gmv[e] - dot); b[e] = m[e] * (gh[e] - dot_r); }
    if (act) { stg_chunk<CH>(p.dl + o0, a); stg_chunk<CH>(p.dl_rec + o0, b); }
}

// The view-0 forward sums chunk-per-lane: a block walks its pixel range 4 x PXW pixels at a time; a lane keeps the four per-part sums of
// ITS chunk's parts (the chunk index of a lane never changes) and its share of the four pixel sums; one slab record per block, as the
// per-pixel form writes it.
template <int P, int LW, int VAR>
__global__ __launch_bounds__(256) void prior_fwd_cpl_kernel(const PriorK p, const int tiles_per_block, const int bpi, const int spb) {
    typedef Cpl<P> C;
    constexpr int W = 1 << LW, CH = C::CH, NCH = C::NCH;
    __shared__ float cst[P][2];
    __shared__ float part[4][64][4 * CH];
    __shared__ float red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int hw = p.h * W;
    const int lb = xcd_logical_block();
    const int n = lb / bpi, bi = lb - n * bpi;
    if (tid < P) {
        cst[tid][0] = (VAR == 0 && p.px) ? (float)p.px[((long long)n * P + tid) * 2] : 0.f;
        cst[tid][1] = (VAR == 0 && p.px) ? (float)p.px[((long long)n * P + tid) * 2 + 1] : 0.f;
    }
    __syncthreads();
    const int pl_raw = lane / NCH, ci = lane - pl_raw * NCH;
    const int pl = min(pl_raw, C::PXW - 1), gb = pl * NCH;
    const int c0 = ci * CH;
    int cy[CH], cx[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { cy[e] = (int)cst[c0 + e][0]; cx[e] = (int)cst[c0 + e][1]; }
    const long long img = (long long)n * hw;
    const int start = bi * tiles_per_block * 256, end = start + tiles_per_block * 256;
    float kl = 0.f, ent = 0.f, patch = 0.f, gmrf = 0.f;
    float S[CH], R[CH], Rs[CH], Rc[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) S[e] = R[e] = Rs[e] = Rc[e] = 0.f;
    // two steps per trip: the second step's eight chunks are requested before the first step's arithmetic (and the next trip's first
    // step before the second's), so that a round trip to HBM is always in flight under the shuffle / accumulate chains
    struct Px { float l[CH], m[CH], lm[CH], hv[CH], mr[CH], lr[CH], md[CH], ld[CH]; int yy, xx; bool act; };
    auto fetch = [&](int base, Px& r) __attribute__((always_inline)) {
        const int q_raw = base + wid * C::PXW + pl;
        r.act = pl_raw < C::PXW && q_raw < end;
        const int q = min(q_raw, end - 1);
        r.yy = q >> LW; r.xx = q & (W - 1);
        const bool vr = r.xx + 1 < W, vd = r.yy + 1 < p.h;
        const long long o0 = (img + q) * P + c0, oR = (img + (vr ? q + 1 : q)) * P + c0, oD = (img + (vd ? q + W : q)) * P + c0;
        ldg_chunk<CH>(p.l + o0, r.l); ldg_chunk<CH>(p.m + o0, r.m); ldg_chunk<CH>(p.l_mean + o0, r.lm); ldg_chunk<CH>(p.hard + o0, r.hv);
        ldg_chunk<CH>(p.m + oR, r.mr); ldg_chunk<CH>(p.l_mean + oR, r.lr);
        ldg_chunk<CH>(p.m + oD, r.md); ldg_chunk<CH>(p.l_mean + oD, r.ld);
    };
    auto step = [&](const Px& r) __attribute__((always_inline)) {
        const bool vr = r.xx + 1 < W, vd = r.yy + 1 < p.h;
        float mx = r.l[0];
#pragma unroll
        for (int e = 1; e < CH; ++e) mx = fmaxf(mx, r.l[e]);
        mx = cpl_max<NCH>(mx, gb);
        float se = 0.f;
#pragma unroll
        for (int e = 0; e < CH; ++e) se += __expf(r.l[e] - mx);
        se = cpl_sum<NCH>(se, gb);
        const float lse = mx + ups_log_fast(se);
        if (r.act) {
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const float mc = r.m[e];
                kl += mc * ups_log_fast((float)P * mc + 1e-20f);
                ent += -(p.entropy_ce ? r.hv[e] : mc) * (r.l[e] - lse);
                const float lmc = r.lm[e];
                const float lrc = vr ? r.lr[e] : 0.f, ldc = vd ? r.ld[e] : 0.f;
                if (VAR == 0) {
                    const bool in_rect = abs(r.yy - cy[e]) <= p.half_h && abs(r.xx - cx[e]) <= p.half_w;
                    patch += in_rect ? 0.f : r.hv[e];
                } else {
                    const float gw = 0.25f * (lmc - lrc), gh = 0.25f * (lmc - ldc);
                    patch += fminf(p.ms_alpha * (gw * gw + gh * gh), p.ms_lambda);
                }
                if (vd) { const float d = ldc - lmc; gmrf += 0.5f * d * d; }
                if (vr) { const float d = lrc - lmc; gmrf += 0.5f * d * d; }
                const float mrc = vr ? r.mr[e] : 0.f, mdc = vd ? r.md[e] : 0.f;
                const float gw = 0.25f * (mc - mrc), gh = 0.25f * (mc - mdc);
                const float g = p.ms_alpha * (gw * gw + gh * gh);
                const float rr = fminf(g, p.ms_lambda);
                S[e] += mc; R[e] += rr;
                if (g < p.ms_lambda) Rs[e] += rr; else Rc[e] += rr;
            }
        }
    };
    Px pa, pb;
    fetch(start, pa);
    for (int base = start; base < end; base += 2 * C::PXB) {
        fetch(base + C::PXB, pb);              // (past the range: shadows the last pixel, act = false)
        step(pa);
        fetch(base + 2 * C::PXB, pa);
        step(pb);
    }
    kl = wave_sum_full(kl); ent = wave_sum_full(ent); patch = wave_sum_full(patch); gmrf = wave_sum_full(gmrf);
    if (lane == 0) { red[wid][0] = kl; red[wid][1] = ent; red[wid][2] = patch; red[wid][3] = gmrf; }
#pragma unroll
    for (int e = 0; e < CH; ++e) {
        part[wid][lane][e] = S[e]; part[wid][lane][CH + e] = R[e]; part[wid][lane][2 * CH + e] = Rs[e]; part[wid][lane][3 * CH + e] = Rc[e];
    }
    __syncthreads();
    // workspace: glob_partial[n][NSLAB][4], np_partial[n][NSLAB][P][4]; this block owns record bi * spb of image n
    float* gpart = p.ws + ((long long)n * NSLAB + (long long)bi * spb) * 4;
    float* npart = p.ws + (long long)p.n * NSLAB * 4 + ((long long)n * NSLAB + (long long)bi * spb) * P * 4;
    if (tid < 4) gpart[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (tid < 4 * P) {          // part c, sum k (S, R, Rsmooth, Rcontour): the lanes that own chunk c / CH, in a fixed order
        const int c = tid >> 2, k = tid & 3, cc = c / CH, e = c - cc * CH;
        float v = 0.f;
        for (int w = 0; w < 4; ++w)
            for (int q = 0; q < C::PXW; ++q) v += part[w][q * NCH + cc][k * CH + e];
        npart[tid] = v;
    }
}

template <int P, int LW, int VAR>
__global__ __launch_bounds__(256) void prior_bwd0_cpl_kernel(const PriorK p, const int bpi) {
    typedef Cpl<P> C;
    constexpr int W = 1 << LW, CH = C::CH, NCH = C::NCH;
    __shared__ float cst[P][4];                      // rectangle centre (y, x), S, R of the image's parts
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int hw = p.h * W;
    const int lb = xcd_logical_block();
    const int n = lb / bpi, bi = lb - n * bpi;
    if (tid < P) {
        cst[tid][0] = (VAR == 0 && p.px) ? (float)p.px[((long long)n * P + tid) * 2] : 0.f;
        cst[tid][1] = (VAR == 0 && p.px) ? (float)p.px[((long long)n * P + tid) * 2 + 1] : 0.f;
        cst[tid][2] = p.per_np[((long long)n * P + tid) * 8];
        cst[tid][3] = p.per_np[((long long)n * P + tid) * 8 + 1];
    }
    __syncthreads();
    // lane -> (pixel of the wave, chunk); the spare lanes of a wave (60 .. 63 at five chunks per pixel) and the pixels past the image's
    // end shadow a valid pixel: same loads, same shuffles, no store
    const int pl_raw = lane / NCH, ci = lane - pl_raw * NCH;
    const int pl = min(pl_raw, C::PXW - 1), gb = pl * NCH;
    const int q_raw = bi * C::PXB + wid * C::PXW + pl;
    const bool act = pl_raw < C::PXW && q_raw < hw;
    const int q = min(q_raw, hw - 1);
    const int c0 = ci * CH;
    const long long img = (long long)n * hw;
    const int yy = q >> LW, xx = q & (W - 1);
    const bool vr = xx + 1 < W, vd = yy + 1 < p.h, vl = xx > 0, vu = yy > 0;
    const long long o0 = (img + q) * P + c0;
    const long long oR = (img + (vr ? q + 1 : q)) * P + c0, oL = (img + (vl ? q - 1 : q)) * P + c0;
    const long long oD = (img + (vd ? q + W : q)) * P + c0, oU = (img + (vu ? q - W : q)) * P + c0;
    const long long oLD = (img + ((vl && vd) ? q + W - 1 : q)) * P + c0, oUR = (img + ((vu && vr) ? q - W + 1 : q)) * P + c0;
    const float inv_pix = 1.f / (float)((long long)p.n * hw), inv_n = 1.f / (float)p.n;
    const float a8 = p.ms_alpha * 0.125f, a16 = p.ms_alpha * 0.0625f;
    const float wkl = p.w_kl * inv_pix, went = p.w_entropy * inv_pix;
    const float wpatch = p.w_patch * inv_n, warea2 = p.w_area * inv_n * 2.f, wms2 = p.w_ms * inv_n * 2.f;
    const float wmsl = p.w_msl * inv_n, wgmrf = p.w_gmrf * inv_n;

    float m[CH], l[CH], hv[CH], gh[CH];
    ldg_chunk<CH>(p.m + o0, m); ldg_chunk<CH>(p.l + o0, l); ldg_chunk<CH>(p.hard + o0, hv); ldg_chunk<CH>(p.g_hard + o0, gh);
    float mr[CH], md[CH], ml[CH], mld[CH], mu[CH], mur[CH];
    ldg_chunk<CH>(p.m + oR, mr); ldg_chunk<CH>(p.m + oD, md); ldg_chunk<CH>(p.m + oL, ml);
    ldg_chunk<CH>(p.m + oLD, mld); ldg_chunk<CH>(p.m + oU, mu); ldg_chunk<CH>(p.m + oUR, mur);
    float lm[CH], lr[CH], ld[CH], ll[CH], lu[CH];
    ldg_chunk<CH>(p.l_mean + o0, lm); ldg_chunk<CH>(p.l_mean + oR, lr); ldg_chunk<CH>(p.l_mean + oD, ld);
    ldg_chunk<CH>(p.l_mean + oL, ll); ldg_chunk<CH>(p.l_mean + oU, lu);

    float mx = l[0];
#pragma unroll
    for (int e = 1; e < CH; ++e) mx = fmaxf(mx, l[e]);
    mx = cpl_max<NCH>(mx, gb);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < CH; ++e) se += __expf(l[e] - mx);
    se = cpl_sum<NCH>(se, gb);
    const float lse = mx + ups_log_fast(se);
    float qs = 0.f, labsum = 0.f;
#pragma unroll
    for (int e = 0; e < CH; ++e) { qs += m[e] * (l[e] - lse); labsum += hv[e]; }
    qs = cpl_sum<NCH>(qs, gb); labsum = cpl_sum<NCH>(labsum, gb);

    float gm[CH], direct[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
        const int c = c0 + e;
        const float mc = m[e];
        const float pm = (float)P * mc;
        float g = wkl * (ups_log_fast(pm + 1e-20f) + __fdividef(pm, pm + 1e-20f)) + gh[e];
        float dr = went * (-mc * ((l[e] - lse) - qs));
        if (p.entropy_ce) dr += went * (-(hv[e] - mc * labsum));
        if (VAR == 0) {
            const bool in_rect = abs(yy - (int)cst[c][0]) <= p.half_h && abs(xx - (int)cst[c][1]) <= p.half_w;
            g += in_rect ? 0.f : wpatch;
        }
        g += warea2 * cst[c][2];
        // Mumford-Shah on the soft masks: own cell, the left neighbour's cell, the upper neighbour's
        const float m_r = vr ? mr[e] : 0.f, m_d = vd ? md[e] : 0.f;
        float dR = 0.f;
        {
            const float gg = a16 * ((mc - m_r) * (mc - m_r) + (mc - m_d) * (mc - m_d));
            if (gg <= p.ms_lambda) dR += a8 * ((mc - m_r) + (mc - m_d));
        }
        if (vl) {
            const float m_l = ml[e], m_ld = vd ? mld[e] : 0.f;
            const float gg = a16 * ((m_l - mc) * (m_l - mc) + (m_l - m_ld) * (m_l - m_ld));
            if (gg <= p.ms_lambda) dR -= a8 * (m_l - mc);
        }
        if (vu) {
            const float m_u = mu[e], m_ur = vr ? mur[e] : 0.f;
            const float gg = a16 * ((m_u - m_ur) * (m_u - m_ur) + (m_u - mc) * (m_u - mc));
            if (gg <= p.ms_lambda) dR -= a8 * (m_u - mc);
        }
        g += wms2 * cst[c][3] * dR;
        // the noise-free logits: GMRF term
        const float lmc = lm[e];
        float gg = 0.f;
        if (vu) gg += lmc - lu[e];
        if (vd) gg -= ld[e] - lmc;
        if (vl) gg += lmc - ll[e];
        if (vr) gg -= lr[e] - lmc;
        dr += wgmrf * gg;
        gm[e] = g; direct[e] = dr;
    }
    if (VAR == 1) {         // (SB_model48c) the Mumford-Shah stencil on the logits too
        float lld[CH], lur[CH];
        ldg_chunk<CH>(p.l_mean + oLD, lld); ldg_chunk<CH>(p.l_mean + oUR, lur);
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const float lmc = lm[e];
            const float l_r = vr ? lr[e] : 0.f, l_d = vd ? ld[e] : 0.f;
            float dL = 0.f;
            {
                const float gg = a16 * ((lmc - l_r) * (lmc - l_r) + (lmc - l_d) * (lmc - l_d));
                if (gg <= p.ms_lambda) dL += a8 * ((lmc - l_r) + (lmc - l_d));
            }
            if (vl) {
                const float l_l = ll[e], l_ld = vd ? lld[e] : 0.f;
                const float gg = a16 * ((l_l - lmc) * (l_l - lmc) + (l_l - l_ld) * (l_l - l_ld));
                if (gg <= p.ms_lambda) dL -= a8 * (l_l - lmc);
            }
            if (vu) {
                const float l_u = lu[e], l_ur = vr ? lur[e] : 0.f;
                const float gg = a16 * ((l_u - l_ur) * (l_u - l_ur) + (l_u - lmc) * (l_u - lmc));
                if (gg <= p.ms_lambda) dL -= a8 * (l_u - lmc);
            }
            direct[e] += wmsl * dL;
        }
    }
    float dot = 0.f, dot_r = 0.f;
#pragma unroll
    for (int e = 0; e < CH; ++e) { dot += m[e] * gm[e]; dot_r += m[e] * gh[e]; }
    dot = cpl_sum<NCH>(dot, gb); dot_r = cpl_sum<NCH>(dot_r, gb);
    float a[CH], b[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { a[e] = m[e] * (gm[e] - dot) + direct[e]; b[e] = m[e] * (gh[e] - dot_r); }
    if (act) { stg_chunk<CH>(p.dl + o0, a); stg_chunk<CH>(p.dl_rec + o0, b); }
}

// Test hook: UPS_PRIOR_PX_BPI caps the blocks per image of the pixel-per-lane kernels, so that a three-image test walks the multi-tile
// loops (ring slots, counted waits) the 64-image benchmark shape walks.  Read at every call (microseconds).
int px_bpi_cap() { const int v = (int)ups_env_int_now("UPS_PRIOR_PX_BPI", 0); return v > 0 ? v : (1 << 30); }
int gp_of(int P) { int g = 2; while (g < P) g *= 2; return g; }

PriorK to_k(const ups_prior_desc* d, float* ws) {
    PriorK k;
    k.n = d->n; k.h = d->h; k.w = d->w; k.P = d->P; k.view = d->view; k.entropy_ce = d->entropy_ce;
    k.half_h = d->half_h; k.half_w = d->half_w; k.gamma = d->gamma; k.ms_alpha = d->ms_alpha; k.ms_lambda = d->ms_lambda;
    k.w_kl = d->w_kl; k.w_entropy = d->w_entropy; k.w_ms = d->w_ms; k.w_area = d->w_area; k.w_patch = d->w_patch;
    k.w_gmrf = d->w_gmrf; k.w_var = d->w_var; k.variant = d->variant; k.w_msl = d->w_ms_logits;
    k.l = d->l; k.l_mean = d->l_mean; k.m = d->m; k.hard = d->hard; k.px = d->px; k.per_np = d->per_np; k.sums = d->sums;
    k.g_hard = d->g_hard; k.dl = d->dl; k.ws = ws; k.dl_rec = d->dl_rec;
    return k;
}

}  // namespace

// (P, w, variant) -> template arguments, here and nowhere else: every launcher below names its kernel in a lambda over the
// std::integral_constants these two hand it.  Every instance with dynamic LDS may need more than the 64 KB default.
constexpr size_t PRIOR_LDS = 160 * 1024;

// The staged kernels KERNEL<PC, LW>: specialised instances for the part counts of the shipped / benchmark configs and 128- / 256-wide
// images, the generic <0, -1> instance otherwise.
template <typename F>
static int prior_dispatch_staged(const ups_prior_desc* d, F&& f) {
    const int lw = d->w == 128 ? 7 : (d->w == 256 ? 8 : -1);
    if (lw < 0 || !(d->P == 10 || d->P == 16 || d->P == 20 || d->P == 25)) return f(std::integral_constant<int, 0>{}, std::integral_constant<int, -1>{});
    return ups_pick<10, 16, 20, 25>(d->P, [&](auto PC) { return ups_pick<7, 8>(lw, [&](auto LW) { return f(PC, LW); }); });
}
// The pixel-per-lane (PS = 10) and chunk-per-lane (PS = 16, 20, 25) kernels KERNEL<P, LW, VAR> of a descriptor their `eligible` took.
template <int... PS, typename F>
static int prior_dispatch(const ups_prior_desc* d, F&& f) {
    return ups_pick<PS...>(d->P, [&](auto PC) {
        return ups_pick<7, 8>(d->w == 128 ? 7 : 8, [&](auto LW) {
            return ups_pick<0, 1>(d->variant == 0 ? 0 : 1, [&](auto VAR) { return f(PC, LW, VAR); });
        });
    });
}
// What both of those forms ask of a descriptor: the view, 128- / 256-wide images in whole 256-pixel tiles, and every map the kernel
// touches present and 16-byte aligned.
static bool prior_tiles_ok(const ups_prior_desc* d, int view, std::initializer_list<const void*> maps) {
    uintptr_t all = 0;
    for (const void* m : maps) { if (!m) return false; all |= (uintptr_t)m; }
    return d->view == view && (d->w == 128 || d->w == 256) && ((long long)d->h * d->w) % 256 == 0 && (all & 15) == 0;
}
// pixel-per-lane form (round 5): P = 10
static bool px_eligible(const ups_prior_desc* d, int view, std::initializer_list<const void*> maps) {
    return d->P == 10 && prior_tiles_ok(d, view, maps);
}
// chunk-per-lane, direct-from-global form (round 6): the part counts the rings cannot hold (UPS_PRIOR_DIRECT=0: off)
static bool cpl_eligible(const ups_prior_desc* d, int view, std::initializer_list<const void*> maps) {
    return UPS_ENV_ON_CACHED("UPS_PRIOR_DIRECT") && (d->P == 16 || d->P == 20 || d->P == 25) && prior_tiles_ok(d, view, maps);
}

extern "C" size_t ups_prior_sums_floats(int32_t n, int32_t P) { return 16 + (size_t)n * NSLAB * 4 + (size_t)n * NSLAB * P * 4 + (size_t)n * 8; }

// workspace convention: `sums` points at 16 floats followed by n*NSLAB*4 + n*NSLAB*P*4 + n*8 floats of scratch.
extern "C" int ups_prior_fwd(const ups_prior_desc* d, void* stream) {
    UPS_CHECK_ARG(d && d->m && d->sums && d->P >= 1 && d->P <= 64 && d->n > 0);
    UPS_CHECK_ARG(d->view == 1 || (d->l && d->l_mean && d->hard && (d->px || d->variant == 1) && d->per_np));
    hipStream_t s = (hipStream_t)stream;
    PriorK k = to_k(d, d->sums + 16);
    const int tiles_img = (int)((long long)d->h * d->w / 256);     // (of the two tiled forms)
    if (px_eligible(d, 0, {d->m, d->l_mean, d->l, d->hard})) {   // pixel-per-lane form: tiles that deal evenly onto the slab records
        // blocks per image: enough blocks for one per CU, a power of two that divides both the tiles and the NSLAB slab records
        int bpi = 1;
        const int cap = px_bpi_cap();
        while (2 * bpi <= cap && bpi < NSLAB && bpi < tiles_img && (long long)d->n * bpi < 256 && tiles_img % (2 * bpi) == 0) bpi *= 2;
        if (tiles_img % bpi == 0 && NSLAB % bpi == 0) {
            constexpr size_t shm_px = 7 * 2 * (size_t)(256 * 10 * 4) + 4 * (4 + 4 * 10) * sizeof(float);
            const dim3 grid(d->n * bpi);
            const int tpb = tiles_img / bpi, spb = NSLAB / bpi;
            const int rc = prior_dispatch<10>(d, [&](auto PC, auto LW, auto VAR) {
                return ups_launch_lds<prior_fwd_px_kernel<PC(), LW(), VAR()>>("prior_fwd_px_kernel", shm_px, grid, dim3(256), shm_px, s, k, tpb, spb);
            });
            if (rc != UPS_OK) return rc;
            UPS_LAUNCH_CHECK();
            hipLaunchKernelGGL(prior_finalize_px_kernel, dim3(1), dim3(1024), 0, s, k, bpi, spb);
            UPS_LAUNCH_CHECK();
            return UPS_OK;
        }
    }
    if (cpl_eligible(d, 0, {d->m, d->l_mean, d->l, d->hard})) {   // direct-from-global form: one slab record per block
        // blocks per image: a power of two that divides the tiles and the NSLAB slab records, two blocks per CU: every record is one more
        // row for the one-block finalize, whose round trips to the other XCDs' records are what a finer grid pays for (measured:
        // 2 048 / 1 024 / 512 blocks = 0.43 / 0.46 / 0.51 of the HBM roof at P = 25, B = 64)
        int bpi = 1;
        while (bpi < NSLAB && (long long)d->n * bpi < 512 && tiles_img % (2 * bpi) == 0) bpi *= 2;
        const dim3 grid(d->n * bpi);
        const int tpb = tiles_img / bpi, spb = NSLAB / bpi;
        const int rc = prior_dispatch<16, 20, 25>(d, [&](auto PC, auto LW, auto VAR) {
            hipLaunchKernelGGL((prior_fwd_cpl_kernel<PC(), LW(), VAR()>), grid, dim3(256), 0, s, k, tpb, bpi, spb);
            return UPS_OK;
        });
        if (rc != UPS_OK) return rc;
        UPS_LAUNCH_CHECK();
        hipLaunchKernelGGL(prior_finalize_px_kernel, dim3(1), dim3(1024), 0, s, k, bpi, spb);
        UPS_LAUNCH_CHECK();
        return UPS_OK;
    }
    const int rows = ups_cdiv(d->h, NSLAB);
    const int PP = d->P | 1, NS = 256 / d->P;
    auto lds_fl = [&](int t) {
        return (d->view == 0 ? (size_t)(4 * t + 2 * (d->w + 1)) : (size_t)t) * PP + (size_t)NS * d->P * 4 + 4 + 2 * d->P + (size_t)t;
    };
    int tpx = 256;
    while (tpx > 32 && lds_fl(tpx) * 4 > 48 * 1024) tpx >>= 1;
    const size_t shm = lds_fl(tpx) * sizeof(float);
    UPS_CHECK_ARG(shm <= 160 * 1024);
    const int rc = prior_dispatch_staged(d, [&](auto PC, auto LW) {
        return ups_launch_lds<prior_fwd_kernel<PC(), LW()>>("prior_fwd_kernel", PRIOR_LDS, dim3(d->n * NSLAB), dim3(256), shm, s, k, rows, tpx);
    });
    if (rc != UPS_OK) return rc;
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(prior_finalize_img_kernel, dim3(d->n), dim3(256), 0, s, k);
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(prior_finalize_kernel, dim3(1), dim3(256), 0, s, k);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_prior_bwd(const ups_prior_desc* d, void* stream) {
    UPS_CHECK_ARG(d && d->m && d->dl && d->per_np && (d->px || d->variant == 1) && d->P >= 1 && d->P <= 64);
    UPS_CHECK_ARG(d->view == 1 || (d->l && d->l_mean && d->hard));
    hipStream_t s = (hipStream_t)stream;
    PriorK k = to_k(d, nullptr);
    // (the tiled forms: both result maps asked for; view 0 reads the logits and the hard mask too)
    const long long hw = (long long)d->h * d->w;
    const int tiles_img = (int)(hw / 256);
    if (px_eligible(d, 1, {d->m, d->g_hard, d->dl, d->dl_rec})) {   // pixel-per-lane form of the view-1 backward
        int bpi = 1;          // ~two blocks per CU
        const int cap = px_bpi_cap();
        while (2 * bpi <= cap && bpi < tiles_img && (long long)d->n * bpi < 512 && tiles_img % (2 * bpi) == 0) bpi *= 2;
        constexpr size_t shm_px = 3 * 2 * (size_t)(256 * 10 * 4) + 10 * 8 * sizeof(float);
        const dim3 grid(d->n * bpi);
        const int tpb = tiles_img / bpi;
        const int rc = prior_dispatch<10>(d, [&](auto PC, auto LW, auto VAR) {
            return ups_launch_lds<prior_bwd1_px_kernel<PC(), LW(), VAR()>>("prior_bwd1_px_kernel", shm_px, grid, dim3(256), shm_px, s, k, tpb);
        });
        if (rc != UPS_OK) return rc;
        UPS_LAUNCH_CHECK();
        return UPS_OK;
    }
    if (px_eligible(d, 0, {d->m, d->g_hard, d->dl, d->dl_rec, d->l, d->l_mean, d->hard})) {
        int bpi = 1;          // one block per CU
        const int cap = px_bpi_cap();
        while (2 * bpi <= cap && bpi < tiles_img && (long long)d->n * bpi < 256 && tiles_img % (2 * bpi) == 0) bpi *= 2;
        constexpr size_t shm_px = (4 * 2 + 2 * 3) * (size_t)(256 * 10 * 4);
        const dim3 grid(d->n * bpi);
        const int tpb = tiles_img / bpi;
        const int rc = prior_dispatch<10>(d, [&](auto PC, auto LW, auto VAR) {
            return ups_launch_lds<prior_bwd0_px_kernel<PC(), LW(), VAR()>>("prior_bwd0_px_kernel", shm_px, grid, dim3(256), shm_px, s, k, tpb);
        });
        if (rc != UPS_OK) return rc;
        UPS_LAUNCH_CHECK();
        return UPS_OK;
    }
    // direct-from-global forms: a grid of chunks of PXB pixels that fits 32 bits
    if (cpl_eligible(d, 1, {d->m, d->g_hard, d->dl, d->dl_rec}) && d->n * (hw / 256) < (1ll << 31)) {
        const int bpi_c = (int)ups_cdiv(hw, d->P == 16 ? Cpl<16>::PXB : Cpl<20>::PXB);
        const dim3 grid((unsigned)(d->n * (long long)bpi_c));
        const int rc = prior_dispatch<16, 20, 25>(d, [&](auto PC, auto LW, auto VAR) {
            hipLaunchKernelGGL((prior_bwd1_cpl_kernel<PC(), LW(), VAR()>), grid, dim3(256), 0, s, k, bpi_c);
            return UPS_OK;
        });
        if (rc != UPS_OK) return rc;
        UPS_LAUNCH_CHECK();
        return UPS_OK;
    }
    if (cpl_eligible(d, 0, {d->m, d->l_mean, d->l, d->hard, d->g_hard, d->dl, d->dl_rec}) && d->n * (hw / 256) < (1ll << 31)) {
        const int bpi_c = (int)ups_cdiv(hw, d->P == 16 ? Cpl<16>::PXB : Cpl<20>::PXB);
        const dim3 grid((unsigned)(d->n * (long long)bpi_c));
        const int rc = prior_dispatch<16, 20, 25>(d, [&](auto PC, auto LW, auto VAR) {
            hipLaunchKernelGGL((prior_bwd0_cpl_kernel<PC(), LW(), VAR()>), grid, dim3(256), 0, s, k, bpi_c);
            return UPS_OK;
        });
        if (rc != UPS_OK) return rc;
        UPS_LAUNCH_CHECK();
        return UPS_OK;
    }
    const int PP = d->P | 1;
    auto lds_fl = [&](int t) { return ((d->view == 0 ? (size_t)(5 * t + 4 * d->w) : (size_t)(4 * t)) * PP + (size_t)d->P * 8 + (size_t)t * 4); };
    int tpx = 256;
    while (tpx > 32 && lds_fl(tpx) * 4 > 56 * 1024) tpx >>= 1;
    const size_t shm = lds_fl(tpx) * sizeof(float);
    UPS_CHECK_ARG(shm <= 160 * 1024);
    const dim3 grid(ups_cdiv((long long)d->h * d->w, tpx) * d->n);
    const int rc = prior_dispatch_staged(d, [&](auto PC, auto LW) {
        return ups_launch_lds<prior_bwd_kernel<PC(), LW()>>("prior_bwd_kernel", PRIOR_LDS, grid, dim3(256), shm, s, k, tpx);
    });
    if (rc != UPS_OK) return rc;
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
