// Landmark regression evaluation (declared in include/upsparts_hip.h): ups_part_moments -- mass and centre of every part of every
// image, from the soft map and from the arg-max map -- ups_landmark_gram -- per keypoint, the normal equations of a linear map from
// the part centres to the keypoint, over the instances where the keypoint is visible -- ups_landmark_solve -- their ridge solution by
// Cholesky -- and ups_landmark_predict.  Neither the reference nor any library this tree links has these; the definitions are this
// project's own and tests/landmarks_ref.py restates all four in NumPy float64 with equal bits.
//
// Arithmetic is fp64, every multiplication, addition, division and square root rounded once (no contraction: pragma below), no
// floating-point atomics, every order of summation fixed: two calls give the same bits.
//
// ups_part_moments.  A streaming kernel: soft [N,h,w,P] fp32 is read once (84 MB at N = 128, 128 x 128, P = 10), everything else is
// small.  One 256-thread block per (image, chunk of kMChunk = 256 pixels).  The chunk's 256 P floats are contiguous in memory: the
// block loads them with lane-consecutive dword loads (a wave instruction = 256 contiguous bytes; a chunk starts at a multiple of
// 1024 P bytes only within its image, images start anywhere, so no wider load is assumed) into LDS, thread j computes pixel j's
// (u_x, u_y) -- the two divisions of the kernel -- into LDS, and, when there is an arg-max map, adds its pixel to the chunk's integer
// sums (LDS integer atomics, one global add per block, part and sum).  Then thread (g, p), p = tid mod Pp, g = tid / Pp with
// Pp = the power of two >= P, adds pixels g Pp .. g Pp + Pp - 1 of part p in ascending order from 0.0 into three accumulators
// (s, s u_x, s u_y: the converted fp32 value, each product rounded), and a fixed LDS tree over g (t[g] += t[g + s], s = G/2 .. 1,
// G = 256 / Pp) leaves the block's partial, written to caller-owned scratch.  Pixels past the image's end are zeros with u = 0.
// LDS reads of the accumulation: lanes of one g read P consecutive floats, lanes of different g are Pp P floats apart -- a 2- or
// 4-way bank conflict for small P, on a kernel whose LDS traffic is a tenth of what the LDS delivers per HBM byte: left alone.
// The loads of a chunk are issued in batches of 8 per thread before any is stored (a rolled load-then-store loop pays a memory latency
// per P).  ups_part_moments' second launch: one block per image stages the image's partials through LDS (all loads of a tile in flight
// together), thread e < 3 P adds entry e in chunk order, thread p < P divides and writes mass, centre, valid.
//
// ups_landmark_gram.  One 256-thread block per (chunk of kLChunk = 64 items, keypoint).  The chunk's features with the constant 1
// appended ([item][D] doubles, <= 33 KB), the keypoint's targets and visibility sit in LDS; thread e of the D D + 2 D + 1 outputs
// (G[a][b], R[a][c], the count) runs over the chunk's items in ascending order from 0.0 and SKIPS the invisible ones, so a target
// that is not visible may hold anything.  G[a][b] and G[b][a] are the same products in the same order: G is symmetric in bits.
// The second launch adds the partials in chunk order.
//
// ups_landmark_solve.  One 256-thread block per keypoint; A = G_k + lambda diag(1, .., 1, 0) and its factor in LDS ([D][D + 1]
// doubles).  Left-looking Cholesky, one barrier per column: every thread computes the pivot of column j itself (the same chain, the
// same bits: the decision "not positive or not finite" is uniform and the block leaves together), thread i > j its own row's
// element.  The two substitutions are right-looking -- thread (i, c) keeps r = rhs[i][c], and once x[m] is final every later row
// subtracts L x[m] -- which gives each row the subtraction chain in ascending m (forward) or descending m (backward): one barrier
// per step.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kMChunk = 256;                     // pixels per ups_part_moments block (= kBlock: thread j owns pixel j)
constexpr int kMaxP = 32;
constexpr int kMLoads = 8;                       // loads in flight per thread while a chunk is staged
constexpr int kFLoads = 12;                      // loads per thread and tile of the second launch
constexpr int kFTile = kFLoads * kBlock;         // doubles per tile of the second launch: at least 32 chunks' partials
constexpr int kLChunk = 64;                      // items per ups_landmark_gram block
constexpr int kMaxD = 65;
constexpr int kMaxKp = 32;
constexpr int kLS = kMaxD + 1;                   // row stride of the solve's matrix, in doubles
constexpr long long kIntMax = 0x7fffffffLL;
static_assert(kMChunk == kBlock, "thread j owns pixel j of the chunk");
static_assert(kMChunk * kMaxP * 4 + 2 * kMChunk * 8 + 3 * kBlock * 8 + kMaxP * 3 * 4 + 4 <= 65536, "static LDS (moments)");
static_assert(kFTile / (3 * kMaxP) >= 1 && kFTile * 8 + 3 * kMaxP * 8 <= 65536, "a tile of the second launch holds whole chunks");
static_assert(kLChunk * kMaxD * 8 + kLChunk * 2 * 8 + kLChunk <= 65536, "static LDS (gram)");
static_assert(kMaxD * kLS * 8 + 2 * kMaxD * 2 * 8 <= 65536, "static LDS (solve)");
static_assert(2 * kMaxD <= kBlock, "a thread per (row, coordinate) of the substitutions");

__device__ __forceinline__ bool finite64(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL; }

__global__ __launch_bounds__(kBlock) void part_moments_kernel(const float* __restrict__ soft, const long long* __restrict__ pred, int h,
                                                              int w, int P, int Pp, int chunks, double* __restrict__ partials,
                                                              int* __restrict__ hard, int* __restrict__ invalid) {
    extern __shared__ float sv[];                // [kMChunk][P]: sized by the launch, so that a small P keeps more blocks per CU
    __shared__ double ux[kMChunk], uy[kMChunk];
    __shared__ double red[3 * kBlock];
    __shared__ int bins[kMaxP * 3];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const int img = blockIdx.x / chunks;
    const int HW = h * w, px0 = (blockIdx.x - img * chunks) * kMChunk;
    const int npx = min(kMChunk, HW - px0);
    if (tid < 3 * P) bins[tid] = 0;
    if (tid == 0) bad = 0;
    const long long pv = (pred && tid < npx) ? pred[(long long)img * HW + px0 + tid] : 0;
    const int y = (px0 + tid) / w, x = (px0 + tid) - y * w;
    const int ix = 2 * x + 1 - w, iy = 2 * y + 1 - h;
    {
        // batches of kMLoads loads per thread, issued together on clamped (always valid) addresses and stored once all have arrived: a
        // rolled loop of load-then-store paid one memory latency per P
        const float* src = soft + ((long long)img * HW + px0) * P;
        const int n = npx * P, total = kMChunk * P;
        for (int base = 0; base < total; base += kMLoads * kBlock) {
            float v[kMLoads];
#pragma unroll
            for (int k = 0; k < kMLoads; ++k)
                if (base + k * kBlock < total) v[k] = src[min(base + k * kBlock + tid, n - 1)];      // (a block-uniform test)
            if (base == 0) {                     // the two divisions, under the first batch's latency
                ux[tid] = tid < npx ? (double)ix / (double)w : 0.0;
                uy[tid] = tid < npx ? (double)iy / (double)h : 0.0;
            }
#pragma unroll
            for (int k = 0; k < kMLoads; ++k) {
                const int i = base + k * kBlock + tid;
                if (base + k * kBlock < total) sv[i] = i < n ? v[k] : 0.f;
            }
        }
    }
    __syncthreads();
    if (pred && tid < npx) {
        if ((unsigned long long)pv < (unsigned long long)P) {
            atomicAdd(&bins[(int)pv * 3], 1);
            atomicAdd(&bins[(int)pv * 3 + 1], ix);
            atomicAdd(&bins[(int)pv * 3 + 2], iy);
        } else {
            atomicAdd(&bad, 1);
        }
    }
    const int p = tid & (Pp - 1), g = tid / Pp;
    double m = 0.0, sx = 0.0, sy = 0.0;
    if (p < P) {
        const int j0 = g * Pp;
        for (int i = 0; i < Pp; ++i) {
            const double s = (double)sv[(j0 + i) * P + p];
            m = m + s;
            sx = sx + s * ux[j0 + i];
            sy = sy + s * uy[j0 + i];
        }
    }
    red[tid] = m;
    red[kBlock + tid] = sx;
    red[2 * kBlock + tid] = sy;
    for (int s = kBlock / Pp / 2; s > 0; s >>= 1) {          // fixed tree over g; its barriers also order the LDS atomics above
        __syncthreads();
        if (g < s) {
            red[tid] = red[tid] + red[tid + s * Pp];
            red[kBlock + tid] = red[kBlock + tid] + red[kBlock + tid + s * Pp];
            red[2 * kBlock + tid] = red[2 * kBlock + tid] + red[2 * kBlock + tid + s * Pp];
        }
    }
    __syncthreads();
    if (tid < 3 * P) {                                       // partials [block][3][P]
        const int k = tid / P, pp = tid - k * P;
        partials[(long long)blockIdx.x * 3 * P + tid] = red[k * kBlock + pp];
    }
    if (pred) {
        if (tid < 3 * P && bins[tid / 3 * 3]) atomicAdd(&hard[(long long)img * P * 3 + tid], bins[tid]);
        if (tid == 0 && bad) atomicAdd(invalid, bad);
    }
}

// One block per image.  The image's partials ([chunk][3][P], contiguous) come through LDS in tiles of whole chunks, every thread's loads of
// a tile issued together; thread e < 3 P adds entry e over the chunks in chunk order; thread p < P divides.
__global__ __launch_bounds__(kBlock) void part_moments_finish_kernel(const double* __restrict__ partials, int P, int chunks,
                                                                     double min_mass, double* __restrict__ mass,
                                                                     double* __restrict__ centre, unsigned char* __restrict__ valid) {
    __shared__ double tile[kFTile];
    __shared__ double acc[3 * kMaxP];
    const int tid = threadIdx.x, img = blockIdx.x, E = 3 * P;
    const double* src = partials + (long long)img * chunks * E;
    const int per = kFTile / E;                  // chunks per tile (>= 32)
    double a = 0.0;
    for (int c0 = 0; c0 < chunks; c0 += per) {
        const int nc = min(per, chunks - c0), cnt = nc * E;
        double v[kFLoads];
#pragma unroll
        for (int k = 0; k < kFLoads; ++k)
            if (k * kBlock < cnt) v[k] = src[(long long)c0 * E + min(k * kBlock + tid, cnt - 1)];
        __syncthreads();                         // the previous tile's reads are done
#pragma unroll
        for (int k = 0; k < kFLoads; ++k)
            if (k * kBlock + tid < cnt) tile[k * kBlock + tid] = v[k];
        __syncthreads();
        if (tid < E) {
#pragma unroll 8
            for (int c = 0; c < nc; ++c) a = a + tile[c * E + tid];
        }
    }
    if (tid < E) acc[tid] = a;
    __syncthreads();
    if (tid < P) {
        const double m = acc[tid], sx = acc[P + tid], sy = acc[2 * P + tid];
        const bool ok = finite64(m) && m > 0.0 && m >= min_mass;
        const long long t = (long long)img * P + tid;
        mass[t] = m;
        centre[2 * t] = ok ? sx / m : 0.0;
        centre[2 * t + 1] = ok ? sy / m : 0.0;
        valid[t] = ok ? 1 : 0;
    }
}

// outputs per keypoint: G [D][D], R [D][2], the count
__host__ __device__ inline int gram_outputs(int D) { return D * D + 2 * D + 1; }

__global__ __launch_bounds__(kBlock) void landmark_gram_kernel(const double* __restrict__ feat, const double* __restrict__ target,
                                                               const unsigned char* __restrict__ vis, int N, int D, int K,
                                                               double* __restrict__ partials) {
    __shared__ double f[kLChunk * kMaxD];
    __shared__ double tg[kLChunk * 2];
    __shared__ unsigned char vs[kLChunk];
    const int tid = threadIdx.x;
    const int c = blockIdx.x / K, k = blockIdx.x - c * K;
    const int n0 = c * kLChunk, nn = min(kLChunk, N - n0);
    for (int i = tid; i < nn * D; i += kBlock) {
        const int n = i / D, a = i - n * D;
        f[i] = a < D - 1 ? feat[(long long)(n0 + n) * (D - 1) + a] : 1.0;
    }
    if (tid < nn) vs[tid] = vis[(long long)(n0 + tid) * K + k];
    __syncthreads();
    if (tid < 2 * nn && vs[tid >> 1]) tg[tid] = target[((long long)(n0 + (tid >> 1)) * K + k) * 2 + (tid & 1)];
    __syncthreads();
    const int E = gram_outputs(D);
    for (int e = tid; e < E; e += kBlock) {
        double acc = 0.0;
        if (e < D * D) {
            const int a = e / D, b = e - a * D;
            for (int n = 0; n < nn; ++n)
                if (vs[n]) acc = acc + f[n * D + a] * f[n * D + b];
        } else if (e < E - 1) {
            const int a = (e - D * D) >> 1, cc = (e - D * D) & 1;
            for (int n = 0; n < nn; ++n)
                if (vs[n]) acc = acc + f[n * D + a] * tg[2 * n + cc];
        } else {
            int cnt = 0;
            for (int n = 0; n < nn; ++n) cnt += vs[n] ? 1 : 0;
            acc = (double)cnt;
        }
        partials[(long long)blockIdx.x * E + e] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void landmark_gram_finish_kernel(const double* __restrict__ partials, int D, int K, int chunks,
                                                                      double* __restrict__ G, double* __restrict__ R,
                                                                      int* __restrict__ cnt) {
    const int E = gram_outputs(D);
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= K * E) return;
    const int k = t / E, e = t - k * E;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + partials[((long long)c * K + k) * E + e];
    if (e < D * D) G[(long long)k * D * D + e] = s;
    else if (e < E - 1) R[(long long)k * 2 * D + (e - D * D)] = s;
    else cnt[k] = (int)s;                                    // (a sum of integers below 2^31: exact)
}

__global__ __launch_bounds__(kBlock) void landmark_solve_kernel(const double* __restrict__ G, const double* __restrict__ R,
                                                                const int* __restrict__ cnt, int D, double lambda,
                                                                double* __restrict__ W, int* __restrict__ n_singular) {
    __shared__ double A[kMaxD * kLS];            // the lower triangle becomes L
    __shared__ double xs[2 * kMaxD];             // the substitutions' finished entries [m][c]
    const int tid = threadIdx.x, k = blockIdx.x;
    const double* Gk = G + (long long)k * D * D;
    for (int e = tid; e < D * D; e += kBlock) {
        const int a = e / D, b = e - a * D;
        const double v = Gk[e];
        A[a * kLS + b] = (a == b && a < D - 1) ? v + lambda : v;
    }
    __syncthreads();
    bool bad = cnt[k] <= 0;                      // uniform
    const int i = tid;
    for (int j = 0; j < D && !bad; ++j) {
        double d = A[j * kLS + j];
        for (int m = 0; m < j; ++m) d = d - A[j * kLS + m] * A[j * kLS + m];
        if (!(d > 0.0) || !finite64(d)) {
            bad = true;                          // every thread computed the same d: the block leaves together
            break;
        }
        const double l = __dsqrt_rn(d);
        double v = 0.0;
        if (i > j && i < D) {
            v = A[i * kLS + j];
            for (int m = 0; m < j; ++m) v = v - A[i * kLS + m] * A[j * kLS + m];
            v = v / l;
        }
        __syncthreads();                         // every read of column j's old contents (A[i][j], A[j][j]) is done
        if (i == j) A[j * kLS + j] = l;
        else if (i > j && i < D) A[i * kLS + j] = v;
        __syncthreads();
    }
    double* Wk = W + (long long)k * 2 * D;
    if (bad) {
        if (tid < 2 * D) Wk[tid] = 0.0;
        if (tid == 0) atomicAdd(n_singular, 1);
        return;
    }
    const int r = tid >> 1, c = tid & 1;         // thread (row r, coordinate c)
    const bool mine = r < D;
    double v = mine ? R[(long long)k * 2 * D + tid] : 0.0;
    for (int m = 0; m < D; ++m) {                // L y = R
        if (mine && r == m) {
            v = v / A[m * kLS + m];
            xs[2 * m + c] = v;
        }
        __syncthreads();
        if (mine && r > m) v = v - A[r * kLS + m] * xs[2 * m + c];
    }
    __syncthreads();                             // (xs is rewritten from the other end)
    for (int m = D - 1; m >= 0; --m) {           // L^T x = y
        if (mine && r == m) {
            v = v / A[m * kLS + m];
            xs[2 * m + c] = v;
        }
        __syncthreads();
        if (mine && r < m) v = v - A[m * kLS + r] * xs[2 * m + c];
    }
    if (mine) Wk[tid] = v;
}

__global__ __launch_bounds__(kBlock) void landmark_predict_kernel(const double* __restrict__ feat, const double* __restrict__ W, int N,
                                                                  int D, int K, const double* __restrict__ target,
                                                                  const unsigned char* __restrict__ vis, double* __restrict__ pred,
                                                                  double* __restrict__ d2) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)N * K) return;
    const int n = (int)(t / K), k = (int)(t - (long long)n * K);
    const double* f = feat + (long long)n * (D - 1);
    const double* w = W + (long long)k * 2 * D;
    double px = 0.0, py = 0.0;
    for (int a = 0; a < D; ++a) {
        const double fa = a < D - 1 ? f[a] : 1.0;
        px = px + fa * w[2 * a];
        py = py + fa * w[2 * a + 1];
    }
    pred[2 * t] = px;
    pred[2 * t + 1] = py;
    if (d2) {
        double v = -1.0;
        if (vis[t]) {
            const double dx = px - target[2 * t], dy = py - target[2 * t + 1];
            v = dx * dx + dy * dy;
        }
        d2[t] = v;
    }
}

// blocks of ups_part_moments, or -1 for sizes it refuses
long long moments_blocks(long long N, long long h, long long w, long long P) {
    if (N < 1 || h < 1 || w < 1 || P < 1 || P > kMaxP || h * w > (1LL << 20)) return -1;
    if (h * w * (h > w ? h : w) > kIntMax) return -1;        // the integer sums of one image: |2x + 1 - w| < w per pixel
    const long long blocks = (h * w + kMChunk - 1) / kMChunk * N;
    return (blocks * 3 * P > kIntMax || N * P * 3 > kIntMax) ? -1 : blocks;
}

long long gram_chunks(long long N, long long D, long long K) {
    if (N < 1 || D < 1 || D > kMaxD || K < 1 || K > kMaxKp) return -1;
    const long long chunks = (N + kLChunk - 1) / kLChunk;
    return (chunks * K * gram_outputs((int)D) > kIntMax || N * K * 2 > kIntMax || N * D > kIntMax) ? -1 : chunks;
}

}  // namespace

extern "C" int32_t ups_part_moments_chunk(void) { return kMChunk; }
extern "C" int32_t ups_landmark_chunk(void) { return kLChunk; }

extern "C" size_t ups_part_moments_scratch_bytes(int32_t N, int32_t h, int32_t w, int32_t P) {
    const long long blocks = moments_blocks(N, h, w, P);
    return blocks < 0 ? 0 : (size_t)blocks * 3 * P * sizeof(double);
}

extern "C" int ups_part_moments(const float* soft, const int64_t* pred, int32_t N, int32_t h, int32_t w, int32_t P, double min_mass,
                                double* mass, double* centre, uint8_t* valid, int32_t* hard, int32_t* invalid, void* scratch,
                                void* stream) {
    UPS_CHECK_ARG(soft && mass && centre && valid && scratch);
    UPS_CHECK_ARG(!pred || (hard && invalid));
    UPS_CHECK_ARG(N >= 1 && h >= 1 && w >= 1 && P >= 1);
    UPS_CHECK_ARG(!(min_mass != min_mass));                  // (NaN)
    if (P > kMaxP) {
        ups_set_error("ups_part_moments: P <= %d (got P = %d)", kMaxP, P);
        return UPS_E_UNSUPPORTED;
    }
    const long long blocks = moments_blocks(N, h, w, P);
    UPS_CHECK_ARG(blocks > 0);
    int Pp = 1;
    while (Pp < P) Pp <<= 1;
    const int chunks = (int)(blocks / N);
    double* part = reinterpret_cast<double*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(part_moments_kernel, dim3((unsigned)blocks), dim3(kBlock), (size_t)kMChunk * P * sizeof(float), s, soft, reinterpret_cast<const long long*>(pred), h,
                       w, P, Pp, chunks, part, hard, invalid);
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_moments_finish_kernel, dim3((unsigned)N), dim3(kBlock), 0, s, part, P, chunks, min_mass, mass, centre, valid);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" size_t ups_landmark_gram_scratch_bytes(int32_t N, int32_t D, int32_t K) {
    const long long chunks = gram_chunks(N, D, K);
    return chunks < 0 ? 0 : (size_t)chunks * K * gram_outputs(D) * sizeof(double);
}

extern "C" int ups_landmark_gram(const double* feat, const double* target, const uint8_t* vis, int32_t N, int32_t D, int32_t K,
                                 double* G, double* R, int32_t* cnt, void* scratch, void* stream) {
    UPS_CHECK_ARG(target && vis && G && R && cnt && scratch);
    UPS_CHECK_ARG(N >= 1 && D >= 1 && K >= 1);
    UPS_CHECK_ARG(feat || D == 1);                           // (D = 1: the constant alone, no feature is read)
    if (D > kMaxD || K > kMaxKp) {
        ups_set_error("ups_landmark_gram: D <= %d and K <= %d (got D = %d, K = %d)", kMaxD, kMaxKp, D, K);
        return UPS_E_UNSUPPORTED;
    }
    const long long chunks = gram_chunks(N, D, K);
    UPS_CHECK_ARG(chunks > 0);
    double* part = reinterpret_cast<double*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(landmark_gram_kernel, dim3((unsigned)(chunks * K)), dim3(kBlock), 0, s, feat, target, vis, N, D, K, part);
    UPS_LAUNCH_CHECK();
    hipLaunchKernelGGL(landmark_gram_finish_kernel, dim3(ups_cdiv((long long)K * gram_outputs(D), kBlock)), dim3(kBlock), 0, s, part, D, K,
                       (int)chunks, G, R, cnt);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_landmark_solve(const double* G, const double* R, const int32_t* cnt, int32_t D, int32_t K, double lambda, double* W,
                                  int32_t* n_singular, void* stream) {
    UPS_CHECK_ARG(G && R && cnt && W && n_singular);
    UPS_CHECK_ARG(D >= 1 && K >= 1);
    UPS_CHECK_ARG(lambda >= 0.0 && lambda <= 1.79769313486231570815e308);       // (NaN and +inf fail too)
    if (D > kMaxD || K > kMaxKp) {
        ups_set_error("ups_landmark_solve: D <= %d and K <= %d (got D = %d, K = %d)", kMaxD, kMaxKp, D, K);
        return UPS_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(landmark_solve_kernel, dim3((unsigned)K), dim3(kBlock), 0, (hipStream_t)stream, G, R, cnt, D, lambda, W, n_singular);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_landmark_predict(const double* feat, const double* W, int32_t N, int32_t D, int32_t K, const double* target,
                                    const uint8_t* vis, double* pred, double* d2, void* stream) {
    UPS_CHECK_ARG(W && pred);
    UPS_CHECK_ARG(N >= 1 && D >= 1 && K >= 1);
    UPS_CHECK_ARG(feat || D == 1);
    UPS_CHECK_ARG((target != nullptr) == (vis != nullptr) && (vis != nullptr) == (d2 != nullptr));
    if (D > kMaxD || K > kMaxKp) {
        ups_set_error("ups_landmark_predict: D <= %d and K <= %d (got D = %d, K = %d)", kMaxD, kMaxKp, D, K);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG((long long)N * K * 2 <= kIntMax && (long long)N * D <= kIntMax);
    hipLaunchKernelGGL(landmark_predict_kernel, dim3(ups_cdiv((long long)N * K, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, feat, W, N,
                       D, K, target, vis, pred, d2);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
