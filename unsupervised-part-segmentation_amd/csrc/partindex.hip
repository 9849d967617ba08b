// Part-appearance index (declared in include/upsparts_hip.h): ups_part_knn -- per part, the K nearest gallery codes of every query
// code -- and ups_part_kmeans_step -- one assignment / accumulation step of a per-part k-means on the code bank.
//
// The distance is the DIRECT form d(x, y) = sum_a (double(x_a) - double(y_a))^2: fp64 on the fp32 source values, accumulated in
// ascending a from 0.0, every subtraction, multiplication and addition rounded once (no contraction, pragma below), so a NumPy loop
// over a gives the same bits (tests/partindex_ref.py).  There is NO matrix-core form |x|^2 + |y|^2 - 2 x.y: it is not bit-equal to
// any restatement, it cancels for near neighbours (the ones a ranking is about), and v_mfma_f64 runs at the vector fp64 rate anyway.
// Neither kernel writes a distance matrix to memory.
//
// ups_part_knn.  One 256-thread block per (part, tile of kTile = 64 queries).  Gallery tiles of 64 items stream through LDS in channel
// chunks of kKC = 32, converted to double once per tile and chunk, channel-major ([channel][item], row stride 65 doubles: the
// half-wave that stages one item's 32 channels hits 32 banks, and the compute reads are 16 consecutive doubles or a broadcast).
// Thread (tq, tg) of the 16 x 16 grid holds the 4 x 4 distances of queries 4 tq .. 4 tq + 3 and gallery items tg, tg + 16, tg + 32,
// tg + 48 in registers across the chunks (32 VGPRs): 8 LDS reads feed 48 fp64 instructions per channel.  The global loads of the
// NEXT (tile, chunk) step are issued before the arithmetic of the current one and held in registers (16 floats), unconditional on
// clamped addresses so that all are in flight at once: a rolled loop of guarded element loads cost a load latency per element.
// The finished 64 x 64 tile goes to LDS over the staging buffers (ineligible pairs as +inf: finite fp32 codes cannot reach it), and
// thread q < 64 scans its query's row in gallery order, eight candidates per test, against the worst entry of its running sorted
// top-K list (LDS, row stride 33; worst and fill count in registers): a candidate is inserted only when it beats the worst in the
// (d, g) order, which after the first tiles is almost never.
// Gallery indices only grow, so an equal distance never displaces an entry.  The K smallest in a total order are a set: the result
// does not depend on any scheduling.
//
// ups_part_kmeans_step.  One 256-thread block per (part, chunk of kChunk = 256 items), a thread per item.  Channel chunks of kMC = 16
// of the items (converted to double, [channel][item], row stride 258) and of kJT = 8 centroids ([centroid][channel], read as
// broadcasts) sit in LDS; a thread keeps 8 distances in registers, takes the first minimum over the centroid tiles in ascending j, and
// the items are re-staged per centroid tile (k / 8 times; once at k <= 8).  Counts: LDS integer atomics, one global add per block and
// cluster.  Floating-point sums use no atomics: the block's inertia is a fixed LDS tree, its per-cluster feature sums add the
// members in item order (a stable member list per cluster, built by one thread per cluster), both go to caller-owned scratch as one
// partial per block, and a second launch adds the partials in block order.  Two calls give the same bits.
// Loads are element loads: A = 5 rows of fp32 have no 16-byte alignment.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 64;                        // queries per block = gallery items per staged tile
constexpr int kKC = 32;                          // channels per staged chunk (knn)
constexpr int kKS = kTile + 1;                   // row stride of the staged chunks and of the distance tile, in doubles
constexpr int kMaxK = 32;
constexpr int kTS = kMaxK + 1;                   // row stride of the top-K lists
constexpr int kChunk = 256;                      // items per k-means block
constexpr int kMC = 16;                          // channels per staged chunk (k-means)
constexpr int kMS = kChunk + 2;                  // row stride of the staged items, in doubles
constexpr int kJT = 8;                           // centroids per register tile
constexpr int kMaxKm = 64;
constexpr int kMaxA = 512;
static_assert(2 * kKC * kKS == kTile * kKS, "the distance tile reuses the two staging buffers exactly");
static_assert(kTile * kKS * 8 + kTile * kTS * 12 + kTile <= 65536, "static LDS (knn)");
static_assert(kMC == 16 && kChunk == kBlock, "a thread stages one channel of kMC items");
static_assert(kMC * kMS * 8 + kJT * kMC * 8 + 2 * kChunk * 8 <= 65536, "static LDS (k-means)");

__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7ff0000000000000LL); }

constexpr int kKPer = kTile * kKC / kBlock;      // staged elements per thread, chunk and operand (8)
static_assert(kKPer * kBlock == kTile * kKC && kKC == 32, "a thread stages one channel of kKPer rows");

// One staged chunk in flight: channels [a0, a0 + kKC) of rows [r0, r0 + kTile) of part p.  The loads are unconditional on clamped
// (always valid) addresses, so all of them are in flight at once; rows >= R and channels >= A become 0 when they are written.
struct Staged {
    float v[kKPer];
    __device__ __forceinline__ void load(const float* __restrict__ x, int r0, int R, int p, int P, int a0, int A, int tid) {
        const int al = tid & (kKC - 1), a = min(a0 + al, A - 1);
#pragma unroll
        for (int k = 0; k < kKPer; ++k) {
            const int r = min(r0 + (tid >> 5) + k * (kBlock / kKC), R - 1);
            v[k] = x[((long long)r * P + p) * A + a];
        }
    }
    __device__ __forceinline__ void store(double* s, int r0, int R, int a0, int A, int tid) const {     // s[channel][row]
        const int al = tid & (kKC - 1);
#pragma unroll
        for (int k = 0; k < kKPer; ++k) {
            const int row = (tid >> 5) + k * (kBlock / kKC);
            s[al * kKS + row] = (r0 + row < R && a0 + al < A) ? (double)v[k] : 0.0;
        }
    }
};

__global__ __launch_bounds__(kBlock) void part_knn_kernel(const float* __restrict__ q, const unsigned char* __restrict__ qvalid, int Nq,
                                                          const float* __restrict__ g, const unsigned char* __restrict__ gvalid, int Ng,
                                                          int P, int A, int K, int exclude, int qtiles, int* __restrict__ idx,
                                                          double* __restrict__ dist) {
    __shared__ double buf[kTile * kKS];          // [0, kKC * kKS): query chunk, then the gallery chunk; afterwards the distance tile
    __shared__ double topd[kTile * kTS];
    __shared__ int topi[kTile * kTS];
    __shared__ unsigned char gok[kTile];
    double* qs = buf;
    double* gs = buf + kKC * kKS;
    const int tid = threadIdx.x;
    const int p = blockIdx.x / qtiles, q0 = (blockIdx.x - p * qtiles) * kTile;
    const int tq = tid >> 4, tg = tid & 15;
    // the scanning thread's list state (threads < kTile)
    const int myq = q0 + tid;
    const bool qok = tid < kTile && myq < Nq && qvalid[(long long)myq * P + p] != 0;
    int cnt = 0;
    double worst_d = inf64();
    double* td = topd + (tid & (kTile - 1)) * kTS;
    int* ti = topi + (tid & (kTile - 1)) * kTS;
    // eligible and before the worst entry in (d, g): gi exceeds every index already held, so `<` decides once the list is full
    auto offer = [&](double d, int gi) {
        if (d < inf64() && (cnt < K || d < worst_d)) {
            int at = cnt < K ? cnt : K - 1;
            while (at > 0 && td[at - 1] > d) {
                td[at] = td[at - 1];
                ti[at] = ti[at - 1];
                --at;
            }
            td[at] = d;
            ti[at] = gi;
            if (cnt < K) ++cnt;
            if (cnt == K) worst_d = td[K - 1];
        }
    };

    // steps = (gallery tile, channel chunk) pairs in order; step s + 1's global loads are issued before step s's arithmetic
    const int nchunks = (A + kKC - 1) / kKC, steps = ((Ng + kTile - 1) / kTile) * nchunks;
    Staged sq, sg;
    unsigned char gv = 0;
    sq.load(q, q0, Nq, p, P, 0, A, tid);
    sg.load(g, 0, Ng, p, P, 0, A, tid);
    if (tid < kTile) gv = gvalid[(long long)min(tid, Ng - 1) * P + p];
    double acc[4][4];
    for (int s = 0; s < steps; ++s) {
        const int t = s / nchunks, c = s - t * nchunks, g0 = t * kTile, a0 = c * kKC;
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        }
        __syncthreads();                         // the previous chunk's reads / the previous tile's scan are done
        sq.store(qs, q0, Nq, a0, A, tid);
        sg.store(gs, g0, Ng, a0, A, tid);
        if (c == 0 && tid < kTile) gok[tid] = (g0 + tid < Ng && gv != 0) ? 1 : 0;
        __syncthreads();
        if (s + 1 < steps) {
            const int t1 = (s + 1) / nchunks, c1 = s + 1 - t1 * nchunks;
            sq.load(q, q0, Nq, p, P, c1 * kKC, A, tid);
            sg.load(g, t1 * kTile, Ng, p, P, c1 * kKC, A, tid);
            if (c1 == 0 && tid < kTile) gv = gvalid[(long long)min(t1 * kTile + tid, Ng - 1) * P + p];
        }
        const int na = min(kKC, A - a0);
#pragma unroll 4
        for (int a = 0; a < na; ++a) {
            double x[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = qs[a * kKS + tq * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = gs[a * kKS + tg + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = x[i] - y[j];
                    acc[i][j] = acc[i][j] + d * d;
                }
        }
        if (c + 1 < nchunks) continue;
        __syncthreads();                         // every thread has left the last chunk: the tile may overwrite it
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ql = tq * 4 + i, gl = tg + 16 * j;
                const bool ok = gok[gl] && !(exclude && g0 + gl == q0 + ql);
                buf[ql * kKS + gl] = ok ? acc[i][j] : inf64();
            }
        __syncthreads();
        if (qok) {
            // groups of 8 candidates: all eight reads in flight, and one test against the bound the group started with (the bound
            // only tightens, so the test lets every candidate through that `offer` would take)
            const double* row = buf + tid * kKS;
            for (int gl = 0; gl < kTile; gl += 8) {
                double d[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) d[e] = row[gl + e];
                const double bound = cnt < K ? inf64() : worst_d;
                bool any = false;
#pragma unroll
                for (int e = 0; e < 8; ++e) any |= d[e] < bound;
                if (any) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) offer(d[e], g0 + gl + e);
                }
            }
        }
    }
    if (tid < kTile && myq < Nq) {
        const long long o = ((long long)myq * P + p) * K;
        for (int j = 0; j < K; ++j) {
            const bool have = qok && j < cnt;
            idx[o + j] = have ? topi[tid * kTS + j] : -1;
            dist[o + j] = have ? topd[tid * kTS + j] : inf64();
        }
    }
}

__global__ __launch_bounds__(kBlock) void part_kmeans_kernel(const float* __restrict__ feat, const unsigned char* __restrict__ valid, int N,
                                                             int P, int A, const double* __restrict__ cent, int k,
                                                             const int* __restrict__ prev, int* __restrict__ label,
                                                             double* __restrict__ mind, int* __restrict__ counts, int chunks,
                                                             double* __restrict__ sum_part, double* __restrict__ inertia_part,
                                                             int* __restrict__ changed) {
    __shared__ double xs[kMC * kMS];
    __shared__ double cs[kJT * kMC];
    __shared__ double red[kChunk];
    __shared__ int lab[kChunk];
    __shared__ int order[kChunk];
    __shared__ int bins[kMaxKm];
    __shared__ int nchanged;
    const int tid = threadIdx.x;
    const int p = blockIdx.x / chunks, c = blockIdx.x - p * chunks;
    const int n0 = c * kChunk, n = n0 + tid;
    if (tid < kMaxKm) bins[tid] = 0;
    if (tid == 0) nchanged = 0;
    double best = inf64();
    int best_j = -1;
    for (int j0 = 0; j0 < k; j0 += kJT) {
        double acc[kJT];
#pragma unroll
        for (int jj = 0; jj < kJT; ++jj) acc[jj] = 0.0;
        for (int a0 = 0; a0 < A; a0 += kMC) {
            __syncthreads();
            {
                float v[kMC];
                const int al = tid & (kMC - 1), ac = min(a0 + al, A - 1);
#pragma unroll
                for (int r = 0; r < kMC; ++r) {
                    const int it = min(n0 + (tid >> 4) + r * (kBlock / kMC), N - 1);
                    v[r] = feat[((long long)it * P + p) * A + ac];
                }
#pragma unroll
                for (int r = 0; r < kMC; ++r) {
                    const int row = (tid >> 4) + r * (kBlock / kMC);
                    xs[al * kMS + row] = (n0 + row < N && a0 + al < A) ? (double)v[r] : 0.0;
                }
            }
            if (tid < kJT * kMC) {
                const int jj = tid / kMC, al = tid % kMC;
                cs[tid] = (j0 + jj < k && a0 + al < A) ? cent[((long long)p * k + j0 + jj) * A + a0 + al] : 0.0;
            }
            __syncthreads();
            const int na = min(kMC, A - a0);
#pragma unroll 4
            for (int a = 0; a < na; ++a) {
                const double x = xs[a * kMS + tid];
#pragma unroll
                for (int jj = 0; jj < kJT; ++jj) {
                    const double d = x - cs[jj * kMC + a];
                    acc[jj] = acc[jj] + d * d;
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < kJT; ++jj)
            if (j0 + jj < k && (best_j < 0 || acc[jj] < best)) {     // the first minimal j
                best = acc[jj];
                best_j = j0 + jj;
            }
    }
    const bool ok = n < N && valid[(long long)n * P + p] != 0;
    const int lb = ok ? best_j : -1;
    if (n < N) {
        const long long o = (long long)n * P + p;
        label[o] = lb;
        mind[o] = ok ? best : inf64();
        if (prev && prev[o] != lb) atomicAdd(&nchanged, 1);
    }
    lab[tid] = lb;
    if (counts) {
        if (ok) atomicAdd(&bins[lb], 1);
        red[tid] = ok ? best : 0.0;
        for (int s = kBlock / 2; s > 0; s >>= 1) {                    // fixed tree; its barriers also order lab / bins / nchanged
            __syncthreads();
            if (tid < s) red[tid] += red[tid + s];
        }
        __syncthreads();
        if (tid == 0) inertia_part[blockIdx.x] = red[0];
        if (tid < k && bins[tid]) atomicAdd(&counts[p * k + tid], bins[tid]);
        // member lists: cluster j's items in index order at order[start_j ..)
        if (tid < k) {
            int at = 0;
            for (int j = 0; j < tid; ++j) at += bins[j];
            for (int t = 0; t < kChunk; ++t)
                if (lab[t] == tid) order[at++] = t;
        }
        __syncthreads();
        for (int ja = tid; ja < k * A; ja += kBlock) {
            const int j = ja / A, a = ja - j * A;
            int at = 0;
            for (int jj = 0; jj < j; ++jj) at += bins[jj];
            const int end = at + bins[j];
            double s = 0.0;
            for (; at < end; ++at) s += (double)feat[((long long)(n0 + order[at]) * P + p) * A + a];
            sum_part[(long long)blockIdx.x * k * A + ja] = s;
        }
    } else {
        __syncthreads();
    }
    if (tid == 0 && changed && nchanged) atomicAdd(changed, nchanged);
}

// sums[p][ja] = the chunks' partials in chunk order, ja < kA; inertia[p] likewise (the last kA-th column of the thread grid)
__global__ __launch_bounds__(kBlock) void part_kmeans_reduce_kernel(const double* __restrict__ sum_part, const double* __restrict__ inertia_part,
                                                                    int P, int kA, int chunks, double* __restrict__ sums,
                                                                    double* __restrict__ inertia) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)P * (kA + 1)) return;
    const int p = (int)(t / (kA + 1)), ja = (int)(t - (long long)p * (kA + 1));
    double s = 0.0;
    if (ja < kA) {
        for (int c = 0; c < chunks; ++c) s += sum_part[((long long)p * chunks + c) * kA + ja];
        sums[(long long)p * kA + ja] = s;
    } else {
        for (int c = 0; c < chunks; ++c) s += inertia_part[(long long)p * chunks + c];
        inertia[p] = s;
    }
}

constexpr long long kIntMax = 0x7fffffffLL;

// doubles of scratch (feature-sum partials, then inertia partials), or -1 when an index would leave int
long long kmeans_scratch_doubles(long long N, long long P, long long A, long long k) {
    const long long chunks = (N + kChunk - 1) / kChunk;
    if (P * chunks > kIntMax) return -1;
    const long long n = P * chunks * k * A + P * chunks;        // (<= 2^31 * 64 * 512: no overflow of long long)
    return n > kIntMax ? -1 : n;
}

}  // namespace

extern "C" int32_t ups_part_knn_tile(void) { return kTile; }
extern "C" int32_t ups_part_kmeans_chunk(void) { return kChunk; }

extern "C" int ups_part_knn(const float* q, const uint8_t* qvalid, int32_t Nq, const float* g, const uint8_t* gvalid, int32_t Ng,
                            int32_t P, int32_t A, int32_t K, int32_t exclude_same_index, int32_t* idx, double* dist, void* stream) {
    UPS_CHECK_ARG(q && qvalid && g && gvalid && idx && dist);
    UPS_CHECK_ARG(Nq >= 1 && Ng >= 1 && P >= 1 && A >= 1 && K >= 1);
    if (K > kMaxK || A > kMaxA) {
        ups_set_error("ups_part_knn: K <= %d and A <= %d (got K = %d, A = %d)", kMaxK, kMaxA, K, A);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG((long long)Nq * P * A <= kIntMax && (long long)Ng * P * A <= kIntMax && (long long)Nq * P * K <= kIntMax);
    const long long qtiles = ((long long)Nq + kTile - 1) / kTile;
    UPS_CHECK_ARG(qtiles * P <= kIntMax);
    hipLaunchKernelGGL(part_knn_kernel, dim3((unsigned)(qtiles * P)), dim3(kBlock), 0, (hipStream_t)stream, q, qvalid, Nq, g, gvalid, Ng,
                       P, A, K, exclude_same_index ? 1 : 0, (int)qtiles, idx, dist);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" size_t ups_part_kmeans_scratch_bytes(int32_t N, int32_t P, int32_t A, int32_t k) {
    if (N < 1 || P < 1 || A < 1 || A > kMaxA || k < 1 || k > kMaxKm) return 0;
    const long long n = kmeans_scratch_doubles(N, P, A, k);
    return n < 0 ? 0 : (size_t)n * sizeof(double);
}

extern "C" int ups_part_kmeans_step(const float* feat, const uint8_t* valid, int32_t N, int32_t P, int32_t A, const double* cent,
                                    int32_t k, const int32_t* prev_label, int32_t* label, double* mind, int32_t* counts, double* sums,
                                    double* inertia, int32_t* changed, void* scratch, void* stream) {
    UPS_CHECK_ARG(feat && valid && cent && label && mind);
    UPS_CHECK_ARG(N >= 1 && P >= 1 && A >= 1 && k >= 1);
    UPS_CHECK_ARG((counts != nullptr) == (sums != nullptr) && (sums != nullptr) == (inertia != nullptr));
    UPS_CHECK_ARG(!sums || scratch);
    UPS_CHECK_ARG(!prev_label || changed);
    if (k > kMaxKm || A > kMaxA) {
        ups_set_error("ups_part_kmeans_step: k <= %d and A <= %d (got k = %d, A = %d)", kMaxKm, kMaxA, k, A);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG((long long)N * P * A <= kIntMax && (long long)P * k * A <= kIntMax);
    const long long doubles = kmeans_scratch_doubles(N, P, A, k);
    UPS_CHECK_ARG(doubles > 0);
    const int chunks = ups_cdiv(N, kChunk);
    double* sum_part = reinterpret_cast<double*>(scratch);
    double* inertia_part = sums ? sum_part + (long long)P * chunks * k * A : nullptr;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(part_kmeans_kernel, dim3((unsigned)((long long)P * chunks)), dim3(kBlock), 0, s, feat, valid, N, P, A, cent, k,
                       prev_label, label, mind, counts, chunks, sum_part, inertia_part, changed);
    UPS_LAUNCH_CHECK();
    if (sums) {
        hipLaunchKernelGGL(part_kmeans_reduce_kernel, dim3(ups_cdiv((long long)P * (k * A + 1), kBlock)), dim3(kBlock), 0, s, sum_part,
                           inertia_part, P, k * A, chunks, sums, inertia);
        UPS_LAUNCH_CHECK();
    }
    return UPS_OK;
}
