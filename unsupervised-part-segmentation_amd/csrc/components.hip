// Part coherence (declared in include/upsparts_hip.h; the definitions are DESIGN.md section 8 "Part coherence", restated twice in
// NumPy by tests/components_ref.py): connected components of integer label maps, their sizes and per-part statistics, and one round
// of speck clean-up.  Integer arithmetic and integer atomics only: every output is a function of the map, whatever the schedule.
//
//   ups_label_components        comp[k] = the smallest in-image index y * w + x of the component of pixel k; -1 at an invalid pixel
//   ups_label_component_stats   area[k], stats[i, p, 0..3] (pixels, components, largest, small ones), invalid[0]
//   ups_label_components_clean  every component smaller than min_area takes the label its edge neighbours vote for
//
// Images are packed by the table of ups_segment_render (segment_common.h: the same checks); a regular [N, h, w] batch is the table
// the Python wrapper builds.  Every kernel runs on a 2-D grid: blockIdx.y is the image, blockIdx.x a tile or a run of 256 pixels of
// it, and a block beyond its image's extent returns at once -- the grid's x extent is the largest image's.
//
// Labelling is a union-find whose parent array IS `comp` (in-image indices, parent <= self), in three launches:
//   1. tiles     a block labels one 32 x 32 tile in LDS: parent[t] = t, then every pixel unites itself with its equal left / upper
//                (conn 8: and upper-left, upper-right) neighbours INSIDE the tile, then writes the image index of its tile root.
//   2. borders   every pixel whose backward neighbour lies in ANOTHER tile unites with it in global memory.
//   3. flatten   comp[k] = root of k.
// unite() links the LARGER root under the smaller with atomicMin, so a parent only ever decreases, every tree's root is its smallest
// index, and once all unions are done a component is one tree: comp is the minimum index whatever order the unions ran in.
// find() may read a parent that another lane is lowering: what it returns is then an ancestor that is no longer a root, the atomicMin
// sees the true word, returns a value other than that ancestor, and the union goes on from the returned (smaller) index.
// Bounds.  A find walks strictly downwards: at most h * w steps.  Each retry of unite() strictly lowers a + b: at most 2 h * w.
// A loop that reaches its bound sets err[0] |= 1 and ends; the wrapper raises (ops.components_check).  No loop is unbounded.
//
// Sizes: one int32 counter per element (the scratch), zeroed, += 1 at the root's slot per valid pixel, read back per pixel.
// Clean-up: votes are collected in one pass per part q into one int32 per root; a fold pass keeps the running (best vote, best q)
// of every small root (strictly greater replaces: the FIRST q of maximal vote) and clears the counter: 12 bytes per element,
// independent of P; 2 P + 2 launches of a fixed maximum of 512.
#include "common.h"
#include "segment_common.h"

#pragma clang fp contract(off)

namespace {

using ups_segment::kWords;

constexpr int kBlock = 256;                      // threads per block: one pixel per thread in the per-pixel kernels
constexpr int kTile = 32;                        // tile edge of the LDS stage
constexpr int kTilePx = kTile * kTile;           // 1024: 4 pixels per thread
constexpr int kMaxP = 255;
constexpr long long kMaxHW = 1LL << 20;          // pixels per image

template <typename T>
__device__ __forceinline__ int load_label(const T* labels, long long at, int P) {          // the label, or -1 when invalid
    if constexpr (sizeof(T) == 1) {
        const int v = labels[at];
        return v < P ? v : -1;
    } else {
        const long long v = labels[at];
        return (v >= 0 && v < (long long)P) ? (int)v : -1;
    }
}

__device__ __forceinline__ int load_parent(const int* parent, int i) {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of i: at most `bound` steps (parents strictly decrease on the way: a longer walk is a bug)
__device__ __forceinline__ int find_root(const int* parent, int i, int bound, int* err) {
    int steps = 0;
    int p = load_parent(parent, i);
    while (p != i) {
        if (++steps > bound) {
            atomicOr(err, 1);
            break;
        }
        i = p;
        p = load_parent(parent, i);
    }
    return i;
}

// a and b are one component: the larger root goes under the smaller.  Every retry lowers a + b: at most 2 * bound + 2 of them.
__device__ __forceinline__ void unite(int* parent, int a, int b, int bound, int* err) {
    for (int tries = 0;; ++tries) {
        if (tries > 2 * bound + 2) {
            atomicOr(err, 1);
            return;
        }
        a = find_root(parent, a, bound, err);
        b = find_root(parent, b, bound, err);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);                            // a > b
        if (old == a) return;                                                // a was a root: linked
        a = old;                                                             // it was not: its former parent joins b too
    }
}

// 1. one tile in LDS
template <typename T>
__global__ __launch_bounds__(kBlock) void cc_tiles_kernel(const T* __restrict__ labels, const int* __restrict__ table, int P, int conn,
                                                          int* __restrict__ comp, int* err) {
    __shared__ int lab[kTilePx];
    __shared__ int par[kTilePx];
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;                        // (block-uniform: before any barrier)
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kTilePx / kBlock; ++j) {
        const int t = tid + j * kBlock;
        const int y = y0 + t / kTile, x = x0 + t % kTile;
        lab[t] = (y < h && x < w) ? load_label(labels, off + (long long)y * w + x, P) : -1;
        par[t] = t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTilePx / kBlock; ++j) {
        const int t = tid + j * kBlock;
        const int ly = t / kTile, lx = t % kTile;
        const int l = lab[t];
        if (l < 0) continue;
        if (lx > 0 && lab[t - 1] == l) unite(par, t, t - 1, kTilePx, err);
        if (ly > 0 && lab[t - kTile] == l) unite(par, t, t - kTile, kTilePx, err);
        if (conn == 8 && ly > 0) {
            if (lx > 0 && lab[t - kTile - 1] == l) unite(par, t, t - kTile - 1, kTilePx, err);
            if (lx < kTile - 1 && lab[t - kTile + 1] == l) unite(par, t, t - kTile + 1, kTilePx, err);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTilePx / kBlock; ++j) {
        const int t = tid + j * kBlock;
        const int y = y0 + t / kTile, x = x0 + t % kTile;
        if (y >= h || x >= w) continue;
        int v = -1;
        if (lab[t] >= 0) {
            const int r = find_root(par, t, kTilePx, err);
            v = (y0 + r / kTile) * w + (x0 + r % kTile);                     // row-major in the tile and in the image: the same order
        }
        comp[off + (long long)y * w + x] = v;
    }
}

// 2. unions across tile borders, in global memory
template <typename T>
__global__ __launch_bounds__(kBlock) void cc_borders_kernel(const T* __restrict__ labels, const int* __restrict__ table, int P, int conn,
                                                            int* comp, int* err) {
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const int hw = h * w;
    const long long kl = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (kl >= hw) return;
    const int k = (int)kl;
    const int y = k / w, x = k - y * w;
    const bool top = (y % kTile) == 0 && y > 0;                              // the upper neighbours are in another tile
    const bool left = (x % kTile) == 0 && x > 0;
    const bool right = (x % kTile) == kTile - 1 && x < w - 1;
    if (!top && !left && !(conn == 8 && right && y > 0)) return;
    const int l = load_label(labels, off + k, P);
    if (l < 0) return;
    int* parent = comp + off;
    if (left && load_label(labels, off + k - 1, P) == l) unite(parent, k, k - 1, hw, err);
    if (top && load_label(labels, off + k - w, P) == l) unite(parent, k, k - w, hw, err);
    if (conn == 8 && y > 0) {
        if (x > 0 && (top || left) && load_label(labels, off + k - w - 1, P) == l) unite(parent, k, k - w - 1, hw, err);
        if (x < w - 1 && (top || right) && load_label(labels, off + k - w + 1, P) == l) unite(parent, k, k - w + 1, hw, err);
    }
}

// 3. every pixel takes its root
__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(const int* __restrict__ table, int* comp, int* err) {
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int hw = table[img * kWords + 1] * table[img * kWords + 2];
    const long long kl = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (kl >= hw) return;
    const int k = (int)kl;
    int* parent = comp + off;
    if (load_parent(parent, k) < 0) return;
    const int r = find_root(parent, k, hw, err);
    if (r != k) parent[k] = r;                                               // (a root is never rewritten: r's own word stays r)
}

// ------------------------------------------------------------------------------------------------------- sizes and statistics
template <typename T>
__global__ __launch_bounds__(kBlock) void cc_count_kernel(const T* __restrict__ labels, const int* __restrict__ comp,
                                                          const int* __restrict__ table, int P, int* __restrict__ cnt,
                                                          int* __restrict__ stats, int* __restrict__ invalid) {
    __shared__ int bins[256];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int hw = table[img * kWords + 1] * table[img * kWords + 2];
    if ((long long)blockIdx.x * kBlock >= hw) return;                        // (block-uniform)
    bins[tid] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    const long long kl = (long long)blockIdx.x * kBlock + tid;
    if (kl < hw) {
        const int l = load_label(labels, off + kl, P);
        if (l >= 0) {
            const int c = comp[off + kl];
            atomicAdd(&bins[l], 1);
            if (c >= 0 && c < hw) atomicAdd(&cnt[off + c], 1);               // (a comp of another map never leaves the image)
        } else {
            atomicAdd(&bad, 1);
        }
    }
    __syncthreads();
    if (tid < P && bins[tid]) atomicAdd(&stats[((long long)img * P + tid) * 4], bins[tid]);
    if (tid == 0 && bad) atomicAdd(invalid, bad);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void cc_area_kernel(const T* __restrict__ labels, const int* __restrict__ comp,
                                                         const int* __restrict__ table, int P, int small, const int* __restrict__ cnt,
                                                         int* __restrict__ area, int* __restrict__ stats) {
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int hw = table[img * kWords + 1] * table[img * kWords + 2];
    const long long kl = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (kl >= hw) return;
    const int c = comp[off + kl];
    const int a = (c >= 0 && c < hw) ? cnt[off + c] : 0;
    area[off + kl] = a;
    const int l = c == (int)kl ? load_label(labels, off + kl, P) : -1;
    if (l >= 0) {                                                            // a root: one component of its part
        int* s = stats + ((long long)img * P + l) * 4;
        atomicAdd(s + 1, 1);
        atomicMax(s + 2, a);
        if (a < small) atomicAdd(s + 3, 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ clean-up
// votes of part q: a pixel of a small component adds the number of its edge neighbours that are valid, of a component that is not
// small, and labelled q, to its root's counter
template <typename T>
__global__ __launch_bounds__(kBlock) void cc_vote_kernel(const T* __restrict__ labels, const int* __restrict__ comp,
                                                         const int* __restrict__ area, const int* __restrict__ table, int P,
                                                         int min_area, int q, int* __restrict__ votes) {
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int h = table[img * kWords + 1], w = table[img * kWords + 2];
    const long long kl = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (kl >= (long long)h * w) return;
    const int k = (int)kl;
    const int c = comp[off + k];
    if (c < 0 || c >= h * w || area[off + k] >= min_area) return;
    const int y = k / w, x = k - y * w;
    int v = 0;
    if (x > 0 && area[off + k - 1] >= min_area && load_label(labels, off + k - 1, P) == q) ++v;       // (area 0: invalid, never >= 1)
    if (x < w - 1 && area[off + k + 1] >= min_area && load_label(labels, off + k + 1, P) == q) ++v;
    if (y > 0 && area[off + k - w] >= min_area && load_label(labels, off + k - w, P) == q) ++v;
    if (y < h - 1 && area[off + k + w] >= min_area && load_label(labels, off + k + w, P) == q) ++v;
    if (v) atomicAdd(&votes[off + c], v);
}

// the roots of the small components keep the first part of maximal vote; q < 0: the first pass, which only clears
__global__ __launch_bounds__(kBlock) void cc_fold_kernel(const int* __restrict__ comp, const int* __restrict__ area,
                                                         const int* __restrict__ table, int min_area, int q, int* __restrict__ votes,
                                                         int* __restrict__ best, int* __restrict__ best_q) {
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int hw = table[img * kWords + 1] * table[img * kWords + 2];
    const long long kl = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (kl >= hw) return;
    if (comp[off + kl] != (int)kl || area[off + kl] >= min_area) return;
    if (q < 0) {
        best[off + kl] = 0;
        best_q[off + kl] = 0;
    } else {
        const int v = votes[off + kl];
        if (v > best[off + kl]) {
            best[off + kl] = v;
            best_q[off + kl] = q;
        }
    }
    votes[off + kl] = 0;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void cc_apply_kernel(const T* labels, const int* __restrict__ comp, const int* __restrict__ area,
                                                          const int* __restrict__ table, int P, int min_area,
                                                          const int* __restrict__ best, const int* __restrict__ best_q, T* out,
                                                          int* __restrict__ changed, const uint8_t* __restrict__ src,
                                                          const uint8_t* __restrict__ colors, double alpha, uint8_t* __restrict__ overlay,
                                                          uint8_t* __restrict__ conf, int* __restrict__ counts) {
    __shared__ int moved;
    const int tid = threadIdx.x;
    const int img = (int)blockIdx.y;
    const long long off = table[img * kWords];
    const int hw = table[img * kWords + 1] * table[img * kWords + 2];
    if ((long long)blockIdx.x * kBlock >= hw) return;                        // (block-uniform)
    if (tid == 0) moved = 0;
    __syncthreads();
    const long long kl = (long long)blockIdx.x * kBlock + tid;
    if (kl < hw) {
        const long long at = off + kl;
        const T raw = labels[at];
        T res = raw;
        const int c = comp[at];
        const int ol = load_label(labels, at, P);
        if (ol >= 0 && c >= 0 && c < hw && area[at] < min_area && best[off + c] > 0) {
            const int nl = best_q[off + c];
            res = (T)nl;                                                     // nl != ol: an equal edge neighbour is the same component
            atomicAdd(&moved, 1);
            if (overlay) {
                const double oma = 1.0 - alpha;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const unsigned col = colors[nl * 3 + ch];
                    overlay[3 * at + ch] = (uint8_t)(src ? ups_segment::blend(alpha, oma, col, src[3 * at + ch]) : col);
                }
            }
            if (conf) conf[at] = 0;
            if (counts) {
                atomicSub(&counts[(long long)img * P + ol], 1);
                atomicAdd(&counts[(long long)img * P + nl], 1);
            }
        }
        out[at] = res;
    }
    __syncthreads();
    if (tid == 0 && moved) atomicAdd(changed, moved);
}

// the checks every entry shares: the table (ups_segment_render's), h * w <= 2^20 per image; the grids of the per-pixel and tile kernels
int check_common(const void* labels, int label_bytes, int n, const int32_t* table_host, const int32_t* table, long long total, int P,
                 dim3* px_grid, dim3* tile_grid) {
    UPS_CHECK_ARG(labels && table_host && table);
    UPS_CHECK_ARG(label_bytes == 1 || label_bytes == 8);
    UPS_CHECK_ARG(n >= 1 && n <= 65535);                                     // blockIdx.y is the image
    UPS_CHECK_ARG(P >= 1);
    if (P > kMaxP) {
        ups_set_error("ups_label_components: P <= 255 (got P = %d)", P);
        return UPS_E_UNSUPPORTED;
    }
    UPS_CHECK_ARG(total >= 1 && total <= 0x7fffffffLL);
    UPS_CHECK_ARG(label_bytes == 1 || ((uintptr_t)labels & 7) == 0);
    long long blocks = 0;
    if (const int rc = ups_segment::check_table(table_host, n, total, &blocks)) return rc;
    long long max_hw = 0, max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const long long h = table_host[(long long)i * kWords + 1], w = table_host[(long long)i * kWords + 2];
        UPS_CHECK_ARG(h * w <= kMaxHW);
        max_hw = h * w > max_hw ? h * w : max_hw;
        const long long t = ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
        max_tiles = t > max_tiles ? t : max_tiles;
    }
    *px_grid = dim3((unsigned)((max_hw + kBlock - 1) / kBlock), (unsigned)n);
    *tile_grid = dim3((unsigned)max_tiles, (unsigned)n);
    return UPS_OK;
}

}  // namespace

extern "C" int32_t ups_components_tile(void) { return kTile; }
extern "C" size_t ups_label_components_scratch_bytes(int64_t total) { (void)total; return 0; }       // comp is the parent array
extern "C" size_t ups_label_component_stats_scratch_bytes(int64_t total) { return total >= 1 ? (size_t)total * 4 : 0; }
extern "C" size_t ups_label_components_clean_scratch_bytes(int64_t total) { return total >= 1 ? (size_t)total * 12 : 0; }

extern "C" int ups_label_components(const void* labels, int32_t label_bytes, int32_t n, const int32_t* table_host, const int32_t* table,
                                    int64_t total, int32_t P, int32_t conn, int32_t* comp, int32_t* err, void* scratch, void* stream) {
    (void)scratch;
    UPS_CHECK_ARG(comp && err);
    UPS_CHECK_ARG(conn == 4 || conn == 8);
    dim3 px, tiles;
    if (const int rc = check_common(labels, label_bytes, n, table_host, table, total, P, &px, &tiles)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 1) {
        const uint8_t* l = (const uint8_t*)labels;
        hipLaunchKernelGGL(cc_tiles_kernel<uint8_t>, tiles, dim3(kBlock), 0, s, l, table, P, conn, comp, err);
        hipLaunchKernelGGL(cc_borders_kernel<uint8_t>, px, dim3(kBlock), 0, s, l, table, P, conn, comp, err);
    } else {
        const int64_t* l = (const int64_t*)labels;
        hipLaunchKernelGGL(cc_tiles_kernel<int64_t>, tiles, dim3(kBlock), 0, s, l, table, P, conn, comp, err);
        hipLaunchKernelGGL(cc_borders_kernel<int64_t>, px, dim3(kBlock), 0, s, l, table, P, conn, comp, err);
    }
    hipLaunchKernelGGL(cc_flatten_kernel, px, dim3(kBlock), 0, s, table, comp, err);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_label_component_stats(const void* labels, int32_t label_bytes, const int32_t* comp, int32_t n,
                                         const int32_t* table_host, const int32_t* table, int64_t total, int32_t P, int32_t small,
                                         int32_t* area, int32_t* stats, int32_t* invalid, void* scratch, void* stream) {
    UPS_CHECK_ARG(comp && area && stats && invalid && scratch);
    UPS_CHECK_ARG(small >= 0);
    UPS_CHECK_ARG(((uintptr_t)scratch & 3) == 0);
    dim3 px, tiles;
    if (const int rc = check_common(labels, label_bytes, n, table_host, table, total, P, &px, &tiles)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* cnt = (int*)scratch;
    if (hipMemsetAsync(cnt, 0, (size_t)total * 4, s) != hipSuccess) {
        ups_set_error("ups_label_component_stats: clearing the scratch failed");
        return UPS_E_LAUNCH;
    }
    if (label_bytes == 1) {
        const uint8_t* l = (const uint8_t*)labels;
        hipLaunchKernelGGL(cc_count_kernel<uint8_t>, px, dim3(kBlock), 0, s, l, comp, table, P, cnt, stats, invalid);
        hipLaunchKernelGGL(cc_area_kernel<uint8_t>, px, dim3(kBlock), 0, s, l, comp, table, P, small, cnt, area, stats);
    } else {
        const int64_t* l = (const int64_t*)labels;
        hipLaunchKernelGGL(cc_count_kernel<int64_t>, px, dim3(kBlock), 0, s, l, comp, table, P, cnt, stats, invalid);
        hipLaunchKernelGGL(cc_area_kernel<int64_t>, px, dim3(kBlock), 0, s, l, comp, table, P, small, cnt, area, stats);
    }
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_label_components_clean(const void* labels, int32_t label_bytes, const int32_t* comp, const int32_t* area, int32_t n,
                                          const int32_t* table_host, const int32_t* table, int64_t total, int32_t P, int32_t min_area,
                                          void* out, int32_t* changed, const uint8_t* src, const uint8_t* colors, double alpha,
                                          uint8_t* overlay, uint8_t* confidence, int32_t* counts, void* scratch, void* stream) {
    UPS_CHECK_ARG(comp && area && out && changed && scratch);
    UPS_CHECK_ARG(min_area >= 1);
    UPS_CHECK_ARG(!overlay || colors);
    UPS_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0);
    UPS_CHECK_ARG(((uintptr_t)scratch & 3) == 0);
    UPS_CHECK_ARG(label_bytes == 1 || ((uintptr_t)out & 7) == 0);
    dim3 px, tiles;
    if (const int rc = check_common(labels, label_bytes, n, table_host, table, total, P, &px, &tiles)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* votes = (int*)scratch;
    int* best = votes + total;
    int* best_q = best + total;
    hipLaunchKernelGGL(cc_fold_kernel, px, dim3(kBlock), 0, s, comp, area, table, min_area, -1, votes, best, best_q);
    for (int q = 0; q < P; ++q) {                                            // P <= 255: at most 512 launches in all
        if (label_bytes == 1)
            hipLaunchKernelGGL(cc_vote_kernel<uint8_t>, px, dim3(kBlock), 0, s, (const uint8_t*)labels, comp, area, table, P, min_area, q,
                               votes);
        else
            hipLaunchKernelGGL(cc_vote_kernel<int64_t>, px, dim3(kBlock), 0, s, (const int64_t*)labels, comp, area, table, P, min_area, q,
                               votes);
        hipLaunchKernelGGL(cc_fold_kernel, px, dim3(kBlock), 0, s, comp, area, table, min_area, q, votes, best, best_q);
    }
    if (label_bytes == 1)
        hipLaunchKernelGGL(cc_apply_kernel<uint8_t>, px, dim3(kBlock), 0, s, (const uint8_t*)labels, comp, area, table, P, min_area, best,
                           best_q, (uint8_t*)out, changed, src, colors, alpha, overlay, confidence, counts);
    else
        hipLaunchKernelGGL(cc_apply_kernel<int64_t>, px, dim3(kBlock), 0, s, (const int64_t*)labels, comp, area, table, P, min_area, best,
                           best_q, (int64_t*)out, changed, src, colors, alpha, overlay, confidence, counts);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
