// Thin-plate-spline parameters and solve (declared in include/upsparts_hip.h): ups_tps_solve -- T of the (K+3) x (K+3) TPS system
// of every sample -- and ups_tps_params -- the augmentation's parameter chain (tps.tps_parameters + tps.make_input_tps_param) and
// that solve in ONE launch, so that a training step with `use_tps` has no library call and no host check in it and can be captured.
//
// One wave64 block per sample.  The augmented system [W | b_x b_y], N = K + 3 rows of N + 2 doubles, sits in LDS (at most
// 35 x 37 x 8 B = 10 360 B) and is built in fp64 from the fp32 control points and vectors exactly as tps.solve_system was handed them:
//   row i < K :  1, x_i, y_i, phi(|c_i - c_j|^2) j < K   |  x_i + vx_i, y_i + vy_i        phi(d2) = d2 log(d2 + 1e-6)
//   row K + r :  0, 0, 0,     (1, x_j, y_j)[r]    j < K   |  0, 0
// Gaussian elimination with PARTIAL PIVOTING (the diagonal of the phi block and the lower-right 3 x 3 block are exact zeros, so an
// unpivoted elimination divides by zero for every input): the pivot of column k is the largest |a| at or below the diagonal, ties to
// the lowest row; every lane finds it by the same scan of the column (broadcast reads, no cross-lane traffic), the lanes swap the
// two rows, then share the (rows below k) x (columns right of k) update.  Column k itself is never written, so the multipliers
// a_ik / a_kk that the lanes of a row recompute are read from values no lane changes in that phase.  Lanes 0 and 1 back-substitute
// one right-hand side each, in ascending column order.  No contraction (pragma below), no floating-point atomics: two launches give
// the same bits, and a NumPy loop with the same pivot rule gives them too.
// A pivot that is exactly 0 (two coincident control points: equal rows stay equal under equal operations, and a - 1 a = 0) or a
// non-finite entry of the solution gives the sample the identity transform and adds 1 to *n_singular (one integer atomic per such
// sample): a captured kernel cannot raise as torch.linalg.solve does.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = 32;                        // TPS_MAXK of ups_tps_warp (pointwise.hip)
constexpr int kMaxN = kMaxK + 3;
constexpr int kLd = kMaxN + 2;                   // row stride of the augmented system, in doubles
constexpr int kWave = 64;
static_assert(kMaxN * kLd * 8 == 10360, "the LDS figure of the header comment");

struct TpsLds {
    double a[kMaxN * kLd];
    float c[2 * kMaxK], v[2 * kMaxK];            // the fp32 control points and vectors the system is built from
    int bad;
};

// s.c / s.v hold the sample's K control points and vectors (visible to the block); writes T[2][K + 3] of the sample
__device__ void tps_solve_block(TpsLds& s, int K, float* __restrict__ T, int* __restrict__ n_singular) {
    const int lane = threadIdx.x, N = K + 3;
    double* A = s.a;
    for (int e = lane; e < N * (N + 2); e += kWave) {
        const int i = e / (N + 2), j = e - i * (N + 2);
        double val;
        if (i < K) {
            const double xi = (double)s.c[2 * i], yi = (double)s.c[2 * i + 1];
            if (j == 0) val = 1.0;
            else if (j == 1) val = xi;
            else if (j == 2) val = yi;
            else if (j < N) {
                const double dx = xi - (double)s.c[2 * (j - 3)], dy = yi - (double)s.c[2 * (j - 3) + 1];
                const double d2 = dx * dx + dy * dy;
                val = d2 * log(d2 + 1e-6);
            } else val = (double)s.c[2 * i + (j - N)] + (double)s.v[2 * i + (j - N)];
        } else {
            const int r = i - K;
            if (j < 3 || j >= N) val = 0.0;
            else val = r == 0 ? 1.0 : (double)s.c[2 * (j - 3) + (r - 1)];
        }
        A[i * kLd + j] = val;
    }
    if (lane == 0) s.bad = 0;
    __syncthreads();
    bool singular = false;
    for (int k = 0; k < N; ++k) {
        int p = k;
        double best = fabs(A[k * kLd + k]);
        for (int i = k + 1; i < N; ++i) {
            const double m = fabs(A[i * kLd + k]);
            if (m > best) { best = m; p = i; }
        }
        if (!(best > 0.0)) { singular = true; break; }       // (uniform: every lane scanned the same column; a NaN column ends here too)
        if (p != k) {
            __syncthreads();                                 // every lane has read column k of rows k and p
            for (int j = k + lane; j < N + 2; j += kWave) {
                const double t = A[k * kLd + j];
                A[k * kLd + j] = A[p * kLd + j];
                A[p * kLd + j] = t;
            }
        }
        __syncthreads();
        const double piv = A[k * kLd + k];
        const int cols = N + 1 - k, rows = N - 1 - k;        // columns k + 1 .. N + 1, rows k + 1 .. N - 1
        for (int e = lane; e < rows * cols; e += kWave) {
            const int i = k + 1 + e / cols, j = k + 1 + e % cols;
            const double f = A[i * kLd + k] / piv;
            A[i * kLd + j] = A[i * kLd + j] - f * A[k * kLd + j];
        }
        __syncthreads();
    }
    if (!singular && lane < 2) {
        const int col = N + lane;
        bool finite = true;
        for (int i = N - 1; i >= 0; --i) {
            double acc = A[i * kLd + col];
            for (int j = i + 1; j < N; ++j) acc = acc - A[i * kLd + j] * A[j * kLd + col];
            acc = acc / A[i * kLd + i];
            A[i * kLd + col] = acc;
            finite = finite && isfinite(acc);
        }
        if (!finite) atomicOr(&s.bad, 1);
    }
    __syncthreads();
    singular = singular || s.bad != 0;
    for (int e = lane; e < 2 * N; e += kWave) {
        const int r = e / N, i = e - r * N;
        T[e] = singular ? (i == r + 1 ? 1.f : 0.f) : (float)A[i * kLd + N + r];
    }
    if (singular && lane == 0) atomicAdd(n_singular, 1);
}

__global__ __launch_bounds__(kWave) void tps_solve_kernel(const float* __restrict__ coord, const float* __restrict__ vector,
                                                          float* __restrict__ T, int* __restrict__ n_singular, int K) {
    __shared__ TpsLds s;
    const long long n = blockIdx.x;
    for (int e = threadIdx.x; e < 2 * K; e += kWave) {
        s.c[e] = coord[n * 2 * K + e];
        s.v[e] = vector[n * 2 * K + e];
    }
    __syncthreads();
    tps_solve_block(s, K, T + n * 2 * (K + 3), n_singular);
}

struct TpsRanges { double scal, tps_scal, rot_scal, off_scal, scal_var, augm_scal; };

__device__ __forceinline__ double rng(double t, double lo, double hi) { return lo + (hi - lo) * t; }

// tps.tps_parameters + tps.make_input_tps_param of one sample in fp64 from its 4 K + 7 fp32 uniforms: jittered control points, TPS
// vectors, scale about `offset`, rotation about `offset_2`.  coord is rounded to fp32 once; vector = fp32(target - double(coord)).
__global__ __launch_bounds__(kWave) void tps_params_kernel(const float* __restrict__ uniforms, const double* __restrict__ base,
                                                           TpsRanges g, float* __restrict__ coord, float* __restrict__ vector,
                                                           float* __restrict__ T, int* __restrict__ n_singular, int K) {
    __shared__ TpsLds s;
    const long long n = blockIdx.x;
    const float* u = uniforms + n * (4 * K + 7);
    const int i = threadIdx.x;
    if (i < K) {
        const double off_x = rng((double)u[4 * K], -g.off_scal, g.off_scal), off_y = rng((double)u[4 * K + 1], -g.off_scal, g.off_scal);
        const double o2_x = rng((double)u[4 * K + 2], -g.off_scal, g.off_scal), o2_y = rng((double)u[4 * K + 3], -g.off_scal, g.off_scal);
        const double lo = g.scal * (1.0 - g.scal_var), hi = g.scal * (1.0 + g.scal_var);
        const double ts_x = rng((double)u[4 * K + 4], lo, hi) * g.augm_scal, ts_y = rng((double)u[4 * K + 5], lo, hi) * g.augm_scal;
        const double rot = rng((double)u[4 * K + 6], -g.rot_scal, g.rot_scal);
        const double cs = cos(rot), sn = sin(rot);
        const double cx = base[2 * i] + rng((double)u[2 * i], -0.2, 0.2), cy = base[2 * i + 1] + rng((double)u[2 * i + 1], -0.2, 0.2);
        const double vx = rng((double)u[2 * K + 2 * i], -g.tps_scal, g.tps_scal);
        const double vy = rng((double)u[2 * K + 2 * i + 1], -g.tps_scal, g.tps_scal);
        const double sx = ts_x * (cx + vx - off_x) + off_x, sy = ts_y * (cy + vy - off_y) + off_y;
        const double dx = sx - o2_x, dy = sy - o2_y;
        const double tx = cs * dx + (-sn) * dy + o2_x, ty = sn * dx + cs * dy + o2_y;
        const float cxf = (float)cx, cyf = (float)cy;
        const float vxf = (float)(tx - (double)cxf), vyf = (float)(ty - (double)cyf);
        s.c[2 * i] = cxf; s.c[2 * i + 1] = cyf;
        s.v[2 * i] = vxf; s.v[2 * i + 1] = vyf;
        coord[n * 2 * K + 2 * i] = cxf; coord[n * 2 * K + 2 * i + 1] = cyf;
        vector[n * 2 * K + 2 * i] = vxf; vector[n * 2 * K + 2 * i + 1] = vyf;
    }
    __syncthreads();
    tps_solve_block(s, K, T + n * 2 * (K + 3), n_singular);
}

}  // namespace

extern "C" int ups_tps_solve(const float* coord, const float* vector, float* T, int32_t* n_singular, int32_t n, int32_t K,
                             void* stream) {
    UPS_CHECK_ARG(coord && vector && T && n_singular && n >= 1);
    if (K < 3 || K > kMaxK) {
        ups_set_error("ups_tps_solve: 3 <= K <= %d (got %d)", kMaxK, K);
        return UPS_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(tps_solve_kernel, dim3(n), dim3(kWave), 0, (hipStream_t)stream, coord, vector, T, n_singular, K);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}

extern "C" int ups_tps_params(const float* uniforms, const double* base_points, int32_t K, double scal, double tps_scal,
                              double rot_scal, double off_scal, double scal_var, double augm_scal, float* coord, float* vector,
                              float* T, int32_t* n_singular, int32_t n, void* stream) {
    UPS_CHECK_ARG(uniforms && base_points && coord && vector && T && n_singular && n >= 1);
    if (K < 3 || K > kMaxK) {
        ups_set_error("ups_tps_params: 3 <= K <= %d (got %d)", kMaxK, K);
        return UPS_E_UNSUPPORTED;
    }
    const TpsRanges g = {scal, tps_scal, rot_scal, off_scal, scal_var, augm_scal};
    hipLaunchKernelGGL(tps_params_kernel, dim3(n), dim3(kWave), 0, (hipStream_t)stream, uniforms, base_points, g, coord, vector, T,
                       n_singular, K);
    UPS_LAUNCH_CHECK();
    return UPS_OK;
}
