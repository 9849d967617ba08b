// The optimizer step's shared kernel bodies: TF-style Adam (tf.train.AdamOptimizer) and the state update, each
// written ONCE and instantiated plain (latent_adam.hip: ups_adam, ups_adam_dev, ups_state_update) and guarded (stepguard.hip:
// ups_adam_guarded, ups_state_update_guarded), so that the guarded entries cannot drift from the bits of the plain ones.
#pragma once
#include "common.h"

// GUARD: the key's ups_step_guard record is read from device memory when the kernel RUNS (a captured graph replays the decision of the
// step at hand): a set `skip` returns the whole grid before anything is touched, else the gradient is (g * gscale) * rec->scale.
template <bool GUARD>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long long count, float lr_t, const float* __restrict__ lr_t_dev, float b1, float b2, float eps,
                            float gscale, const ups_step_guard* __restrict__ rec) {
    if (lr_t_dev) lr_t = *lr_t_dev;       // device scalar: lets a captured HIP graph be replayed with the step's learning rate
    float clip = 1.f;
    if constexpr (GUARD) {
        if (rec->skip) return;
        clip = rec->scale;
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x) {
        float gg = g[i] * gscale;
        if constexpr (GUARD) gg = gg * clip;
        const float mm = b1 * m[i] + (1.f - b1) * gg;
        const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
        m[i] = mm; v[i] = vv;
        p[i] = p[i] - lr_t * mm / (sqrtf(vv) + eps);
    }
}

static inline unsigned ups_adam_grid(long long count) {
    long long grid = (count + 255) / 256;
    return (unsigned)(grid > 8192 ? 8192 : grid);
}

// Element i of the new state vector (include/upsparts_hip.h, "state update").  Every product and sum below is rounded on its own, as the
// torch expressions it replaces round them (the test holds it to them bit for bit).  __fmul_rn / __fadd_rn do NOT stop hipcc's
// contraction (their bodies are compiled under the header's fp-contract=fast: the build without packed fp32 forms fused
// decay * o + gain * val into v_fmac_f32, round 6); plain operators under this pragma are not fused.
__device__ __forceinline__ float ups_state_value(int i, const float* __restrict__ stats, float o, float decay, float gain, int up_loa,
                                                 float loa_lr, float loa_target, int up_lor, float lor_lr, float lor_target,
                                                 float lor_min, float lor_max) {
#pragma clang fp contract(off)
    const float mim = stats[0], ind = stats[1], acc0 = stats[2], acc1 = stats[3], l0 = stats[4], l1 = stats[5];
    float v;
    if (i < 7) {
        const float val = i == 0 ? acc0 : i == 1 ? acc1 : i == 2 ? acc1 - acc0 : i == 3 ? l0 : i == 4 ? l1 : i == 5 ? mim : ind;
        const float a = decay * o, b = gain * val;
        v = a + b;
    } else if (i == 7) {
        const float d = loa_lr * (mim - loa_target);
        v = up_loa ? fmaxf(o + d, 0.f) : o;
    } else {
        const float d = lor_lr * (ind - lor_target);
        v = up_lor ? fminf(fmaxf(o + d, lor_min), lor_max) : o;
    }
    return v;
}
