// torch.optim.AdamW on one element.  ONE definition for the flat pass over the transformer's parameters (vit.hip: adamw_kernel)
// and for the per-head segments of the linear-probe grid (probe.hip: probe_adamw_kernel).
#pragma once
#include "common.h"

// The step's bias corrections from the 1-based step count on the device: step_size = lr / (1 - b1^t), bc2s = sqrt(1 - b2^t).
__device__ __forceinline__ void adamw_bias(const long long* __restrict__ step, float lr, float b1, float b2, float& step_size,
                                           float& bc2s) {
    const float t = (float)step[0];
    const float bc1 = 1.f - powf(b1, t);
    bc2s = sqrtf(1.f - powf(b2, t));
    step_size = lr / bc1;
}

// p *= 1 - lr wd;  m = b1 m + omb1 g;  v = b2 v + omb2 g^2;  p -= step_size m / (sqrt(v) / bc2s + eps), with g scaled by
// gscale first; omb1 / omb2 are the caller's 1 - b1 / 1 - b2 (vit.hip forms them in fp32 from the fp32 betas, probe.hip rounds
// the fp64 differences).  lr == 0 and wd == 0 leave p bit-unchanged (step_size is 0 then, and p * 1 - 0 is p).
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float lr, float wd, float b1, float omb1, float b2,
                                           float omb2, float eps, float gscale, float step_size, float bc2s) {
    const float gg = g * gscale;
    p *= 1.f - lr * wd;
    m = b1 * m + omb1 * gg;
    v = b2 * v + omb2 * gg * gg;
    p -= step_size * m / (sqrtf(v) / bc2s + eps);
}
