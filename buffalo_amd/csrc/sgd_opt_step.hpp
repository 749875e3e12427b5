// The optimizer arithmetic of one float4 of a row: SGDAlgorithm::update_adam / update_adagrad (/root/reference/lib/algo.cc:382-465).  Shared by
// the epoch-end pass (sgd_kernels.hpp) and by WARP's fold-in (warp_fold_kernels.hpp), whose rows take exactly the trainer's step.
// Quirks kept: grad keeps the transformed step (Q-6), FEPS outside the sqrt (Q-5).
#pragma once
#include "common.hpp"

namespace bfh {

struct OptConsts {
    float reg2, lr, b1, omb1, b2, omb2, c1, c2;
};

template <bool ADAM>
__device__ __forceinline__ void opt_step4(float4& x, float4& g, float4& m, float4& v, bool has_cnt, float cntf,
                                          const OptConsts& k, float& nrm) {
    const float FEPS = 1e-10f;
    float* xp = reinterpret_cast<float*>(&x);
    float* gp = reinterpret_cast<float*>(&g);
    float* vp = reinterpret_cast<float*>(&v);
    float* mp = reinterpret_cast<float*>(&m);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float ge = gp[e];
        if (has_cnt) ge = ge / cntf;
        ge = ge - xp[e] * k.reg2;
        if (ADAM) {
            mp[e] = k.b1 * mp[e] + k.omb1 * ge;
            vp[e] = k.b2 * vp[e] + k.omb2 * (ge * ge);
            const float m_hat = mp[e] / k.c1;
            const float v_hat = vp[e] / k.c2;
            ge = m_hat / (sqrtf(v_hat) + FEPS);
        } else {
            vp[e] = vp[e] + ge * ge;
            ge = ge / (sqrtf(vp[e]) + FEPS);
        }
        gp[e] = ge;
        xp[e] = xp[e] + k.lr * ge;
        nrm += xp[e] * xp[e];
    }
}

}  // namespace bfh
