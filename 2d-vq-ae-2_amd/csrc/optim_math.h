// The per-element arithmetic of the optimiser steps, shared by classifier_optim.hip (the slide classifier's seven tensors
// on its packed image) and optim.hip (any list of tensors): torch.optim.Adam / AdamW in their single-tensor, non-capturable
// form, the reference's Lamb (vq_ae/optim/lamb.py:78-114) and SAM's climb (vq_ae/optim/sam.py:31-46, 96-111).  fp32 in
// torch's rounding order -- Tensor.lerp_, addcdiv_, correctly rounded sqrtf and division -- with every scalar formed in double
// on the host and rounded once, as torch rounds the Python scalars it is handed.  Both files are built without fast-math and
// without contraction; nothing here may be respelled in one of them alone.  Private to csrc/.
#pragma once
#include "common.h"

#include <cmath>

namespace vqae_om {

// One parameter group at one step count.
struct Hyper {
    float decay, w1, b1, b2, w2, bc1, bc2, bc2_sqrt, eps, neg_step, wd, neg_lr, rho;
    int decoupled, adaptive, wd_nonzero;
};

// lamb.py:84-104: the Adam step u of one element from its (already updated) moments
__device__ __forceinline__ float lamb_u(const Hyper& a, float m, float v, float p) {
    float u = (m / a.bc1) / (sqrtf(v / a.bc2) + a.eps);
    if (a.wd_nonzero) u = u + a.wd * p;
    return u;
}

// lamb.py:84-88: exp_avg.mul_(b1).add_(g, alpha = 1 - b1), exp_avg_sq.mul_(b2).addcmul_(g, g, value = 1 - b2)
__device__ __forceinline__ void lamb_moments(const Hyper& a, float g, float& m, float& v) {
    m = m * a.b1 + a.w1 * g;
    v = v * a.b2 + (a.w2 * g) * g;
}

// lamb.py:106-114: -lr * trust ratio from the two squared norms (ratio 1 where either norm is 0)
__device__ __forceinline__ float lamb_step(const Hyper& a, double p2, double u2) {
    const float wn = (float)sqrt(p2), un = (float)sqrt(u2);
    const float r = (wn > 0.0f && un > 0.0f) ? wn / un : 1.0f;
    return a.neg_lr * r;
}

// torch.optim.adam._single_tensor_adam, the non-capturable branch (decoupled = AdamW), of one element
__device__ __forceinline__ void adam_element(const Hyper& a, float g, float& p, float& m, float& v) {
    if (a.wd_nonzero) {
        if (a.decoupled) p = p * a.decay;
        else g = g + a.wd * p;
    }
    const float d = g - m;
    m = fabsf(a.w1) < 0.5f ? m + a.w1 * d : g - d * (1.0f - a.w1);  // Tensor.lerp_
    v = v * a.b2 + (a.w2 * g) * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p + (a.neg_step * m) / denom;                                // addcdiv_
}

// sam.py:96-111: what an element adds (squared) to the gradient norm
__device__ __forceinline__ float climb_q(const Hyper& a, float p, float g) { return a.adaptive ? fabsf(p) * g : g; }

// sam.py:33-35: rho / (norm + 1e-12) from the squared norm
__device__ __forceinline__ float climb_scale(const Hyper& a, double n2) { return a.rho / ((float)sqrt(n2) + 1e-12f); }

// sam.py:36-46: the climbed element
__device__ __forceinline__ float climb(const Hyper& a, float p, float g, float scale) {
    return p + (a.adaptive ? ((p * p) * g) * scale : g * scale);
}

// The ValueErrors of lamb.py:34-41 and torch.optim.Adam, and a nan rho.
inline int check_config(const char* who, const vqae_classifier_optim_config* cfg) {
    VQAE_REQUIRE(cfg, VQAE_ERR_INVALID, "%s: null config", who);
    VQAE_REQUIRE(cfg->kind == VQAE_OPTIM_ADAM || cfg->kind == VQAE_OPTIM_ADAMW || cfg->kind == VQAE_OPTIM_LAMB, VQAE_ERR_INVALID,
                 "%s: unknown optimiser kind %d", who, cfg->kind);
    VQAE_REQUIRE(cfg->lr >= 0.0, VQAE_ERR_INVALID, "%s: invalid learning rate %g", who, cfg->lr);
    VQAE_REQUIRE(cfg->eps >= 0.0, VQAE_ERR_INVALID, "%s: invalid epsilon value %g", who, cfg->eps);
    VQAE_REQUIRE(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0, VQAE_ERR_INVALID, "%s: invalid beta parameter at index 0: %g", who, cfg->beta1);
    VQAE_REQUIRE(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0, VQAE_ERR_INVALID, "%s: invalid beta parameter at index 1: %g", who, cfg->beta2);
    VQAE_REQUIRE(cfg->weight_decay >= 0.0, VQAE_ERR_INVALID, "%s: invalid weight_decay value %g", who, cfg->weight_decay);
    VQAE_REQUIRE(!std::isnan(cfg->sam_rho), VQAE_ERR_INVALID, "%s: sam_rho is nan", who);
    return VQAE_OK;
}

// The scalars of step number t (counted from 1) of one group; t = 0 for the climb, which reads rho and adaptive only.
inline Hyper make_hyper(const vqae_classifier_optim_config& f, double t) {
    Hyper a{};
    const double bc1 = 1.0 - std::pow(f.beta1, t), bc2 = 1.0 - std::pow(f.beta2, t);
    a.decoupled = f.kind == VQAE_OPTIM_ADAMW;
    a.adaptive = f.sam_adaptive != 0;
    a.wd_nonzero = f.weight_decay != 0.0;
    a.rho = (float)f.sam_rho;
    a.decay = (float)(1.0 - f.lr * f.weight_decay);
    a.w1 = (float)(1.0 - f.beta1); a.b1 = (float)f.beta1; a.b2 = (float)f.beta2; a.w2 = (float)(1.0 - f.beta2);
    a.bc1 = (float)bc1; a.bc2 = (float)bc2; a.bc2_sqrt = (float)std::sqrt(bc2);
    a.eps = (float)f.eps; a.neg_step = (float)(-(f.lr / bc1)); a.wd = (float)f.weight_decay; a.neg_lr = (float)(-f.lr);
    return a;
}

}  // namespace vqae_om
