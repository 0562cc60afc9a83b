// What classifier.hip (the fused forward), classifier_train.hip (loss and gradients) and classifier_optim.hip (the
// optimiser step on the device image) share: the tile constants, the device arithmetic the first two must spell identically
// (ELU, softplus, code loads, the shuffle sums), the handle and its host helpers.  Private to csrc/.
#pragma once
#include "common.h"

#include <mutex>
#include <vector>

namespace vqae_cls {

constexpr int NT = 256;                 // threads per workgroup
constexpr int TH = 14;                  // output rows per tile
constexpr int SK = VQAE_CLS_STATS_K;
constexpr int CEK = VQAE_CE_STATS_K;    // columns of a cross-entropy stats row

// ELU(alpha = 1) with the negative side to <= 3 ulp of expm1: the degree-7 Taylor series for v > -0.3 (next term
// 0.3^7 / 40320 = 5e-9 relative), the hardware exponential minus one beyond (no cancellation there: |result| >= 0.26).
__device__ __forceinline__ float elu1(float v) {
    const float e = __builtin_amdgcn_exp2f(v * 1.44269504088896341f) - 1.0f;
    float p = 1.0f / 5040.0f;
    p = fmaf(p, v, 1.0f / 720.0f);
    p = fmaf(p, v, 1.0f / 120.0f);
    p = fmaf(p, v, 1.0f / 24.0f);
    p = fmaf(p, v, 1.0f / 6.0f);
    p = fmaf(p, v, 0.5f);
    p = fmaf(p, v, 1.0f);
    const float n = v > -0.3f ? p * v : e;
    return v > 0.0f ? v : n;
}

__device__ __forceinline__ int64_t load_code(const void* __restrict__ p, int dt, int64_t i) {
    switch (dt) {
        case VQAE_IDX_U8: return ((const uint8_t*)p)[i];
        case VQAE_IDX_U16: return ((const uint16_t*)p)[i];
        case VQAE_IDX_I32: return ((const int32_t*)p)[i];
        default: return ((const int64_t*)p)[i];
    }
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

using vqae::wave_sum;                   // double / int shuffle sums (common.h)

inline bool idx_dtype_ok(int dt) { return dt == VQAE_IDX_I64 || dt == VQAE_IDX_U8 || dt == VQAE_IDX_U16 || dt == VQAE_IDX_I32; }

}  // namespace vqae_cls

struct vqae_classifier {
    int K = 0, E = 0, C = 0, NO = 0;
    int tw = 0;                       // tile width of the geometry this (E, C) runs on: 62 or 30
    // one packed image, on the host and on the device: table [K][E], w1 [E][9][C], b1 [C], w2 [C][9][C], b2 [C],
    // w3 [C][9][NO], b3 [NO]  (conv weights repacked from PyTorch's [cout][cin][3][3] to [cin][tap][cout]; every block
    // starts on a multiple of 16 floats and the padding is 0).  Either copy can be the newer one, never both:
    //   host_newer  vqae_classifier_create / _update wrote the host image; ensure_device uploads it before the next launch;
    //   dev_newer   a vqae_classifier_optim step rewrote the device image in place; ensure_device must NOT upload, and the
    //               host image is brought up to date only by vqae_classifier_download.
    // vqae_classifier_update sets host_newer and clears dev_newer (the host weights win); a step uploads a pending host
    // image first, then sets dev_newer.
    std::vector<float> host;
    size_t o_table = 0, o_w1 = 0, o_b1 = 0, o_w2 = 0, o_b2 = 0, o_w3 = 0, o_b3 = 0;
    float* dev = nullptr;
    int dev_id = -1;
    bool host_newer = false;          // the host image changed after the upload
    bool dev_newer = false;           // an optimiser step changed the device image after the upload
    std::mutex mu;
};

namespace vqae_cls {

int64_t tile_count(const vqae_classifier* c, int h, int w, int* tiles_x);
// the device image of the weights on the current device, uploaded (again) on `st` where it is missing or the host image is
// the newer one; never uploaded over a device image that holds optimiser steps (VQAE_ERR_INVALID where those steps were made
// on another device: download them there first)
int ensure_device(vqae_classifier* c, hipStream_t st);
// PyTorch parameter order: the dense start of tensor i in the packed gradient (start[7] = the total), its offset in the
// image, and for the conv weights cout and cin * 9 (cout = 0 for the table and the biases, which are stored as they are)
struct ParamMap { int start[8]; int off[7]; int cout[7]; int cin9[7]; };
ParamMap param_map(const vqae_classifier* c);
// The forward launch (and, with stats_dev, its stats reduction) after validation, batch >= 1.  target_dev (fp32 [B][h][w],
// optional) replaces the hard target mask - 1 in the loss sum; grad_logit_dev (fp32 [B][h][w], optional; needs the mask)
// receives dL/dlogit of the summed loss: sigmoid(x) * (1 - t + pos_weight * t) - pos_weight * t where mask != 0, 0 elsewhere.
// With `ce` (n_out > 1) the epilogue is the cross-entropy one instead: mask_dev holds the class indices, the stats rows have
// CEK columns (VQAE_CE_*), grad_logit_dev is fp32 [B][n_out][h][w] and heat / target / pos_weight are not read.
struct CeArgs {
    uint8_t* prob = nullptr;          // uint8 [B][n_out][h][w] = rintf(255 * softmax), optional
    uint8_t* cls = nullptr;           // uint8 [B][h][w] = argmax, lowest index on ties, optional
    float w[4] = {1.0f, 1.0f, 1.0f, 1.0f};   // class weights (entries >= n_out are not read)
    float keep = 1.0f, smooth = 0.0f; // 1 - label_smoothing and label_smoothing / n_out, rounded once from double
};
int forward_launch(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w, float* logits_dev,
                   uint8_t* heat_u8_dev, const uint8_t* mask_dev, const float* target_dev, float pos_weight,
                   float* grad_logit_dev, double* stats_dev, void* workspace_dev, hipStream_t st, const CeArgs* ce = nullptr);
// What the cross-entropy entry points share: weight (host [n_out] or null = ones) and label_smoothing checked and rounded.
int ce_args(const char* who, const vqae_classifier* c, const float* weight, float label_smoothing, CeArgs* out);

}  // namespace vqae_cls
