// The optimiser step of the slide classifier on the handle's own device image (gfx950): torch.optim.Adam / AdamW in their
// single-tensor form, the reference's Lamb (vq_ae/optim/lamb.py:78-114) and its SAM wrapper (vq_ae/optim/sam.py:31-60,
// 96-111).  The packed fp64 gradient of vqae_classifier_loss_grad is read once (rounded to fp32 on read, as `.grad` is), the
// fp32 moments live dense in PyTorch parameter order, and the weights are read and rewritten where the forward and backward
// kernels read them: the conv weights' [cout][cin][tap] index is permuted to the image's [cin][tap][cout] on the fly, the
// padding between the blocks is never touched.
//
// Every element is independent but for the norms: LAMB needs ||p|| and ||u|| of each of the seven tensors, SAM's climb one
// norm over all of them (formed, as sam.py does, from the seven tensors' own).  They are sums of fp32 squares in fp64, taken
// in an order that depends on the shapes only: a thread adds its elements of a tensor in index order, the 64 lanes of a wave
// fold by shuffles, the four waves are added in order, and (beyond one workgroup) the workgroups' rows of `partial` are added
// the same way by every workgroup of the second launch.  No atomics: two runs give the same bits.
//   G <= ONE_WG_MAX   one launch of one workgroup: moments and norms, barrier, apply (u is recomputed from the stored
//                     moments by the thread that wrote them);
//   larger            optim_norms (one workgroup per CHUNK elements, one row of partials each) then optim_apply.
// Adam and AdamW have no norm: one elementwise launch at any size.
// Division and square root are the correctly rounded ones (eps = 1e-8 stands next to sqrt(v)); the file is built like the
// rest, without fast-math and without contraction.
#include "classifier_impl.h"
#include "optim_math.h"

#include <cmath>

using namespace vqae_cls;
using vqae_om::check_config;

namespace {

constexpr int NS = 14;                  // norm slots: (||p||^2, ||u||^2) of the seven tensors; SAM's climb uses the first of each pair
constexpr int ONE_WG_MAX = 4096;        // parameters one workgroup steps in one launch (16 per thread)
constexpr int CHUNK = 1024;             // parameters per workgroup beyond that

enum { MODE_ADAM = 0, MODE_LAMB = 1, MODE_CLIMB = 2 };

struct Args {
    float* img; float* m; float* v; float* saved; const double* g; double* partial;
    int G, mode, restore;
    ParamMap map;
    vqae_om::Hyper h;                // the per-element arithmetic and these scalars are optim_math.h's, shared with optim.hip
};

// The elements of tensor I among the dense indices j0 .. j1-1, NT apart from the thread's own: f(j, place of j in the
// image).  The walks over the seven tensors are compile-time recursions: every index into the map and into the sums is a
// constant, so both stay in registers, and what a tensor shares (its offsets, LAMB's trust ratio) is scalar.
template <int I, class F>
__device__ __forceinline__ void for_tensor(const ParamMap& mp, int j0, int j1, F&& f) {
    const int start = mp.start[I], off = mp.off[I], cout = mp.cout[I], cin9 = mp.cin9[I];
    const int s = max(j0, start), e = min(j1, mp.start[I + 1]);
    for (int j = s + (int)threadIdx.x; j < e; j += NT) {
        const int l = j - start;
        int ii = off + l;
        if (cout != 0) {
            const int co = l / cin9, r = l - co * cin9;
            ii = off + r * cout + co;
        }
        f(j, ii);
    }
}

// torch.optim.adam._single_tensor_adam, the non-capturable branch (decoupled = AdamW)
template <int I>
__device__ __forceinline__ void adam_tensors(const Args& a, int j0, int j1) {
    if constexpr (I < 7) {
        for_tensor<I>(a.map, j0, j1, [&](int j, int ii) {
            const float g = (float)a.g[j];
            float p = a.restore ? a.saved[j] : a.img[ii];
            float m = a.m[j], v = a.v[j];
            vqae_om::adam_element(a.h, g, p, m, v);
            a.m[j] = m; a.v[j] = v; a.img[ii] = p;
        });
        adam_tensors<I + 1>(a, j0, j1);
    }
}

// first half of a norm mode: LAMB's moments (stored) and this thread's share of ||p||^2, ||u||^2 per tensor; SAM's
// ||a * g||^2 per tensor (sam.py:96-111)
template <int I>
__device__ __forceinline__ void norm_tensors(const Args& a, int j0, int j1, double (&acc)[NS]) {
    if constexpr (I < 7) {
        double sp = 0.0, su = 0.0;                                              // (no lambda here: captured sums go to scratch)
        const int start = a.map.start[I], off = a.map.off[I], cout = a.map.cout[I], cin9 = a.map.cin9[I];
        const int e = min(j1, a.map.start[I + 1]);
        for (int j = max(j0, start) + (int)threadIdx.x; j < e; j += NT) {
            const int l = j - start;
            int ii = off + l;
            if (cout != 0) {
                const int co = l / cin9, r = l - co * cin9;
                ii = off + r * cout + co;
            }
            const float g = (float)a.g[j];
            const float p = a.restore ? a.saved[j] : a.img[ii];
            if (a.mode == MODE_LAMB) {
                float m = a.m[j], v = a.v[j];
                vqae_om::lamb_moments(a.h, g, m, v);
                a.m[j] = m; a.v[j] = v;
                const float u = vqae_om::lamb_u(a.h, m, v, p);
                sp += (double)(p * p);
                su += (double)(u * u);
            } else {
                const float q = vqae_om::climb_q(a.h, p, g);
                sp += (double)(q * q);
            }
        }
        acc[2 * I] = sp; acc[2 * I + 1] = su;
        norm_tensors<I + 1>(a, j0, j1, acc);
    }
}

template <int I>
__device__ __forceinline__ void apply_tensors(const Args& a, int j0, int j1, const double* sums, float scale) {
    if constexpr (I < 7) {
        float step = 0.0f;
        if (a.mode == MODE_LAMB) step = vqae_om::lamb_step(a.h, sums[2 * I], sums[2 * I + 1]);   // lamb.py:106-114
        for_tensor<I>(a.map, j0, j1, [&](int j, int ii) {
            const float p = a.restore ? a.saved[j] : a.img[ii];
            if (a.mode == MODE_LAMB) {
                a.img[ii] = p + step * vqae_om::lamb_u(a.h, a.m[j], a.v[j], p);
            } else {                                                             // sam.py:36-46
                const float g = (float)a.g[j];
                a.saved[j] = p;
                a.img[ii] = vqae_om::climb(a.h, p, g, scale);
            }
        });
        apply_tensors<I + 1>(a, j0, j1, sums, scale);
    }
}

__device__ __forceinline__ void apply_pass(const Args& a, int j0, int j1, const double* sums) {
    float scale = 0.0f;
    if (a.mode == MODE_CLIMB) {                                                  // sam.py:33-35: the norm of the seven norms
        double n2 = sums[0];
#pragma unroll
        for (int i = 1; i < 7; ++i) n2 += sums[2 * i];
        scale = vqae_om::climb_scale(a.h, n2);
    }
    apply_tensors<0>(a, j0, j1, sums, scale);
}

// per-thread sums -> sums[NS] in LDS, in a fixed order; ends behind a barrier
__device__ __forceinline__ void block_sums(double (&acc)[NS], double (*red)[NS], double* sums) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < NS; ++k) red[tid >> 6][k] = acc[k];
    __syncthreads();
    if (tid < NS) {
        double s = red[0][tid];
        for (int w = 1; w < NT / 64; ++w) s += red[w][tid];
        sums[tid] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void optim_adam(Args a) {
    const int j0 = blockIdx.x * NT;
    adam_tensors<0>(a, j0, min(j0 + NT, a.G));
}

__global__ __launch_bounds__(NT) void optim_one_wg(Args a) {
    __shared__ double red[NT / 64][NS], sums[NS];
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    norm_tensors<0>(a, 0, a.G, acc);
    block_sums(acc, red, sums);
    apply_pass(a, 0, a.G, sums);
}

__global__ __launch_bounds__(NT) void optim_norms(Args a) {
    __shared__ double red[NT / 64][NS], sums[NS];
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const int j0 = blockIdx.x * CHUNK, j1 = min(j0 + CHUNK, a.G);
    norm_tensors<0>(a, j0, j1, acc);
    block_sums(acc, red, sums);
    if (threadIdx.x < NS) a.partial[(size_t)blockIdx.x * NS + threadIdx.x] = sums[threadIdx.x];
}

__global__ __launch_bounds__(NT) void optim_apply(Args a, int n_rows) {
    __shared__ double red[NT / 64][NS], sums[NS];
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    for (int r = threadIdx.x; r < n_rows; r += NT)                 // every workgroup adds the rows in the same order
#pragma unroll
        for (int k = 0; k < NS; ++k) acc[k] += a.partial[(size_t)r * NS + k];
    block_sums(acc, red, sums);
    const int j0 = blockIdx.x * CHUNK, j1 = min(j0 + CHUNK, a.G);
    apply_pass(a, j0, j1, sums);
}

}  // namespace

struct vqae_classifier_optim {
    vqae_classifier* c = nullptr;
    vqae_classifier_optim_config cfg{};
    int G = 0, n_rows = 0, dev_id = -1;
    int64_t step = 0;
    bool climbed = false;             // a SAM first step is waiting for its second
    float* state = nullptr;           // one allocation: exp_avg [G], exp_avg_sq [G], SAM's old_p [G], then the partials
    float *m = nullptr, *v = nullptr, *saved = nullptr;
    double* partial = nullptr;
};

// The step kernels walk the packed gradient and the image through param_map, which follows n_out (out_conv's [NO][C][9] and
// [NO] are tensors 5 and 6, each with its own LAMB norms): the two entry points differ in the n_out they accept only.
static int optim_create(const char* who, bool ce, vqae_classifier* c, const vqae_classifier_optim_config* cfg,
                        vqae_classifier_optim** out) {
    VQAE_REQUIRE(out, VQAE_ERR_INVALID, "%s: null out", who);
    *out = nullptr;
    VQAE_REQUIRE(c, VQAE_ERR_INVALID, "%s: null classifier", who);
    if (int rc = check_config(who, cfg)) return rc;
    if (ce) VQAE_REQUIRE(c->NO > 1, VQAE_ERR_UNSUPPORTED, "%s: cross-entropy needs n_out >= 2; vqae_classifier_optim_create trains n_out == 1", who);
    else VQAE_REQUIRE(c->NO == 1, VQAE_ERR_UNSUPPORTED, "%s: the loss is defined for n_out == 1, this classifier has %d", who, c->NO);
    if (int rc = ensure_device(c, nullptr)) return rc;             // the image this optimiser steps, on the current device
    vqae_classifier_optim* o = new vqae_classifier_optim;
    o->c = c; o->cfg = *cfg; o->dev_id = c->dev_id;
    o->G = (int)vqae_classifier_grad_floats(c);
    o->n_rows = (int)vqae::ceil_div(o->G, CHUNK);
    const size_t gpad = (size_t)vqae::round_up(o->G, 64);
    const size_t bytes = 3 * gpad * sizeof(float) + (size_t)o->n_rows * NS * sizeof(double);
    hipError_t e = hipMalloc((void**)&o->state, bytes);
    if (e == hipSuccess) e = hipMemset(o->state, 0, bytes);
    if (e != hipSuccess) {
        if (o->state) (void)hipFree(o->state);
        delete o;
        return vqae::fail(VQAE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    o->m = o->state; o->v = o->m + gpad; o->saved = o->v + gpad; o->partial = (double*)(o->saved + gpad);
    *out = o;
    return VQAE_OK;
}

extern "C" int vqae_classifier_optim_create(vqae_classifier* c, const vqae_classifier_optim_config* cfg,
                                            vqae_classifier_optim** out) {
    return optim_create("classifier_optim_create", false, c, cfg, out);
}

extern "C" int vqae_classifier_optim_create_ce(vqae_classifier* c, const vqae_classifier_optim_config* cfg,
                                               vqae_classifier_optim** out) {
    return optim_create("classifier_optim_create_ce", true, c, cfg, out);
}

extern "C" void vqae_classifier_optim_destroy(vqae_classifier_optim* o) {
    if (!o) return;
    if (o->state) (void)hipFree(o->state);
    delete o;
}

extern "C" int vqae_classifier_optim_set(vqae_classifier_optim* o, const vqae_classifier_optim_config* cfg) {
    VQAE_REQUIRE(o, VQAE_ERR_INVALID, "classifier_optim_set: null optimiser");
    if (int rc = check_config("classifier_optim_set", cfg)) return rc;
    VQAE_REQUIRE(cfg->kind == o->cfg.kind, VQAE_ERR_INVALID, "classifier_optim_set: the kind is fixed at creation (%d, not %d)",
                 o->cfg.kind, cfg->kind);
    VQAE_REQUIRE((cfg->sam_rho < 0.0) == (o->cfg.sam_rho < 0.0), VQAE_ERR_INVALID,
                 "classifier_optim_set: SAM is switched on or off at creation");
    o->cfg = *cfg;
    return VQAE_OK;
}

namespace {

// what both entry points check and prepare: the image on this device, a pending host image uploaded first
int begin(const char* who, vqae_classifier_optim* o, const double* grads_dev, hipStream_t st, Args* a) {
    VQAE_REQUIRE(o && grads_dev, VQAE_ERR_INVALID, "%s: null pointer", who);
    vqae_classifier* c = o->c;
    if (int rc = ensure_device(c, st)) return rc;
    VQAE_REQUIRE(c->dev_id == o->dev_id, VQAE_ERR_INVALID, "%s: the optimiser state lives on device %d, the weights on %d", who,
                 o->dev_id, c->dev_id);
    const vqae_classifier_optim_config& f = o->cfg;
    a->img = c->dev; a->m = o->m; a->v = o->v; a->saved = o->saved; a->g = grads_dev; a->partial = o->partial;
    a->G = o->G;
    a->restore = 0;
    a->map = param_map(c);
    a->h = vqae_om::make_hyper(f, 0.0);                          // the climb reads rho and adaptive only
    return VQAE_OK;
}

int launch_norm_mode(const vqae_classifier_optim* o, const Args& a, hipStream_t st) {
    if (a.G <= ONE_WG_MAX) {
        optim_one_wg<<<1, NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
    } else {
        optim_norms<<<o->n_rows, NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
        optim_apply<<<o->n_rows, NT, 0, st>>>(a, o->n_rows);
        VQAE_LAUNCH_CHECK();
    }
    return VQAE_OK;
}

}  // namespace

extern "C" int vqae_classifier_optim_sam_first(vqae_classifier_optim* o, const double* grads_dev, void* stream) {
    Args a{};
    VQAE_REQUIRE(o && grads_dev, VQAE_ERR_INVALID, "classifier_optim_sam_first: null pointer");
    VQAE_REQUIRE(o->cfg.sam_rho >= 0.0, VQAE_ERR_INVALID, "classifier_optim_sam_first: the optimiser was created without SAM");
    VQAE_REQUIRE(!o->climbed, VQAE_ERR_INVALID, "classifier_optim_sam_first: a first step is already waiting for its step");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = begin("classifier_optim_sam_first", o, grads_dev, st, &a)) return rc;
    a.mode = MODE_CLIMB;
    if (int rc = launch_norm_mode(o, a, st)) return rc;
    std::lock_guard<std::mutex> lock(o->c->mu);
    o->c->dev_newer = true;
    o->climbed = true;
    return VQAE_OK;
}

extern "C" int vqae_classifier_optim_step(vqae_classifier_optim* o, const double* grads_dev, void* stream) {
    Args a{};
    hipStream_t st = (hipStream_t)stream;
    if (int rc = begin("classifier_optim_step", o, grads_dev, st, &a)) return rc;
    const vqae_classifier_optim_config& f = o->cfg;
    a.restore = o->climbed;                                        // sam.py:53-56: back to w, then the base step
    a.h = vqae_om::make_hyper(f, (double)(o->step + 1));
    if (f.kind == VQAE_OPTIM_LAMB) {
        a.mode = MODE_LAMB;
        if (int rc = launch_norm_mode(o, a, st)) return rc;
    } else {
        a.mode = MODE_ADAM;
        optim_adam<<<(unsigned)vqae::ceil_div(a.G, NT), NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
    }
    std::lock_guard<std::mutex> lock(o->c->mu);
    o->c->dev_newer = true;
    o->climbed = false;
    o->step += 1;
    return VQAE_OK;
}

extern "C" int vqae_classifier_optim_export(vqae_classifier_optim* o, float* exp_avg, float* exp_avg_sq, int64_t* step, void* stream) {
    VQAE_REQUIRE(o && exp_avg && exp_avg_sq && step, VQAE_ERR_INVALID, "classifier_optim_export: null pointer");
    hipStream_t st = (hipStream_t)stream;
    VQAE_HIP_CHECK(hipMemcpyAsync(exp_avg, o->m, (size_t)o->G * sizeof(float), hipMemcpyDeviceToHost, st));
    VQAE_HIP_CHECK(hipMemcpyAsync(exp_avg_sq, o->v, (size_t)o->G * sizeof(float), hipMemcpyDeviceToHost, st));
    VQAE_HIP_CHECK(hipStreamSynchronize(st));
    *step = o->step;
    return VQAE_OK;
}

extern "C" int vqae_classifier_optim_import(vqae_classifier_optim* o, const float* exp_avg, const float* exp_avg_sq, int64_t step,
                                            void* stream) {
    VQAE_REQUIRE(o && exp_avg && exp_avg_sq, VQAE_ERR_INVALID, "classifier_optim_import: null pointer");
    VQAE_REQUIRE(step >= 0, VQAE_ERR_INVALID, "classifier_optim_import: step %lld < 0", (long long)step);
    VQAE_REQUIRE(!o->climbed, VQAE_ERR_INVALID, "classifier_optim_import: a SAM first step is waiting for its step");
    hipStream_t st = (hipStream_t)stream;
    VQAE_HIP_CHECK(hipMemcpyAsync(o->m, exp_avg, (size_t)o->G * sizeof(float), hipMemcpyHostToDevice, st));
    VQAE_HIP_CHECK(hipMemcpyAsync(o->v, exp_avg_sq, (size_t)o->G * sizeof(float), hipMemcpyHostToDevice, st));
    VQAE_HIP_CHECK(hipStreamSynchronize(st));                      // the host buffers may be pageable
    o->step = step;
    return VQAE_OK;
}
