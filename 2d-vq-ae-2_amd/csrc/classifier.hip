// The downstream slide classifier on stored code grids (gfx950): the reference's validation_nn CNNClassifier
// (validation_nn/model.py:141-142 over the layers of conf/model/cnn_classifier.yaml) in ONE launch per batch of grids:
//   nn.Embedding(K, E) -> FlattenAfterEmbedding (layers/misc.py:9-22) -> Conv2d(E, C, 3, zero pad, bias) -> ELU
//   -> Conv2d(C, C, 3) -> ELU -> Conv2d(C, n_out, 3)
// and, for n_out == 1, the uint8 probability map and the masked confusion counts / BCE sum of Camelyon16BCELoss
// (utils/train_helpers.py:101-138) from the same registers.
//
// A workgroup of 256 threads owns an output tile of TH = 14 rows x TW columns of a [B][H][W] grid and recomputes the halos:
//   stage 0  the table [K][E] -> LDS (when it fits beside the planes; read from global memory otherwise)
//   stage 1  embedding of the tile + 3:  plane E0 [E][TH+6][TW+6]      (0 outside the grid and for a code outside 0 .. K-1)
//   stage 2  in_conv + ELU on tile + 2:  plane A  [C][TH+4][TW+4]      (0 outside the grid: the next conv pads ITS input)
//   stage 3  hidden_conv1 + ELU, tile+1: plane B  [C][TH+2][TW+2]      (0 outside the grid), B overlays E0 (dead by then)
//   stage 4  out_conv on the tile -> logits / heat / stats partials
// Planes are channel-major, so the lanes of a wave (consecutive x) read consecutive LDS words.  Stage 3 carries 88 % of the
// arithmetic: a thread owns a column strip of P rows x all C channels (P * C = 32 accumulators), so the (P + 2) x 3 inputs
// it reads per input channel feed 9 * C * P fmaf; (TW + 2) * (TH + 2) / P = 256 strips, one per thread.  Weights are
// repacked [cin][tap][cout] and indexed uniformly, so they arrive through the scalar cache as FMA operands and cost no LDS
// or vector-memory traffic.  Two geometries: TW = 62, P = 4 (C = 8, E <= 6: 70.8 KB of planes) and TW = 30, P = 2 (C = 16,
// or E > 6: at most 72 KB): two workgroups per CU in every case.
// Stats: per-thread integer counts and an fp64 loss sum -> wave shuffles -> the workgroup's row of `part`; a second launch
// sums a slide's rows in a fixed order.  No atomics; the partition depends on (h, w) only, so a slide's stats are
// bit-identical run to run and at any batch position.
#include "classifier_impl.h"

#include <cmath>
#include <string>

using namespace vqae_cls;

namespace {

constexpr int LDS_PER_WG = 80 * 1024;   // half a CU's 160 KiB: two workgroups per CU

template <int TW> struct Geo {
    static constexpr int EW = TW + 6, EH = TH + 6;     // embedding region
    static constexpr int AW = TW + 4, AH = TH + 4;     // layer-1 region
    static constexpr int BW = TW + 2, BH = TH + 2;     // layer-2 region
};

// floats of LDS the planes take: A + max(E0, B)
int plane_floats(int tw, int E, int C) {
    const int e0 = E * (TH + 6) * (tw + 6), a = C * (TH + 4) * (tw + 4), b = C * (TH + 2) * (tw + 2);
    return a + (e0 > b ? e0 : b);
}

template <int C, int NO, int TW, int P>
__global__ __launch_bounds__(NT)
void classifier_kernel(const void* __restrict__ codes, int idx_dtype, int H, int W, int tiles_x,
                       const float* __restrict__ table, int K, int E, int table_lds,
                       const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                       const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
                       float* __restrict__ logits, uint8_t* __restrict__ heat, const uint8_t* __restrict__ mask,
                       const float* __restrict__ target, float pos_weight, float* __restrict__ glogit,
                       double* __restrict__ part, CeArgs ce) {
    using G = Geo<TW>;
    constexpr int EN = G::EH * G::EW, AN = G::AH * G::AW, BN = G::BH * G::BW;
    static_assert(BN / P == NT && G::BH % P == 0, "stage 3: one column strip per thread");
    static_assert(TH % 2 == 0, "stage 4 walks strips of two rows");
    extern __shared__ float lds[];
    float* const pa = lds;                                        // A  [C][AH][AW]
    float* const pe = pa + C * AN;                                // E0 [E][EH][EW], then B [C][BH][BW]
    float* const pt = pe + (E * EN > C * BN ? E * EN : C * BN);   // table [K][E] when table_lds
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const int64_t hw = (int64_t)H * W;

    // ---- stage 0 / 1: table and embedding of the tile + 3 --------------------------------------------------------------
    if (table_lds) {
        for (int i = tid; i < K * E; i += NT) pt[i] = table[i];
        __syncthreads();
    }
    for (int i = tid; i < EN; i += NT) {
        const int ly = i / G::EW, lx = i - ly * G::EW;
        const int gy = y0 - 3 + ly, gx = x0 - 3 + lx;
        int64_t code = -1;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) code = load_code(codes, idx_dtype, (int64_t)b * hw + (int64_t)gy * W + gx);
        const bool ok = code >= 0 && code < K;
        const int64_t row = ok ? code * E : 0;
        if (table_lds) {
            for (int e = 0; e < E; ++e) pe[e * EN + i] = ok ? pt[row + e] : 0.0f;
        } else {
            for (int e = 0; e < E; ++e) pe[e * EN + i] = ok ? table[row + e] : 0.0f;
        }
    }
    __syncthreads();

    // ---- stage 2: in_conv + ELU on the tile + 2 ------------------------------------------------------------------------
    for (int i = tid; i < AN; i += NT) {
        const int ly = i / G::AW, lx = i - ly * G::AW;
        const int gy = y0 - 2 + ly, gx = x0 - 2 + lx;
        float acc[C];
#pragma unroll
        for (int co = 0; co < C; ++co) acc[co] = b1[co];
#pragma unroll 1
        for (int e = 0; e < E; ++e) {
            const float* ep = pe + e * EN + ly * G::EW + lx;      // region E0 starts one code further out than A
            const float* wp = w1 + e * 9 * C;
            float in[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) in[t] = ep[(t / 3) * G::EW + (t % 3)];
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int co = 0; co < C; ++co) acc[co] = fmaf(wp[t * C + co], in[t], acc[co]);
        }
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
        for (int co = 0; co < C; ++co) pa[co * AN + i] = inside ? elu1(acc[co]) : 0.0f;
    }
    __syncthreads();                                              // A complete; E0 dead: B may overwrite it

    // ---- stage 3: hidden_conv1 + ELU on the tile + 1: one strip of P rows per thread --------------------------------------
    {
        const int s = tid / G::BW, lx = tid - s * G::BW, ly0 = s * P;
        float acc[P][C];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int co = 0; co < C; ++co) acc[p][co] = b2[co];
#pragma unroll 1
        for (int ci = 0; ci < C; ++ci) {
            const float* ap = pa + ci * AN + ly0 * G::AW + lx;
            const float* wp = w2 + ci * 9 * C;
            float in[P + 2][3];
#pragma unroll
            for (int r = 0; r < P + 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) in[r][k] = ap[r * G::AW + k];
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int co = 0; co < C; ++co) {
                    const float wv = wp[t * C + co];
#pragma unroll
                    for (int p = 0; p < P; ++p) acc[p][co] = fmaf(wv, in[p + t / 3][t % 3], acc[p][co]);
                }
        }
        const int gx = x0 - 1 + lx;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int gy = y0 - 1 + ly0 + p;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
            for (int co = 0; co < C; ++co) pe[co * BN + (ly0 + p) * G::BW + lx] = inside ? elu1(acc[p][co]) : 0.0f;
        }
    }
    __syncthreads();

    // ---- stage 4: out_conv on the tile, strips of two rows; logits / heat / stats ---------------------------------------
    int n_tp = 0, n_fp = 0, n_fn = 0, n_tn = 0;
    double loss = 0.0;
    int conf[NO][NO], n_bad = 0;                                  // cross-entropy (NO > 1): counts at [label][prediction]
    double s_w = 0.0, s_nll = 0.0, s_sm = 0.0;
#pragma unroll
    for (int l = 0; l < NO; ++l)
#pragma unroll
        for (int q = 0; q < NO; ++q) conf[l][q] = 0;
    for (int it = tid; it < (TH / 2) * TW; it += NT) {
        const int s = it / TW, lx = it - s * TW, ly0 = 2 * s;
        float acc[2][NO];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[p][o] = b3[o];
#pragma unroll 1
        for (int ci = 0; ci < C; ++ci) {
            const float* bp = pe + ci * BN + ly0 * G::BW + lx;
            const float* wp = w3 + ci * 9 * NO;
            float in[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) in[r][k] = bp[r * G::BW + k];
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    const float wv = wp[t * NO + o];
#pragma unroll
                    for (int p = 0; p < 2; ++p) acc[p][o] = fmaf(wv, in[p + t / 3][t % 3], acc[p][o]);
                }
        }
        const int gx = x0 + lx;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int gy = y0 + ly0 + p;
            if (gy < H && gx < W) {
                const int64_t pos = (int64_t)gy * W + gx;
                if (logits) {
#pragma unroll
                    for (int o = 0; o < NO; ++o) logits[((int64_t)b * NO + o) * hw + pos] = acc[p][o];
                }
                if constexpr (NO == 1) {
                    const float x = acc[p][0];
                    if (heat) heat[(int64_t)b * hw + pos] = (uint8_t)rintf(255.0f * (1.0f / (1.0f + expf(-x))));
                    if (mask) {
                        const uint8_t m = mask[(int64_t)b * hw + pos];
                        float g = 0.0f;
                        if (m != 0) {
                            const bool t = m >= 2, pr = x > 0.0f;
                            n_tp += pr && t; n_fp += pr && !t; n_fn += !pr && t; n_tn += !pr && !t;
                            if (target) {                          // soft target (label smoothing), read where valid only
                                const float ts = target[(int64_t)b * hw + pos];
                                loss += (double)pos_weight * (double)ts * (double)softplus(-x) +
                                        (1.0 - (double)ts) * (double)softplus(x);
                                if (glogit) {
                                    const float pt = pos_weight * ts;
                                    g = (1.0f / (1.0f + expf(-x))) * ((1.0f - ts) + pt) - pt;
                                }
                            } else {
                                loss += t ? (double)pos_weight * (double)softplus(-x) : (double)softplus(x);
                                if (glogit) {
                                    const float sg = 1.0f / (1.0f + expf(-x));
                                    g = t ? pos_weight * sg - pos_weight : sg;
                                }
                            }
                        }
                        if (glogit) glogit[(int64_t)b * hw + pos] = g;
                    }
                } else {
                    // nn.CrossEntropyLoss(weight, label_smoothing) on the NO logits of this position: a log-softmax on
                    // the max-subtracted logits in fp32, the loss terms summed in fp64.  -log p_c = lse - (x_c - max).
                    float mx = acc[p][0];
                    int am = 0;
#pragma unroll
                    for (int o = 1; o < NO; ++o)
                        if (acc[p][o] > mx) { mx = acc[p][o]; am = o; }   // strict: the lowest index wins a tie
                    if (ce.cls) ce.cls[(int64_t)b * hw + pos] = (uint8_t)am;
                    if (ce.prob || mask) {
                        float ex[NO], se = 0.0f;
#pragma unroll
                        for (int o = 0; o < NO; ++o) { ex[o] = expf(acc[p][o] - mx); se += ex[o]; }
                        const float inv = 1.0f / se;
                        if (ce.prob) {
#pragma unroll
                            for (int o = 0; o < NO; ++o)
                                ce.prob[((int64_t)b * NO + o) * hw + pos] = (uint8_t)rintf(255.0f * (ex[o] * inv));
                        }
                        if (mask) {
                            const int y = mask[(int64_t)b * hw + pos];
                            float g[NO];
#pragma unroll
                            for (int o = 0; o < NO; ++o) g[o] = 0.0f;
                            if (y < NO) {
                                const float lse = logf(se);
                                float wy = 0.0f, nly = 0.0f, wsum = 0.0f;
                                double sm = 0.0;
#pragma unroll
                                for (int o = 0; o < NO; ++o) {
                                    const float nl = lse - (acc[p][o] - mx);
                                    wsum += ce.w[o];
                                    sm += (double)ce.w[o] * (double)nl;
                                    if (o == y) { wy = ce.w[o]; nly = nl; }
#pragma unroll
                                    for (int q = 0; q < NO; ++q) conf[o][q] += (o == y && q == am);
                                }
                                s_w += (double)wy;
                                s_nll += (double)wy * (double)nly;
                                s_sm += sm;
                                if (glogit) {
                                    // p_y - 1 = -(sum of the other classes' p): no cancellation where p_y is close to 1
                                    float others = 0.0f;
#pragma unroll
                                    for (int o = 0; o < NO; ++o) others += o == y ? 0.0f : ex[o];
#pragma unroll
                                    for (int o = 0; o < NO; ++o) {
                                        const float po = ex[o] * inv;
                                        g[o] = ce.keep * wy * (o == y ? -(others * inv) : po) + ce.smooth * (wsum * po - ce.w[o]);
                                    }
                                }
                            } else {
                                ++n_bad;                           // counted aside, never indexed; its gradient is 0
                            }
                            if (glogit) {
#pragma unroll
                                for (int o = 0; o < NO; ++o) glogit[((int64_t)b * NO + o) * hw + pos] = g[o];
                            }
                        }
                    }
                }
            }
        }
    }
    if constexpr (NO > 1) {
        if (part) {                                               // (workgroup-uniform)
            __shared__ double red[NT / 64][CEK];
            double v[CEK];
#pragma unroll
            for (int k = 0; k < CEK; ++k) v[k] = 0.0;
#pragma unroll
            for (int l = 0; l < NO; ++l)
#pragma unroll
                for (int q = 0; q < NO; ++q) v[l * 4 + q] = conf[l][q];
            v[VQAE_CE_WEIGHT_SUM] = s_w; v[VQAE_CE_NLL_SUM] = s_nll; v[VQAE_CE_SMOOTH_SUM] = s_sm; v[VQAE_CE_N_BAD] = n_bad;
#pragma unroll
            for (int k = 0; k < CEK; ++k) v[k] = wave_sum(v[k]);
            const int wv = tid >> 6;
            if ((tid & 63) == 0)
#pragma unroll
                for (int k = 0; k < CEK; ++k) red[wv][k] = v[k];
            __syncthreads();
            if (tid < CEK) {
                double r = red[0][tid];
                for (int w = 1; w < NT / 64; ++w) r += red[w][tid];
                part[((int64_t)b * gridDim.x + tile) * CEK + tid] = r;
            }
        }
    }
    if constexpr (NO == 1) {
        if (part) {                                               // (workgroup-uniform)
            __shared__ double red[NT / 64][SK];
            n_tp = wave_sum(n_tp); n_fp = wave_sum(n_fp); n_fn = wave_sum(n_fn); n_tn = wave_sum(n_tn);
            loss = wave_sum(loss);
            const int wv = tid >> 6;
            if ((tid & 63) == 0) {
                red[wv][VQAE_CLS_TP] = n_tp; red[wv][VQAE_CLS_FP] = n_fp; red[wv][VQAE_CLS_FN] = n_fn;
                red[wv][VQAE_CLS_TN] = n_tn; red[wv][VQAE_CLS_N_VALID] = n_tp + n_fp + n_fn + n_tn;
                red[wv][VQAE_CLS_LOSS_SUM] = loss;
            }
            __syncthreads();
            if (tid < SK) {
                double r = red[0][tid];
                for (int w = 1; w < NT / 64; ++w) r += red[w][tid];
                part[((int64_t)b * gridDim.x + tile) * SK + tid] = r;
            }
        }
    }
}

// One workgroup per slide (NK columns: the BCE rows or the cross-entropy rows): thread j sums rows j, j + 256, ... in
// order, then the fixed shuffle / LDS order above.
template <int NK>
__global__ __launch_bounds__(NT) void classifier_stats_final(const double* __restrict__ part, int ntiles, double* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* q = part + (int64_t)b * ntiles * NK;
    double r[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) r[k] = 0.0;
    for (int j = tid; j < ntiles; j += NT)
#pragma unroll
        for (int k = 0; k < NK; ++k) r[k] += q[(int64_t)j * NK + k];
    __shared__ double red[NT / 64][NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) r[k] = wave_sum(r[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < NK; ++k) red[tid >> 6][k] = r[k];
    __syncthreads();
    if (tid < NK) {
        double s = red[0][tid];
        for (int w = 1; w < NT / 64; ++w) s += red[w][tid];
        out[(int64_t)b * NK + tid] = s;
    }
}

}  // namespace

namespace {

const vqae_tensor* find_tensor(const vqae_tensor* ts, int n, const char* name) {
    for (int i = 0; i < n; ++i)
        if (ts[i].name && std::strcmp(ts[i].name, name) == 0) return &ts[i];
    return nullptr;
}

void pack_conv(const float* w, int cout, int cin, float* dst) {
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) dst[((size_t)ci * 9 + t) * cout + co] = w[((size_t)co * cin + ci) * 9 + t];
}

// The seven named tensors of a (K, E, C, NO) classifier, checked and found: what create and update share.
int find_weights(const char* who, int K, int E, int C, int NO, const vqae_tensor* tensors, int n_tensors, const vqae_tensor* t[7]) {
    struct Want { const char* name; int64_t numel; };
    const Want want[7] = {{"layers.embedding.weight", (int64_t)K * E},
                          {"layers.in_conv.weight", (int64_t)C * E * 9}, {"layers.in_conv.bias", C},
                          {"layers.hidden_conv1.weight", (int64_t)C * C * 9}, {"layers.hidden_conv1.bias", C},
                          {"layers.out_conv.weight", (int64_t)NO * C * 9}, {"layers.out_conv.bias", NO}};
    for (int i = 0; i < 7; ++i) {
        t[i] = find_tensor(tensors, n_tensors, want[i].name);
        VQAE_REQUIRE(t[i], VQAE_ERR_NOT_FOUND, "%s: tensor '%s' is missing", who, want[i].name);
        VQAE_REQUIRE(t[i]->data && t[i]->numel == want[i].numel, VQAE_ERR_INVALID,
                     "%s: tensor '%s' has %lld elements, expected %lld", who, want[i].name, (long long)t[i]->numel,
                     (long long)want[i].numel);
    }
    return VQAE_OK;
}

void pack_weights(vqae_classifier* c, const vqae_tensor* const t[7]) {
    const int K = c->K, E = c->E, C = c->C, NO = c->NO;
    float* h = c->host.data();
    std::memcpy(h + c->o_table, t[0]->data, sizeof(float) * (size_t)K * E);
    pack_conv(t[1]->data, C, E, h + c->o_w1);
    std::memcpy(h + c->o_b1, t[2]->data, sizeof(float) * C);
    pack_conv(t[3]->data, C, C, h + c->o_w2);
    std::memcpy(h + c->o_b2, t[4]->data, sizeof(float) * C);
    pack_conv(t[5]->data, NO, C, h + c->o_w3);
    std::memcpy(h + c->o_b3, t[6]->data, sizeof(float) * NO);
}

struct Launch {
    const void* codes; int idx_dtype, H, W, tiles_x;
    const float* table; int K, E, table_lds;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float* logits; uint8_t* heat; const uint8_t* mask; const float* target; float pos_weight; float* glogit; double* part;
    CeArgs ce;
    dim3 grid; int lds_bytes; hipStream_t st;
};

template <int C, int NO, int TW, int P>
int launch(const Launch& a) {
    auto kern = classifier_kernel<C, NO, TW, P>;
    if (int rc = vqae::set_max_dynamic_lds((const void*)kern, LDS_PER_WG)) return rc;
    kern<<<a.grid, NT, a.lds_bytes, a.st>>>(a.codes, a.idx_dtype, a.H, a.W, a.tiles_x, a.table, a.K, a.E, a.table_lds, a.w1,
                                           a.b1, a.w2, a.b2, a.w3, a.b3, a.logits, a.heat, a.mask, a.target, a.pos_weight,
                                           a.glogit, a.part, a.ce);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

template <int C, int TW, int P>
int launch_no(int no, const Launch& a) {
    switch (no) {
        case 1: return launch<C, 1, TW, P>(a);
        case 2: return launch<C, 2, TW, P>(a);
        case 3: return launch<C, 3, TW, P>(a);
        default: return launch<C, 4, TW, P>(a);
    }
}

}  // namespace

int64_t vqae_cls::tile_count(const vqae_classifier* c, int h, int w, int* tiles_x) {
    const int64_t tx = vqae::ceil_div(w, c->tw), ty = vqae::ceil_div(h, TH);
    if (tiles_x) *tiles_x = (int)tx;
    return tx * ty;
}

int vqae_cls::ensure_device(vqae_classifier* c, hipStream_t st) {
    int dev = 0;
    VQAE_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->dev && c->dev_id == dev && !c->host_newer) return VQAE_OK;
    VQAE_REQUIRE(!(c->dev_newer && !c->host_newer), VQAE_ERR_INVALID,
                 "classifier: the weights were stepped on device %d and not downloaded; device %d cannot take them", c->dev_id, dev);
    if (c->dev && c->dev_id != dev) {
        (void)hipFree(c->dev);
        c->dev = nullptr;
    }
    if (!c->dev) VQAE_HIP_CHECK(hipMalloc((void**)&c->dev, c->host.size() * sizeof(float)));
    c->dev_id = dev;
    VQAE_HIP_CHECK(hipMemcpyAsync(c->dev, c->host.data(), c->host.size() * sizeof(float), hipMemcpyHostToDevice, st));
    VQAE_HIP_CHECK(hipStreamSynchronize(st));     // once per upload: the host image may be pageable
    c->host_newer = false;
    c->dev_newer = false;
    return VQAE_OK;
}

int vqae_cls::forward_launch(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w, float* logits_dev,
                             uint8_t* heat_u8_dev, const uint8_t* mask_dev, const float* target_dev, float pos_weight,
                             float* grad_logit_dev, double* stats_dev, void* workspace_dev, hipStream_t st, const CeArgs* ce) {
    int tiles_x = 0;
    const int64_t ntiles = tile_count(c, h, w, &tiles_x);
    if (int rc = ensure_device(c, st)) return rc;
    const int planes = plane_floats(c->tw, c->E, c->C) * 4, table = c->K * c->E * 4;
    // (the kernel's static reduction scratch: 4 x 6 doubles, 4 x 20 in the cross-entropy instantiations)
    const bool table_lds = planes + table + (c->NO == 1 ? 256 : 768) <= LDS_PER_WG;
    Launch a;
    a.codes = codes_dev; a.idx_dtype = idx_dtype; a.H = h; a.W = w; a.tiles_x = tiles_x;
    a.table = c->dev + c->o_table; a.K = c->K; a.E = c->E; a.table_lds = table_lds;
    a.w1 = c->dev + c->o_w1; a.b1 = c->dev + c->o_b1; a.w2 = c->dev + c->o_w2; a.b2 = c->dev + c->o_b2;
    a.w3 = c->dev + c->o_w3; a.b3 = c->dev + c->o_b3;
    a.logits = logits_dev; a.heat = heat_u8_dev; a.mask = (stats_dev || grad_logit_dev) ? mask_dev : nullptr;
    a.target = target_dev; a.pos_weight = pos_weight; a.glogit = grad_logit_dev;
    a.part = stats_dev ? (double*)workspace_dev : nullptr;
    if (ce) a.ce = *ce;
    a.grid = dim3((unsigned)ntiles, (unsigned)batch);
    a.lds_bytes = planes + (table_lds ? table : 0);
    a.st = st;
    int rc;
    if (c->tw == 62) rc = launch_no<8, 62, 4>(c->NO, a);
    else if (c->C == 8) rc = launch_no<8, 30, 2>(c->NO, a);
    else rc = launch_no<16, 30, 2>(c->NO, a);
    if (rc) return rc;
    if (stats_dev) {
        if (ce) classifier_stats_final<CEK><<<(unsigned)batch, NT, 0, st>>>((const double*)workspace_dev, (int)ntiles, stats_dev);
        else classifier_stats_final<SK><<<(unsigned)batch, NT, 0, st>>>((const double*)workspace_dev, (int)ntiles, stats_dev);
        VQAE_LAUNCH_CHECK();
    }
    return VQAE_OK;
}

static int check_dims(const char* who, int K, int E, int C, int NO) {
    VQAE_REQUIRE(E >= 1 && E <= 8, VQAE_ERR_UNSUPPORTED, "%s: embedding_dim %d is outside 1 .. 8", who, E);
    VQAE_REQUIRE(C == 8 || C == 16, VQAE_ERR_UNSUPPORTED, "%s: hidden width %d is not 8 or 16", who, C);
    VQAE_REQUIRE(NO >= 1 && NO <= 4, VQAE_ERR_UNSUPPORTED, "%s: n_out %d is outside 1 .. 4", who, NO);
    VQAE_REQUIRE(K >= 1 && K <= 65536, VQAE_ERR_UNSUPPORTED, "%s: num_embeddings %d is outside 1 .. 65536", who, K);
    return VQAE_OK;
}

extern "C" int vqae_classifier_create(int num_embeddings, int embedding_dim, int hidden, int n_out, const vqae_tensor* tensors,
                                      int n_tensors, vqae_classifier** out) {
    VQAE_REQUIRE(out, VQAE_ERR_INVALID, "classifier_create: null out");
    *out = nullptr;
    VQAE_REQUIRE(n_tensors >= 0 && (tensors || n_tensors == 0), VQAE_ERR_INVALID, "classifier_create: null tensors");
    const int K = num_embeddings, E = embedding_dim, C = hidden, NO = n_out;
    if (int rc = check_dims("classifier_create", K, E, C, NO)) return rc;
    const vqae_tensor* t[7];
    if (int rc = find_weights("classifier_create", K, E, C, NO, tensors, n_tensors, t)) return rc;
    vqae_classifier* c = new vqae_classifier;
    c->K = K; c->E = E; c->C = C; c->NO = NO;
    c->tw = (C == 8 && E <= 6) ? 62 : 30;
    size_t n = 0;
    auto take = [&n](int64_t numel) { const size_t o = n; n += (size_t)vqae::round_up(numel, 16); return o; };   // 64-byte rows
    c->o_table = take((int64_t)K * E); c->o_w1 = take((int64_t)C * E * 9); c->o_b1 = take(C); c->o_w2 = take((int64_t)C * C * 9);
    c->o_b2 = take(C); c->o_w3 = take((int64_t)NO * C * 9); c->o_b3 = take(NO);
    c->host.assign(n, 0.0f);
    pack_weights(c, t);
    *out = c;
    return VQAE_OK;
}

extern "C" int vqae_classifier_update(vqae_classifier* c, const vqae_tensor* tensors, int n_tensors) {
    VQAE_REQUIRE(c, VQAE_ERR_INVALID, "classifier_update: null classifier");
    VQAE_REQUIRE(n_tensors >= 0 && (tensors || n_tensors == 0), VQAE_ERR_INVALID, "classifier_update: null tensors");
    const vqae_tensor* t[7];
    if (int rc = find_weights("classifier_update", c->K, c->E, c->C, c->NO, tensors, n_tensors, t)) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    pack_weights(c, t);
    c->host_newer = true;             // the next call uploads on its own stream, behind the launches that read the old image
    c->dev_newer = false;             // ... also over a device image an optimiser stepped: the host weights win
    return VQAE_OK;
}

vqae_cls::ParamMap vqae_cls::param_map(const vqae_classifier* c) {
    const int K = c->K, E = c->E, C = c->C, NO = c->NO;
    const int numel[7] = {K * E, C * E * 9, C, C * C * 9, C, NO * C * 9, NO};
    const size_t off[7] = {c->o_table, c->o_w1, c->o_b1, c->o_w2, c->o_b2, c->o_w3, c->o_b3};
    const int cout[7] = {0, C, 0, C, 0, NO, 0}, cin9[7] = {0, E * 9, 0, C * 9, 0, C * 9, 0};
    ParamMap m;
    m.start[0] = 0;
    for (int i = 0; i < 7; ++i) {
        m.start[i + 1] = m.start[i] + numel[i];
        m.off[i] = (int)off[i]; m.cout[i] = cout[i]; m.cin9[i] = cin9[i];
    }
    return m;
}

extern "C" int vqae_classifier_download(vqae_classifier* c, float* const tensors[7], void* stream) {
    VQAE_REQUIRE(c && tensors, VQAE_ERR_INVALID, "classifier_download: null pointer");
    for (int i = 0; i < 7; ++i) VQAE_REQUIRE(tensors[i], VQAE_ERR_INVALID, "classifier_download: tensor %d is null", i);
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->dev && c->dev_newer && !c->host_newer) {       // the device image is the truth: fetch it, the host copy follows
        int dev = 0;
        VQAE_HIP_CHECK(hipGetDevice(&dev));
        VQAE_REQUIRE(dev == c->dev_id, VQAE_ERR_INVALID, "classifier_download: the weights live on device %d, current is %d",
                     c->dev_id, dev);
        hipStream_t st = (hipStream_t)stream;
        VQAE_HIP_CHECK(hipMemcpyAsync(c->host.data(), c->dev, c->host.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        VQAE_HIP_CHECK(hipStreamSynchronize(st));
        c->dev_newer = false;
    }
    const ParamMap m = param_map(c);
    const float* h = c->host.data();
    for (int i = 0; i < 7; ++i) {
        const int n = m.start[i + 1] - m.start[i];
        for (int l = 0; l < n; ++l) {                      // pack_conv's permutation, read backwards
            const int co = m.cout[i] ? l / m.cin9[i] : 0, r = m.cout[i] ? l - co * m.cin9[i] : 0;
            tensors[i][l] = h[m.off[i] + (m.cout[i] ? r * m.cout[i] + co : l)];
        }
    }
    return VQAE_OK;
}

extern "C" size_t vqae_classifier_image_floats(const vqae_classifier* c) { return c ? c->host.size() : 0; }

extern "C" int vqae_classifier_image(vqae_classifier* c, float* image_host, void* stream) {
    VQAE_REQUIRE(c && image_host, VQAE_ERR_INVALID, "classifier_image: null pointer");
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->dev && !c->host_newer) {
        int dev = 0;
        VQAE_HIP_CHECK(hipGetDevice(&dev));
        VQAE_REQUIRE(dev == c->dev_id, VQAE_ERR_INVALID, "classifier_image: the weights live on device %d, current is %d", c->dev_id, dev);
        hipStream_t st = (hipStream_t)stream;
        VQAE_HIP_CHECK(hipMemcpyAsync(image_host, c->dev, c->host.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        VQAE_HIP_CHECK(hipStreamSynchronize(st));
    } else {
        std::memcpy(image_host, c->host.data(), c->host.size() * sizeof(float));
    }
    return VQAE_OK;
}

extern "C" void vqae_classifier_destroy(vqae_classifier* c) {
    if (!c) return;
    if (c->dev) (void)hipFree(c->dev);
    delete c;
}

extern "C" size_t vqae_classifier_workspace_bytes(const vqae_classifier* c, int batch, int h, int w) {
    if (!c || batch <= 0 || h < 1 || w < 1) return 0;
    return (size_t)vqae::round_up((int64_t)batch * tile_count(c, h, w, nullptr) * SK * 8, 256);
}

extern "C" int vqae_classifier_forward(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                                       float* logits_dev, uint8_t* heat_u8_dev, const uint8_t* mask_dev, float pos_weight,
                                       double* stats_dev, void* workspace_dev, void* stream) {
    VQAE_REQUIRE(c && codes_dev, VQAE_ERR_INVALID, "classifier_forward: null pointer");
    VQAE_REQUIRE(logits_dev || heat_u8_dev || stats_dev, VQAE_ERR_INVALID, "classifier_forward: no output requested");
    VQAE_REQUIRE(!stats_dev || mask_dev, VQAE_ERR_INVALID, "classifier_forward: stats need a mask");
    VQAE_REQUIRE(!stats_dev || workspace_dev, VQAE_ERR_INVALID, "classifier_forward: stats need the workspace");
    VQAE_REQUIRE(c->NO == 1 || (!heat_u8_dev && !stats_dev), VQAE_ERR_INVALID,
                 "classifier_forward: heat and stats are defined for n_out == 1, this classifier has %d", c->NO);
    VQAE_REQUIRE(idx_dtype_ok(idx_dtype), VQAE_ERR_INVALID, "classifier_forward: bad index dtype %d", idx_dtype);
    VQAE_REQUIRE(batch >= 0 && h >= 1 && w >= 1, VQAE_ERR_INVALID, "classifier_forward: bad shape batch=%d h=%d w=%d", batch, h, w);
    VQAE_REQUIRE(!stats_dev || (std::isfinite(pos_weight) && pos_weight >= 0.f), VQAE_ERR_INVALID,
                 "classifier_forward: pos_weight must be finite and >= 0");
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "classifier_forward: batch %d > 65535", batch);
    VQAE_REQUIRE(tile_count(c, h, w, nullptr) < (1ll << 31), VQAE_ERR_UNSUPPORTED, "classifier_forward: a grid of %d x %d codes", h, w);
    if (batch == 0) return VQAE_OK;
    return forward_launch(c, codes_dev, idx_dtype, batch, h, w, logits_dev, heat_u8_dev, mask_dev, nullptr, pos_weight, nullptr,
                          stats_dev, workspace_dev, (hipStream_t)stream);
}

// ---- Multi-class: nn.CrossEntropyLoss scores from the same launch ---------------------------------------------------------
int vqae_cls::ce_args(const char* who, const vqae_classifier* c, const float* weight, float label_smoothing, CeArgs* out) {
    VQAE_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, VQAE_ERR_INVALID, "%s: label_smoothing %g is outside [0, 1]", who,
                 (double)label_smoothing);
    CeArgs a;
    for (int o = 0; o < c->NO && weight; ++o) {
        VQAE_REQUIRE(std::isfinite(weight[o]) && weight[o] >= 0.f, VQAE_ERR_INVALID, "%s: weight[%d] must be finite and >= 0", who, o);
        a.w[o] = weight[o];
    }
    a.keep = (float)(1.0 - (double)label_smoothing);
    a.smooth = (float)((double)label_smoothing / c->NO);
    *out = a;
    return VQAE_OK;
}

extern "C" size_t vqae_classifier_ce_workspace_bytes(const vqae_classifier* c, int batch, int h, int w) {
    if (!c || c->NO == 1 || batch <= 0 || h < 1 || w < 1) return 0;
    return (size_t)vqae::round_up((int64_t)batch * tile_count(c, h, w, nullptr) * CEK * 8, 256);
}

extern "C" int vqae_classifier_forward_ce(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                                          float* logits_dev, uint8_t* prob_u8_dev, uint8_t* class_u8_dev, const uint8_t* labels_dev,
                                          const float* weight, float label_smoothing, double* stats_dev, void* workspace_dev,
                                          void* stream) {
    VQAE_REQUIRE(c && codes_dev, VQAE_ERR_INVALID, "classifier_forward_ce: null pointer");
    VQAE_REQUIRE(logits_dev || prob_u8_dev || class_u8_dev || stats_dev, VQAE_ERR_INVALID, "classifier_forward_ce: no output requested");
    VQAE_REQUIRE(!stats_dev || labels_dev, VQAE_ERR_INVALID, "classifier_forward_ce: stats need labels");
    VQAE_REQUIRE(!stats_dev || workspace_dev, VQAE_ERR_INVALID, "classifier_forward_ce: stats need the workspace");
    VQAE_REQUIRE(idx_dtype_ok(idx_dtype), VQAE_ERR_INVALID, "classifier_forward_ce: bad index dtype %d", idx_dtype);
    VQAE_REQUIRE(batch >= 0 && h >= 1 && w >= 1, VQAE_ERR_INVALID, "classifier_forward_ce: bad shape batch=%d h=%d w=%d", batch, h, w);
    CeArgs ce;
    if (int rc = ce_args("classifier_forward_ce", c, weight, label_smoothing, &ce)) return rc;
    VQAE_REQUIRE(c->NO > 1, VQAE_ERR_UNSUPPORTED,
                 "classifier_forward_ce: cross-entropy needs n_out >= 2; vqae_classifier_forward scores n_out == 1");
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "classifier_forward_ce: batch %d > 65535", batch);
    VQAE_REQUIRE(tile_count(c, h, w, nullptr) < (1ll << 31), VQAE_ERR_UNSUPPORTED, "classifier_forward_ce: a grid of %d x %d codes", h, w);
    if (batch == 0) return VQAE_OK;
    ce.prob = prob_u8_dev; ce.cls = class_u8_dev;
    return forward_launch(c, codes_dev, idx_dtype, batch, h, w, logits_dev, nullptr, stats_dev ? labels_dev : nullptr, nullptr, 1.0f,
                          nullptr, stats_dev, workspace_dev, (hipStream_t)stream, &ce);
}
