// How does v_mfma_f32_16x16x32_bf16 add its 32 products into C?  Stand-alone probe for the split (bf16x6) form of the
// F(4x4, 3x3) trunk (conv_wino43.hip).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/probe_bf16_accum.hip -o probe_bf16_accum && ./probe_bf16_accum
// Part 1 (width): C = 1, 32 products of 2^-25 each.  An fp32 chain that rounds after every add keeps 1; a wider internal sum gives
//   1 + 2^-20.  Also C = 1 with products that cancel in pairs, and a sum that lands on a tie.
// Part 2 (GEMM error): D = A B, 16 x 16, K = 128 and 1152, random signed operands over 2^[-4, 4], against fp64, in units of
//   sum_k |a b| per output: fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 fmaf chain, split bf16x6 in three product orders.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__device__ void split8(const float* v, bf16x8 (&h)[3]) {
    for (int j = 0; j < 8; ++j) {
        float r = v[j];
        for (int p = 0; p < 3; ++p) { h[p][j] = (__bf16)r; r -= (float)h[p][j]; }
    }
}

// one wave; A [16][K], B [K][16] row-major fp32; D [16][16]
__global__ void gemm_kernel(const float* A, const float* B, int K, int method, float* D) {
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, lo = {0.f, 0.f, 0.f, 0.f};
    if (method == 0) {
        for (int k = 0; k < K; k += 4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[li * K + k + q], B[(k + q) * 16 + li], acc, 0, 0, 0);
    } else if (method == 4) {
        for (int i = 0; i < 4; ++i) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) s = fmaf(A[(4 * q + i) * K + k], B[k * 16 + li], s);
            acc[i] = s;
        }
    } else {
        for (int k = 0; k < K; k += 32) {
            float av[8], bv[8];
            for (int j = 0; j < 8; ++j) { av[j] = A[li * K + k + 8 * q + j]; bv[j] = B[(k + 8 * q + j) * 16 + li]; }
            bf16x8 a[3], b[3];
            split8(av, a);
            split8(bv, b);
#define M(x, y, c) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[x], b[y], c, 0, 0, 0)
            if (method == 1) { M(0, 0, acc); M(0, 1, acc); M(1, 0, acc); M(0, 2, acc); M(1, 1, acc); M(2, 0, acc); }
            if (method == 2) { M(1, 1, acc); M(1, 0, acc); M(2, 0, acc); M(0, 2, acc); M(0, 1, acc); M(0, 0, acc); }
            if (method == 3) { M(1, 1, lo); M(1, 0, lo); M(2, 0, lo); M(0, 2, lo); M(0, 1, lo); M(0, 0, acc); }
#undef M
        }
        if (method == 3) acc = acc + lo;
    }
    for (int i = 0; i < 4; ++i) D[(4 * q + i) * 16 + li] = acc[i];
}

// one bf16 MFMA: C = c0 everywhere, A row 0 = a, B column 0 = b (others 0); returns D[0][0]
__global__ void width_kernel(const float* a, const float* b, float c0, float* out) {
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    bf16x8 av, bv;
    for (int j = 0; j < 8; ++j) { av[j] = (__bf16)(li == 0 ? a[8 * q + j] : 0.f); bv[j] = (__bf16)(li == 0 ? b[8 * q + j] : 0.f); }
    f32x4 acc = {c0, c0, c0, c0};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
    if (l == 0) out[0] = acc[0];
}

int main() {
    float *da, *db, *dd, *dout;
    CK(hipMalloc(&da, 16 * 1152 * 4)); CK(hipMalloc(&db, 16 * 1152 * 4)); CK(hipMalloc(&dd, 256 * 4)); CK(hipMalloc(&dout, 4));
    // ---- part 1
    struct Case { const char* name; float c0; float a[32]; float b[32]; double exact; };
    std::vector<Case> cs(3);
    cs[0].name = "1 + 32 x 2^-25"; cs[0].c0 = 1.f;
    for (int k = 0; k < 32; ++k) { cs[0].a[k] = ldexpf(1.f, -12); cs[0].b[k] = ldexpf(1.f, -13); }
    cs[0].exact = 1.0 + ldexp(1.0, -20);
    cs[1].name = "1 + (2^-2 - 2^-2) x 16 + 2^-30"; cs[1].c0 = 1.f;
    for (int k = 0; k < 32; ++k) { cs[1].a[k] = (k & 1) ? -0.5f : 0.5f; cs[1].b[k] = 0.5f; }
    cs[1].a[31] = ldexpf(1.f, -15); cs[1].b[31] = ldexpf(1.f, -15); cs[1].a[30] = 0.f;
    cs[1].exact = 1.0 + ldexp(1.0, -30);
    cs[2].name = "2^24 + 1 + 2^-8 (tie broken by the small product)"; cs[2].c0 = ldexpf(1.f, 24);
    for (int k = 0; k < 32; ++k) { cs[2].a[k] = 0.f; cs[2].b[k] = 0.f; }
    cs[2].a[0] = 1.f; cs[2].b[0] = 1.f; cs[2].a[1] = ldexpf(1.f, -4); cs[2].b[1] = ldexpf(1.f, -4);
    cs[2].exact = ldexp(1.0, 24) + 1.0 + ldexp(1.0, -8);
    for (auto& c : cs) {
        CK(hipMemcpy(da, c.a, 128, hipMemcpyHostToDevice)); CK(hipMemcpy(db, c.b, 128, hipMemcpyHostToDevice));
        width_kernel<<<1, 64>>>(da, db, c.c0, dout);
        float r;
        CK(hipMemcpy(&r, dout, 4, hipMemcpyDeviceToHost));
        printf("width  %-52s got %.10e  exact %.10e  fp32(exact) %.10e\n", c.name, r, c.exact, (float)c.exact);
    }
    // ---- part 2
    const char* names[5] = {"fp32 MFMA 16x16x4", "bf16x6 big first", "bf16x6 small first (kernel)", "bf16x6 two accumulators", "fp32 fmaf chain"};
    std::mt19937 rng(1234);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(-4.f, 4.f);
    for (int K : {128, 1152}) {
        double emax[5] = {0}, esq[5] = {0};
        long n = 0;
        const int trials = 64;
        for (int t = 0; t < trials; ++t) {
            std::vector<float> A(16 * K), B(16 * K);
            for (auto& v : A) v = nd(rng) * exp2f(ud(rng));
            for (auto& v : B) v = nd(rng) * exp2f(ud(rng));
            CK(hipMemcpy(da, A.data(), A.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(db, B.data(), B.size() * 4, hipMemcpyHostToDevice));
            for (int m = 0; m < 5; ++m) {
                gemm_kernel<<<1, 64>>>(da, db, K, m, dd);
                CK(hipGetLastError());
                std::vector<float> D(256);
                CK(hipMemcpy(D.data(), dd, 1024, hipMemcpyDeviceToHost));
                for (int i = 0; i < 16; ++i)
                    for (int j = 0; j < 16; ++j) {
                        double ex = 0, ab = 0;
                        for (int k = 0; k < K; ++k) { const double p = (double)A[i * K + k] * B[k * 16 + j]; ex += p; ab += fabs(p); }
                        const double e = fabs(D[i * 16 + j] - ex) / ab;
                        emax[m] = fmax(emax[m], e); esq[m] += e * e;
                        if (m == 0) ++n;
                    }
            }
        }
        for (int m = 0; m < 5; ++m)
            printf("K=%-5d %-30s |err| / sum|ab|: max %.3e  rms %.3e\n", K, names[m], emax[m], sqrt(esq[m] / n));
    }
    CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dd)); CK(hipFree(dout));
    return 0;
}
