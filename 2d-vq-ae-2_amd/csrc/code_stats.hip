// Exact joint (label x code) histograms of stored code grids (gfx950): the counts the reference commits as data under
// scripts/create_wsi_histograms/ and reads its loss weights from.  Integers end to end.
//
// One streaming launch (after a memset of the destination when the call does not accumulate):
//   grid (nb, batch): workgroup j of grid b counts the positions [j * chunk, (j + 1) * chunk) of that grid, chunk <= 2^30, so
//   a 32-bit workgroup-private count cannot wrap; what leaves the workgroup is added to the int64 table with 64-bit integer
//   atomics (zero bins are skipped), which makes the result independent of order, partition and batch position.
//   key = label * K + code; a code outside 0 .. K-1 is key T = n_labels * K, a label >= n_labels key T + 1: the two `bad`
//   counters are bins T and T + 1 of the same table, so an invalid position is counted like any other and indexes nothing.
//   Each lane loads 16 bytes of codes (and as many mask bytes as that holds codes); a scalar head up to the first 16-byte
//   boundary of the codes and a scalar tail make any base alignment legal.  A mask that is not aligned like the codes at that
//   boundary is read bytewise.
//   Run combining, per element slot of the lane vectors, wave-wide: lanes whose key equals the wave's `hot` key are only
//   counted (ballot + population count into a wave-uniform register: NO atomic); of the remaining lanes those that share the
//   first one's key add their population count with ONE atomic; only what is left adds 1 per lane.  When the second key beat
//   the hot one it becomes the hot key.  A wave that sees a single key issues one atomic when it is done; a wave that
//   straddles the boundary between two runs issues one per slot.
//   LDS route (n_labels * K + 2 <= 32768 bins, i.e. <= 128 KB): uint32 tables in LDS, one per wave while four fit 64 KB (two,
//   then one, above), summed over the copies at the end.  Global route (larger tables, up to K = 65536 x 8 labels): the same
//   wave combining, the atomics go straight to the int64 table in HBM.
#include "common.h"

namespace {

constexpr int THREADS = 256;                  // 4 waves
constexpr int NW = THREADS / 64;
constexpr int64_t CHUNK_MAX = (int64_t)1 << 30;
constexpr int64_t LDS_MAX_BINS = 32768;       // 128 KB of uint32 (a CU has 160 KB)
constexpr int64_t LDS_COPY_BYTES = 65536;     // per-wave copies only while they fit the default 64 KB

template <int IDX> struct CodeT;
template <> struct CodeT<VQAE_IDX_I64> { using type = int64_t; };
template <> struct CodeT<VQAE_IDX_U8> { using type = uint8_t; };
template <> struct CodeT<VQAE_IDX_U16> { using type = uint16_t; };
template <> struct CodeT<VQAE_IDX_I32> { using type = int32_t; };

struct HistArgs {
    const void* codes;
    const uint8_t* mask;                      // or null (label 0)
    int64_t n;                                // positions per grid
    int64_t chunk;                            // positions per workgroup, <= 2^30
    unsigned long long* hist;                 // [rows][T]
    unsigned long long* bad;                  // [rows][2]
    uint32_t K, L, T;                         // T = L * K
    int pooled;                               // rows == 1
    int copies;                               // LDS tables per workgroup (1, 2 or 4); LDS route only
};

template <typename C>
__device__ __forceinline__ uint32_t make_key(C c, uint32_t label, uint32_t K, uint32_t L, uint32_t T) {
    bool in_range;
    if constexpr (sizeof(C) == 8) in_range = (uint64_t)c < (uint64_t)K;
    else in_range = (uint32_t)c < K;          // a negative int32 wraps above any K <= 65536
    return !in_range ? T : (label >= L ? T + 1 : label * K + (uint32_t)c);
}

// Bins 0 .. T-1 live in hist, bins T and T + 1 in bad.
__device__ __forceinline__ unsigned long long* bin_addr(unsigned long long* hist, unsigned long long* bad, uint32_t key, uint32_t T) {
    return key < T ? hist + key : bad + (key - T);
}

template <bool LDS>
struct Counter {
    uint32_t* tab;                            // LDS: this wave's table
    unsigned long long* hist;                 // global route: this grid's rows
    unsigned long long* bad;
    uint32_t T;
    uint32_t hot, hot_cnt;                    // wave-uniform

    __device__ __forceinline__ void add(uint32_t key, uint32_t v) {
        if constexpr (LDS) atomicAdd(tab + key, v);
        else atomicAdd(bin_addr(hist, bad, key, T), (unsigned long long)v);
    }
    __device__ __forceinline__ void flush_hot() {
        if (hot_cnt != 0 && (threadIdx.x & 63) == 0) add(hot, hot_cnt);
        hot_cnt = 0;
    }
    // Wave-collective: every lane of the wave calls it, `act` says whether the lane holds a position.
    __device__ __forceinline__ void count(uint32_t key, bool act) {
        const bool is_hot = act && key == hot;
        const uint32_t nh = (uint32_t)__popcll(__ballot(is_hot));
        hot_cnt += nh;
        const bool rest = act && !is_hot;
        const uint64_t r = __ballot(rest);
        if (r != 0) {                                               // wave-uniform
            const int first = __ffsll((unsigned long long)r) - 1;
            const uint32_t k2 = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
            const bool is2 = rest && key == k2;
            const uint32_t n2 = (uint32_t)__popcll(__ballot(is2));
            if (rest && !is2) add(key, 1u);
            if (n2 > nh) {                                          // the second key beat the hot one: it becomes hot
                flush_hot();
                hot = k2;
                hot_cnt = n2;
            } else if ((int)(threadIdx.x & 63) == first) {
                add(k2, n2);
            }
        }
    }
};

template <int VEC>
__device__ __forceinline__ void load_mask(const uint8_t* p, bool aligned, uint8_t (&m)[VEC]) {
    if (aligned) {
        __builtin_memcpy(m, __builtin_assume_aligned(p, VEC), VEC);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) m[e] = p[e];
    }
}

template <int IDX, bool LDS>
__global__ __launch_bounds__(THREADS) void hist_kernel(HistArgs a) {
    using C = typename CodeT<IDX>::type;
    constexpr int VEC = 16 / (int)sizeof(C);
    extern __shared__ uint32_t lds_tab[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int64_t lo = (int64_t)blockIdx.x * a.chunk, hi = std::min(lo + a.chunk, a.n);
    const C* codes = (const C*)a.codes + (int64_t)b * a.n;
    const uint8_t* mask = a.mask ? a.mask + (int64_t)b * a.n : nullptr;
    const int row = a.pooled ? 0 : b;
    unsigned long long* hist = a.hist + (int64_t)row * a.T;
    unsigned long long* bad = a.bad + (int64_t)row * 2;
    const uint32_t K = a.K, L = a.L, T = a.T, TT = T + 2;

    Counter<LDS> ctr;
    ctr.T = T;
    ctr.hist = hist;
    ctr.bad = bad;
    ctr.tab = nullptr;
    ctr.hot = T;                              // any valid bin; nothing is added for it while hot_cnt == 0
    ctr.hot_cnt = 0;
    if constexpr (LDS) {
        const uint32_t total = TT * (uint32_t)a.copies;
        for (uint32_t i = tid; i < total; i += THREADS) lds_tab[i] = 0;
        ctr.tab = lds_tab + (uint32_t)(wave & (a.copies - 1)) * TT;
        __syncthreads();
    }

    // head: positions before the first 16-byte boundary of the codes (fewer than 16); tail: fewer than VEC after the last vector
    const uintptr_t addr_lo = (uintptr_t)(codes + lo);
    const int64_t head_n = (int64_t)(((16 - (addr_lo & 15)) & 15) / sizeof(C));
    const int64_t head_end = std::min(hi, lo + head_n);
    const int64_t tail_begin = head_end + (hi - head_end) / VEC * VEC;
    if (wave == 0) {
        {
            const int64_t i = lo + lane;
            const bool act = i < head_end;
            uint32_t key = T;
            if (act) key = make_key<C>(codes[i], mask ? mask[i] : 0u, K, L, T);
            ctr.count(key, act);
        }
        {
            const int64_t i = tail_begin + lane;
            const bool act = i < hi;
            uint32_t key = T;
            if (act) key = make_key<C>(codes[i], mask ? mask[i] : 0u, K, L, T);
            ctr.count(key, act);
        }
    }

    // body: one 16-byte vector of codes per lane and iteration, the next one in flight while this one is counted
    const bool mask_aligned = mask && ((uintptr_t)(mask + head_end) % VEC) == 0;
    union CV { uint4 v; C c[VEC]; };
    CV cur, nxt;
    uint8_t mcur[VEC], mnxt[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { mcur[e] = 0; mnxt[e] = 0; }
    nxt.v = make_uint4(0, 0, 0, 0);
    auto fetch = [&](int64_t base) {
        const int64_t i = base + (int64_t)tid * VEC;
        if (i < tail_begin) {
            nxt.v = *reinterpret_cast<const uint4*>(codes + i);
            if (mask) load_mask<VEC>(mask + i, mask_aligned, mnxt);
        }
    };
    fetch(head_end);
    for (int64_t base = head_end; base < tail_begin; base += (int64_t)THREADS * VEC) {      // workgroup-uniform trip count
        cur = nxt;
#pragma unroll
        for (int e = 0; e < VEC; ++e) mcur[e] = mnxt[e];
        if (base + (int64_t)THREADS * VEC < tail_begin) fetch(base + (int64_t)THREADS * VEC);
        const bool act = base + (int64_t)tid * VEC < tail_begin;
#pragma unroll
        for (int e = 0; e < VEC; ++e) ctr.count(make_key<C>(cur.c[e], mcur[e], K, L, T), act);
    }
    ctr.flush_hot();

    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t k = tid; k < TT; k += THREADS) {
            uint32_t s = 0;
            for (int c = 0; c < a.copies; ++c) s += lds_tab[(uint32_t)c * TT + k];          // <= chunk <= 2^30 in all
            if (s != 0) atomicAdd(bin_addr(hist, bad, k, T), (unsigned long long)s);
        }
    }
}

template <int IDX>
int launch(const HistArgs& a, bool lds, size_t lds_bytes, dim3 grid, hipStream_t st) {
    if (lds) {
        // the limit is set once per (kernel, device): ask for the largest table this route takes
        if (int rc = vqae::set_max_dynamic_lds((const void*)hist_kernel<IDX, true>, (int)(LDS_MAX_BINS * 4))) return rc;
        hist_kernel<IDX, true><<<grid, THREADS, lds_bytes, st>>>(a);
    } else {
        hist_kernel<IDX, false><<<grid, THREADS, 0, st>>>(a);
    }
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace

extern "C" size_t vqae_code_histogram_workspace_bytes(int batch, int64_t n_per_grid, int n_codes, int n_labels) {
    if (batch <= 0 || n_per_grid < 1 || n_codes < 1 || n_labels < 1) return 0;
    return (size_t)vqae::round_up((int64_t)batch * 16, 256);          // the `bad` rows of a call that passes no bad_dev
}

extern "C" int vqae_code_histogram(const void* codes_dev, int idx_dtype, const uint8_t* mask_dev, int batch, int64_t n_per_grid,
                                   int n_codes, int n_labels, int pooled, int accumulate, int64_t* hist_dev, int64_t* bad_dev,
                                   void* workspace_dev, void* stream) {
    using vqae::fail;
    VQAE_REQUIRE(codes_dev && hist_dev && workspace_dev, VQAE_ERR_INVALID, "code_histogram: null codes / hist / workspace");
    VQAE_REQUIRE(mask_dev || n_labels <= 1, VQAE_ERR_INVALID, "code_histogram: n_labels=%d needs a mask", n_labels);
    VQAE_REQUIRE(idx_dtype == VQAE_IDX_I64 || idx_dtype == VQAE_IDX_U8 || idx_dtype == VQAE_IDX_U16 || idx_dtype == VQAE_IDX_I32,
                 VQAE_ERR_INVALID, "code_histogram: bad idx_dtype %d", idx_dtype);
    VQAE_REQUIRE(n_per_grid >= 1, VQAE_ERR_INVALID, "code_histogram: n_per_grid=%lld < 1", (long long)n_per_grid);
    VQAE_REQUIRE(batch >= 0, VQAE_ERR_INVALID, "code_histogram: batch=%d < 0", batch);
    VQAE_REQUIRE(n_codes >= 1 && n_codes <= 65536, VQAE_ERR_UNSUPPORTED, "code_histogram: n_codes=%d outside 1 .. 65536", n_codes);
    VQAE_REQUIRE(n_labels >= 1 && n_labels <= VQAE_HIST_MAX_LABELS, VQAE_ERR_UNSUPPORTED,
                 "code_histogram: n_labels=%d outside 1 .. %d", n_labels, (int)VQAE_HIST_MAX_LABELS);
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "code_histogram: batch %d > 65535", batch);

    const hipStream_t st = (hipStream_t)stream;
    const int64_t T = (int64_t)n_labels * n_codes, rows = pooled ? 1 : batch;
    int64_t* bad = bad_dev ? bad_dev : (int64_t*)workspace_dev;
    if (!accumulate && rows > 0) {
        VQAE_HIP_CHECK(hipMemsetAsync(hist_dev, 0, (size_t)(rows * T * 8), st));
        if (bad_dev) VQAE_HIP_CHECK(hipMemsetAsync(bad_dev, 0, (size_t)(rows * 16), st));
    }
    if (batch == 0) return VQAE_OK;

    const bool lds = T + 2 <= LDS_MAX_BINS;
    int copies = 1;
    if (lds) {
        while (copies < NW && (T + 2) * 4 * (copies * 2) <= LDS_COPY_BYTES) copies *= 2;
    }
    const size_t lds_bytes = lds ? (size_t)((T + 2) * 4 * copies) : 0;
    // Enough workgroups to fill the chip four times over, but none smaller than 64 K positions (or 16 passes over its own
    // LDS tables, whichever is more), and none larger than 2^30 so that 32-bit partials cannot wrap.
    const int64_t chunk_min = std::max<int64_t>(65536, lds ? 16 * (T + 2) * copies : 0);
    const int64_t nb_max = std::max<int64_t>(1, vqae::ceil_div(4 * (int64_t)vqae::cu_count(), batch));
    int64_t nb = std::min(nb_max, std::max<int64_t>(1, n_per_grid / chunk_min));
    int64_t chunk = std::min(CHUNK_MAX, vqae::ceil_div(n_per_grid, nb));
    nb = vqae::ceil_div(n_per_grid, chunk);
    VQAE_REQUIRE(nb <= 0x7fffffff, VQAE_ERR_UNSUPPORTED, "code_histogram: n_per_grid=%lld is too large", (long long)n_per_grid);

    HistArgs a;
    a.codes = codes_dev;
    a.mask = mask_dev;
    a.n = n_per_grid;
    a.chunk = chunk;
    a.hist = (unsigned long long*)hist_dev;
    a.bad = (unsigned long long*)bad;
    a.K = (uint32_t)n_codes;
    a.L = (uint32_t)n_labels;
    a.T = (uint32_t)T;
    a.pooled = pooled ? 1 : 0;
    a.copies = copies;
    const dim3 grid((unsigned)nb, (unsigned)batch);
    switch (idx_dtype) {
        case VQAE_IDX_U8: return launch<VQAE_IDX_U8>(a, lds, lds_bytes, grid, st);
        case VQAE_IDX_U16: return launch<VQAE_IDX_U16>(a, lds, lds_bytes, grid, st);
        case VQAE_IDX_I32: return launch<VQAE_IDX_I32>(a, lds, lds_bytes, grid, st);
        default: return launch<VQAE_IDX_I64>(a, lds, lds_bytes, grid, st);
    }
}
