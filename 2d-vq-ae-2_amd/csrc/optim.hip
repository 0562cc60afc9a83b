// One optimiser step over any list of fp32 tensors at any addresses (gfx950): torch.optim.Adam / AdamW, the reference's Lamb
// (vq_ae/optim/lamb.py:78-114) and its SAM wrapper (vq_ae/optim/sam.py:31-60, 96-111), for the ~1 600 parameter tensors of an
// auto-encoder, three quarters of them single numbers.  The per-element arithmetic is optim_math.h's, the one
// classifier_optim.hip runs; what is new here is the walk.
//
// Work.  Fixed by the element counts at create, uploaded once:
//   chunks   a tensor of more than SMALL elements is cut into pieces of CHUNK elements from its start, one workgroup and one
//            row of fp64 partial sums each;
//   small    a tensor of at most SMALL = 64 elements is one element per lane of one wave, four tensors per workgroup; its
//            norms finish inside the wave.
// What changes from step to step travels in a table of one 32-byte Row per tensor (parameter and gradient address, offset of
// its moments in the dense state, element count, index of its scalars, flags) and the distinct sets of scalars (one per
// (group, step count): the step count is per tensor, because a tensor without a gradient does not advance).  The table goes up
// from page-locked memory on the caller's stream into one of SLOTS device slots; an event recorded behind the step's last
// kernel guards both copies of the slot, and the host waits on it only when it is SLOTS tables ahead.
//
// Launches.  Adam / AdamW: optim_first.  LAMB: optim_first (moments stored, partial ||p||^2 and ||u||^2; small tensors are
// finished), optim_tensor_sums (one wave per chunked tensor adds its rows), optim_apply (u recomputed from the stored
// moments).  SAM's climb: optim_first (partial ||a g||^2 of every item, small tensors included), optim_total (one workgroup
// adds all rows), optim_apply (the scale rho / (norm + 1e-12) is formed there).
//
// Sums.  fp64 of fp32 squares.  Thread t of a chunk owns the groups of four elements t, t + 256, ... from the chunk's start and
// adds them in index order -- the same elements whether the group is read as one 16-byte access or, where a pointer is only
// 4-byte aligned or the group is the tensor's tail, one by one -- the 64 lanes fold by shuffles, the four waves are added in
// order, a tensor's rows lane by lane in index order and folded the same way.  No atomics: the order depends on the shapes
// alone and two runs give the same bits.  A tensor whose gradient pointer is null is skipped by every kernel (its items write
// zeros into the climb's rows).
#include "common.h"
#include "optim_math.h"

#include <climits>
#include <new>
#include <vector>

using vqae_om::Hyper;

namespace {

constexpr int NT = 256;                     // threads per workgroup
constexpr int WAVES = NT / 64;
constexpr int CHUNK = VQAE_OPTIM_CHUNK;     // elements per workgroup of a chunked tensor (16 per thread)
constexpr int SMALL = VQAE_OPTIM_SMALL;     // a tensor up to here is one wave's, one element per lane
constexpr int SLOTS = 8;                    // table slots in flight
static_assert(CHUNK % (4 * NT) == 0 && SMALL == 64, "the walk below assumes both");

enum { MODE_ADAM = 0, MODE_LAMB = 1, MODE_CLIMB = 2 };
enum { ROW_RESTORE = 1 };                   // read the parameter from SAM's saved copy (sam.py:53-56)

struct Row { float* p; const float* g; int off, numel, hyper, flags; };
struct Chunk { int tensor, start; };
struct Large { int tensor, row0, n_rows, pad; };
static_assert(sizeof(Row) == 32 && sizeof(Hyper) == 64, "table layout");

struct Args {
    const Row* rows; const Hyper* hyper;    // this step's slot
    const Chunk* chunks; const int* small; const Large* large;
    float *m, *v, *saved;
    double* partial;                        // [n_chunks + n_small][2]
    double* sums;                           // [n_tensors][2]: LAMB's ||p||^2, ||u||^2 of the chunked tensors
    double* total;                          // [1]: the climb's squared norm
    int n_chunks, n_small, n_large, mode;
};

__device__ __forceinline__ void load4(const float* q, bool vec, int c, float (&x)[4]) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < c ? q[k] : 0.0f;
    }
}

__device__ __forceinline__ void store4(float* q, bool vec, int c, const float (&x)[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(q) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < c) q[k] = x[k];
    }
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b) {
    return (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

// two per-thread sums -> thread 0 of the workgroup, in a fixed order
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[2]) {
    const int tid = threadIdx.x;
    a = vqae::wave_sum(a); b = vqae::wave_sum(b);
    if ((tid & 63) == 0) { red[tid >> 6][0] = a; red[tid >> 6][1] = b; }
    __syncthreads();
    if (tid == 0) {
        a = red[0][0]; b = red[0][1];
        for (int w = 1; w < WAVES; ++w) { a += red[w][0]; b += red[w][1]; }
    }
}

// First launch of every mode.  Adam: the whole step.  LAMB: the moments and the partial norms (a small tensor is finished).
// Climb: the partial norm.
__global__ __launch_bounds__(NT) void optim_first(Args a) {
    __shared__ double red[WAVES][2];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b < a.n_chunks) {
        const Chunk it = a.chunks[b];
        const Row r = a.rows[it.tensor];
        if (r.g == nullptr) {                                                   // lamb.py:81-82, sam.py:104
            if (a.mode == MODE_CLIMB && tid == 0) { a.partial[2 * (size_t)b] = 0.0; a.partial[2 * (size_t)b + 1] = 0.0; }
            return;
        }
        const Hyper h = a.hyper[r.hyper];
        const int n = min(CHUNK, r.numel - it.start);
        const size_t so = (size_t)r.off + it.start;
        float* p = r.p + it.start;
        const float* g = r.g + it.start;
        const float* src = (r.flags & ROW_RESTORE) ? a.saved + so : p;
        float *m = a.m + so, *v = a.v + so;
        const bool al = aligned16(r.p, r.g);
        double sp = 0.0, su = 0.0;
        for (int e = tid * 4; e < n; e += NT * 4) {
            const int c = min(4, n - e);
            const bool vec = al && c == 4;
            float g4[4], p4[4], m4[4], v4[4];
            load4(g + e, vec, c, g4);
            load4(src + e, vec, c, p4);
            if (a.mode == MODE_CLIMB) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < c) {
                        const float q = vqae_om::climb_q(h, p4[k], g4[k]);
                        sp += (double)(q * q);
                    }
                continue;
            }
            load4(m + e, vec, c, m4);
            load4(v + e, vec, c, v4);
            if (a.mode == MODE_ADAM) {
#pragma unroll
                for (int k = 0; k < 4; ++k) vqae_om::adam_element(h, g4[k], p4[k], m4[k], v4[k]);
                store4(p + e, vec, c, p4);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < c) {
                        vqae_om::lamb_moments(h, g4[k], m4[k], v4[k]);
                        const float u = vqae_om::lamb_u(h, m4[k], v4[k], p4[k]);
                        sp += (double)(p4[k] * p4[k]);
                        su += (double)(u * u);
                    }
            }
            store4(m + e, vec, c, m4);
            store4(v + e, vec, c, v4);
        }
        if (a.mode == MODE_ADAM) return;
        block_sum2(sp, su, red);
        if (tid == 0) { a.partial[2 * (size_t)b] = sp; a.partial[2 * (size_t)b + 1] = su; }
        return;
    }
    // small tensors: one wave each, one element per lane
    const int idx = (b - a.n_chunks) * WAVES + (tid >> 6), lane = tid & 63;
    if (idx >= a.n_small) return;
    const Row r = a.rows[a.small[idx]];
    const size_t row = (size_t)a.n_chunks + idx;
    if (r.g == nullptr) {
        if (a.mode == MODE_CLIMB && lane == 0) { a.partial[2 * row] = 0.0; a.partial[2 * row + 1] = 0.0; }
        return;
    }
    const Hyper h = a.hyper[r.hyper];
    const bool on = lane < r.numel;
    const size_t so = (size_t)r.off + lane;
    float g = 0.0f, p = 0.0f, m = 0.0f, v = 0.0f;
    if (on) {
        g = r.g[lane];
        p = (r.flags & ROW_RESTORE) ? a.saved[so] : r.p[lane];
    }
    if (a.mode == MODE_CLIMB) {
        const float q = vqae_om::climb_q(h, p, g);
        const double s = vqae::wave_sum(on ? (double)(q * q) : 0.0);
        if (lane == 0) { a.partial[2 * row] = s; a.partial[2 * row + 1] = 0.0; }
        return;
    }
    if (on) { m = a.m[so]; v = a.v[so]; }
    if (a.mode == MODE_ADAM) {
        if (on) {
            vqae_om::adam_element(h, g, p, m, v);
            a.m[so] = m; a.v[so] = v; r.p[lane] = p;
        }
        return;
    }
    float u = 0.0f;
    if (on) {
        vqae_om::lamb_moments(h, g, m, v);
        a.m[so] = m; a.v[so] = v;
        u = vqae_om::lamb_u(h, m, v, p);
    }
    double sp = vqae::wave_sum(on ? (double)(p * p) : 0.0), su = vqae::wave_sum(on ? (double)(u * u) : 0.0);
    sp = __shfl(sp, 0, 64); su = __shfl(su, 0, 64);
    if (on) r.p[lane] = p + vqae_om::lamb_step(h, sp, su) * u;
}

// LAMB's middle launch: one wave per chunked tensor adds its rows, lane by lane in index order
__global__ __launch_bounds__(NT) void optim_tensor_sums(Args a) {
    const int idx = blockIdx.x * WAVES + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= a.n_large) return;
    const Large L = a.large[idx];
    double sp = 0.0, su = 0.0;
    for (int r = lane; r < L.n_rows; r += 64) {
        sp += a.partial[2 * (size_t)(L.row0 + r)];
        su += a.partial[2 * (size_t)(L.row0 + r) + 1];
    }
    sp = vqae::wave_sum(sp); su = vqae::wave_sum(su);
    if (lane == 0) { a.sums[2 * (size_t)L.tensor] = sp; a.sums[2 * (size_t)L.tensor + 1] = su; }
}

// The climb's middle launch: one workgroup adds every item's row (sam.py:96-111: one norm over all tensors)
__global__ __launch_bounds__(NT) void optim_total(Args a) {
    __shared__ double red[WAVES][2];
    double s = 0.0, z = 0.0;
    const int n = a.n_chunks + a.n_small;
    for (int r = threadIdx.x; r < n; r += NT) s += a.partial[2 * (size_t)r];
    block_sum2(s, z, red);
    if (threadIdx.x == 0) a.total[0] = s;
}

// Third launch.  LAMB: the chunks' p += -lr * trust * u.  Climb: every item's old_p = p, p += e(w).
__global__ __launch_bounds__(NT) void optim_apply(Args a) {
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b < a.n_chunks) {
        const Chunk it = a.chunks[b];
        const Row r = a.rows[it.tensor];
        if (r.g == nullptr) return;
        const Hyper h = a.hyper[r.hyper];
        const int n = min(CHUNK, r.numel - it.start);
        const size_t so = (size_t)r.off + it.start;
        float* p = r.p + it.start;
        const float* g = r.g + it.start;
        const float* src = (r.flags & ROW_RESTORE) ? a.saved + so : p;
        const bool al = aligned16(r.p, r.g);
        float step = 0.0f, scale = 0.0f;
        if (a.mode == MODE_LAMB) step = vqae_om::lamb_step(h, a.sums[2 * (size_t)it.tensor], a.sums[2 * (size_t)it.tensor + 1]);
        else scale = vqae_om::climb_scale(h, a.total[0]);
        for (int e = tid * 4; e < n; e += NT * 4) {
            const int c = min(4, n - e);
            const bool vec = al && c == 4;
            float p4[4], x4[4], y4[4];
            load4(src + e, vec, c, p4);
            if (a.mode == MODE_LAMB) {
                load4(a.m + so + e, vec, c, x4);
                load4(a.v + so + e, vec, c, y4);
#pragma unroll
                for (int k = 0; k < 4; ++k) y4[k] = p4[k] + step * vqae_om::lamb_u(h, x4[k], y4[k], p4[k]);
            } else {
                load4(g + e, vec, c, x4);
                store4(a.saved + so + e, vec, c, p4);
#pragma unroll
                for (int k = 0; k < 4; ++k) y4[k] = vqae_om::climb(h, p4[k], x4[k], scale);
            }
            store4(p + e, vec, c, y4);
        }
        return;
    }
    const int idx = (b - a.n_chunks) * WAVES + (tid >> 6), lane = tid & 63;                   // climb only
    if (idx >= a.n_small) return;
    const Row r = a.rows[a.small[idx]];
    if (r.g == nullptr || lane >= r.numel) return;
    const Hyper h = a.hyper[r.hyper];
    const float p = r.p[lane];
    a.saved[(size_t)r.off + lane] = p;
    r.p[lane] = vqae_om::climb(h, p, r.g[lane], vqae_om::climb_scale(h, a.total[0]));
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace

struct vqae_optim {
    int n = 0, dev_id = -1, kind = 0;
    bool sam = false, pending = false;           // pending: a SAM first step is waiting for its step
    std::vector<vqae_classifier_optim_config> groups;
    std::vector<int> group_of, off, numel;
    std::vector<int64_t> steps;
    std::vector<uint8_t> climbed;                // the tensors the pending first step moved
    struct Key { int group; int64_t step; };
    std::vector<Key> keys;                       // the distinct scalar sets of the table being written
    int64_t total = 0, padded = 0;               // elements; floats of one state plane (every tensor starts on a multiple of 4)
    int n_chunks = 0, n_small = 0, n_large = 0;
    char* dev = nullptr;                         // one allocation: the state, the sums, the static tables, the table slots
    char* host = nullptr;                        // page-locked: the table slots
    size_t slot_bytes = 0;
    char* dev_slots = nullptr;
    hipEvent_t ev[SLOTS] = {};
    int n_ev = 0, next = 0;
    Args args{};
};

extern "C" void vqae_optim_destroy(vqae_optim* o) {
    if (!o) return;
    for (int i = 0; i < o->n_ev; ++i) (void)hipEventDestroy(o->ev[i]);
    if (o->host) (void)hipHostFree(o->host);
    if (o->dev) (void)hipFree(o->dev);
    delete o;
}

static int check_groups(const char* who, int n_groups, const vqae_classifier_optim_config* groups) {
    for (int k = 0; k < n_groups; ++k) {
        if (int rc = vqae_om::check_config(who, groups + k)) return rc;
        VQAE_REQUIRE(groups[k].kind == groups[0].kind, VQAE_ERR_INVALID, "%s: group %d is of kind %d, group 0 of kind %d", who, k,
                     groups[k].kind, groups[0].kind);
        VQAE_REQUIRE((groups[k].sam_rho < 0.0) == (groups[0].sam_rho < 0.0), VQAE_ERR_INVALID,
                     "%s: SAM is on in some groups and off in others (group %d)", who, k);
    }
    return VQAE_OK;
}

extern "C" int vqae_optim_create(int n_tensors, const int64_t* numel, const int* group_of, int n_groups,
                                 const vqae_classifier_optim_config* groups, vqae_optim** out) {
    const char* who = "optim_create";
    VQAE_REQUIRE(out, VQAE_ERR_INVALID, "%s: null out", who);
    *out = nullptr;
    VQAE_REQUIRE(numel && group_of && groups, VQAE_ERR_INVALID, "%s: null pointer", who);
    VQAE_REQUIRE(n_tensors >= 1, VQAE_ERR_INVALID, "%s: n_tensors %d < 1", who, n_tensors);
    VQAE_REQUIRE(n_groups >= 1, VQAE_ERR_INVALID, "%s: n_groups %d < 1", who, n_groups);
    int64_t total = 0, padded = 0;
    for (int i = 0; i < n_tensors; ++i) {
        VQAE_REQUIRE(numel[i] >= 1, VQAE_ERR_INVALID, "%s: tensor %d has numel %lld < 1", who, i, (long long)numel[i]);
        VQAE_REQUIRE(group_of[i] >= 0 && group_of[i] < n_groups, VQAE_ERR_INVALID, "%s: tensor %d is in group %d of %d", who, i,
                     group_of[i], n_groups);
        total += numel[i];
        VQAE_REQUIRE(numel[i] <= INT_MAX && total <= INT_MAX, VQAE_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 elements in all", who);
        padded += (numel[i] + 3) / 4 * 4;
    }
    if (int rc = check_groups(who, n_groups, groups)) return rc;
    VQAE_REQUIRE(padded <= INT_MAX, VQAE_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 elements in all", who);

    vqae_optim* o = new (std::nothrow) vqae_optim;
    VQAE_REQUIRE(o, VQAE_ERR_NOMEM, "%s: out of memory", who);
    o->n = n_tensors;
    o->kind = groups[0].kind;
    o->sam = groups[0].sam_rho >= 0.0;
    o->groups.assign(groups, groups + n_groups);
    o->group_of.assign(group_of, group_of + n_tensors);
    o->steps.assign(n_tensors, 0);
    o->climbed.assign(n_tensors, 0);
    o->keys.reserve(n_tensors);
    o->total = total; o->padded = padded;
    std::vector<Chunk> chunks;
    std::vector<int> small;
    std::vector<Large> large;
    int at = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const int ne = (int)numel[i];
        o->numel.push_back(ne);
        o->off.push_back(at);
        at += (ne + 3) / 4 * 4;
        if (ne <= SMALL) {
            small.push_back(i);
        } else {
            large.push_back(Large{i, (int)chunks.size(), (int)vqae::ceil_div(ne, CHUNK), 0});
            for (int s = 0; s < ne; s += CHUNK) chunks.push_back(Chunk{i, s});
        }
    }
    o->n_chunks = (int)chunks.size(); o->n_small = (int)small.size(); o->n_large = (int)large.size();
    const size_t n_items = chunks.size() + small.size();
    o->slot_bytes = up256((size_t)n_tensors * (sizeof(Row) + sizeof(Hyper)));
    const size_t b_plane = up256((size_t)padded * sizeof(float));
    const size_t b_partial = up256(n_items * 2 * sizeof(double)), b_sums = up256((size_t)n_tensors * 2 * sizeof(double));
    const size_t b_total = 256, b_chunks = up256(chunks.size() * sizeof(Chunk) + 1), b_small = up256(small.size() * sizeof(int) + 1);
    const size_t b_large = up256(large.size() * sizeof(Large) + 1);
    const size_t bytes = 3 * b_plane + b_partial + b_sums + b_total + b_chunks + b_small + b_large + SLOTS * o->slot_bytes;

    hipError_t e = hipGetDevice(&o->dev_id);
    if (e == hipSuccess) e = hipMalloc((void**)&o->dev, bytes);
    if (e == hipSuccess) e = hipMemset(o->dev, 0, bytes);
    Args& a = o->args;
    if (e == hipSuccess) {
        char* q = o->dev;
        a.m = (float*)q; q += b_plane;
        a.v = (float*)q; q += b_plane;
        a.saved = (float*)q; q += b_plane;
        a.partial = (double*)q; q += b_partial;
        a.sums = (double*)q; q += b_sums;
        a.total = (double*)q; q += b_total;
        a.chunks = (const Chunk*)q; q += b_chunks;
        a.small = (const int*)q; q += b_small;
        a.large = (const Large*)q; q += b_large;
        o->dev_slots = q;
        a.n_chunks = o->n_chunks; a.n_small = o->n_small; a.n_large = o->n_large;
        if (!chunks.empty()) e = hipMemcpy((void*)a.chunks, chunks.data(), chunks.size() * sizeof(Chunk), hipMemcpyHostToDevice);
        if (e == hipSuccess && !small.empty()) e = hipMemcpy((void*)a.small, small.data(), small.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess && !large.empty()) e = hipMemcpy((void*)a.large, large.data(), large.size() * sizeof(Large), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipHostMalloc((void**)&o->host, SLOTS * o->slot_bytes, hipHostMallocDefault);
    for (; e == hipSuccess && o->n_ev < SLOTS; ++o->n_ev) {
        e = hipEventCreateWithFlags(&o->ev[o->n_ev], hipEventDisableTiming);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess) {
        vqae_optim_destroy(o);
        return vqae::fail(VQAE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    *out = o;
    return VQAE_OK;
}

extern "C" int vqae_optim_set(vqae_optim* o, const vqae_classifier_optim_config* groups) {
    const char* who = "optim_set";
    VQAE_REQUIRE(o && groups, VQAE_ERR_INVALID, "%s: null pointer", who);
    const int ng = (int)o->groups.size();
    if (int rc = check_groups(who, ng, groups)) return rc;
    VQAE_REQUIRE(groups[0].kind == o->kind, VQAE_ERR_INVALID, "%s: the kind is fixed at creation (%d, not %d)", who, o->kind,
                 groups[0].kind);
    VQAE_REQUIRE((groups[0].sam_rho >= 0.0) == o->sam, VQAE_ERR_INVALID, "%s: SAM is switched on or off at creation", who);
    o->groups.assign(groups, groups + ng);
    return VQAE_OK;
}

// What both entry points do: the table of this call into the next slot, up on `st`, the launches, the slot's event.
static int run(const char* who, vqae_optim* o, float* const* params, const float* const* grads, hipStream_t st, bool climb) {
    VQAE_REQUIRE(o && params && grads, VQAE_ERR_INVALID, "%s: null pointer", who);
    for (int i = 0; i < o->n; ++i) VQAE_REQUIRE(params[i], VQAE_ERR_INVALID, "%s: the pointer of parameter %d is null", who, i);
    if (climb) {
        VQAE_REQUIRE(o->sam, VQAE_ERR_INVALID, "%s: the optimiser was created without SAM", who);
        VQAE_REQUIRE(!o->pending, VQAE_ERR_INVALID, "%s: a first step is already waiting for its step", who);
    }
    int dev = -1;
    VQAE_HIP_CHECK(hipGetDevice(&dev));
    VQAE_REQUIRE(dev == o->dev_id, VQAE_ERR_INVALID, "%s: the optimiser state lives on device %d, the current device is %d", who,
                 o->dev_id, dev);
    const int slot = o->next;
    VQAE_HIP_CHECK(hipEventSynchronize(o->ev[slot]));             // blocks only when the host is SLOTS tables ahead
    Row* rows = (Row*)(o->host + (size_t)slot * o->slot_bytes);
    Hyper* hyper = (Hyper*)(rows + o->n);
    o->keys.clear();
    for (int i = 0; i < o->n; ++i) {
        Row r{params[i], grads[i], o->off[i], o->numel[i], 0, 0};
        if (grads[i]) {
            const int gi = o->group_of[i];
            const int64_t t = climb ? 0 : o->steps[i] + 1;
            int k = (int)o->keys.size() - 1;                      // the last set first: neighbours share it
            while (k >= 0 && !(o->keys[k].group == gi && o->keys[k].step == t)) --k;
            if (k < 0) {
                k = (int)o->keys.size();
                o->keys.push_back({gi, t});
                hyper[k] = vqae_om::make_hyper(o->groups[gi], (double)t);
            }
            r.hyper = k;
            if (!climb && o->pending && o->climbed[i]) r.flags |= ROW_RESTORE;
        }
        rows[i] = r;
    }
    char* dslot = o->dev_slots + (size_t)slot * o->slot_bytes;
    const size_t used = (size_t)o->n * sizeof(Row) + o->keys.size() * sizeof(Hyper);
    VQAE_HIP_CHECK(hipMemcpyAsync(dslot, rows, used, hipMemcpyHostToDevice, st));
    Args a = o->args;
    a.rows = (const Row*)dslot;
    a.hyper = (const Hyper*)(dslot + (size_t)o->n * sizeof(Row));
    a.mode = climb ? MODE_CLIMB : o->kind == VQAE_OPTIM_LAMB ? MODE_LAMB : MODE_ADAM;
    const unsigned g_all = (unsigned)(o->n_chunks + vqae::ceil_div(o->n_small, WAVES));
    optim_first<<<g_all, NT, 0, st>>>(a);
    VQAE_LAUNCH_CHECK();
    if (a.mode == MODE_CLIMB) {
        optim_total<<<1, NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
        optim_apply<<<g_all, NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
    } else if (a.mode == MODE_LAMB && o->n_large > 0) {
        optim_tensor_sums<<<(unsigned)vqae::ceil_div(o->n_large, WAVES), NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
        optim_apply<<<(unsigned)o->n_chunks, NT, 0, st>>>(a);
        VQAE_LAUNCH_CHECK();
    }
    VQAE_HIP_CHECK(hipEventRecord(o->ev[slot], st));
    o->next = (slot + 1) % SLOTS;
    for (int i = 0; i < o->n; ++i) {
        if (climb) o->climbed[i] = grads[i] != nullptr;
        else if (grads[i]) o->steps[i] += 1;
    }
    o->pending = climb;
    return VQAE_OK;
}

extern "C" int vqae_optim_step(vqae_optim* o, float* const* params_dev, const float* const* grads_dev, void* stream) {
    return run("optim_step", o, params_dev, grads_dev, (hipStream_t)stream, false);
}

extern "C" int vqae_optim_sam_first(vqae_optim* o, float* const* params_dev, const float* const* grads_dev, void* stream) {
    return run("optim_sam_first", o, params_dev, grads_dev, (hipStream_t)stream, true);
}

extern "C" int vqae_optim_export(vqae_optim* o, float* exp_avg, float* exp_avg_sq, int64_t* steps, void* stream) {
    VQAE_REQUIRE(o && exp_avg && exp_avg_sq && steps, VQAE_ERR_INVALID, "optim_export: null pointer");
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> plane((size_t)o->padded);
    float* const dst[2] = {exp_avg, exp_avg_sq};
    const float* const src[2] = {o->args.m, o->args.v};
    for (int k = 0; k < 2; ++k) {
        VQAE_HIP_CHECK(hipMemcpyAsync(plane.data(), src[k], plane.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        VQAE_HIP_CHECK(hipStreamSynchronize(st));
        size_t at = 0;
        for (int i = 0; i < o->n; ++i) {
            memcpy(dst[k] + at, plane.data() + o->off[i], (size_t)o->numel[i] * sizeof(float));
            at += (size_t)o->numel[i];
        }
    }
    for (int i = 0; i < o->n; ++i) steps[i] = o->steps[i];
    return VQAE_OK;
}

extern "C" int vqae_optim_import(vqae_optim* o, const float* exp_avg, const float* exp_avg_sq, const int64_t* steps, void* stream) {
    VQAE_REQUIRE(o && exp_avg && exp_avg_sq && steps, VQAE_ERR_INVALID, "optim_import: null pointer");
    VQAE_REQUIRE(!o->pending, VQAE_ERR_INVALID, "optim_import: a SAM first step is waiting for its step");
    for (int i = 0; i < o->n; ++i)
        VQAE_REQUIRE(steps[i] >= 0, VQAE_ERR_INVALID, "optim_import: step %lld of tensor %d < 0", (long long)steps[i], i);
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> plane((size_t)o->padded, 0.0f);
    const float* const src[2] = {exp_avg, exp_avg_sq};
    float* const dst[2] = {o->args.m, o->args.v};
    for (int k = 0; k < 2; ++k) {
        size_t at = 0;
        for (int i = 0; i < o->n; ++i) {
            memcpy(plane.data() + o->off[i], src[k] + at, (size_t)o->numel[i] * sizeof(float));
            at += (size_t)o->numel[i];
        }
        VQAE_HIP_CHECK(hipMemcpyAsync(dst[k], plane.data(), plane.size() * sizeof(float), hipMemcpyHostToDevice, st));
        VQAE_HIP_CHECK(hipStreamSynchronize(st));
    }
    for (int i = 0; i < o->n; ++i) o->steps[i] = steps[i];
    return VQAE_OK;
}
