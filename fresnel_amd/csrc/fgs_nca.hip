// Neighbour perception and state update of the reference's NCAGaussianDecoder (scripts/models/nca_gaussian_decoder.py, "NCA":
// _nca_step 232-286, _gather_neighbors 288-322).  One of its 16 steps is cdist (O(N^2) distances written to memory), topk, a
// gather over a (B, N, N, D) expanded view, cat, the two MLPs, rand, compare, cast, mul, mul, add; autograd replays all of it.
// Here the k-nearest-neighbour search, the gather and the concatenation are ONE launch forward and one backward, and the tail of
// the step behind the MLPs (mask, scale, add) one launch forward and two backward.  The MLPs stay rocBLAS through torch.
//
// Canonical neighbours (include/fgs.h): d2(i, j) = (dx dx + dy dy) + dz dz of the differences, every operation rounded to fp32
// (-ffp-contract=off, fresnel_amd/build.py), NaN counting as +inf; the neighbours of i are the k points j != i with the smallest
// (d2, j), in ascending (d2, j) order.
//
// k_nca_perceive<K>.  Block = 64 query points of one image, FOUR lanes per point (256 threads).  The image's positions sit in LDS
// as three arrays (x, y, z); the candidates go round the four lanes in groups of four (one ds_read_b128 per array and group; the
// lanes of a wave that share a group read the same address: broadcasts).  Every lane keeps a top-K list of 2 K registers,
// indexed statically (K is a template parameter: no scratch memory), ordered by (d2, j) -- ONE comparison everywhere, which is the
// definition itself.  Lane 0's list is FILLED FIRST with the first K indices other than i, inserted with their distances: from
// then on it holds K distinct valid indices whatever the input; the other lanes start from (inf, INT_MAX) sentinels, which lose
// every comparison.  A candidate replaces a list's worst entry behind an `is it smaller than the worst` guard (false for NaN --
// a NaN candidate could only displace entries that are not larger than (inf, its index)).  The lists are then merged into
// lane 0's by two shuffle steps (1 -> 0 and 3 -> 2, then 2 -> 0): lanes scan disjoint candidates, so the merged list stays
// distinct.  Why four lanes: one lane per point left one wave per SIMD scanning 377 candidates with the insertion executed for
// nearly every candidate (SOME lane of 64 inserts); the steps and their times are in DESIGN.md section 7.4.  The block then copies its
// 64 x (K + 1) rows: the indices go through LDS, and all lanes walk the block's contiguous piece of `perception` in 16- / 8- /
// 4-byte elements (the widest that divides D), so the stores are coalesced and each neighbour row is read by D / 4 consecutive lanes.
//
// k_nca_perceive_bwd<K>.  Block = 64 DESTINATION points j of one image.  The inverted index is a bit matrix in LDS, one row per
// destination: bit i of row j says "j is a neighbour of i".  The block reads the image's whole neighbour table once and sets the
// bits of its own 64 rows (integer LDS atomics: the result does not depend on their order); then four threads per destination
// walk the row's set bits in ascending i, find the slot s among i's K entries (K independent loads, no search loop), and add
// g_perception[b, i, slot s + 1] to the self term -- ascending (i, s), the order include/fgs.h states.  No float atomics, no
// global scratch, any in-degree 0 ... N - 1.  A neighbour table with out-of-range entries (not one of fgs_nca_perceive_forward's)
// is never dereferenced out of bounds: an entry outside the block's 64 rows sets no bit, and the slot is one of [0, K).
//
// k_nca_update / k_nca_update_bwd / k_nca_step_sum.  new = state + step (delta mask), three roundings as torch's expression;
// g_delta = (g step) mask; g_step = sum g (delta mask): products and partial sums in double (a product of two floats is exact
// there), a fixed number of blocks each striding the tensor in a fixed order, a fixed-shape tree per block, the block partials
// added in block order by one thread.  Results repeat bit for bit.
#include "fgs_internal.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int PB = 64;          // query / destination points per block
constexpr int QL = 4;           // lanes per query point of k_nca_perceive
constexpr int PT = PB * QL;     // its threads
constexpr int BWD_T = 256;      // threads of k_nca_perceive_bwd: four per destination
constexpr int UB = 256;         // threads of the update kernels
constexpr int MAX_K = 16, MAX_N = 4096, MIN_D = 3, MAX_D = 64;
constexpr int MAX_PARTIALS = 1024;

// ---- perception forward ---------------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void bubble(float (&d)[K], int (&ix)[K], int from) {
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
        // the (d2, j) order; `|` and `&`, not `||` and `&&`: selects, no branches
        const bool sw = (s <= from) & ((d[s] < d[s - 1]) | ((d[s] == d[s - 1]) & (ix[s] < ix[s - 1])));
        const float da = d[s - 1], db = d[s];
        const int ia = ix[s - 1], ib = ix[s];
        d[s - 1] = sw ? db : da; d[s] = sw ? da : db;
        ix[s - 1] = sw ? ib : ia; ix[s] = sw ? ia : ib;
    }
}

__device__ __forceinline__ float dist2(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}

template <int V>
__device__ __forceinline__ void copy_rows(float *dst, const float *img, const int *l_idx, int rows, int D, int tid) {
    // dst: the block's `rows` output rows of D floats, contiguous; row r comes from point l_idx[r] of the image
    const int per = D / V, n = rows * per;
    for (int e = tid; e < n; e += PT) {
        const int r = e / per, c = e - r * per;
        const float *src = img + (size_t)l_idx[r] * D;
        if constexpr (V == 4) reinterpret_cast<float4 *>(dst)[e] = reinterpret_cast<const float4 *>(src)[c];
        else if constexpr (V == 2) reinterpret_cast<float2 *>(dst)[e] = reinterpret_cast<const float2 *>(src)[c];
        else dst[e] = src[c];
    }
}

template <int K>
__global__ __launch_bounds__(PT) void k_nca_perceive(int32_t N, int32_t D, const float *__restrict__ state,
                                                     float *__restrict__ perception, int32_t *__restrict__ neighbors) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NP = (N + 3) & ~3;
    float *lx = lds, *ly = lds + NP, *lz = lds + 2 * NP;
    int *l_idx = reinterpret_cast<int *>(lds + 3 * NP);  // [PB][K + 1]: self, then the neighbours
    const int tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * PB;
    const int npts = min(PB, N - p0);
    const float *img = state + (size_t)b * N * D;
    for (int j = tid; j < N; j += PT) {
        lx[j] = img[(size_t)j * D]; ly[j] = img[(size_t)j * D + 1]; lz[j] = img[(size_t)j * D + 2];
    }
    __syncthreads();
    const int ql = tid >> 2, q = tid & 3;
    // (the lanes of a point past the image's end work on the last point and drop the result: the merge's shuffles need every lane)
    const int i = min(p0 + ql, N - 1);
    const float xi = lx[i], yi = ly[i], zi = lz[i];
    float d[K];
    int ix[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { d[t] = INFINITY; ix[t] = INT_MAX; }
    if (q == 0) {  // the first K indices other than i, with their distances: K distinct valid entries from here on (N >= K + 1)
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int j = t < i ? t : t + 1;
            const float v = dist2(xi, yi, zi, lx[j], ly[j], lz[j]);
            d[t] = v == v ? v : INFINITY;
            ix[t] = j;
            bubble<K>(d, ix, t);
        }
    }
    auto offer = [&](float v, int j) {
        if ((v < d[K - 1]) | ((v == d[K - 1]) & (j < ix[K - 1]))) {
            d[K - 1] = v; ix[K - 1] = j;
            bubble<K>(d, ix, K - 1);
        }
    };
    const int j0 = i <= K ? K + 1 : K;  // the first index that is not in lane 0's list yet
    auto candidate = [&](float xj, float yj, float zj, int j) {
        const float v = dist2(xi, yi, zi, xj, yj, zj);
        if ((j >= j0) & (j != i) & ((v < d[K - 1]) | ((v == d[K - 1]) & (j < ix[K - 1])))) {
            d[K - 1] = v; ix[K - 1] = j;
            bubble<K>(d, ix, K - 1);
        }
    };
    for (int jb = (j0 & ~3) + 4 * q; jb < N; jb += 4 * QL) {
        if (jb + 4 <= N) {
            const float4 x4 = *reinterpret_cast<const float4 *>(lx + jb), y4 = *reinterpret_cast<const float4 *>(ly + jb),
                         z4 = *reinterpret_cast<const float4 *>(lz + jb);
            candidate(x4.x, y4.x, z4.x, jb); candidate(x4.y, y4.y, z4.y, jb + 1);
            candidate(x4.z, y4.z, z4.z, jb + 2); candidate(x4.w, y4.w, z4.w, jb + 3);
        } else {
            for (int j = jb; j < N; ++j) candidate(lx[j], ly[j], lz[j], j);
        }
    }
    // merge: lanes 1 -> 0 and 3 -> 2, then 2 -> 0.  All shuffles of a step come before its insertions, and only the receiving
    // lanes insert: a list is read by its neighbour as the scan (or the previous step) left it
#pragma unroll
    for (int step = 1; step <= 2; step <<= 1) {
        float od[K];
        int oi[K];
#pragma unroll
        for (int t = 0; t < K; ++t) { od[t] = __shfl_down(d[t], step); oi[t] = __shfl_down(ix[t], step); }
        if ((q & (2 * step - 1)) == 0) {
#pragma unroll
            for (int t = 0; t < K; ++t) offer(od[t], oi[t]);
        }
    }
    if (q == 0 && ql < npts) {
        l_idx[ql * (K + 1)] = i;
#pragma unroll
        for (int t = 0; t < K; ++t) l_idx[ql * (K + 1) + 1 + t] = ix[t];
    }
    __syncthreads();
    const size_t pt0 = (size_t)b * N + p0;
    for (int e = tid; e < npts * K; e += PT) {
        const int p = e / K, s = e - p * K;
        neighbors[pt0 * K + e] = l_idx[p * (K + 1) + 1 + s];
    }
    float *dst = perception + pt0 * (K + 1) * D;
    const int rows = npts * (K + 1);
    if ((D & 3) == 0) copy_rows<4>(dst, img, l_idx, rows, D, tid);
    else if ((D & 1) == 0) copy_rows<2>(dst, img, l_idx, rows, D, tid);
    else copy_rows<1>(dst, img, l_idx, rows, D, tid);
}

// ---- perception backward --------------------------------------------------------------------------------------------------------
template <int V>
struct Vec;
template <> struct Vec<4> { using T = float4; };
template <> struct Vec<1> { using T = float; };

__device__ __forceinline__ void vadd(float4 &a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__device__ __forceinline__ void vadd(float &a, const float v) { a += v; }

template <int V, int K>
__device__ __forceinline__ void sum_rows(const uint32_t *row, int words, int N, int D, int j, int q,
                                         const int32_t *__restrict__ nb, const float *__restrict__ gp, float *__restrict__ gs) {
    // gs: g_state row of destination j; gp / nb: the image's g_perception / neighbour table; q: 0 ... 3, this thread's share of the row
    using T = typename Vec<V>::T;
    const int per = D / V;
    const size_t prow = (size_t)(K + 1) * D;
    for (int c = q; c < per; c += 4) {
        T acc = reinterpret_cast<const T *>(gp + (size_t)j * prow)[c];  // the self term
        for (int w = 0; w < words; ++w) {
            uint32_t bits = row[w];
            while (bits) {
                const int i = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                int s = 0;  // the slot of j among i's K entries: K independent loads
#pragma unroll
                for (int t = 0; t < K; ++t) s = nb[(size_t)i * K + t] == j ? t : s;
                vadd(acc, reinterpret_cast<const T *>(gp + (size_t)i * prow + (size_t)(s + 1) * D)[c]);
            }
        }
        reinterpret_cast<T *>(gs)[c] = acc;
    }
}

template <int K>
__global__ __launch_bounds__(BWD_T) void k_nca_perceive_bwd(int32_t N, int32_t D, const int32_t *__restrict__ neighbors,
                                                            const float *__restrict__ g_perception, float *__restrict__ g_state) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint32_t *rows = reinterpret_cast<uint32_t *>(lds);
    const int words = (N + 31) >> 5, WP = words | 1;  // odd row stride: the 16 rows a wave reads at once sit on different banks
    const int tid = threadIdx.x, b = blockIdx.y;
    const int j0 = blockIdx.x * PB;
    const int npts = min(PB, N - j0);
    for (int e = tid; e < PB * WP; e += BWD_T) rows[e] = 0u;
    __syncthreads();
    const int32_t *nb = neighbors + (size_t)b * N * K;
    const int edges = N * K;
    for (int e = tid; e < edges; e += BWD_T) {
        const uint32_t r = (uint32_t)(nb[e] - j0);
        if (r < (uint32_t)npts) {
            const int i = e / K;
            atomicOr(&rows[r * WP + (i >> 5)], 1u << (i & 31));
        }
    }
    __syncthreads();
    const int jl = tid >> 2, q = tid & 3;
    if (jl < npts) {
        const int j = j0 + jl;
        const float *gp = g_perception + (size_t)b * N * (K + 1) * D;
        float *gs = g_state + ((size_t)b * N + j) * D;
        if ((D & 3) == 0) sum_rows<4, K>(rows + jl * WP, words, N, D, j, q, nb, gp, gs);
        else sum_rows<1, K>(rows + jl * WP, words, N, D, j, q, nb, gp, gs);
    }
}

// ---- update ---------------------------------------------------------------------------------------------------------------------
// V floats per thread and access: 4 where D is a multiple of 4 (a float4 then lies within one point), else 1
__device__ __forceinline__ float lane(const float4 &v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
__device__ __forceinline__ float lane(const float &v, int) { return v; }
__device__ __forceinline__ void set_lane(float4 &v, int c, float x) { if (c == 0) v.x = x; else if (c == 1) v.y = x; else if (c == 2) v.z = x; else v.w = x; }
__device__ __forceinline__ void set_lane(float &v, int, float x) { v = x; }

// mask of the point that unit u (V floats) belongs to: (uniform < update_prob) as a float; eval mode (no uniforms) has no mask
__device__ __forceinline__ float mask_of(const float *uniform, uint32_t point, float prob) { return uniform[point] < prob ? 1.0f : 0.0f; }

template <int V>
__global__ __launch_bounds__(UB) void k_nca_update(uint32_t units, uint32_t per_point, const float *__restrict__ state,
                                                   const float *__restrict__ delta, const float *__restrict__ step_size,
                                                   const float *__restrict__ uniform, float prob, float *__restrict__ new_state) {
    using T = typename Vec<V>::T;
    const float step = *step_size;
    const uint32_t stride = gridDim.x * UB;
    for (uint32_t u = blockIdx.x * UB + threadIdx.x; u < units; u += stride) {
        const T s = reinterpret_cast<const T *>(state)[u], dl = reinterpret_cast<const T *>(delta)[u];
        const float m = uniform ? mask_of(uniform, u / per_point, prob) : 1.0f;
        T o;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            float dm = lane(dl, c);
            if (uniform) dm = dm * m;  // (the reference multiplies by the mask in training mode only, NCA:276-279)
            const float sd = step * dm;
            set_lane(o, c, lane(s, c) + sd);
        }
        reinterpret_cast<T *>(new_state)[u] = o;
    }
}

template <int V>
__global__ __launch_bounds__(UB) void k_nca_update_bwd(uint32_t units, uint32_t per_point, const float *__restrict__ delta,
                                                       const float *__restrict__ step_size, const float *__restrict__ uniform, float prob,
                                                       const float *__restrict__ g, float *__restrict__ g_delta, double *__restrict__ partial) {
    using T = typename Vec<V>::T;
    __shared__ double l_sum[UB];
    const float step = *step_size;
    const uint32_t stride = gridDim.x * UB;
    double acc = 0.0;
    for (uint32_t u = blockIdx.x * UB + threadIdx.x; u < units; u += stride) {
        const T gv = reinterpret_cast<const T *>(g)[u], dl = reinterpret_cast<const T *>(delta)[u];
        const float m = uniform ? mask_of(uniform, u / per_point, prob) : 1.0f;
        T o;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const float ge = lane(gv, c);
            float gd = ge * step, dm = lane(dl, c);
            if (uniform) { gd = gd * m; dm = dm * m; }
            set_lane(o, c, gd);
            acc += (double)ge * (double)dm;  // exact product; the thread's units and channels in a fixed order
        }
        reinterpret_cast<T *>(g_delta)[u] = o;
    }
    l_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int w = UB / 2; w > 0; w >>= 1) {  // fixed-shape tree: the same association every call
        if ((int)threadIdx.x < w) l_sum[threadIdx.x] += l_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = l_sum[0];
}

// dL/d step_size = the block partials, added in block order
__global__ __launch_bounds__(64) void k_nca_step_sum(int32_t blocks, const double *__restrict__ partial, float *__restrict__ g_step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int t = 0; t < blocks; ++t) s += partial[t];
    *g_step = (float)s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int check_dims(const FgsNcaDims *d, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    if (d->batch < 1 || d->points < 1 || d->state_dim < 1 || d->k < 1 || d->points < d->k + 1) {
        fgs_set_error("%s: invalid dims B=%d N=%d D=%d k=%d (needs N >= k + 1)", who, d->batch, d->points, d->state_dim, d->k);
        return FGS_EINVAL;
    }
    if (d->k > MAX_K || d->points > MAX_N || d->state_dim < MIN_D || d->state_dim > MAX_D || d->batch > 65535 ||
        (uint64_t)d->batch * (uint64_t)d->points * (uint64_t)(d->k + 1) * (uint64_t)d->state_dim >= (1ull << 31)) {
        fgs_set_error("%s: B=%d N=%d D=%d k=%d is beyond the supported shapes (k <= %d, N <= %d, %d <= D <= %d, B <= 65535, "
                      "B N (k + 1) D < 2^31)", who, d->batch, d->points, d->state_dim, d->k, MAX_K, MAX_N, MIN_D, MAX_D);
        return FGS_EUNSUPPORTED;
    }
    return FGS_OK;
}

// the update kernels' shape: V floats per unit, units per point, units in all, blocks (= partial sums of dL/d step_size)
struct UpdateShape { int V; uint32_t per_point, units; int32_t blocks; };
UpdateShape update_shape(const FgsNcaDims *d) {
    UpdateShape u;
    u.V = d->state_dim % 4 == 0 ? 4 : 1;
    u.per_point = (uint32_t)(d->state_dim / u.V);
    u.units = (uint32_t)d->batch * (uint32_t)d->points * u.per_point;
    const uint32_t blocks = (u.units + UB - 1) / UB;
    u.blocks = (int32_t)(blocks < (uint32_t)MAX_PARTIALS ? blocks : (uint32_t)MAX_PARTIALS);
    return u;
}

template <int K>
void launch_perceive(const FgsNcaDims *d, const float *state, float *perception, int32_t *neighbors, hipStream_t st) {
    const int NP = (d->points + 3) & ~3;
    const size_t lds = (size_t)3 * NP * sizeof(float) + (size_t)PB * (K + 1) * sizeof(int);
    hipLaunchKernelGGL(k_nca_perceive<K>, dim3((d->points + PB - 1) / PB, d->batch), dim3(PT), lds, st, d->points, d->state_dim,
                       state, perception, neighbors);
}

template <int K>
void launch_perceive_bwd(const FgsNcaDims *d, const int32_t *neighbors, const float *g_perception, float *g_state, hipStream_t st) {
    const int words = (d->points + 31) >> 5;
    const size_t lds = (size_t)PB * (words | 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_nca_perceive_bwd<K>, dim3((d->points + PB - 1) / PB, d->batch), dim3(BWD_T), lds, st, d->points,
                       d->state_dim, neighbors, g_perception, g_state);
}

// K is a template parameter of both perception kernels: the lists are registers, the slot search is K independent loads
#define FGS_NCA_EVERY_K(CALL)                                                                                             \
    switch (dims->k) {                                                                                                    \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                       \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break;                       \
    case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;                 \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break;               \
    }

}  // namespace

extern "C" {

int fgs_nca_workspace_bytes(const FgsNcaDims *dims, size_t *scratch_bytes) {
    int rc = check_dims(dims, "fgs_nca_workspace_bytes");
    if (rc) return rc;
    if (!scratch_bytes) { fgs_set_error("fgs_nca_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *scratch_bytes = (((size_t)update_shape(dims).blocks * sizeof(double)) + 255) & ~(size_t)255;
    return FGS_OK;
}

int fgs_nca_perceive_forward(const FgsNcaDims *dims, const float *state, float *perception, int32_t *neighbors, void *stream) {
    int rc = check_dims(dims, "fgs_nca_perceive_forward");
    if (rc) return rc;
    if (!state || !perception || !neighbors) { fgs_set_error("fgs_nca_perceive_forward: null pointer argument"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define FGS_NCA_CALL(KK) launch_perceive<KK>(dims, state, perception, neighbors, st)
    FGS_NCA_EVERY_K(FGS_NCA_CALL)
#undef FGS_NCA_CALL
    FGS_LAUNCH_CHECK("k_nca_perceive");
    return FGS_OK;
}

int fgs_nca_perceive_backward(const FgsNcaDims *dims, const int32_t *neighbors, const float *g_perception, float *g_state,
                              void *stream) {
    int rc = check_dims(dims, "fgs_nca_perceive_backward");
    if (rc) return rc;
    if (!neighbors || !g_perception || !g_state) { fgs_set_error("fgs_nca_perceive_backward: null pointer argument"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define FGS_NCA_CALL(KK) launch_perceive_bwd<KK>(dims, neighbors, g_perception, g_state, st)
    FGS_NCA_EVERY_K(FGS_NCA_CALL)
#undef FGS_NCA_CALL
    FGS_LAUNCH_CHECK("k_nca_perceive_bwd");
    return FGS_OK;
}

int fgs_nca_update_forward(const FgsNcaDims *dims, const float *state, const float *delta, const float *step_size,
                           const float *uniform, float update_prob, float *new_state, void *stream) {
    int rc = check_dims(dims, "fgs_nca_update_forward");
    if (rc) return rc;
    if (!state || !delta || !step_size || !new_state) { fgs_set_error("fgs_nca_update_forward: null pointer argument"); return FGS_EINVAL; }
    const UpdateShape u = update_shape(dims);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (u.V == 4) hipLaunchKernelGGL(k_nca_update<4>, dim3(u.blocks), dim3(UB), 0, st, u.units, u.per_point, state, delta, step_size,
                                     uniform, update_prob, new_state);
    else hipLaunchKernelGGL(k_nca_update<1>, dim3(u.blocks), dim3(UB), 0, st, u.units, u.per_point, state, delta, step_size, uniform,
                            update_prob, new_state);
    FGS_LAUNCH_CHECK("k_nca_update");
    return FGS_OK;
}

int fgs_nca_update_backward(const FgsNcaDims *dims, const float *delta, const float *step_size, const float *uniform,
                            float update_prob, const float *g_new_state, float *g_delta, float *g_step_size, void *scratch,
                            void *stream) {
    int rc = check_dims(dims, "fgs_nca_update_backward");
    if (rc) return rc;
    if (!delta || !step_size || !g_new_state || !g_delta || !g_step_size || !scratch) {
        fgs_set_error("fgs_nca_update_backward: null pointer argument");
        return FGS_EINVAL;
    }
    const UpdateShape u = update_shape(dims);
    const int32_t blocks = u.blocks;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *partial = reinterpret_cast<double *>(scratch);
    if (u.V == 4) hipLaunchKernelGGL(k_nca_update_bwd<4>, dim3(blocks), dim3(UB), 0, st, u.units, u.per_point, delta, step_size, uniform,
                                     update_prob, g_new_state, g_delta, partial);
    else hipLaunchKernelGGL(k_nca_update_bwd<1>, dim3(blocks), dim3(UB), 0, st, u.units, u.per_point, delta, step_size, uniform,
                            update_prob, g_new_state, g_delta, partial);
    FGS_LAUNCH_CHECK("k_nca_update_bwd");
    hipLaunchKernelGGL(k_nca_step_sum, dim3(1), dim3(64), 0, st, blocks, partial, g_step_size);
    FGS_LAUNCH_CHECK("k_nca_step_sum");
    return FGS_OK;
}

}  // extern "C"
