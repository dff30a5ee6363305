// Score fusion of separately trained stream models (include/fgcn.h, fgcn_score_fuse / fgcn_fuse_sweep): the
// weighted sum of S models' class scores, raw or as float64-formed softmax probabilities, and the top-1 / top-k hit counts of that sum
// under G candidate weight vectors at once.  Both kernels take the transformed scores from fuse_row_stat + fuse_transform and the fused
// value from fuse_value, so the sweep counts exactly what fgcn_classify_update counts on fgcn_score_fuse's output.
//   score_fuse:  one wave per row, lane-strided classes; the softmax statistics of a stream's row are wave reductions.  No LDS.
//   fuse_sweep:  one workgroup per row.  Its waves form the row's S x classes transformed values once in LDS (one stream per wave at a
//                time, float32, class-major: the S values of a class are neighbours), then every LANE ranks the row under one candidate
//                of its own: S weights in registers, the label's fused value first, then one walk over the classes in which all lanes
//                read the same LDS words (broadcasts, no bank conflict) -- no cross-lane reduction anywhere.  The two counters of a
//                candidate live in LDS and belong to one lane for the whole launch; they are added to `counts` with integer atomics at
//                the end.  One launch holds FGCN_FUSE_PASS candidates; the host loops over passes.
// The only index formed from a label is clamped into [0, classes) first.
#include "fgcn_common.hpp"

namespace fgcn {

constexpr int FUSE_WAVES = 4;           // score_fuse: rows in flight per workgroup; fuse_sweep: waves that share one row
constexpr int FUSE_THREADS = 64 * FUSE_WAVES;
constexpr int FUSE_MAX_BLOCKS = 2048;

// torch's order of floats, as in fgcn_metrics.hip: NaN above every number and equal to NaN
__device__ __forceinline__ bool fuse_gt(float a, float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool fuse_eq(float a, float b) { return a == b || (a != a && b != b); }

struct FuseStat {
    float m;        // the row's maximum, NaN skipped
    double sum;     // the float64 sum of exp(z - m) over the row
};

// The softmax statistics of one stream's row, by ONE wave (all 64 lanes call it; every lane returns the same bits: a butterfly adds
// a + b in one lane and b + a in its partner).  The order of the additions depends on `classes` alone.
__device__ __forceinline__ FuseStat fuse_row_stat(const float* z, int classes, int transform, int lane) {
    FuseStat st = {0.f, 1.0};
    if (transform != FGCN_FUSE_SOFTMAX) return st;
    float m = -INFINITY;
    for (int c = lane; c < classes; c += 64) m = fmaxf(m, z[c]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    double sum = 0.0;
    for (int c = lane; c < classes; c += 64) sum += exp((double)z[c] - (double)m);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    st.m = m, st.sum = sum;
    return st;
}

__device__ __forceinline__ float fuse_transform(float z, int transform, FuseStat st) {
    if (transform != FGCN_FUSE_SOFTMAX) return z;
    return (float)(exp((double)z - (double)st.m) / st.sum);
}

// THE fused value: float32 of the float64 sum, in stream order from +0.0, of the exact products w_s * t_s
template <int S>
__device__ __forceinline__ float fuse_value(const float* t, const double (&w)[S]) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) acc += w[s] * (double)t[s];
    return (float)acc;
}

template <int S>
__global__ __launch_bounds__(FUSE_THREADS) void score_fuse_kernel(FgcnFuseIn in, int transform, float* out, int ld_out, int rows,
                                                                   int classes) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * FUSE_WAVES + (threadIdx.x >> 6), nwaves = gridDim.x * FUSE_WAVES;
    double w[S];
#pragma unroll
    for (int s = 0; s < S; ++s) w[s] = (double)in.weight[s];
    for (int r = wave; r < rows; r += nwaves) {
        const float* z[S];
        FuseStat st[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            z[s] = in.scores[s] + (long long)r * in.ld[s];
            st[s] = fuse_row_stat(z[s], classes, transform, lane);
        }
        float* o = out + (long long)r * ld_out;
        for (int c = lane; c < classes; c += 64) {
            float t[S];
#pragma unroll
            for (int s = 0; s < S; ++s) t[s] = fuse_transform(z[s][c], transform, st[s]);
            o[c] = fuse_value<S>(t, w);
        }
    }
}

// Dynamic LDS: float t[classes * S] (class-major), then unsigned cnt[2 * gn]: {top-1, top-k} of local candidate j, owned by thread
// j % FUSE_THREADS from the zeroing to the atomics -- no other thread touches them, so they need no barrier.
template <int S>
__global__ __launch_bounds__(FUSE_THREADS) void fuse_sweep_kernel(FgcnFuseIn in, int transform, const float* candidates, int g0, int gn,
                                                                   const long long* labels, int rows, int classes, int k,
                                                                   unsigned long long* counts, int header) {
    extern __shared__ float fuse_lds[];
    float* t = fuse_lds;
    unsigned* cnt = reinterpret_cast<unsigned*>(fuse_lds + classes * S);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < gn; j += FUSE_THREADS) cnt[2 * j] = 0u, cnt[2 * j + 1] = 0u;
    unsigned examples = 0, ignored = 0, invalid = 0;         // workgroup-uniform
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const long long y = labels[r];
        const bool valid = y >= 0 && y < classes;
        if (!valid) {                                        // such a row counts for no candidate: it is not even read
            if (y == -100) ++ignored;
            else ++invalid;
            continue;
        }
        ++examples;
        const int yi = (int)y;                               // in [0, classes): the only index derived from a label
        __syncthreads();                                     // the walks over the row before this one are done
        for (int s = wave; s < S; s += FUSE_WAVES) {
            const float* z = in.scores[s] + (long long)r * in.ld[s];
            const FuseStat st = fuse_row_stat(z, classes, transform, lane);
            for (int c = lane; c < classes; c += 64) t[c * S + s] = fuse_transform(z[c], transform, st);
        }
        __syncthreads();
        for (int j = tid; j < gn; j += FUSE_THREADS) {
            const float* cw = candidates + (long long)(g0 + j) * S;
            double w[S];
#pragma unroll
            for (int s = 0; s < S; ++s) w[s] = (double)cw[s];
            const float fy = fuse_value<S>(t + yi * S, w);
            int above = 0;
            for (int c = 0; c < classes; ++c) {
                const float v = fuse_value<S>(t + c * S, w);
                above += (fuse_gt(v, fy) || (c < yi && fuse_eq(v, fy))) ? 1 : 0;
            }
            cnt[2 * j] += above == 0 ? 1u : 0u;
            cnt[2 * j + 1] += above < k ? 1u : 0u;
        }
    }
    for (int j = tid; j < gn; j += FUSE_THREADS) {
        unsigned long long* dst = counts + FGCN_FUSE_HEADER + 2ll * (g0 + j);
        if (cnt[2 * j]) atomicAdd(dst, (unsigned long long)cnt[2 * j]);
        if (cnt[2 * j + 1]) atomicAdd(dst + 1, (unsigned long long)cnt[2 * j + 1]);
    }
    if (header && tid == 0) {
        if (examples) atomicAdd(&counts[FGCN_FUSE_EXAMPLES], (unsigned long long)examples);
        if (ignored) atomicAdd(&counts[FGCN_FUSE_IGNORED], (unsigned long long)ignored);
        if (invalid) atomicAdd(&counts[FGCN_FUSE_INVALID], (unsigned long long)invalid);
    }
}

// what both entry points refuse: the streams, the transform and the shape
static int fuse_check(const char* what, const FgcnFuseIn* in, int S, int transform, int rows, int classes) {
    FGCN_REQUIRE(in, FGCN_E_BADARG, "%s: null pointer (in)", what);
    FGCN_REQUIRE(S >= 1 && S <= FGCN_FUSE_MAX_STREAMS, FGCN_E_BADARG, "%s: bad stream count S=%d (1..%d)", what, S, FGCN_FUSE_MAX_STREAMS);
    FGCN_REQUIRE(transform == FGCN_FUSE_NONE || transform == FGCN_FUSE_SOFTMAX, FGCN_E_BADARG, "%s: unknown transform %d", what, transform);
    FGCN_REQUIRE(rows > 0, FGCN_E_BADARG, "%s: bad row count rows=%d", what, rows);
    FGCN_REQUIRE(classes >= 1 && classes <= FGCN_CLS_MAX_CLASSES, FGCN_E_BADARG, "%s: bad class count classes=%d (1..%d)", what, classes,
                 FGCN_CLS_MAX_CLASSES);
    for (int s = 0; s < S; ++s) {
        FGCN_REQUIRE(in->scores[s], FGCN_E_BADARG, "%s: null pointer (scores[%d])", what, s);
        FGCN_REQUIRE(in->ld[s] >= classes, FGCN_E_BADARG, "%s: bad row stride ld[%d]=%d < classes=%d", what, s, in->ld[s], classes);
    }
    return FGCN_OK;
}

}  // namespace fgcn

using namespace fgcn;

#define FUSE_DISPATCH(S, CALL)  \
    switch (S) {                \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        default: CALL(8); break; \
    }

extern "C" int fgcn_score_fuse(const FgcnFuseIn* in, int S, int transform, float* out, int ld_out, int rows, int classes, void* stream) {
    if (int rc = fuse_check("score_fuse", in, S, transform, rows, classes)) return rc;
    FGCN_REQUIRE(out, FGCN_E_BADARG, "score_fuse: null pointer (out)");
    FGCN_REQUIRE(ld_out >= classes, FGCN_E_BADARG, "score_fuse: bad row stride ld_out=%d < classes=%d", ld_out, classes);
    for (int s = 0; s < S; ++s) FGCN_REQUIRE(out != in->scores[s], FGCN_E_BADARG, "score_fuse: out must not alias an input (scores[%d])", s);
    const long long blocks = cdiv(rows, FUSE_WAVES);
    const dim3 grid((unsigned)(blocks < FUSE_MAX_BLOCKS ? blocks : FUSE_MAX_BLOCKS));
#define FUSE_CALL(N) \
    hipLaunchKernelGGL(score_fuse_kernel<N>, grid, dim3(FUSE_THREADS), 0, (hipStream_t)stream, *in, transform, out, ld_out, rows, classes)
    FUSE_DISPATCH(S, FUSE_CALL)
#undef FUSE_CALL
    return launch_status("score_fuse");
}

extern "C" int fgcn_fuse_sweep(const FgcnFuseIn* in, int S, int transform, const float* candidates, int G, const long long* labels, int rows,
                               int classes, int k, unsigned long long* counts, void* stream) {
    if (int rc = fuse_check("fuse_sweep", in, S, transform, rows, classes)) return rc;
    FGCN_REQUIRE(candidates && labels && counts, FGCN_E_BADARG, "fuse_sweep: null pointer (candidates, labels or counts)");
    FGCN_REQUIRE(k >= 1 && k <= classes, FGCN_E_BADARG, "fuse_sweep: bad k=%d (1..classes=%d)", k, classes);
    FGCN_REQUIRE(G >= 1 && G <= FGCN_FUSE_MAX_CANDIDATES, FGCN_E_BADARG, "fuse_sweep: bad candidate count G=%d (1..%d)", G,
                 FGCN_FUSE_MAX_CANDIDATES);
    FGCN_REQUIRE(((uintptr_t)counts & 7) == 0, FGCN_E_ALIGN, "fuse_sweep: counts must be 8-byte aligned");
    const dim3 grid((unsigned)(rows < FUSE_MAX_BLOCKS ? rows : FUSE_MAX_BLOCKS));
    for (int g0 = 0; g0 < G; g0 += FGCN_FUSE_PASS) {
        const int gn = G - g0 < FGCN_FUSE_PASS ? G - g0 : FGCN_FUSE_PASS;
        const size_t lds = sizeof(float) * ((size_t)classes * S + 2 * (size_t)gn);        // <= 32 KiB + 16 KiB
#define FUSE_CALL(N)                                                                                                                   \
    hipLaunchKernelGGL(fuse_sweep_kernel<N>, grid, dim3(FUSE_THREADS), lds, (hipStream_t)stream, *in, transform, candidates, g0, gn, labels, \
                       rows, classes, k, counts, g0 == 0 ? 1 : 0)
        FUSE_DISPATCH(S, FUSE_CALL)
#undef FUSE_CALL
        if (int rc = launch_status("fuse_sweep")) return rc;
    }
    return FGCN_OK;
}
