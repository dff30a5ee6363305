// Selection of a clip's most energetic bodies as the batch is gathered (ClipBatches(bodies=...); contract in include/fgcn.h, DESIGN.md
// section 8o): the reference's SkeletonSample._filter_bodies -- every tracked body of source row idx[k] scored with body_score, the sum over
// the channels of the standard deviation of its non-null frames, and the M bodies with the highest score kept, in descending order.
// Two launches.  bodies_score_kernel, one workgroup per (clip, body): the lanes walk the body's floats twice in groups of four neighbours --
// pass 1 flags the frames that hold a value (a bit image in LDS) and sums every channel, pass 2 sums the squared deviations from the channel
// means over the flagged frames (the body was just read: 90 KB of the real workload, the second read comes from L2) -- all in float64, the
// lanes' partial sums reduced in a fixed tree (wave shuffle, then LDS across the waves).  Which lane adds which element in which order
// depends on (T, V, C) alone: a body whose address is 16-byte aligned is loaded 16 bytes at a time and any other 4 bytes at a time, but the
// groups and their order are the same, so a clip's score has the same bits wherever the clip lies.  No floating-point atomics.
// bodies_gather_kernel, workgroups (x = (clip, kept body), y = piece of the body): its first Mr lanes rank the clip's Mr scores by counting
// (rank(m) = the number of bodies that beat m), then the workgroup copies its piece of the body at its rank, 16 bytes a lane where source
// and destination allow it and 4 bytes otherwise.  The rank never becomes an address before it is known to lie in [0, Mr): it is a count
// of at most Mr - 1 comparisons.
#include "fgcn_common.hpp"

namespace fgcn {

constexpr int BODIES_THREADS = 256, BODIES_WAVES = BODIES_THREADS / 64;
constexpr int BODIES_MAX_LDS = FGCN_BODIES_MAX_T / 8;      // bytes of the frame bit image, at most
constexpr unsigned GATHER_PIECE = 16384;                    // floats of a body one workgroup copies: y < 2^29 / 2^14

struct BodiesArgs {
    const float* src;
    const long long* idx;
    float* out;
    int* order;
    double* scores;
    int b, Mr, M, T, V;
    unsigned per_body;      // T * V * C
    FastDiv by_inner;       // element of a body -> its frame
};

// The body as groups of four neighbouring floats: lane `tid` owns groups tid, tid + 256, ...; f(e, v, slot) is called for element e with
// value v, per lane in ascending e: the ONE order of both passes, whatever the alignment (WIDE only loads 16 bytes at once).  Three groups
// a turn: 3 * 256 * 4 floats are whole frames' worth of channels, so the channel of the element in group w of a turn, place c of the group,
// is (4 tid + 1024 w + c) mod C in every turn -- `slot` = (1024 w + c) mod C is a compile-time number and the lane's own 4 tid mod C is
// taken out once, behind the loop (bodies_rotate), instead of a select per element.  The up to three floats behind the last whole group
// are the caller's.
template <int C, unsigned W, class F>
__device__ __forceinline__ void bodies_group(unsigned q0, unsigned nvec, f32x4 v, F& f) {
    const unsigned q = q0 + W * BODIES_THREADS;
    if (q >= nvec) return;
    f(4 * q, v[0], std::integral_constant<unsigned, (1024u * W) % C>{});
    f(4 * q + 1, v[1], std::integral_constant<unsigned, (1024u * W + 1) % C>{});
    f(4 * q + 2, v[2], std::integral_constant<unsigned, (1024u * W + 2) % C>{});
    f(4 * q + 3, v[3], std::integral_constant<unsigned, (1024u * W + 3) % C>{});
}
template <int C, bool WIDE, class F>
__device__ __forceinline__ void bodies_walk_groups(const float* body, unsigned nvec, unsigned tid, F&& f) {
    for (unsigned q0 = tid; q0 < nvec; q0 += 3 * BODIES_THREADS) {
        f32x4 v[3];
#pragma unroll
        for (unsigned w = 0; w < 3; ++w) {
            const unsigned q = q0 + w * BODIES_THREADS;
            v[w] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q < nvec) {
                if constexpr (WIDE) v[w] = reinterpret_cast<const f32x4*>(body)[q];
                else v[w] = f32x4{body[4 * q], body[4 * q + 1], body[4 * q + 2], body[4 * q + 3]};
            }
        }
        bodies_group<C, 0>(q0, nvec, v[0], f);
        bodies_group<C, 1>(q0, nvec, v[1], f);
        bodies_group<C, 2>(q0, nvec, v[2], f);
    }
}
template <int C, class F>
__device__ __forceinline__ void bodies_walk(const float* body, unsigned n, unsigned tid, F&& f) {
    if ((reinterpret_cast<uintptr_t>(body) & 15u) == 0) bodies_walk_groups<C, true>(body, n >> 2, tid, f);
    else bodies_walk_groups<C, false>(body, n >> 2, tid, f);
}
// out[i] = in[(i + r) mod C], r < C: between a lane's slots and the channels (slot s of lane tid holds channel (4 tid + s) mod C)
template <int C>
__device__ __forceinline__ void bodies_rotate(const double (&in)[C], unsigned r, double (&out)[C]) {
    if constexpr (C == 3) {
        const double a0 = in[0], a1 = in[1], a2 = in[2];
        out[0] = r == 1u ? a1 : (r == 2u ? a2 : a0);
        out[1] = r == 1u ? a2 : (r == 2u ? a0 : a1);
        out[2] = r == 1u ? a0 : (r == 2u ? a1 : a2);
    } else {                                                // C == 2: 4 tid mod 2 is 0
        out[0] = in[0], out[1] = in[1];
    }
}

// The lanes' partial sums -> their total in every lane: xor butterfly over the wave (both partners of a step add the same two numbers),
// then the waves' sums from LDS in ascending wave order.
template <int C>
__device__ __forceinline__ void bodies_reduce(double (&s)[C], double (*wave_sum)[BODIES_WAVES], unsigned tid) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[c] += __shfl_xor(s[c], d);
        if ((tid & 63) == 0) wave_sum[c][tid >> 6] = s[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double t = wave_sum[c][0];
#pragma unroll
        for (int w = 1; w < BODIES_WAVES; ++w) t += wave_sum[c][w];
        s[c] = t;
    }
    __syncthreads();        // the next reduction writes wave_sum again
}

template <int C>
__global__ __launch_bounds__(BODIES_THREADS) void bodies_score_kernel(BodiesArgs a) {
    extern __shared__ unsigned frame_bits[];                // bit t: frame t of the body holds a value
    __shared__ double wave_sum[C][BODIES_WAVES];
    __shared__ int wave_count[BODIES_WAVES];
    const unsigned tid = threadIdx.x;
    const unsigned k = blockIdx.x / (unsigned)a.Mr, m = blockIdx.x - k * (unsigned)a.Mr;
    const float* body = a.src + (a.idx[k] * a.Mr + m) * (long long)a.per_body;
    const int words = (a.T + 31) >> 5;
    for (int w = tid; w < words; w += BODIES_THREADS) frame_bits[w] = 0u;
    __syncthreads();
    // pass 1: the frame flags and the channel sums.  x != 0 is false for -0 and true for a NaN.  A null frame adds its zeros to the sums,
    // which changes no bit of them.  A flag is set once: the lanes that find it set (a plain read of the word; a stale one only repeats
    // the atomic) leave it alone.  Lane 0 takes the floats behind the last whole group, by their channel e mod C.
    const unsigned r0 = (4u * tid) % (unsigned)C, tail = a.per_body & ~3u;
    auto flag = [&](unsigned e, float v) {
        if (v != 0.0f) {
            const unsigned t = fastdiv(e, a.by_inner), bit = 1u << (t & 31u);
            if (!(*(volatile unsigned*)&frame_bits[t >> 5] & bit)) atomicOr(&frame_bits[t >> 5], bit);
        }
    };
    double acc[C], s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    bodies_walk<C>(body, a.per_body, tid, [&](unsigned e, float v, auto slot) {
        flag(e, v);
        acc[slot] += (double)v;
    });
    bodies_rotate<C>(acc, ((unsigned)C - r0) % (unsigned)C, s);
    if (tid == 0) {
        for (unsigned e = tail; e < a.per_body; ++e) {
            const float v = body[e];
            flag(e, v);
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] += e % (unsigned)C == (unsigned)c ? (double)v : 0.0;
        }
    }
    bodies_reduce<C>(s, wave_sum, tid);                     // (its barrier also publishes the flags)
    int count = 0;
    for (int w = tid; w < words; w += BODIES_THREADS) count += __popc(frame_bits[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d);
    if ((tid & 63) == 0) wave_count[tid >> 6] = count;
    __syncthreads();
    count = 0;
#pragma unroll
    for (int w = 0; w < BODIES_WAVES; ++w) count += wave_count[w];
    double* score = a.scores + blockIdx.x;
    if (count == 0) {                                       // no frame holds a value: +0 (uniform over the workgroup)
        if (tid == 0) *score = 0.0;
        return;
    }
    const double n = (double)((long long)count * a.V);
    double mean[C], slot_mean[C], sq[C];
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = s[c] / n, acc[c] = 0.0;
    bodies_rotate<C>(mean, r0, slot_mean);
    // pass 2: the squared deviations of the flagged frames
    auto flagged = [&](unsigned e) {
        const unsigned t = fastdiv(e, a.by_inner);
        return ((frame_bits[t >> 5] >> (t & 31u)) & 1u) != 0u;
    };
    bodies_walk<C>(body, a.per_body, tid, [&](unsigned e, float v, auto slot) {
        const double d = (double)v - slot_mean[slot];
        acc[slot] += flagged(e) ? d * d : 0.0;
    });
    bodies_rotate<C>(acc, ((unsigned)C - r0) % (unsigned)C, sq);
    if (tid == 0) {
        for (unsigned e = tail; e < a.per_body; ++e) {
            const bool in = flagged(e);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double d = (double)body[e] - mean[c];
                sq[c] += (in && e % (unsigned)C == (unsigned)c) ? d * d : 0.0;
            }
        }
    }
    bodies_reduce<C>(sq, wave_sum, tid);
    if (tid != 0) return;
    double total = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) total += sqrt(sq[c] / n);
    *score = total;
}

// key j beats key m: a NaN above every number, then the larger score, then the HIGHER source index
__device__ __forceinline__ bool bodies_beats(double sj, int j, double sm, int m) {
    const bool nj = sj != sj, nm = sm != sm;
    if (nj || nm) return nj && (!nm || j > m);
    return sj > sm || (sj == sm && j > m);
}

__global__ __launch_bounds__(256) void bodies_gather_kernel(BodiesArgs a) {
    __shared__ int ord[FGCN_BODIES_MAX];
    const unsigned tid = threadIdx.x;
    const unsigned k = blockIdx.x / (unsigned)a.M, j = blockIdx.x - k * (unsigned)a.M;
    if (tid < (unsigned)a.Mr) {
        const double* sc = a.scores + (long long)k * a.Mr;
        const double mine = sc[tid];
        int rank = 0;                                       // < Mr: the keys are totally ordered, so the ranks are a permutation
        for (int i = 0; i < a.Mr; ++i) rank += bodies_beats(sc[i], i, mine, (int)tid);
        ord[rank] = (int)tid;
    }
    __syncthreads();
    if (j == 0 && blockIdx.y == 0 && tid < (unsigned)a.Mr) a.order[(long long)k * a.Mr + tid] = ord[tid];
    const unsigned lo = blockIdx.y * GATHER_PIECE, cnt = min(GATHER_PIECE, a.per_body - lo);
    const float* from = a.src + (a.idx[k] * a.Mr + ord[j]) * (long long)a.per_body + lo;
    float* to = a.out + (long long)blockIdx.x * a.per_body + lo;
    if (((reinterpret_cast<uintptr_t>(from) | reinterpret_cast<uintptr_t>(to)) & 15u) == 0) {
        const unsigned nvec = cnt >> 2;
        const f32x4* from4 = reinterpret_cast<const f32x4*>(from);
        f32x4* to4 = reinterpret_cast<f32x4*>(to);
#pragma unroll 4
        for (unsigned q = tid; q < nvec; q += 256) to4[q] = from4[q];
        if (tid < cnt - 4 * nvec) to[4 * nvec + tid] = from[4 * nvec + tid];
    } else {
#pragma unroll 4
        for (unsigned e = tid; e < cnt; e += 256) to[e] = from[e];
    }
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_clip_bodies(const float* src, const long long* idx, float* out, int* order, double* scores, int b, int Mr, int M, int T, int V,
                                int C, void* stream) {
    FGCN_REQUIRE(src && idx && out && order && scores, FGCN_E_BADARG, "clip_bodies: null pointer");
    FGCN_REQUIRE(b > 0 && Mr > 0 && M > 0 && T > 0 && V > 0, FGCN_E_BADARG, "clip_bodies: bad b/Mr/M/T/V (%d, %d, %d, %d, %d)", b, Mr, M, T, V);
    FGCN_REQUIRE(M <= Mr, FGCN_E_BADARG, "clip_bodies: M=%d bodies kept of Mr=%d", M, Mr);
    FGCN_REQUIRE(Mr <= FGCN_BODIES_MAX, FGCN_E_BADARG, "clip_bodies: Mr=%d bodies, at most %d", Mr, FGCN_BODIES_MAX);
    FGCN_REQUIRE(C == 2 || C == 3, FGCN_E_BADARG, "clip_bodies: C=%d, expected 2 or 3 coordinates", C);
    // a lane's index inside a body is 32-bit and goes through FastDiv (exact below 2^29)
    const long long per_body = (long long)T * V * C;
    FGCN_REQUIRE(per_body < (1ll << 29), FGCN_E_BADARG, "clip_bodies: T * V * C = %d * %d * %d elements in a body are more than a lane indexes", T,
                 V, C);
    FGCN_REQUIRE(T <= FGCN_BODIES_MAX_T, FGCN_E_BADARG, "clip_bodies: T=%d frames, at most %d (their flags stay in LDS)", T, FGCN_BODIES_MAX_T);
    const long long bodies = (long long)b * Mr;
    FGCN_REQUIRE(bodies < (1ll << 31), FGCN_E_BADARG, "clip_bodies: b * Mr = %lld bodies are more than one grid holds", bodies);
    FGCN_REQUIRE(out != src, FGCN_E_BADARG, "clip_bodies: out must not alias src");
    BodiesArgs a;
    a.src = src, a.idx = idx, a.out = out, a.order = order, a.scores = scores;
    a.b = b, a.Mr = Mr, a.M = M, a.T = T, a.V = V;
    a.per_body = (unsigned)per_body, a.by_inner = make_fastdiv((unsigned)(V * C));
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)((T + 31) / 32) * 4;
    const dim3 score_grid((unsigned)bodies), gather_grid((unsigned)((long long)b * M), (unsigned)cdiv(per_body, GATHER_PIECE));
    if (C == 3) launch_lds<bodies_score_kernel<3>>(score_grid, dim3(BODIES_THREADS), BODIES_MAX_LDS, lds, s, a);
    else launch_lds<bodies_score_kernel<2>>(score_grid, dim3(BODIES_THREADS), BODIES_MAX_LDS, lds, s, a);
    hipLaunchKernelGGL(bodies_gather_kernel, gather_grid, dim3(256), 0, s, a);
    return launch_status("clip_bodies");
}
