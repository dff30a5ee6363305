// Normalisation of raw skeleton clips as the batch is gathered (ClipBatches(normalize=...); contract in include/fgcn.h, DESIGN.md
// section 8g): the reference's normalize_skeleton -- frames without a skeleton padded with the frames that have one, the centre joint of
// the first body moved to the origin, the spine turned to the z axis and the shoulders to the x axis -- on row idx[k] of the source.
// Two launches.  normalize_plan_kernel, one workgroup per clip: per body, the lanes stride over the body's floats and flag the frames that
// hold a value, one scan over the flags gives the body's frame map, and one lane forms the clip's rotation in float64 from the four
// joints of body 0's first output frame.  normalize_apply_kernel, one lane per (clip, body, frame, joint): gathers the joint through the map, subtracts
// the centre, masks a missing joint and multiplies by R, all in float64, rounded once at the store.  Its loads and stores are 4 bytes
// wide: a row of 75 floats has no wider alignment (the plan kernel, which only looks for values, reads a body in 16-byte pieces).  The frame map travels through memory between the launches: the apply kernel clamps what it reads
// back into [0, T), so that no stored value becomes an address.
#include <cmath>

#include "fgcn_common.hpp"

namespace fgcn {

constexpr int NORMALIZE_MAX_T = FGCN_NORMALIZE_MAX_T;      // frames per clip, at most: the plan kernel holds one body's flags and base list in LDS
constexpr int PLAN_THREADS = 1024, PLAN_WAVES = PLAN_THREADS / 64;

struct NormalizeArgs {
    const float* src;
    const long long* idx;
    float* out;
    int* frame_map;
    double* params;
    int b, M, T, V, origin, z0, z1, x0, x1;
    FastDiv by_inner, by_V; // float of a body -> its frame; joint of a body -> its frame
};

// One pass of the reference's parallelize_joints_to_axis on the bone p1 - p0: the Rodrigues matrix that turns it to unit axis `ax` (2 = z,
// 0 = x) into r (row-major), or false where the pass is skipped (a bone, a rotation axis or an angle below 1e-6; an antiparallel bone has
// a zero rotation axis and is skipped with them).  The argument of acos is clamped: |bone_ax| / |bone| can exceed 1 by a rounding.
__device__ inline bool normalize_rotation(const double (&p0)[3], const double (&p1)[3], int ax, double (&r)[9]) {
    constexpr double eps = 1e-6;
    const double bx = p1[0] - p0[0], by = p1[1] - p0[1], bz = p1[2] - p0[2];
    if (fabs(bx) + fabs(by) + fabs(bz) < eps) return false;
    // bone x axis: (by, -bx, 0) for z, (0, bz, -by) for x
    double kx = ax == 2 ? by : 0.0, ky = ax == 2 ? -bx : bz, kz = ax == 2 ? 0.0 : -by;
    const double bn = sqrt(bx * bx + by * by + bz * bz), c = fmin(fmax((ax == 2 ? bz : bx) / bn, -1.0), 1.0);
    const double theta = acos(c);
    if (fabs(kx) + fabs(ky) + fabs(kz) < eps || fabs(theta) < eps) return false;
    const double kn = sqrt(kx * kx + ky * ky + kz * kz);
    kx /= kn, ky /= kn, kz /= kn;
    const double s = kn / bn, co = c, v = 1.0 - co;        // sin(theta) = |bone x axis| / |bone| (theta is in [0, pi]), cos(theta) = c
    // I + s K + (1 - cos) K^2 with K^2 = k k^T - I for a unit k
    r[0] = co + v * kx * kx, r[1] = v * kx * ky - s * kz, r[2] = v * kx * kz + s * ky;
    r[3] = v * ky * kx + s * kz, r[4] = co + v * ky * ky, r[5] = v * ky * kz - s * kx;
    r[6] = v * kz * kx - s * ky, r[7] = v * kz * ky + s * kx, r[8] = co + v * kz * kz;
    return true;
}

__device__ inline void normalize_matvec(const double (&r)[9], const double (&p)[3], double (&q)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = fma(r[3 * c + 2], p[2], fma(r[3 * c + 1], p[1], r[3 * c] * p[0]));
}

template <int C>
__global__ __launch_bounds__(PLAN_THREADS) void normalize_plan_kernel(NormalizeArgs a) {
    __shared__ unsigned char nonnull[NORMALIZE_MAX_T];      // of the current body: frame t holds a skeleton
    __shared__ int base[NORMALIZE_MAX_T];                   // of the current body: the frames the padding repeats, in order
    __shared__ int wave_count[PLAN_WAVES], wave_last[PLAN_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, inner = a.V * C;
    const long long s = a.idx[k];
    int valid_bodies = 0, first_frame = 0;                  // (thread 0's copy is the one that is used: map[0] of body 0)
    for (int m = 0; m < a.M; ++m) {
        const float* body = a.src + (s * a.M + m) * (long long)T * inner;
        for (int t = tid; t < T; t += PLAN_THREADS) nonnull[t] = 0;
        __syncthreads();
        // the body as one run of n = T * inner floats: up to three floats in front of the first 16-byte boundary and behind the last one go
        // a lane each, the rest as 16-byte loads, a lane per load -- independent iterations, so a lane's loads are all in flight together.
        // Every value that is not zero sets its frame's flag (-0 == 0; a NaN counts as a value; the lanes of a frame all store the same 1).
        const int n = T * inner;
        const int head = min(n, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(body) & 15u)) & 15u) >> 2);
        const int nvec = (n - head) >> 2, rest = head + 4 * nvec;
        auto flag = [&](int e, float v) {
            if (v != 0.0f) nonnull[fastdiv((unsigned)e, a.by_inner)] = 1;
        };
        if (tid < head) flag(tid, body[tid]);
        if (tid < n - rest) flag(rest + tid, body[rest + tid]);
        const f32x4* wide = reinterpret_cast<const f32x4*>(body + head);
#pragma unroll 8
        for (int q = tid; q < nvec; q += PLAN_THREADS) {
            const f32x4 v = wide[q];
#pragma unroll
            for (int c = 0; c < 4; ++c) flag(head + 4 * q + c, v[c]);
        }
        __syncthreads();
        // thread i owns frames [i L, (i + 1) L): their count of non-null frames and the last of them, then a scan over the threads
        const int L = (T + PLAN_THREADS - 1) / PLAN_THREADS, lo = min(tid * L, T), hi = min(lo + L, T);
        int count = 0, last = -1;
        for (int t = lo; t < hi; ++t)
            if (nonnull[t]) ++count, last = t;
        int incl = count;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
            last = max(last, __shfl_xor(last, d));
        }
        if (lane == 63) wave_count[wave] = incl;
        if (lane == 0) wave_last[wave] = last;
        __syncthreads();
        int before = incl - count, total = 0;
        last = -1;
#pragma unroll
        for (int w = 0; w < PLAN_WAVES; ++w) {
            if (w < wave) before += wave_count[w];
            total += wave_count[w];
            last = max(last, wave_last[w]);
        }
        const bool compact = !nonnull[0];                   // frame 0 is null: the null frames are removed; else they stay where they are
        const int f = compact ? total : last + 1;
        for (int t = lo; t < hi; ++t) {
            if (compact) {
                if (nonnull[t]) base[before++] = t;
            } else {
                base[t] = t;
            }
        }
        __syncthreads();
        int* map = a.frame_map + ((long long)k * a.M + m) * T;
        for (int t = tid; t < T; t += PLAN_THREADS) {
            const int from = f == 0 ? t : (t < f ? base[t] : base[(t - f) % f]);      // f == 0: an invalid body, the identity map
            map[t] = from;
            if (m == 0 && t == 0) first_frame = from;
        }
        valid_bodies += f > 0;
        __syncthreads();                                    // the next body reuses the flags and the base list
    }
    if (tid != 0) return;
    // the rotation, from body 0's first output frame after centring; missing joints are zero (an invalid body 0: every bone is zero)
    double r[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double z_applied = 0.0, x_applied = 0.0;
    if constexpr (C == 3) {
        const float* frame = a.src + (s * a.M * (long long)T + min(max(first_frame, 0), T - 1)) * inner;
        const float* ctr = frame + a.origin * 3;
        auto joint = [&](int j, double (&p)[3]) {
            const float* x = frame + j * 3;
            const bool present = x[0] != 0.0f || x[1] != 0.0f || x[2] != 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = present ? (double)x[c] - (double)ctr[c] : 0.0;
        };
        double p0[3], p1[3];
        if (a.z0 >= 0) {
            joint(a.z0, p0), joint(a.z1, p1);
            double rz[9];
            if (normalize_rotation(p0, p1, 2, rz)) {
#pragma unroll
                for (int e = 0; e < 9; ++e) r[e] = rz[e];
                z_applied = 1.0;
            }
        }
        if (a.x0 >= 0) {
            double q0[3], q1[3], rx[9];
            joint(a.x0, p0), joint(a.x1, p1);
            normalize_matvec(r, p0, q0), normalize_matvec(r, p1, q1);      // the bone of the clip as it stands: after the z pass
            if (normalize_rotation(q0, q1, 0, rx)) {
                double rr[9];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) rr[3 * i + j] = fma(rx[3 * i + 2], r[6 + j], fma(rx[3 * i + 1], r[3 + j], rx[3 * i] * r[j]));
#pragma unroll
                for (int e = 0; e < 9; ++e) r[e] = rr[e];
                x_applied = 1.0;
            }
        }
    }
    double* P = a.params + (long long)k * 12;
#pragma unroll
    for (int e = 0; e < 9; ++e) P[e] = r[e];
    P[9] = z_applied, P[10] = x_applied, P[11] = (double)valid_bodies;
}

// Workgroups (x, y): x = row * M + m is the body, y the piece of 256 of its T * V joints; a lane owns joint j of output frame t.  (The
// body in the grid keeps every per-lane index inside 32 bits: one multiply-shift division per lane instead of three 64-bit ones.)
template <int C>
__global__ __launch_bounds__(256) void normalize_apply_kernel(NormalizeArgs a) {
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= a.T * a.V) return;
    const int t = (int)fastdiv((unsigned)e, a.by_V), j = e - t * a.V;
    const int row = (int)(blockIdx.x / (unsigned)a.M), m = (int)(blockIdx.x % (unsigned)a.M);
    const long long frame = (long long)blockIdx.x * a.T + t;      // (row * M + m) * T + t
    const long long s = a.idx[row];
    const int inner = a.V * C;
    // (a stored frame number must not become an address: clamped)
    const int from = min(max(a.frame_map[frame], 0), a.T - 1), from0 = min(max(a.frame_map[((long long)row * a.M) * a.T + t], 0), a.T - 1);
    const float* x = a.src + ((s * a.M + m) * a.T + from) * (long long)inner + j * C;
    const float* ctr = a.src + ((s * a.M) * a.T + from0) * (long long)inner + a.origin * C;      // body 0, its own map
    float v[C];
    bool present = false;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x[c], present |= v[c] != 0.0f;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = present ? (double)v[c] - (double)ctr[c] : 0.0;
    float* dst = a.out + frame * inner + j * C;
    if constexpr (C == 3) {
        const double* P = a.params + (long long)row * 12;
        if (P[9] != 0.0 || P[10] != 0.0) {                  // (no rotation: the centred value itself, whatever it is)
            double r[9], q[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) r[e] = P[e];
            normalize_matvec(r, p, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = q[c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = (float)p[c];
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_clip_normalize(const float* src, const long long* idx, float* out, int* frame_map, double* params, int b, int M, int T, int V,
                                   int C, int origin, int z0, int z1, int x0, int x1, void* stream) {
    FGCN_REQUIRE(src && idx && out && frame_map && params, FGCN_E_BADARG, "clip_normalize: null pointer");
    FGCN_REQUIRE(b > 0 && M > 0 && T > 0 && V > 0, FGCN_E_BADARG, "clip_normalize: bad b/M/T/V (%d, %d, %d, %d)", b, M, T, V);
    FGCN_REQUIRE(V <= 64, FGCN_E_BADARG, "clip_normalize: V=%d joints, at most 64", V);
    FGCN_REQUIRE(C == 2 || C == 3, FGCN_E_BADARG, "clip_normalize: C=%d, expected 2 or 3 coordinates", C);
    FGCN_REQUIRE(T <= NORMALIZE_MAX_T, FGCN_E_BADARG, "clip_normalize: T=%d frames, at most %d", T, NORMALIZE_MAX_T);
    FGCN_REQUIRE(origin >= 0 && origin < V, FGCN_E_BADARG, "clip_normalize: origin joint %d outside [0, %d)", origin, V);
    const int pair[2][2] = {{z0, z1}, {x0, x1}};
    for (int e = 0; e < 2; ++e) {
        const int j0 = pair[e][0], j1 = pair[e][1];
        if (j0 < 0) continue;                               // no pair for this axis
        FGCN_REQUIRE(j0 < V && j1 >= 0 && j1 < V && j0 != j1, FGCN_E_BADARG,
                     "clip_normalize: %c axis joints (%d, %d): two different joints of [0, %d) expected", e ? 'x' : 'z', j0, j1, V);
        FGCN_REQUIRE(C == 3, FGCN_E_BADARG, "clip_normalize: an axis pair needs C == 3 (C=%d)", C);
    }
    FGCN_REQUIRE(out != src, FGCN_E_BADARG, "clip_normalize: out must not alias src");
    NormalizeArgs a;
    a.src = src, a.idx = idx, a.out = out, a.frame_map = frame_map, a.params = params;
    a.b = b, a.M = M, a.T = T, a.V = V, a.origin = origin, a.z0 = z0 < 0 ? -1 : z0, a.z1 = z1, a.x0 = x0 < 0 ? -1 : x0, a.x1 = x1;
    a.by_inner = make_fastdiv((unsigned)(V * C)), a.by_V = make_fastdiv((unsigned)V);      // T * V * C <= 4096 * 192 < 2^29
    const long long bodies = (long long)b * M;
    FGCN_REQUIRE(bodies < (1ll << 31), FGCN_E_BADARG, "clip_normalize: %lld bodies are more than one grid holds", bodies);
    const dim3 grid((unsigned)bodies, (unsigned)cdiv((long long)T * V, 256));      // y <= 4096 * 64 / 256
    hipStream_t s = (hipStream_t)stream;
    if (C == 3) {
        hipLaunchKernelGGL(normalize_plan_kernel<3>, dim3((unsigned)b), dim3(PLAN_THREADS), 0, s, a);
        hipLaunchKernelGGL(normalize_apply_kernel<3>, grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(normalize_plan_kernel<2>, dim3((unsigned)b), dim3(PLAN_THREADS), 0, s, a);
        hipLaunchKernelGGL(normalize_apply_kernel<2>, grid, dim3(256), 0, s, a);
    }
    return launch_status("clip_normalize");
}
