// The second-order input streams of the two-stream AGCN family, derived as the batch is gathered (ClipBatches(streams=...); contract in
// include/fgcn.h).  Row k of every output is source row idx[k]: the joints themselves, the bones (joint minus
// parent joint), the motion (frame t+1 minus frame t inside the row's valid frames) and the motion of the bones.  Every value is one
// correctly rounded float32 subtraction, a copy or a zero -- no product, so nothing can be contracted into an fma.
// One launch, one lane per (row, person, frame, joint): it loads the joint, its parent and the two of the next frame -- at most 4 C floats,
// neighbours in memory of what the lanes beside it load (a frame is V C consecutive floats, the next frame the V C behind them) -- and
// stores C floats to each output that was asked for.  4-byte loads and stores: a row of 75 floats has no wider alignment.  Which
// outputs exist is the same for every lane of a launch (kernel arguments: scalar branches); the one value read from memory that shapes
// an address or a select is the row's valid frame count, clamped into [1, T], and a parent number, clamped into [-1, V).
#include "fgcn_clip.hpp"
#include "fgcn_common.hpp"

namespace fgcn {

struct StreamsArgs {
    const float* src;
    const long long* idx;
    const int* parents;
    const int* valid;
    float *joint, *bone, *motion, *bone_motion;
    long long threads;      // b * M * T * V
    int b, M, T, V;
};

// Lane i owns joint v of frame t of person o of batch row `row`: i = ((row * M + o) * T + t) * V + v.
template <int C>
__global__ __launch_bounds__(256) void streams_kernel(StreamsArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.threads) return;
    const int v = (int)(i % a.V);
    const long long frame = i / a.V;                     // (row * M + o) * T + t
    const int t = (int)(frame % a.T);
    const long long ro = frame / a.T;
    const int row = (int)(ro / a.M), o = (int)(ro % a.M);
    const long long s = a.idx[row];
    const int L = clip_valid(a.valid, s, a.T);
    const bool parent = a.bone || a.bone_motion, next = a.motion || a.bone_motion;      // what this launch has to load
    const int pv = parent ? min(max(a.parents[v], -1), a.V - 1) : -1;
    const bool through = pv < 0;                         // a sensor joint: the bone is the joint itself
    const int p = through ? v : pv;
    // frame t+1 is read only when it is a valid frame; the lanes of the last valid frame and behind it read frame L-1 (< L <= T) and
    // select the zero: no branch on a value from memory
    const bool live = t + 1 < L;
    const int t1 = min(t + 1, L - 1);
    const float* x0 = a.src + ((s * a.M + o) * a.T + t) * ((long long)a.V * C);
    const float* x1 = x0 + (long long)(t1 - t) * (a.V * C);
    const long long at = i * C;                          // this joint in every output
    float j0[C], b0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) j0[c] = x0[v * C + c];
    if (parent) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float xp = x0[p * C + c];
            b0[c] = through ? j0[c] : j0[c] - xp;
        }
    }
    if (a.joint) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.joint[at + c] = j0[c];
    }
    if (a.bone) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.bone[at + c] = b0[c];
    }
    if (next) {
        float j1[C];
#pragma unroll
        for (int c = 0; c < C; ++c) j1[c] = x1[v * C + c];
        if (a.motion) {
#pragma unroll
            for (int c = 0; c < C; ++c) a.motion[at + c] = live ? j1[c] - j0[c] : 0.0f;
        }
        if (a.bone_motion) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float xp = x1[p * C + c];
                const float b1 = through ? j1[c] : j1[c] - xp;      // rounded to float32 before the difference of the bones
                a.bone_motion[at + c] = live ? b1 - b0[c] : 0.0f;
            }
        }
    }
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_clip_streams(const float* src, const long long* idx, const int* parents, const int* valid, float* joint, float* bone,
                                 float* motion, float* bone_motion, int b, int M, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(src, FGCN_E_BADARG, "clip_streams: null pointer (src)");
    FGCN_REQUIRE(idx, FGCN_E_BADARG, "clip_streams: null pointer (idx)");
    FGCN_REQUIRE(parents, FGCN_E_BADARG, "clip_streams: null pointer (parents)");
    FGCN_REQUIRE(bone || motion || bone_motion, FGCN_E_BADARG, "clip_streams: no derived output (bone, motion and bone_motion are all null)");
    FGCN_REQUIRE(b > 0 && M > 0 && T > 0 && V > 0, FGCN_E_BADARG, "clip_streams: bad b/M/T/V (%d, %d, %d, %d)", b, M, T, V);
    FGCN_REQUIRE(C == 2 || C == 3, FGCN_E_BADARG, "clip_streams: C=%d, expected 2 or 3", C);
    FGCN_REQUIRE(joint != src && bone != src && motion != src && bone_motion != src, FGCN_E_BADARG,
                 "clip_streams: an output must not alias src (joint, bone, motion, bone_motion)");
    StreamsArgs a;
    a.src = src, a.idx = idx, a.parents = parents, a.valid = valid;
    a.joint = joint, a.bone = bone, a.motion = motion, a.bone_motion = bone_motion;
    a.b = b, a.M = M, a.T = T, a.V = V;
    // 2^31 - 1 workgroups of 256 lanes; the factors are below 2^31 each, so b * M fits and the two quotients keep the rest from overflowing
    const long long max_lanes = ((1ll << 31) - 1) * 256, bodies = (long long)b * M;
    FGCN_REQUIRE(bodies <= max_lanes / T && bodies * T <= max_lanes / V, FGCN_E_BADARG,
                 "clip_streams: b * M * T * V = %d * %d * %d * %d lanes are more than one grid holds", b, M, T, V);
    a.threads = bodies * T * V;
    const long long blocks = cdiv(a.threads, 256);
    if (C == 3) hipLaunchKernelGGL(streams_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(streams_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("clip_streams");
}
