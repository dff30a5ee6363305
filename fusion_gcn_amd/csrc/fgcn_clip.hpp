// What the clip kernels of ClipBatches' stages share (fgcn_augment.hip, fgcn_window.hip, fgcn_streams.hip, fgcn_sensors.hip): the uniform
// float of a generator word, the clamped valid-frame count of a source row, the rotation matrix of three angles, and the two source frames
// and the weight of a resampled frame.  One definition each: the copies these replace were meant to produce the same bits.
#pragma once

#include <cmath>

#include "fgcn_common.hpp"

namespace fgcn {

// a word of the generator -> a float in [0, 1): the top 24 bits, exact
__host__ __device__ inline float clip_uniform(unsigned w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }

// The valid frames of source row s of a clip of T frames; without a table, all T
__host__ __device__ inline int clip_valid(const int* valid, long long s, int T) {
    int v = T;
    if (valid) v = min(max(valid[s], 1), T);             // the contract says 1 <= valid <= T; a value outside must not become an address
    return v;
}

// s Rz(tz) Ry(ty) Rx(tx), row-major, each entry s * (the sum of its one or two products of sinf / cosf values).  The ONE definition of the
// matrix fgcn_clip_augment and fgcn_clip_sensors (s = 1: the entries themselves) draw: every product is written out and contraction is off,
// so the host and the device differ in sinf / cosf alone.  Zero angles and s = 1 give exactly the identity.
__host__ __device__ inline void clip_rotation(float tx, float ty, float tz, float s, float* out) {
#pragma clang fp contract(off)
    const float sx = sinf(tx), cx = cosf(tx), sy = sinf(ty), cy = cosf(ty), sz = sinf(tz), cz = cosf(tz);
    out[0] = s * (cz * cy);
    out[1] = s * (cz * sy * sx - sz * cx);
    out[2] = s * (cz * sy * cx + sz * sx);
    out[3] = s * (sz * cy);
    out[4] = s * (sz * sy * sx + cz * cx);
    out[5] = s * (sz * sy * cx - cz * sx);
    out[6] = s * (-sy);
    out[7] = s * (cy * sx);
    out[8] = s * (cy * cx);
}

// Output frame t of frames_out, of the part [off, off + win] of a clip's v valid frames, is x[f0] + w (x[f1] - x[f0])
struct ClipLerp {
    int f0, f1;
    float w;
};

// pos = (off + win t / (frames_out - 1)) (v - 1) as off (v - 1) + (win t) ((v - 1) / (frames_out - 1)): the quotient is exactly 1 for a
// full clip resampled to its own length, so that the identity parameters read frame t itself.  Frame: the caller's int or unsigned,
// which convert to float by different instructions.
template <typename Frame>
__host__ __device__ inline ClipLerp clip_lerp(Frame t, int frames_out, int v, float off, float win) {
#pragma clang fp contract(off)
    const float vm1 = (float)(v - 1), ratio = frames_out > 1 ? vm1 / (float)(frames_out - 1) : 0.0f;
    const float pos = fmaf(win * (float)t, ratio, off * vm1);
    const int f0 = min(max((int)floorf(pos), 0), v - 1), f1 = min(f0 + 1, v - 1);
    return {f0, f1, pos - (float)f0};
}

}  // namespace fgcn
