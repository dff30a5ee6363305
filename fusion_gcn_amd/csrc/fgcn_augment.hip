// Augmentation of skeleton / inertial clips as the batch is gathered (ClipBatches(augment=...); contract in include/fgcn.h, DESIGN.md
// section 8f).  Row k of the batch is source row idx[k] resampled in time (a random window of the recording, linearly interpolated) and,
// for joints with three coordinates, rotated and scaled about the origin.  The random numbers of a row come from the counter-based
// generator (fgcn_rng.hpp) at (sample_ids[k], site, epoch) under the key `seed`: the augmented clip is a pure function of those and of the
// source row, whatever the batch order, the number of ranks or the path the row took to the device.
// Two launches: augment_params_kernel, one lane per row, draws the row's twelve parameters (two Philox blocks, three sincos) into the
// table the call returns; augment_kernel, one lane per (row, person, frame, joint), reads them back (the table of a batch is a few KB:
// every read after the first is a cache hit) and moves the joint's floats.  4-byte loads and stores: a row of 75 floats has no wider
// alignment.
#include <cmath>

#include "fgcn_clip.hpp"
#include "fgcn_common.hpp"
#include "fgcn_rng.hpp"

namespace fgcn {

// The table row of one sample: A (3 x 3, row-major) = s Rz Ry Rx, then o, r, 0.  The ONE definition: the kernel and fgcn_augment_params
// both call it.  Every product here and in clip_rotation is written out and contraction is off, so the host and the device differ in sinf /
// cosf alone.
// 2u - 1 is exact (a multiple of 2^-23 of magnitude <= 1); 1 - r is formed as (1 - u4) (1 - min_window), whose first factor is exact: o
// keeps its relative accuracy when the window nearly fills the recording.  Zero magnitudes and min_window = 1 give the identity, 0 and 1.
__host__ __device__ inline void augment_params(unsigned sample, unsigned site, unsigned epoch, unsigned k0, unsigned k1, float ax, float ay,
                                               float az, float scale, float min_window, float* out) {
#pragma clang fp contract(off)
    const philox4 p0 = philox4x32_10(sample, site, epoch, 0u, k0, k1), p1 = philox4x32_10(sample, site, epoch, 1u, k0, k1);
    const float tx = (2.0f * clip_uniform(p0.w[0]) - 1.0f) * ax, ty = (2.0f * clip_uniform(p0.w[1]) - 1.0f) * ay,
                tz = (2.0f * clip_uniform(p0.w[2]) - 1.0f) * az;
    const float s = 1.0f + (2.0f * clip_uniform(p0.w[3]) - 1.0f) * scale;
    clip_rotation(tx, ty, tz, s, out);
    const float u4 = clip_uniform(p1.w[0]), u5 = clip_uniform(p1.w[1]), span = 1.0f - min_window;
    out[9] = u5 * ((1.0f - u4) * span);
    out[10] = min_window + u4 * span;
    out[11] = 0.0f;
}

struct AugmentArgs {
    const float* src;
    const long long* idx;
    const long long* sample_ids;
    const int* valid;
    float* out;
    float* params;
    long long threads;      // b * outer * T * units
    int b, outer, T, inner, units, joint_lo, joint_hi;
    float ax, ay, az, scale, min_window;
    unsigned k0, k1, site, epoch;
};

__global__ __launch_bounds__(64) void augment_params_kernel(AugmentArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.b) return;
    float row[12];
    augment_params((unsigned)a.sample_ids[k], a.site, a.epoch, a.k0, a.k1, a.ax, a.ay, a.az, a.scale, a.min_window, row);
#pragma unroll
    for (int e = 0; e < 12; ++e) a.params[(long long)k * 12 + e] = row[e];
}

// W floats per lane: 3 = one joint (x, y, z), 1 = one element of a modality without a spatial part.  Lane i owns unit j of frame t of
// person o of batch row `row`: i = ((row * outer + o) * T + t) * units + j.
template <int W>
__global__ __launch_bounds__(256) void augment_kernel(AugmentArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.threads) return;
    const int j = (int)(i % a.units);
    const long long frame = i / a.units;                 // (row * outer + o) * T + t
    const int t = (int)(frame % a.T);
    const long long ro = frame / a.T;
    const int row = (int)(ro / a.outer), o = (int)(ro % a.outer);
    const long long s = a.idx[row];
    const int v = clip_valid(a.valid, s, a.T);
    const float* P = a.params + (long long)row * 12;
    const float off = P[9], win = P[10];
    const ClipLerp l = clip_lerp(t, a.T, v, off, win);   // the window [o, o + r] of the valid frames resampled to the clip's T frames
    const float* base = a.src + ((s * a.outer + o) * a.T) * (long long)a.inner + (long long)j * W;
    const float *x0 = base + (long long)l.f0 * a.inner, *x1 = base + (long long)l.f1 * a.inner;
    float y[W];
#pragma unroll
    for (int c = 0; c < W; ++c) y[c] = fmaf(l.w, x1[c] - x0[c], x0[c]);
    float* dst = a.out + frame * a.inner + (long long)j * W;
    if constexpr (W == 3) {
        if (j >= a.joint_lo && j < a.joint_hi) {
            float z[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) z[c] = fmaf(P[3 * c + 2], y[2], fmaf(P[3 * c + 1], y[1], P[3 * c] * y[0]));
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = z[c];
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c) dst[c] = y[c];
}

}  // namespace fgcn

using namespace fgcn;

static int check_augment_magnitudes(const char* what, const float* max_angle, float scale, float min_window) {
    FGCN_REQUIRE(max_angle, FGCN_E_BADARG, "%s: null pointer (max_angle)", what);
    for (int e = 0; e < 3; ++e)
        FGCN_REQUIRE(std::isfinite(max_angle[e]), FGCN_E_BADARG, "%s: max_angle[%d]=%g is not finite", what, e, (double)max_angle[e]);
    FGCN_REQUIRE(scale >= 0.f && scale < 1.f, FGCN_E_BADARG, "%s: scale=%g outside [0, 1)", what, (double)scale);      // (NaN fails both)
    FGCN_REQUIRE(min_window > 0.f && min_window <= 1.f, FGCN_E_BADARG, "%s: min_window=%g outside (0, 1]", what, (double)min_window);
    return FGCN_OK;
}

extern "C" int fgcn_augment_params(unsigned sample, unsigned site, unsigned epoch, unsigned long long seed, const float max_angle[3], float scale,
                                   float min_window, float out12[12]) {
    if (int e = check_augment_magnitudes("augment_params", max_angle, scale, min_window)) return e;
    FGCN_REQUIRE(out12, FGCN_E_BADARG, "augment_params: null pointer (out12)");
    augment_params(sample, site, epoch, (unsigned)seed, (unsigned)(seed >> 32), max_angle[0], max_angle[1], max_angle[2], scale, min_window, out12);
    return FGCN_OK;
}

extern "C" int fgcn_clip_augment(const float* src, const long long* idx, const long long* sample_ids, const int* valid, float* out, float* params,
                                 int b, int outer, int T, int inner, int C, int joint_lo, int joint_hi, const float max_angle[3], float scale,
                                 float min_window, unsigned long long seed, unsigned site, unsigned epoch, void* stream) {
    FGCN_REQUIRE(src && idx && sample_ids && out && params, FGCN_E_BADARG, "clip_augment: null pointer");
    FGCN_REQUIRE(b > 0 && outer > 0 && T > 0 && inner > 0, FGCN_E_BADARG, "clip_augment: bad b/outer/T/inner (%d, %d, %d, %d)", b, outer, T, inner);
    FGCN_REQUIRE(C > 0 && inner % C == 0, FGCN_E_BADARG, "clip_augment: C=%d does not divide inner=%d", C, inner);
    FGCN_REQUIRE(joint_lo >= 0 && joint_lo <= joint_hi && joint_hi <= inner / C, FGCN_E_BADARG,
                 "clip_augment: joint range [%d, %d) outside [0, %d]", joint_lo, joint_hi, inner / C);
    FGCN_REQUIRE(joint_hi == joint_lo || C == 3, FGCN_E_BADARG, "clip_augment: a joint range needs C == 3 (C=%d)", C);
    if (int e = check_augment_magnitudes("clip_augment", max_angle, scale, min_window)) return e;
    FGCN_REQUIRE(src != out, FGCN_E_BADARG, "clip_augment: out must not alias src");
    const bool spatial = joint_hi > joint_lo;
    AugmentArgs a;
    a.src = src, a.idx = idx, a.sample_ids = sample_ids, a.valid = valid, a.out = out, a.params = params;
    a.b = b, a.outer = outer, a.T = T, a.inner = inner, a.units = spatial ? inner / 3 : inner, a.joint_lo = joint_lo, a.joint_hi = joint_hi;
    a.threads = (long long)b * outer * T * a.units;
    a.ax = max_angle[0], a.ay = max_angle[1], a.az = max_angle[2], a.scale = scale, a.min_window = min_window;
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32), a.site = site, a.epoch = epoch;
    const long long blocks = cdiv(a.threads, 256);
    FGCN_REQUIRE(blocks < (1ll << 31), FGCN_E_BADARG, "clip_augment: %lld lanes are more than one grid holds", a.threads);
    hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)cdiv(b, 64)), dim3(64), 0, (hipStream_t)stream, a);
    if (spatial) hipLaunchKernelGGL(augment_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(augment_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("clip_augment");
}
