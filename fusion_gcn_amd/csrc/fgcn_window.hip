// Cropping clips to their valid frames and resizing the crop to a window of W frames as the batch is gathered (ClipBatches(window=...);
// contract in include/fgcn.h), and the count of a clip's valid frames that the crop is taken from.
// fgcn_clip_window: row k of the batch is a part of the valid frames of source row idx[k] -- a random interval (training) or the centred
// one (evaluation) -- linearly interpolated to W frames, W smaller than, equal to or larger than the stored T.  The random numbers of a
// row come from the counter-based generator (fgcn_rng.hpp) at (sample_ids[k], site, epoch, 2) under the key `seed`: counter word 3 is 2,
// the augmentation (fgcn_augment.hip) uses 0 and 1 at the same (seed, site), so the crop is independent of the rotation.
// Two launches: window_params_kernel, one lane per row, writes the row's {o, r} into the table the call returns; window_kernel, one lane
// per output element, reads them back (a batch's table is a few hundred bytes: every read after the first is a cache hit) and
// interpolates its float.  A workgroup stays inside one (row, body): the row's numbers are uniform over it and the lanes' indices are
// 32-bit.  4-byte loads and stores: a row of 75 floats has no wider alignment.
// fgcn_clip_valid_frames: one workgroup per row looks for the last frame that holds a value in any body -- a maximum over the lanes, no
// atomics; the lanes stride over a body's floats (4-byte loads, neighbours in memory) and keep the largest frame number they saw.
#include <cmath>

#include "fgcn_clip.hpp"
#include "fgcn_common.hpp"
#include "fgcn_rng.hpp"

namespace fgcn {

// The table row of one sample, {o, r}: the part [o, o + r] of the recording, as fractions of it.  The ONE definition: the kernel and
// fgcn_window_params both call it; there is no transcendental function and contraction is off, so the two give the same bits.
// RANDOM: r = lo + u0 (hi - lo) and o = u1 (1 - r), with 1 - r formed as (1 - hi) + (1 - u0) (hi - lo): 1 - u0 is exact, every term is
// >= 0 (nothing cancels, o keeps its relative accuracy when the part nearly fills the recording) and it is exactly 0 for lo = hi = 1.
// The two min() hold r <= hi and o + r <= 1 against the last rounding (at most one float32 spacing each): the part never leaves the
// recording.  CENTRE: r = hi, o = (1 - r) / 2, no random numbers.
__host__ __device__ inline void window_params(unsigned sample, unsigned site, unsigned epoch, unsigned k0, unsigned k1, float lo, float hi,
                                              int mode, float* out) {
#pragma clang fp contract(off)
    if (mode == FGCN_WINDOW_CENTRE) {
        out[0] = (1.0f - hi) * 0.5f;
        out[1] = hi;
        return;
    }
    const philox4 p = philox4x32_10(sample, site, epoch, 2u, k0, k1);
    const float u0 = clip_uniform(p.w[0]), u1 = clip_uniform(p.w[1]), span = hi - lo;
    const float r = fminf(lo + u0 * span, hi);
    const float rest = (1.0f - hi) + (1.0f - u0) * span;
    out[0] = fminf(u1 * rest, 1.0f - r);
    out[1] = r;
}

struct WindowArgs {
    const float* src;
    const long long* idx;
    const long long* sample_ids;
    const int* valid;
    float* out;
    float* params;
    int b, outer, T, W, inner, mode;
    unsigned per_body, blocks_per_body;     // W * inner; workgroups of 256 lanes that cover them
    FastDiv by_inner;                       // element of a body of `out` -> its frame
    float lo, hi;
    unsigned k0, k1, site, epoch;
};

__global__ __launch_bounds__(64) void window_params_kernel(WindowArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.b) return;
    float row[2];
    const unsigned sample = a.mode == FGCN_WINDOW_CENTRE ? 0u : (unsigned)a.sample_ids[k];
    window_params(sample, a.site, a.epoch, a.k0, a.k1, a.lo, a.hi, a.mode, row);
    a.params[2 * (long long)k] = row[0];
    a.params[2 * (long long)k + 1] = row[1];
}

// Workgroup g owns elements [256 c, 256 c + 256) of body o of batch row `row`: g = (row * outer + o) * blocks_per_body + c.
__global__ __launch_bounds__(256) void window_kernel(WindowArgs a) {
    const unsigned body = blockIdx.x / a.blocks_per_body, chunk = blockIdx.x - body * a.blocks_per_body;
    const unsigned e = chunk * 256u + threadIdx.x;       // < 2^29: the launcher refuses larger bodies
    if (e >= a.per_body) return;
    const unsigned row = body / (unsigned)a.outer, o = body - row * (unsigned)a.outer;
    const unsigned t = fastdiv(e, a.by_inner), j = e - t * (unsigned)a.inner;
    const long long s = a.idx[row];
    const int v = clip_valid(a.valid, s, a.T);
    const float off = a.params[2 * (long long)row], win = a.params[2 * (long long)row + 1];
    const ClipLerp l = clip_lerp(t, a.W, v, off, win);   // the part [o, o + r] of the valid frames resized to W frames
    const float* base = a.src + ((s * a.outer + o) * a.T) * (long long)a.inner + j;
    const float x0 = base[(long long)l.f0 * a.inner], x1 = base[(long long)l.f1 * a.inner];
    a.out[(long long)body * a.per_body + e] = fmaf(l.w, x1 - x0, x0);
}

struct ValidFramesArgs {
    const float* src;
    const long long* idx;
    int* out;
    int outer;
    unsigned per_body;      // T * inner
    FastDiv by_inner;       // element of a body of `src` -> its frame
};

constexpr int VALID_THREADS = 256, VALID_WAVES = VALID_THREADS / 64;

__global__ __launch_bounds__(VALID_THREADS) void valid_frames_kernel(ValidFramesArgs a) {
    __shared__ int wave_last[VALID_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x;
    const float* clip = a.src + a.idx[k] * a.outer * (long long)a.per_body;
    int last = -1;                                       // the largest frame in which this lane saw a value
    for (int m = 0; m < a.outer; ++m) {
        const float* body = clip + (long long)m * a.per_body;
        // independent iterations: a lane's loads are all in flight together.  x != 0 is false for -0 and true for a NaN.
#pragma unroll 8
        for (unsigned e = tid; e < a.per_body; e += VALID_THREADS)
            if (body[e] != 0.0f) last = max(last, (int)fastdiv(e, a.by_inner));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d));
    if ((tid & 63) == 0) wave_last[tid >> 6] = last;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 0; w < VALID_WAVES; ++w) last = max(last, wave_last[w]);
    a.out[k] = max(last + 1, 1);                         // a clip without a value counts as one frame: the table lies in [1, T]
}

}  // namespace fgcn

using namespace fgcn;

static int check_window_interval(const char* what, float lo, float hi, int mode) {
    FGCN_REQUIRE(mode == FGCN_WINDOW_RANDOM || mode == FGCN_WINDOW_CENTRE, FGCN_E_BADARG, "%s: unknown mode %d", what, mode);
    FGCN_REQUIRE(std::isfinite(lo) && std::isfinite(hi), FGCN_E_BADARG, "%s: interval (%g, %g) is not finite", what, (double)lo, (double)hi);
    FGCN_REQUIRE(lo > 0.f && lo <= hi && hi <= 1.f, FGCN_E_BADARG, "%s: interval (%g, %g) outside 0 < lo <= hi <= 1", what, (double)lo,
                 (double)hi);
    return FGCN_OK;
}

extern "C" int fgcn_window_params(unsigned sample, unsigned site, unsigned epoch, unsigned long long seed, float lo, float hi, int mode,
                                  float out2[2]) {
    if (int e = check_window_interval("window_params", lo, hi, mode)) return e;
    FGCN_REQUIRE(out2, FGCN_E_BADARG, "window_params: null pointer (out2)");
    window_params(sample, site, epoch, (unsigned)seed, (unsigned)(seed >> 32), lo, hi, mode, out2);
    return FGCN_OK;
}

extern "C" int fgcn_clip_window(const float* src, const long long* idx, const long long* sample_ids, const int* valid, float* out, float* params,
                                int b, int outer, int T, int W, int inner, float lo, float hi, int mode, unsigned long long seed, unsigned site,
                                unsigned epoch, void* stream) {
    FGCN_REQUIRE(src && idx && out && params, FGCN_E_BADARG, "clip_window: null pointer");
    if (int e = check_window_interval("clip_window", lo, hi, mode)) return e;
    FGCN_REQUIRE(sample_ids || mode == FGCN_WINDOW_CENTRE, FGCN_E_BADARG, "clip_window: null pointer (sample_ids, which mode RANDOM reads)");
    FGCN_REQUIRE(b > 0 && outer > 0 && T > 0 && W > 0 && inner > 0, FGCN_E_BADARG, "clip_window: bad b/outer/T/W/inner (%d, %d, %d, %d, %d)", b,
                 outer, T, W, inner);
    FGCN_REQUIRE(src != out, FGCN_E_BADARG, "clip_window: out must not alias src");
    // a lane's index inside a body is 32-bit and goes through FastDiv (exact below 2^29); one grid holds 2^31 - 1 workgroups
    const long long per_body = (long long)W * inner, blocks_per_body = cdiv(per_body, 256);
    FGCN_REQUIRE(per_body < (1ll << 29), FGCN_E_BADARG, "clip_window: W * inner = %d * %d elements in a body are more than a lane indexes", W,
                 inner);
    FGCN_REQUIRE((long long)b * outer <= ((1ll << 31) - 1) / blocks_per_body, FGCN_E_BADARG,
                 "clip_window: b * outer * W * inner = %d * %d * %d * %d elements are more than one grid holds", b, outer, W, inner);
    WindowArgs a;
    a.src = src, a.idx = idx, a.sample_ids = sample_ids, a.valid = valid, a.out = out, a.params = params;
    a.b = b, a.outer = outer, a.T = T, a.W = W, a.inner = inner, a.mode = mode;
    a.per_body = (unsigned)per_body, a.blocks_per_body = (unsigned)blocks_per_body, a.by_inner = make_fastdiv((unsigned)inner);
    a.lo = lo, a.hi = hi, a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32), a.site = site, a.epoch = epoch;
    const long long blocks = (long long)b * outer * blocks_per_body;
    hipLaunchKernelGGL(window_params_kernel, dim3((unsigned)cdiv(b, 64)), dim3(64), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(window_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("clip_window");
}

extern "C" int fgcn_clip_valid_frames(const float* src, const long long* idx, int* out, int b, int outer, int T, int inner, void* stream) {
    FGCN_REQUIRE(src && idx && out, FGCN_E_BADARG, "clip_valid_frames: null pointer");
    FGCN_REQUIRE(b > 0 && outer > 0 && T > 0 && inner > 0, FGCN_E_BADARG, "clip_valid_frames: bad b/outer/T/inner (%d, %d, %d, %d)", b, outer, T,
                 inner);
    const long long per_body = (long long)T * inner;
    FGCN_REQUIRE(per_body < (1ll << 29), FGCN_E_BADARG, "clip_valid_frames: T * inner = %d * %d elements in a body are more than a lane indexes",
                 T, inner);
    ValidFramesArgs a;
    a.src = src, a.idx = idx, a.out = out, a.outer = outer, a.per_body = (unsigned)per_body, a.by_inner = make_fastdiv((unsigned)inner);
    hipLaunchKernelGGL(valid_frames_kernel, dim3((unsigned)b), dim3(VALID_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("clip_valid_frames");
}
