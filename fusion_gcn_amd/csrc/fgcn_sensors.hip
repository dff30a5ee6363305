// Augmentation of inertial recordings as the batch is gathered (ClipBatches(sensors=...); contract in include/fgcn.h, DESIGN.md section
// 8p).  A sensor is a triple of values: columns 3g .. 3g+2 of a (T, S) signal, or joint lo + g of every body of an (M, T, V, 3) array.
// Row k of the batch is source row idx[k] with, in its valid frames, every sensor rotated (one rotation per sample: the sensors sit in
// one device frame), scaled by its own gain, warped by a smooth magnitude curve over time, jittered and -- for a fusion model -- dropped
// as a whole.  The random numbers come from the counter-based generator (fgcn_rng.hpp) at (sample_ids[k], site, epoch) under the key
// `seed`, in counter words that fgcn_clip_augment (0, 1) and fgcn_clip_window (2) leave free, keyed by (frame, sensor) and never by body:
// every body of a 4-d array, and the signal beside it, receive the same values.
// Launches: sensors_params_kernel, one lane per (row, table group), draws the row's 12 + 12 G parameters into the table the call returns.
// Then either sensors_kernel, one lane per (row, body, frame, unit of three floats), which reads them back (the table of a batch is a few
// KB: every read after the first is a cache hit) and moves the unit -- or, with minmax, sensors_minmax_kernel, one workgroup per clip:
// pass 1 stores the augmented values into `out` and takes their minimum and maximum (order-independent), pass 2 has every lane read
// back what it stored itself and normalise it, so that the two passes cannot disagree about a value.  4-byte loads and stores: a row of
// 6 or 66 floats has no wider alignment.
#include <cmath>

#include "fgcn_clip.hpp"
#include "fgcn_common.hpp"
#include "fgcn_rng.hpp"

namespace fgcn {

constexpr int SENSORS_THREADS = 256, SENSORS_WAVES = SENSORS_THREADS / 64;
constexpr unsigned SENSORS_JITTER_BASE = 1u << 20;      // the counter word of the jitter of (frame 0, sensor 0)

// What every lane knows of the draw: the generator's key and counter words, and the magnitudes
struct SensorsDraw {
    unsigned k0, k1, site, epoch, drop_thr;              // drop_thr = (unsigned)(drop * 2^32)
    float ax, ay, az, scale, warp;
    int knots;                                           // K: 0, or 2 .. FGCN_SENSORS_MAX_KNOTS
};

// Floats 0..11 of the table row of one sample: R = Rz Ry Rx row-major, then three zeros.  The ONE definition: the kernel and
// fgcn_sensors_params both call it.  2u - 1 is exact; zero angles give exactly the identity.
__host__ __device__ inline void sensors_header(unsigned sample, const SensorsDraw& d, float* out) {
#pragma clang fp contract(off)
    const philox4 p = philox4x32_10(sample, d.site, d.epoch, 3u, d.k0, d.k1);
    const float tx = (2.0f * clip_uniform(p.w[0]) - 1.0f) * d.ax, ty = (2.0f * clip_uniform(p.w[1]) - 1.0f) * d.ay,
                tz = (2.0f * clip_uniform(p.w[2]) - 1.0f) * d.az;
    clip_rotation(tx, ty, tz, 1.0f, out);
    out[9] = out[10] = out[11] = 0.0f;
}

// Floats 12 + 12 g .. 12 + 12 g + 11 of the row: the gain, the drop flag, two zeros, the eight knot values (the unused ones 0).  No
// transcendental function and contraction off: the host's copy has the device's bits.
__host__ __device__ inline void sensors_group(unsigned sample, int g, const SensorsDraw& d, float* out) {
#pragma clang fp contract(off)
    const unsigned j = 16u + 4u * (unsigned)g;
    const philox4 p = philox4x32_10(sample, d.site, d.epoch, j, d.k0, d.k1);
    out[0] = 1.0f + (2.0f * clip_uniform(p.w[0]) - 1.0f) * d.scale;
    out[1] = p.w[1] < d.drop_thr ? 1.0f : 0.0f;
    out[2] = out[3] = 0.0f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        philox4 q = {{0u, 0u, 0u, 0u}};
        if (d.knots > 4 * half) q = philox4x32_10(sample, d.site, d.epoch, j + 1u + (unsigned)half, d.k0, d.k1);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 + 4 * half + e] = 4 * half + e < d.knots ? (2.0f * clip_uniform(q.w[e]) - 1.0f) * d.warp : 0.0f;
    }
}

struct SensorsArgs {
    const float* src;
    const long long* idx;
    const long long* sample_ids;
    const int* valid;
    float* out;
    float* params;
    float* stats;
    long long threads;      // b * outer * T * units
    int b, outer, T, units, lo, G, row_floats;           // units = inner / 3; sensors are units [lo, lo + G); row_floats = 12 + 12 G
    SensorsDraw d;
    float sigma[FGCN_SENSORS_MAX];
};

__global__ __launch_bounds__(64) void sensors_params_kernel(SensorsArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, groups = a.G + 1;
    if (i >= a.b * groups) return;
    const int k = i / groups, slot = i % groups;
    float row[12];
    if (slot == 0) sensors_header((unsigned)a.sample_ids[k], a.d, row);
    else sensors_group((unsigned)a.sample_ids[k], slot - 1, a.d, row);
    float* dst = a.params + (long long)k * a.row_floats + 12 * slot;
#pragma unroll
    for (int e = 0; e < 12; ++e) dst[e] = row[e];
}

// One standard normal value from two generator words (Box-Muller, the cosine branch; `sine`: the other branch of the same pair)
__device__ inline float sensors_normal(unsigned w0, unsigned w1, bool sine) {
#pragma clang fp contract(off)
    const float u1 = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-08f, u2 = clip_uniform(w1);      // (0, 1] and [0, 1)
    const float rad = sqrtf(-2.0f * logf(u1));
    return rad * (sine ? sinpif(2.0f * u2) : cospif(2.0f * u2));
}

// The triple of sensor g in valid frame t of a clip of v valid frames, from the source triple x: gain and rotation, warp, jitter, drop,
// in that order.  P: the sample's table row.  The ONE definition: both kernels call it.
__device__ inline void sensors_triple(const SensorsArgs& a, const float* P, unsigned sample, int t, int g, int v, const float* x, float* y) {
#pragma clang fp contract(off)
    const float* grp = P + 12 + 12 * g;
    const float s = grp[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = s * fmaf(P[3 * c + 2], x[2], fmaf(P[3 * c + 1], x[1], P[3 * c] * x[0]));
    const int K = a.d.knots;
    if (K > 0) {
        const float q = v > 1 ? (float)t * ((float)(K - 1) / (float)(v - 1)) : 0.0f;
        const int i = min((int)floorf(q), K - 2);
        const float f = q - (float)i;
        const float* kn = grp + 4;
        const float p0 = kn[max(i - 1, 0)], p1 = kn[i], p2 = kn[i + 1], p3 = kn[min(i + 2, K - 1)];
        const float ca = p2 - p0, cb = ((2.0f * p0 - 5.0f * p1) + 4.0f * p2) - p3, cc = (3.0f * (p1 - p2) + p3) - p0;
        const float m = 1.0f + (p1 + 0.5f * (f * (ca + f * (cb + f * cc))));
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = m * y[c];
    }
    float sigma = 0.0f;                                  // (a select per sensor: an index into the argument block would go through scratch)
#pragma unroll
    for (int e = 0; e < FGCN_SENSORS_MAX; ++e) sigma = g == e ? a.sigma[e] : sigma;
    if (sigma != 0.0f) {                                 // no addition otherwise: a -0 survives
        const philox4 p = philox4x32_10(sample, a.d.site, a.d.epoch, SENSORS_JITTER_BASE + (unsigned)t * (unsigned)a.G + (unsigned)g, a.d.k0,
                                        a.d.k1);
        y[0] = y[0] + sigma * sensors_normal(p.w[0], p.w[1], false);
        y[1] = y[1] + sigma * sensors_normal(p.w[0], p.w[1], true);
        y[2] = y[2] + sigma * sensors_normal(p.w[2], p.w[3], false);
    }
    if (grp[1] != 0.0f) y[0] = y[1] = y[2] = 0.0f;
}

// Unit j (three floats) of frame t of body o of batch row `row`, source row s, into y: a sensor's valid frames are transformed, every
// other unit and every frame at or behind the valid count is copied bit for bit
__device__ inline void sensors_unit(const SensorsArgs& a, int row, long long s, int o, int t, int j, float* y) {
    const float* x = a.src + (((s * a.outer + o) * a.T + t) * (long long)a.units + j) * 3;
    const int g = j - a.lo, v = clip_valid(a.valid, s, a.T);
    if (g >= 0 && g < a.G && t < v) {
        const float x3[3] = {x[0], x[1], x[2]};
        sensors_triple(a, a.params + (long long)row * a.row_floats, (unsigned)a.sample_ids[row], t, g, v, x3, y);
    } else {
        y[0] = x[0], y[1] = x[1], y[2] = x[2];
    }
}

// Lane i owns unit j of frame t of body o of batch row `row`: i = ((row * outer + o) * T + t) * units + j.
__global__ __launch_bounds__(SENSORS_THREADS) void sensors_kernel(SensorsArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.threads) return;
    if (i < a.b) a.stats[2 * i] = 0.0f, a.stats[2 * i + 1] = 1.0f;
    const int j = (int)(i % a.units);
    const long long frame = i / a.units;                 // (row * outer + o) * T + t
    const int t = (int)(frame % a.T);
    const long long ro = frame / a.T;
    const int row = (int)(ro / a.outer), o = (int)(ro % a.outer);
    float y[3];
    sensors_unit(a, row, a.idx[row], o, t, j, y);
    float* dst = a.out + i * 3;
    dst[0] = y[0], dst[1] = y[1], dst[2] = y[2];
}

// One workgroup per clip (outer == 1): mn = min, mx = fl32(max - mn), y = fl32(fl32(x - mn) / mx) over the whole augmented (T, inner)
// array, the padding included -- fgcn_signal_prepare's step 3a, applied behind the augmentation.
__global__ __launch_bounds__(SENSORS_THREADS) void sensors_minmax_kernel(SensorsArgs a) {
    __shared__ float wave_min[SENSORS_WAVES], wave_max[SENSORS_WAVES];
    __shared__ int wave_nan[SENSORS_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = a.idx[k];
    const int n = a.T * a.units;
    float* dst = a.out + (long long)k * n * 3;
    // numpy's min and max return NaN where the array holds one: kept as a flag, since fminf / fmaxf drop a NaN
    float lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    for (int e = tid; e < n; e += SENSORS_THREADS) {
        float y[3];
        sensors_unit(a, k, s, 0, e / a.units, e % a.units, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dst[(long long)e * 3 + c] = y[c];
            lo = fminf(lo, y[c]), hi = fmaxf(hi, y[c]), nan |= y[c] != y[c];
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d)), hi = fmaxf(hi, __shfl_xor(hi, d)), nan |= __shfl_xor(nan, d);
    }
    if (lane == 0) wave_min[wave] = lo, wave_max[wave] = hi, wave_nan[wave] = nan;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SENSORS_WAVES; ++w) lo = fminf(lo, wave_min[w]), hi = fmaxf(hi, wave_max[w]), nan |= wave_nan[w];
    const float mn = nan ? NAN : lo, mx = nan ? NAN : hi - lo;      // the maximum of the shifted array: subtraction is monotone
    if (tid == 0) a.stats[2 * (long long)k] = mn, a.stats[2 * (long long)k + 1] = mx;
    // every lane reads back the elements it stored itself (program order: no fence is needed), so pass 2 sees pass 1's bits.  The quotient
    // of two floats formed in float64 and rounded once is the correctly rounded float32 quotient (0 / 0 for a constant clip)
    for (int e = tid; e < n; e += SENSORS_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* p = dst + (long long)e * 3 + c;
            *p = (float)((double)(*p - mn) / (double)mx);
        }
    }
}

}  // namespace fgcn

using namespace fgcn;

static int check_sensors_draw(const char* what, const float* max_angle, float scale, float warp, int warp_knots, float drop, int sensors,
                              SensorsDraw* d) {
    FGCN_REQUIRE(max_angle, FGCN_E_BADARG, "%s: null pointer (max_angle)", what);
    for (int e = 0; e < 3; ++e)
        FGCN_REQUIRE(std::isfinite(max_angle[e]), FGCN_E_BADARG, "%s: max_angle[%d]=%g is not finite", what, e, (double)max_angle[e]);
    FGCN_REQUIRE(scale >= 0.f && scale < 1.f, FGCN_E_BADARG, "%s: scale=%g outside [0, 1)", what, (double)scale);      // (NaN fails both)
    FGCN_REQUIRE(warp >= 0.f && warp < 1.f, FGCN_E_BADARG, "%s: warp=%g outside [0, 1)", what, (double)warp);
    FGCN_REQUIRE(drop >= 0.f && drop < 1.f, FGCN_E_BADARG, "%s: drop=%g outside [0, 1)", what, (double)drop);
    FGCN_REQUIRE(warp_knots == 0 || (warp_knots >= 2 && warp_knots <= FGCN_SENSORS_MAX_KNOTS), FGCN_E_BADARG,
                 "%s: warp_knots=%d is neither 0 nor in [2, %d]", what, warp_knots, FGCN_SENSORS_MAX_KNOTS);
    FGCN_REQUIRE(sensors >= 1 && sensors <= FGCN_SENSORS_MAX, FGCN_E_BADARG, "%s: %d sensors outside [1, %d]", what, sensors, FGCN_SENSORS_MAX);
    d->ax = max_angle[0], d->ay = max_angle[1], d->az = max_angle[2], d->scale = scale, d->warp = warp, d->knots = warp_knots;
    d->drop_thr = (unsigned)((double)drop * 4294967296.0);
    return FGCN_OK;
}

extern "C" int fgcn_sensors_params(unsigned sample, unsigned site, unsigned epoch, unsigned long long seed, const float max_angle[3], float scale,
                                   float warp, int warp_knots, float drop, int sensors, float* out) {
    SensorsDraw d;
    if (int e = check_sensors_draw("sensors_params", max_angle, scale, warp, warp_knots, drop, sensors, &d)) return e;
    FGCN_REQUIRE(out, FGCN_E_BADARG, "sensors_params: null pointer (out)");
    d.k0 = (unsigned)seed, d.k1 = (unsigned)(seed >> 32), d.site = site, d.epoch = epoch;
    sensors_header(sample, d, out);
    for (int g = 0; g < sensors; ++g) sensors_group(sample, g, d, out + 12 + 12 * g);
    return FGCN_OK;
}

extern "C" int fgcn_clip_sensors(const float* src, const long long* idx, const long long* sample_ids, const int* valid, float* out, float* params,
                                 float* stats, int b, int outer, int T, int inner, int joint_lo, int joint_hi, const float max_angle[3],
                                 float scale, float warp, int warp_knots, const float* jitter, float drop, int minmax, unsigned long long seed,
                                 unsigned site, unsigned epoch, void* stream) {
    FGCN_REQUIRE(src && idx && sample_ids && out && params && stats && jitter, FGCN_E_BADARG, "clip_sensors: null pointer");
    FGCN_REQUIRE(b > 0 && outer > 0 && T > 0 && inner > 0, FGCN_E_BADARG, "clip_sensors: bad b/outer/T/inner (%d, %d, %d, %d)", b, outer, T, inner);
    FGCN_REQUIRE(inner % 3 == 0, FGCN_E_BADARG, "clip_sensors: inner=%d is not a number of triples", inner);
    FGCN_REQUIRE(joint_lo >= 0 && joint_lo < joint_hi && joint_hi <= inner / 3, FGCN_E_BADARG,
                 "clip_sensors: sensor range [%d, %d) is empty or outside [0, %d]", joint_lo, joint_hi, inner / 3);
    const int G = joint_hi - joint_lo;
    SensorsArgs a;
    if (int e = check_sensors_draw("clip_sensors", max_angle, scale, warp, warp_knots, drop, G, &a.d)) return e;
    for (int g = 0; g < G; ++g)
        FGCN_REQUIRE(std::isfinite(jitter[g]) && jitter[g] >= 0.f, FGCN_E_BADARG, "clip_sensors: jitter[%d]=%g is not a finite value >= 0", g,
                     (double)jitter[g]);
    FGCN_REQUIRE(!minmax || outer == 1, FGCN_E_BADARG, "clip_sensors: minmax normalises a (T, S) signal (outer=%d)", outer);
    FGCN_REQUIRE(src != out, FGCN_E_BADARG, "clip_sensors: out must not alias src");
    FGCN_REQUIRE((long long)T * G < (1ll << 31) - (1ll << 20), FGCN_E_BADARG, "clip_sensors: T * sensors = %lld leaves the jitter no counter words",
                 (long long)T * G);
    FGCN_REQUIRE((long long)T * inner < (1ll << 29), FGCN_E_BADARG, "clip_sensors: T * inner = %lld is 2^29 or more", (long long)T * inner);
    a.src = src, a.idx = idx, a.sample_ids = sample_ids, a.valid = valid, a.out = out, a.params = params, a.stats = stats;
    a.b = b, a.outer = outer, a.T = T, a.units = inner / 3, a.lo = joint_lo, a.G = G, a.row_floats = 12 + 12 * G;
    a.threads = (long long)b * outer * T * a.units;
    a.d.k0 = (unsigned)seed, a.d.k1 = (unsigned)(seed >> 32), a.d.site = site, a.d.epoch = epoch;
    for (int g = 0; g < FGCN_SENSORS_MAX; ++g) a.sigma[g] = g < G ? jitter[g] : 0.0f;
    const long long blocks = cdiv(a.threads, SENSORS_THREADS);
    FGCN_REQUIRE(blocks < (1ll << 31) && (long long)b * (G + 1) < (1ll << 31), FGCN_E_BADARG, "clip_sensors: %lld lanes are more than one grid holds",
                 a.threads);
    hipLaunchKernelGGL(sensors_params_kernel, dim3((unsigned)cdiv((long long)b * (G + 1), 64)), dim3(64), 0, (hipStream_t)stream, a);
    if (minmax) hipLaunchKernelGGL(sensors_minmax_kernel, dim3((unsigned)b), dim3(SENSORS_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sensors_kernel, dim3((unsigned)blocks), dim3(SENSORS_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("clip_sensors");
}
