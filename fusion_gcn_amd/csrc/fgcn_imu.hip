// Preparation of raw inertial recordings as the batch is gathered (ClipBatches(inertial=...); contract in include/fgcn.h, DESIGN.md
// section 8h): the reference's offline preprocessing of the accelerometer / gyroscope recording -- nearest-neighbour resampling to the
// skeleton's frame count, zero padding to the clip's T frames, then either min-max normalisation over the padded array (InertialProcessor,
// the `inertial` feature) or appending the samples as extra joints behind the normalised skeleton (SkeletonProcessor("imu_enhanced"), the
// `skeleton_imu_enhanced` feature).  resample_index is the ONE definition of the frame a resampled frame reads: both kernels and
// fgcn_resample_index call it.
// signal_prepare_kernel, one workgroup per clip: pass 1 takes the minimum and the maximum of the resampled, padded (T, S) array (both are
// order-independent: the bits do not depend on how the lanes share the work), pass 2 reads the values again (a clip is a few KB: cache
// hits) and stores fl32(fl32(x - mn) / mx).  imu_enhance_kernel, one lane per output joint: a skeleton joint is copied (a third
// coordinate of zero where the skeleton has two), an appended joint gathers three samples of the resampled recording.  4-byte loads and
// stores: rows of 6, 21 or 66 floats have no wider alignment.
#include <cmath>
#include <initializer_list>

#include "fgcn_common.hpp"

namespace fgcn {

constexpr int SIGNAL_THREADS = 256, SIGNAL_WAVES = SIGNAL_THREADS / 64;

// The frame of a recording of src_len frames that frame t of its resampling to dst_len frames reads: the reference's
// rint(t * ((src_len - 1) / (dst_len - 1))) -- the quotient first, then the product, both float64, ties to even -- and t itself where the
// lengths are equal (the reference does not resample then).  Clamped into [0, src_len - 1]: a length or a t outside the contract must
// not become an address.
__host__ __device__ inline int resample_index(int t, int src_len, int dst_len) {
    double r = (double)t;
    if (src_len != dst_len) {
        if (dst_len <= 1) return 0;
        const double factor = (double)(src_len - 1) / (double)(dst_len - 1);
        r = rint((double)t * factor);
    }
    const double last = (double)(src_len - 1);          // (clamped before the conversion: every int fits a double)
    return r < 0.0 ? 0 : (int)(r > last ? last : r);
}

struct SignalArgs {
    const float* src;
    const long long* idx;
    const int* src_len;
    const int* dst_len;
    float* out;
    float* stats;
    int L, S, T, minmax;
    FastDiv by_S;
};

__global__ __launch_bounds__(SIGNAL_THREADS) void signal_prepare_kernel(SignalArgs a) {
    __shared__ float wave_min[SIGNAL_WAVES], wave_max[SIGNAL_WAVES];
    __shared__ int wave_nan[SIGNAL_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = a.idx[k];
    const int li = min(max(a.src_len[s], 1), a.L), ls = min(max(a.dst_len[s], 1), a.T);      // (a length outside the contract: clamped)
    const float* rec = a.src + s * (long long)a.L * a.S;
    const int n = a.T * a.S;
    auto value = [&](int e) {
        const int t = (int)fastdiv((unsigned)e, a.by_S), c = e - t * a.S;
        return t < ls ? rec[(long long)resample_index(t, li, ls) * a.S + c] : 0.0f;
    };
    float mn = 0.0f, mx = 1.0f;
    if (a.minmax) {
        // numpy's min and max return NaN where the array holds one: kept as a flag, since fminf / fmaxf drop a NaN
        float lo = INFINITY, hi = -INFINITY;
        int nan = 0;
        for (int e = tid; e < n; e += SIGNAL_THREADS) {
            const float v = value(e);
            lo = fminf(lo, v), hi = fmaxf(hi, v), nan |= v != v;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, d)), hi = fmaxf(hi, __shfl_xor(hi, d)), nan |= __shfl_xor(nan, d);
        }
        if (lane == 0) wave_min[wave] = lo, wave_max[wave] = hi, wave_nan[wave] = nan;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < SIGNAL_WAVES; ++w) lo = fminf(lo, wave_min[w]), hi = fmaxf(hi, wave_max[w]), nan |= wave_nan[w];
        mn = nan ? NAN : lo;
        mx = nan ? NAN : hi - mn;                        // the maximum of the shifted array: subtraction is monotone
    }
    if (tid == 0) a.stats[2 * (long long)k] = mn, a.stats[2 * (long long)k + 1] = mx;
    float* dst = a.out + (long long)k * n;
    for (int e = tid; e < n; e += SIGNAL_THREADS) {
        const float v = value(e);
        // the quotient of two floats formed in float64 and rounded once is the correctly rounded float32 quotient, whatever the
        // division the compile flags select for float32 (0 / 0 for a constant signal, as in the reference)
        dst[e] = a.minmax ? (float)((double)(v - mn) / (double)mx) : v;
    }
}

struct EnhanceArgs {
    const float* skel;
    const long long* skel_idx;
    const float* imu;
    const long long* imu_idx;
    const int* src_len;
    const int* dst_len;
    float* out;
    long long lanes;        // b * M * T * (V + S / 3)
    int M, T, V, C, L, S, joints;      // joints = V + S / 3
};

// Lane i owns joint j of frame t of body m of batch row `row`: i = ((row * M + m) * T + t) * joints + j.
template <int C>
__global__ __launch_bounds__(256) void imu_enhance_kernel(EnhanceArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.lanes) return;
    const int j = (int)(i % a.joints);
    const long long frame = i / a.joints;               // (row * M + m) * T + t
    const int t = (int)(frame % a.T);
    const long long rm = frame / a.T;
    const int row = (int)(rm / a.M), m = (int)(rm % a.M);
    float y[3] = {0.0f, 0.0f, 0.0f};
    if (j < a.V) {
        const float* x = a.skel + (((a.skel_idx[row] * a.M + m) * a.T + t) * (long long)a.V + j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = x[c];
    } else {
        const long long s = a.imu_idx[row];
        const int li = min(max(a.src_len[s], 1), a.L), ls = min(max(a.dst_len[s], 1), a.T);
        if (t < ls) {
            const float* x = a.imu + (s * a.L + resample_index(t, li, ls)) * (long long)a.S + (j - a.V) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = x[c];
        }
    }
    float* dst = a.out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = y[c];
}

}  // namespace fgcn

using namespace fgcn;

// the product of positive factors, or -1 once it reaches 2^31 (formed so that no intermediate overflows 64 bits)
static long long elements_below_2_31(std::initializer_list<long long> factors) {
    long long p = 1;
    for (long long f : factors) {
        if (f >= (1ll << 31)) return -1;
        p *= f;
        if (p >= (1ll << 31)) return -1;
    }
    return p;
}

extern "C" int fgcn_resample_index(int t, int src_len, int dst_len, int* out) {
    FGCN_REQUIRE(out, FGCN_E_BADARG, "resample_index: null pointer (out)");
    FGCN_REQUIRE(src_len > 0 && dst_len > 0, FGCN_E_BADARG, "resample_index: bad lengths (%d, %d)", src_len, dst_len);
    *out = resample_index(t, src_len, dst_len);
    return FGCN_OK;
}

extern "C" int fgcn_signal_prepare(const float* src, const long long* idx, const int* src_len, const int* dst_len, float* out, float* stats,
                                   int b, int L, int S, int T, int minmax, void* stream) {
    FGCN_REQUIRE(src && idx && src_len && dst_len && out && stats, FGCN_E_BADARG, "signal_prepare: null pointer");
    FGCN_REQUIRE(b > 0 && L > 0 && S > 0 && T > 0, FGCN_E_BADARG, "signal_prepare: bad b/L/S/T (%d, %d, %d, %d)", b, L, S, T);
    FGCN_REQUIRE(out != src, FGCN_E_BADARG, "signal_prepare: out must not alias src");
    FGCN_REQUIRE(elements_below_2_31({b, T, S}) > 0 && elements_below_2_31({L, S}) > 0, FGCN_E_BADARG,
                 "signal_prepare: (%d, %d, %d) output elements or (%d, %d) elements of a recording are 2^31 or more", b, T, S, L, S);
    SignalArgs a;
    a.src = src, a.idx = idx, a.src_len = src_len, a.dst_len = dst_len, a.out = out, a.stats = stats;
    a.L = L, a.S = S, a.T = T, a.minmax = minmax != 0;
    a.by_S = make_fastdiv((unsigned)S);
    hipLaunchKernelGGL(signal_prepare_kernel, dim3((unsigned)b), dim3(SIGNAL_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("signal_prepare");
}

extern "C" int fgcn_imu_enhance(const float* skel, const long long* skel_idx, const float* imu, const long long* imu_idx, const int* src_len,
                                const int* dst_len, float* out, int b, int M, int T, int V, int C, int L, int S, void* stream) {
    FGCN_REQUIRE(skel && skel_idx && imu && imu_idx && src_len && dst_len && out, FGCN_E_BADARG, "imu_enhance: null pointer");
    FGCN_REQUIRE(b > 0 && M > 0 && T > 0 && V > 0 && L > 0 && S > 0, FGCN_E_BADARG, "imu_enhance: bad b/M/T/V/L/S (%d, %d, %d, %d, %d, %d)", b,
                 M, T, V, L, S);
    FGCN_REQUIRE(C == 2 || C == 3, FGCN_E_BADARG, "imu_enhance: C=%d, expected 2 or 3 coordinates", C);
    FGCN_REQUIRE(S % 3 == 0, FGCN_E_BADARG, "imu_enhance: S=%d values per frame do not form joints of three", S);
    FGCN_REQUIRE(out != skel && out != imu, FGCN_E_BADARG, "imu_enhance: out must not alias skel or imu");
    EnhanceArgs a;
    a.skel = skel, a.skel_idx = skel_idx, a.imu = imu, a.imu_idx = imu_idx, a.src_len = src_len, a.dst_len = dst_len, a.out = out;
    a.M = M, a.T = T, a.V = V, a.C = C, a.L = L, a.S = S;
    const long long joints = (long long)V + S / 3, n = elements_below_2_31({b, M, T, joints, 3});
    FGCN_REQUIRE(n > 0 && elements_below_2_31({M, T, V, C}) > 0 && elements_below_2_31({L, S}) > 0, FGCN_E_BADARG,
                 "imu_enhance: (%d, %d, %d, %lld, 3) output elements, or the elements of a clip or a recording, are 2^31 or more", b, M, T, joints);
    a.lanes = n / 3, a.joints = (int)joints;
    const dim3 grid((unsigned)cdiv(a.lanes, 256));
    if (C == 3) hipLaunchKernelGGL(imu_enhance_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(imu_enhance_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("imu_enhance");
}
