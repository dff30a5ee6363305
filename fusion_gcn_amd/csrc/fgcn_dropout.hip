// Dropout with masks from a counter-based generator (fgcn_rng.hpp; contract in include/fgcn.h).
// The masks are a pure function of (seed, site, step, element index): the forward keeps element i iff word i & 3 of
// philox(ctr = {i >> 2, site, lo32(step), hi32(step)}, key = seed) is >= p * 2^32, and writes the kept bits as an image in the layout
// of fgcn_bn_act's sign image (bit i & 7 of byte i >> 3) for the backward.  `step` is a word in device memory that
// fgcn_rng_advance bumps in a launch of its own behind the forward: a recorded HIP graph draws new masks on every replay without
// the host, and two runs from one state draw the same.
// Pure HBM streams, eight elements per thread: two 16-byte loads, two Philox calls, two 16-byte stores, one byte of the image --
// a byte has one writer.  n % 8 == 4: the last thread owns four elements and the low nibble of the last byte.
#include "fgcn_common.hpp"
#include "fgcn_rng.hpp"

namespace fgcn {

// 16 bytes per lane, plain or non-temporal (`stream`: a kernel argument, fgcn_common.hpp stream_out; as fgcn_elem.hip's 16-byte kernels)
__device__ __forceinline__ f32x4 drop_load4(const float* ptr, int stream) {
    return stream ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ptr)) : *reinterpret_cast<const f32x4*>(ptr);
}
__device__ __forceinline__ void drop_store4(float* ptr, f32x4 val, int stream) {
    if (stream) __builtin_nontemporal_store(val, reinterpret_cast<f32x4*>(ptr));
    else *reinterpret_cast<f32x4*>(ptr) = val;
}

// four elements of group g: -> x * s where kept, 0 elsewhere (selects, no branch), and the four kept bits
__device__ __forceinline__ f32x4 drop4(f32x4 x, unsigned g, unsigned site, unsigned step_lo, unsigned step_hi, unsigned k0, unsigned k1,
                                       unsigned thr, float s, int& bits) {
    const philox4 r = philox4x32_10(g, site, step_lo, step_hi, k0, k1);
    f32x4 y;
    bits = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool keep = r.w[e] >= thr;
        y[e] = keep ? x[e] * s : 0.f;
        bits |= keep ? 1 << e : 0;
    }
    return y;
}

// threads = n8 + (n % 8 == 4): thread i < n8 owns elements 8i .. 8i + 7, thread n8 (if any) the last four
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const float* x, float* y, unsigned char* mask, long long n8, long long threads,
                                                          unsigned thr, float s, unsigned k0, unsigned k1, unsigned site,
                                                          const unsigned long long* step, int stream) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= threads) return;
    const unsigned long long st = *step;
    const unsigned step_lo = (unsigned)st, step_hi = (unsigned)(st >> 32);
    const unsigned g = (unsigned)(i * 2);                // n < 2^34 (host check): the group index fits 32 bits
    const bool full = i < n8;
    const f32x4 a = drop_load4(x + i * 8, stream);
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (full) b = drop_load4(x + i * 8 + 4, stream);
    int lo, hi = 0;
    drop_store4(y + i * 8, drop4(a, g, site, step_lo, step_hi, k0, k1, thr, s, lo), stream);
    if (full) drop_store4(y + i * 8 + 4, drop4(b, g + 1u, site, step_lo, step_hi, k0, k1, thr, s, hi), stream);
    mask[i] = (unsigned char)(lo | (hi << 4));           // (the tail thread: high nibble zero)
}

// dx = kept ? dy * s : 0 from the bit image; dx may be dy (a thread reads its elements before it writes them)
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const float* dy, const unsigned char* mask, float* dx, long long n8, long long threads,
                                                          float s, int stream) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= threads) return;
    const bool full = i < n8;
    const int bits = mask[i];
    const f32x4 a = drop_load4(dy + i * 8, stream);
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (full) b = drop_load4(dy + i * 8 + 4, stream);
    f32x4 ga, gb;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        ga[e] = (bits >> e) & 1 ? a[e] * s : 0.f;
        gb[e] = (bits >> (4 + e)) & 1 ? b[e] * s : 0.f;
    }
    drop_store4(dx + i * 8, ga, stream);
    if (full) drop_store4(dx + i * 8 + 4, gb, stream);
}

// One lane, an ordinary vector store (the address depends on the lane index).  A launch of its own, stream-ordered behind the forward that read
// the word: no workgroup of that forward can see the new value.
__global__ void rng_advance_kernel(unsigned long long* step) {
    unsigned long long* w = step + threadIdx.x;
    *w = *w + 1ull;
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_philox4x32_10(const unsigned ctr[4], const unsigned key[2], unsigned out[4]) {
    FGCN_REQUIRE(ctr && key && out, FGCN_E_BADARG, "philox4x32_10: null pointer");
    const philox4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int e = 0; e < 4; ++e) out[e] = r.w[e];
    return FGCN_OK;
}

static int check_dropout(const char* what, long long n, float p) {
    FGCN_REQUIRE(n > 0 && n % 4 == 0 && n < (1ll << 34), FGCN_E_BADARG, "%s: n=%lld (a positive multiple of 4 below 2^34)", what, n);
    FGCN_REQUIRE(p >= 0.f && p < 1.f, FGCN_E_BADARG, "%s: p=%g outside [0, 1)", what, (double)p);      // (NaN fails both comparisons)
    return FGCN_OK;
}

extern "C" int fgcn_dropout_fwd(const float* x, float* y, unsigned char* keep_mask, long long n, float p, unsigned long long seed,
                                unsigned site, const unsigned long long* step, void* stream) {
    if (int e = check_dropout("dropout_fwd", n, p)) return e;
    FGCN_REQUIRE(x && y && keep_mask && step, FGCN_E_BADARG, "dropout_fwd: null pointer");
    FGCN_REQUIRE(aligned16(x) && aligned16(y), FGCN_E_BADARG, "dropout_fwd: x and y must be 16-byte aligned");
    FGCN_REQUIRE((reinterpret_cast<uintptr_t>(step) & 7u) == 0, FGCN_E_BADARG, "dropout_fwd: step must be 8-byte aligned");
    const unsigned thr = (unsigned)((double)p * 4294967296.0);
    const float s = 1.0f / (1.0f - p);
    const long long n8 = n / 8, threads = n8 + (n % 8 ? 1 : 0);
    hipLaunchKernelGGL(dropout_fwd_kernel, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, x, y, keep_mask, n8, threads,
                       thr, s, (unsigned)seed, (unsigned)(seed >> 32), site, step, fgcn::stream_out(n * 4) ? 1 : 0);
    return launch_status("dropout_fwd");
}

extern "C" int fgcn_dropout_bwd(const float* dy, const unsigned char* keep_mask, float* dx, long long n, float p, void* stream) {
    if (int e = check_dropout("dropout_bwd", n, p)) return e;
    FGCN_REQUIRE(dy && keep_mask && dx, FGCN_E_BADARG, "dropout_bwd: null pointer");
    FGCN_REQUIRE(aligned16(dy) && aligned16(dx), FGCN_E_BADARG, "dropout_bwd: dy and dx must be 16-byte aligned");
    const float s = 1.0f / (1.0f - p);
    const long long n8 = n / 8, threads = n8 + (n % 8 ? 1 : 0);
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, dy, keep_mask, dx, n8, threads,
                       s, fgcn::stream_out(n * 4) ? 1 : 0);
    return launch_status("dropout_bwd");
}

extern "C" int fgcn_rng_advance(unsigned long long* step, void* stream) {
    FGCN_REQUIRE(step && (reinterpret_cast<uintptr_t>(step) & 7u) == 0, FGCN_E_BADARG, "rng_advance: step must be a non-null, 8-byte aligned pointer");
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    return launch_status("rng_advance");
}
