// The STC (spatial-temporal-channel) attention module of MS-AAGCN between the graph convolution and the temporal convolution of an AGCN
// block (contract in include/fgcn.h, "STC attention").  G (B, T, V, C) float32 channels-last, C in 64s, V <= 64.
//
//   forward    stc_mean_t    (a)  mt[b, v, c] = mean_t G                                   one pass over G
//              stc_gate_s         s = sigmoid(conv_sa(mt))                                 one workgroup per sample
//              stc_mean_v    (b)  m[b, t, c] = mean_v G (1 + s)                            one pass over G
//              stc_gates_tc       tg = sigmoid(conv_ta(m)), cm = mean_t (1 + tg) m, h, cg  one workgroup per sample
//              stc_apply     (c)  G' = G (1 + s)(1 + tg)(1 + cg)                           one pass over G, one store
//   backward   stc_bwd_qr    (A)  q[b, t, c] = sum_v p (1 + s), r[b, v, c] = sum_t p (1 + tg), p = dG' G       one pass over dG' and G
//              stc_bwd_tc         channel gate and conv_ta back to dm[b, t, c]             one workgroup per sample
//              stc_bwd_ds    (B)  ds[b, v] += sum_{t, c} dm G / V                          one pass over G
//              stc_bwd_s          conv_sa back to dmt[b, v, c]                             one workgroup per sample
//              stc_bwd_apply (C)  dG = dG' (1 + s)(1 + tg)(1 + cg) + dm (1 + s) / V + dmt / T
//              stc_param_grads    the eight parameter gradients: sums over the samples in sample order
//
// Every sum has one order, fixed by the shape alone: a lane adds its terms in index order, lanes are combined by the xor butterfly of
// wave_sum, waves through LDS in wave order, the frame splits of the two backward reductions in split order (the split count depends on
// (B, T) only) and samples in sample order.  No atomics.  No forward kernel reads another sample's data.  Nothing is skipped on a value:
// a NaN reaches exactly the sums the definition gives it; the two gate convolutions and their weight gradients
// multiply the zero padding (0 . NaN = NaN, as the reference's do), the data gradients have no padded term.
//
// Lane = channel in the reductions (a wave reads 256 contiguous bytes of a row), 16-byte accesses in the three elementwise passes.
// The small kernels hand their intermediate vectors to their own later stages through global memory (they are results the backward reads
// anyway) with a workgroup barrier in between.
#include <cmath>

#include "fgcn_common.hpp"

namespace fgcn {

constexpr int STC_THREADS = 256, STC_WAVES = STC_THREADS / 64;
// the four kernels that run one workgroup per sample: 16 waves, so that a batch of 128 samples still fills the chip's wave slots
constexpr int STC_SMALL_THREADS = 1024, STC_SMALL_WAVES = STC_SMALL_THREADS / 64;
constexpr int STC_TA_TAPS = 9, STC_TA_PAD = 4;
constexpr int STC_TILE_ROWS = 128;       // (frame, joint) rows of 64 channels one stc_bwd_qr stage holds in LDS: 4 frames of <= 32 joints, 2 of <= 64

__device__ __forceinline__ float stc_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// out[c] = sum over r < rows of term(r, c), c < cols: wave w adds rows w, w + 16, .. in order, the sixteen partial sums are added in wave
// order.  Called by the whole workgroup of STC_SMALL_THREADS; ends with a barrier (what `store` wrote is visible to the workgroup afterwards).
template <class Term, class Store>
__device__ __forceinline__ void stc_col_reduce(int rows, int cols, float (*part)[64], Term term, Store store) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c0 = 0; c0 < cols; c0 += 64) {
        const int c = c0 + lane;
        float acc = 0.f;
        if (c < cols)
            for (int r = w; r < rows; r += STC_SMALL_WAVES) acc += term(r, c);
        part[w][lane] = acc;
        __syncthreads();
        if (w == 0 && c < cols) {
            float sum = part[0][lane];
#pragma unroll
            for (int i = 1; i < STC_SMALL_WAVES; ++i) sum += part[i][lane];
            store(c, sum);
        }
        __syncthreads();
    }
}

// ---- forward (a): mt = mean_t G -----------------------------------------------------------------------------------------------------
struct StcMeanTArgs {
    const float* g;
    float* mt;
    int T;
    unsigned vc4;        // V * C / 4
};

// grid (ceil(vc4 / 64), B), block (64, 4): thread (x, y) adds frames y, y + 4, .. of 16-byte group x
__global__ __launch_bounds__(STC_THREADS) void stc_mean_t_kernel(StcMeanTArgs a) {
    __shared__ f32x4 part[STC_WAVES][64];
    const unsigned e = blockIdx.x * 64u + threadIdx.x;
    const int y = threadIdx.y;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (e < a.vc4) {
        const f32x4* base = reinterpret_cast<const f32x4*>(a.g) + (long long)blockIdx.y * a.T * a.vc4 + e;
#pragma unroll 4
        for (int t = y; t < a.T; t += STC_WAVES) acc += base[(long long)t * a.vc4];
    }
    part[y][threadIdx.x] = acc;
    __syncthreads();
    if (y == 0 && e < a.vc4) {
        const f32x4 s = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        reinterpret_cast<f32x4*>(a.mt)[(long long)blockIdx.y * a.vc4 + e] = s / (float)a.T;
    }
}

// ---- s = sigmoid(conv_sa(mt)) -------------------------------------------------------------------------------------------------------
struct StcGateSArgs {
    const float* mt;
    const float* w;      // (1, C, k)
    const float* bias;   // (1)
    float* s;
    int V, C, k, p;
};

__global__ __launch_bounds__(STC_SMALL_THREADS) void stc_gate_s_kernel(StcGateSArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* mt = a.mt + (long long)b * a.V * a.C;
    for (int v = w; v < a.V; v += STC_SMALL_WAVES) {
        float acc = 0.f;
        for (int c = lane; c < a.C; c += 64) {
            const float* wc = a.w + (long long)c * a.k;
            for (int j = 0; j < a.k; ++j) {
                const int u = v + j - a.p;       // (a tap beyond the joints multiplies the padding's zero: nothing is skipped)
                acc = fmaf(wc[j], (u >= 0 && u < a.V) ? mt[u * a.C + c] : 0.f, acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) a.s[(long long)b * a.V + v] = stc_sigmoid(acc + a.bias[0]);
    }
}

// ---- forward (b): m = mean_v G (1 + s) ----------------------------------------------------------------------------------------------
struct StcMeanVArgs {
    const float* g;
    const float* s;
    float* m;
    int T, V, C4;
    unsigned tc4;        // T * C / 4
    FastDiv by_c4;
};

// grid (ceil(tc4 / 256), B): one thread per (frame, 16-byte channel group)
__global__ __launch_bounds__(STC_THREADS) void stc_mean_v_kernel(StcMeanVArgs a) {
    const unsigned e = blockIdx.x * (unsigned)STC_THREADS + threadIdx.x;
    if (e >= a.tc4) return;
    const int b = blockIdx.y;
    const unsigned t = fastdiv(e, a.by_c4), c4 = e - t * (unsigned)a.C4;
    const f32x4* base = reinterpret_cast<const f32x4*>(a.g) + ((long long)b * a.T + t) * a.V * a.C4 + c4;
    const float* s = a.s + (long long)b * a.V;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
    for (int v = 0; v < a.V; ++v) acc += base[(long long)v * a.C4] * (1.0f + s[v]);
    reinterpret_cast<f32x4*>(a.m)[(long long)b * a.tc4 + e] = acc / (float)a.V;
}

// ---- tg, cm, h, cg from m -----------------------------------------------------------------------------------------------------------
struct StcGatesTCArgs {
    const float* m;
    const float *w_ta, *b_ta;    // (1, C, 9), (1)
    const float *w1, *b1;        // (C / 2, C), (C / 2)
    const float *w2, *b2;        // (C, C / 2), (C)
    float *tg, *cm, *h, *cg;
    int T, C;
};

__global__ __launch_bounds__(STC_SMALL_THREADS) void stc_gates_tc_kernel(StcGatesTCArgs a) {
    __shared__ float part[STC_SMALL_WAVES][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int T = a.T, C = a.C, C2 = a.C / 2;
    const float* m = a.m + (long long)b * T * C;
    float *tg = a.tg + (long long)b * T, *cm = a.cm + (long long)b * C, *h = a.h + (long long)b * C2, *cg = a.cg + (long long)b * C;
    for (int t = w; t < T; t += STC_SMALL_WAVES) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float* wc = a.w_ta + c * STC_TA_TAPS;
#pragma unroll
            for (int j = 0; j < STC_TA_TAPS; ++j) {
                const int u = t + j - STC_TA_PAD;
                acc = fmaf(wc[j], (u >= 0 && u < T) ? m[(long long)u * C + c] : 0.f, acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) tg[t] = stc_sigmoid(acc + a.b_ta[0]);
    }
    __syncthreads();
    stc_col_reduce(T, C, part, [&](int t, int c) { return (1.0f + tg[t]) * m[(long long)t * C + c]; },
                   [&](int c, float sum) { cm[c] = sum / (float)T; });
    for (int j = w; j < C2; j += STC_SMALL_WAVES) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(a.w1[(long long)j * C + c], cm[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) h[j] = relu_nan(acc + a.b1[j]);
    }
    __syncthreads();
    for (int c = w; c < C; c += STC_SMALL_WAVES) {
        float acc = 0.f;
        for (int j = lane; j < C2; j += 64) acc = fmaf(a.w2[(long long)c * C2 + j], h[j], acc);
        acc = wave_sum(acc);
        if (lane == 0) cg[c] = stc_sigmoid(acc + a.b2[c]);
    }
}

// ---- forward (c) and backward (C): the two elementwise passes -------------------------------------------------------------------------
struct StcApplyArgs {
    const float* in;             // G (forward), dG' (backward)
    const float *s, *tg, *cg;
    const float *dm, *dmt;       // backward only
    float* out;
    int T, V, C4;
    unsigned per_sample;         // T * V * C / 4
    FastDiv by_vc4, by_c4;
};

// grid (ceil(per_sample / 256), B): one thread per 16 bytes.  BWD: out = in (1 + s)(1 + tg)(1 + cg) + dm (1 + s) / V + dmt / T
template <int BWD>
__global__ __launch_bounds__(STC_THREADS) void stc_apply_kernel(StcApplyArgs a) {
    const unsigned e = blockIdx.x * (unsigned)STC_THREADS + threadIdx.x;
    if (e >= a.per_sample) return;
    const int b = blockIdx.y;
    const unsigned t = fastdiv(e, a.by_vc4), rem = e - t * (unsigned)(a.V * a.C4);
    const unsigned v = fastdiv(rem, a.by_c4), c4 = rem - v * (unsigned)a.C4;
    const long long at = (long long)b * a.per_sample + e;
    const float av = 1.0f + a.s[(long long)b * a.V + v], et = 1.0f + a.tg[(long long)b * a.T + t];
    const f32x4 fc = reinterpret_cast<const f32x4*>(a.cg)[(long long)b * a.C4 + c4] + 1.0f;
    f32x4 r = ((reinterpret_cast<const f32x4*>(a.in)[at] * av) * et) * fc;
    if constexpr (BWD) {
        const f32x4 dm = reinterpret_cast<const f32x4*>(a.dm)[((long long)b * a.T + t) * a.C4 + c4];
        const f32x4 dmt = reinterpret_cast<const f32x4*>(a.dmt)[((long long)b * a.V + v) * a.C4 + c4];
        r += dm * (av / (float)a.V) + dmt / (float)a.T;
    }
    reinterpret_cast<f32x4*>(a.out)[at] = r;
}

// ---- backward (A): q and the per-split partial sums of r ----------------------------------------------------------------------------
struct StcBwdQRArgs {
    const float *dout, *g, *s, *tg;
    float *q, *rpart;            // (B, T, C), (B, nsplit, V, C)
    int T, V, C, fps, nsplit, TC;        // fps: frames per split; TC: frames per LDS stage (TC * V <= STC_TILE_ROWS, TC <= 4)
};

// grid (C / 64, nsplit, B).  Wave w owns joints w, w + 4, .. (NI of them at most), lane = channel of the 64-channel slab.  Per stage of TC
// frames: p = dG' G is formed once, p (1 + tg) goes into the lane's r accumulators, p (1 + s) into LDS; then thread (frame w, channel
// lane) adds its frame's joints in joint order -> q.
template <int NI>
__global__ __launch_bounds__(STC_THREADS) void stc_bwd_qr_kernel(StcBwdQRArgs a) {
    __shared__ float tile[STC_TILE_ROWS * 64];
    const int slab = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = slab * 64 + lane;
    const int T = a.T, V = a.V, C = a.C;
    const int t0 = split * a.fps, t1 = min(T, t0 + a.fps);
    const float *s = a.s + (long long)b * V, *tg = a.tg + (long long)b * T;
    float racc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) racc[i] = 0.f;
    for (int tc0 = t0; tc0 < t1; tc0 += a.TC) {
        const int n = min(a.TC, t1 - tc0);
        for (int tl = 0; tl < n; ++tl) {
            const int t = tc0 + tl;
            const float et = 1.0f + tg[t];
            const long long row0 = ((long long)b * T + t) * V;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int v = w + STC_WAVES * i;
                if (v < V) {
                    const long long off = (row0 + v) * C + c;
                    const float p = a.dout[off] * a.g[off];
                    racc[i] = fmaf(p, et, racc[i]);
                    tile[(tl * V + v) * 64 + lane] = p * (1.0f + s[v]);
                }
            }
        }
        __syncthreads();
        if (w < n) {
            float acc = 0.f;
            for (int v = 0; v < V; ++v) acc += tile[(w * V + v) * 64 + lane];
            a.q[((long long)b * T + tc0 + w) * C + c] = acc;
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int v = w + STC_WAVES * i;
        if (v < V) a.rpart[(((long long)b * a.nsplit + split) * V + v) * C + c] = racc[i];
    }
}

// ---- backward, small kernel 1: the channel gate and conv_ta -----------------------------------------------------------------------------
struct StcBwdTCArgs {
    const float *q, *m, *tg, *cg, *cm, *h;
    const float *w_ta, *w1, *w2;
    float *dzc, *dhpre, *dcm, *dzt, *dm;         // (B, C), (B, C / 2), (B, C), (B, T), (B, T, C)
    float *dwta_part, *dbta_part;                // (B, C, 9), (B)
    int T, C;
};

__global__ __launch_bounds__(STC_SMALL_THREADS) void stc_bwd_tc_kernel(StcBwdTCArgs a) {
    __shared__ float part[STC_SMALL_WAVES][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int T = a.T, C = a.C, C2 = a.C / 2;
    const float *q = a.q + (long long)b * T * C, *m = a.m + (long long)b * T * C, *tg = a.tg + (long long)b * T;
    const float *cg = a.cg + (long long)b * C, *h = a.h + (long long)b * C2;
    float *dzc = a.dzc + (long long)b * C, *dhpre = a.dhpre + (long long)b * C2, *dcm = a.dcm + (long long)b * C;
    float *dzt = a.dzt + (long long)b * T, *dm = a.dm + (long long)b * T * C;
    const float inv_t = 1.0f / (float)T;
    // dcg[c] = sum_t (1 + tg) q;  through the sigmoid
    stc_col_reduce(T, C, part, [&](int t, int c) { return (1.0f + tg[t]) * q[(long long)t * C + c]; },
                   [&](int c, float sum) { dzc[c] = sum * (cg[c] * (1.0f - cg[c])); });
    // dh = W2^T dzc, gated by the ReLU (a NaN h passes the gradient on, as torch's does)
    stc_col_reduce(C, C2, part, [&](int c, int j) { return a.w2[(long long)c * C2 + j] * dzc[c]; },
                   [&](int j, float sum) { dhpre[j] = relu_open(h[j]) ? sum : 0.f; });
    // dcm = W1^T dhpre
    stc_col_reduce(C2, C, part, [&](int j, int c) { return a.w1[(long long)j * C + c] * dhpre[j]; }, [&](int c, float sum) { dcm[c] = sum; });
    // dtg[t] = sum_c (1 + cg) q + dcm m / T;  through the sigmoid
    for (int t = w; t < T; t += STC_SMALL_WAVES) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += (1.0f + cg[c]) * q[(long long)t * C + c] + dcm[c] * m[(long long)t * C + c] * inv_t;
        acc = wave_sum(acc);
        if (lane == 0) dzt[t] = acc * (tg[t] * (1.0f - tg[t]));
    }
    __syncthreads();
    // dm[t, c] = dcm (1 + tg) / T + sum_j w_ta[c, j] dzt[t - j + 4]
    for (int e = threadIdx.x; e < T * C; e += STC_SMALL_THREADS) {
        const int t = e / C, c = e - t * C;
        float acc = dcm[c] * (1.0f + tg[t]) * inv_t;
        const float* wc = a.w_ta + c * STC_TA_TAPS;
#pragma unroll
        for (int j = 0; j < STC_TA_TAPS; ++j) {
            const int u = t - j + STC_TA_PAD;
            if (u >= 0 && u < T) acc = fmaf(wc[j], dzt[u], acc);
        }
        dm[e] = acc;
    }
    // this sample's terms of conv_ta's gradients
    for (int j = 0; j < STC_TA_TAPS; ++j)
        stc_col_reduce(T, C, part,
                       [&](int t, int c) {
                           const int u = t + j - STC_TA_PAD;
                           return dzt[t] * ((u >= 0 && u < T) ? m[(long long)u * C + c] : 0.f);
                       },
                       [&](int c, float sum) { a.dwta_part[((long long)b * C + c) * STC_TA_TAPS + j] = sum; });
    if (w == 0) {
        float acc = 0.f;
        for (int t = lane; t < T; t += 64) acc += dzt[t];
        acc = wave_sum(acc);
        if (lane == 0) a.dbta_part[b] = acc;
    }
}

// ---- backward (B): the per-split partial sums of sum_{t, c} dm G --------------------------------------------------------------------
struct StcBwdDsArgs {
    const float *dm, *g;
    float* dspart;               // (B, nsplit, V)
    int T, V, C, fps, nsplit;
};

// grid (nsplit, B): wave w owns joints w, w + 4, ..; lane = channel, over all 64-channel slabs and the split's frames
template <int NI>
__global__ __launch_bounds__(STC_THREADS) void stc_bwd_ds_kernel(StcBwdDsArgs a) {
    const int split = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int T = a.T, V = a.V, C = a.C;
    const int t0 = split * a.fps, t1 = min(T, t0 + a.fps);
    float acc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = 0.f;
    for (int t = t0; t < t1; ++t) {
        const long long row0 = ((long long)b * T + t) * V;
        for (int c = lane; c < C; c += 64) {
            const float d = a.dm[((long long)b * T + t) * C + c];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int v = w + STC_WAVES * i;
                if (v < V) acc[i] = fmaf(d, a.g[(row0 + v) * C + c], acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int v = w + STC_WAVES * i;       // (uniform over the wave)
        if (v < V) {
            const float sum = wave_sum(acc[i]);
            if (lane == 0) a.dspart[((long long)b * a.nsplit + split) * V + v] = sum;
        }
    }
}

// ---- backward, small kernel 2: conv_sa ----------------------------------------------------------------------------------------------
struct StcBwdSArgs {
    const float *rpart, *dspart, *cg, *s, *mt, *w_sa;
    float *dzs, *dmt;                            // (B, V), (B, V, C)
    float *dwsa_part, *dbsa_part;                // (B, C, k), (B)
    int V, C, k, p, nsplit;
};

__global__ __launch_bounds__(STC_SMALL_THREADS) void stc_bwd_s_kernel(StcBwdSArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int V = a.V, C = a.C, k = a.k, p = a.p, ns = a.nsplit;
    const float *cg = a.cg + (long long)b * C, *s = a.s + (long long)b * V, *mt = a.mt + (long long)b * V * C;
    float *dzs = a.dzs + (long long)b * V, *dmt = a.dmt + (long long)b * V * C;
    // ds[v] = sum_c (1 + cg) r[v, c] + (sum_{t, c} dm G) / V, both from their split partials in split order;  through the sigmoid
    for (int v = w; v < V; v += STC_SMALL_WAVES) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) {
            float r = 0.f;
            for (int i = 0; i < ns; ++i) r += a.rpart[(((long long)b * ns + i) * V + v) * C + c];
            acc = fmaf(1.0f + cg[c], r, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            float d = 0.f;
            for (int i = 0; i < ns; ++i) d += a.dspart[((long long)b * ns + i) * V + v];
            dzs[v] = (acc + d / (float)V) * (s[v] * (1.0f - s[v]));
        }
    }
    __syncthreads();
    // dmt[u, c] = sum_j w_sa[c, j] dzs[u - j + p]
    for (int e = threadIdx.x; e < V * C; e += STC_SMALL_THREADS) {
        const int u = e / C, c = e - u * C;
        const float* wc = a.w_sa + (long long)c * k;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) {
            const int v = u - j + p;
            if (v >= 0 && v < V) acc = fmaf(wc[j], dzs[v], acc);
        }
        dmt[e] = acc;
    }
    // this sample's terms of conv_sa's gradients (consecutive lanes: consecutive channels of one tap)
    for (int e = threadIdx.x; e < k * C; e += STC_SMALL_THREADS) {
        const int j = e / C, c = e - j * C;
        float acc = 0.f;
        for (int v = 0; v < V; ++v) {
            const int u = v + j - p;
            acc = fmaf(dzs[v], (u >= 0 && u < V) ? mt[u * C + c] : 0.f, acc);
        }
        a.dwsa_part[((long long)b * C + c) * k + j] = acc;
    }
    if (w == 0) {
        const float acc = wave_sum(lane < V ? dzs[lane] : 0.f);      // (V <= 64)
        if (lane == 0) a.dbsa_part[b] = acc;
    }
}

// ---- the eight parameter gradients ----------------------------------------------------------------------------------------------------
struct StcParamGradArgs {
    const float *dzc, *dhpre, *cm, *h, *dwta_part, *dbta_part, *dwsa_part, *dbsa_part;
    float *d_wsa, *d_bsa, *d_wta, *d_bta, *d_w1, *d_b1, *d_w2, *d_b2;
    int B, C, k;
};

// one thread per gradient element, the samples added in sample order
__global__ __launch_bounds__(STC_THREADS) void stc_param_grads_kernel(StcParamGradArgs a) {
    const int B = a.B, C = a.C, C2 = a.C / 2;
    long long e = (long long)blockIdx.x * STC_THREADS + threadIdx.x;
    float acc = 0.f;
    if (e < (long long)C * C2) {             // d fc2c.weight[c, j] = sum_b dzc[b, c] h[b, j]
        const int c = (int)(e / C2), j = (int)(e - (long long)c * C2);
        for (int b = 0; b < B; ++b) acc = fmaf(a.dzc[(long long)b * C + c], a.h[(long long)b * C2 + j], acc);
        a.d_w2[e] = acc;
        return;
    }
    e -= (long long)C * C2;
    if (e < (long long)C2 * C) {             // d fc1c.weight[j, c] = sum_b dhpre[b, j] cm[b, c]
        const int j = (int)(e / C), c = (int)(e - (long long)j * C);
        for (int b = 0; b < B; ++b) acc = fmaf(a.dhpre[(long long)b * C2 + j], a.cm[(long long)b * C + c], acc);
        a.d_w1[e] = acc;
        return;
    }
    e -= (long long)C2 * C;
    const long long n_ta = (long long)C * STC_TA_TAPS, n_sa = (long long)C * a.k;
    const float* src;
    float* dst;
    long long ld;
    if (e < C) src = a.dzc, dst = a.d_b2, ld = C;
    else if ((e -= C) < C2) src = a.dhpre, dst = a.d_b1, ld = C2;
    else if ((e -= C2) < n_ta) src = a.dwta_part, dst = a.d_wta, ld = n_ta;
    else if ((e -= n_ta) < n_sa) src = a.dwsa_part, dst = a.d_wsa, ld = n_sa;
    else if ((e -= n_sa) < 1) src = a.dbta_part, dst = a.d_bta, ld = 1;
    else if ((e -= 1) < 1) src = a.dbsa_part, dst = a.d_bsa, ld = 1;
    else return;
    for (int b = 0; b < B; ++b) acc += src[(long long)b * ld + e];
    dst[e] = acc;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static int stc_check_dims(const char* what, int B, int T, int V, int C) {
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0 && V > 0 && V <= FGCN_MAX_V_WIDE, FGCN_E_BADARG, "%s: bad B/T/V (%d, %d, %d): B <= 65535, V <= %d", what,
                 B, T, V, FGCN_MAX_V_WIDE);
    FGCN_REQUIRE(C > 0 && C % 64 == 0, FGCN_E_BADARG, "%s: C = %d is not a multiple of 64", what, C);
    // a lane's index inside a sample is 32-bit and goes through FastDiv (exact below 2^29 16-byte groups)
    FGCN_REQUIRE((long long)T * V * C < (1ll << 31), FGCN_E_BADARG, "%s: T * V * C = %d * %d * %d elements in a sample are more than a lane indexes",
                 what, T, V, C);
    return FGCN_OK;
}

static int stc_sa_kernel(int V) { return V % 2 ? V : V - 1; }

static int stc_split_frames(int B, int T) {      // frames per split: about 1024 workgroups, at least 4 frames each
    const long long want = cdiv(1024, B), nsplit = want < 1 ? 1 : (want > cdiv(T, 4) ? cdiv(T, 4) : want);
    return (int)cdiv(T, nsplit);
}

}  // namespace fgcn

using namespace fgcn;

#define STC_ALIGNED(what, ...)                                                                                   \
    do {                                                                                                         \
        const void* ptrs_[] = {__VA_ARGS__};                                                                     \
        for (const void* p_ : ptrs_) FGCN_REQUIRE(aligned16(p_), FGCN_E_ALIGN, what ": a tensor is not 16-byte aligned"); \
    } while (0)

extern "C" int fgcn_stc_splits(int B, int T) {
    if (B <= 0 || T <= 0) return 0;
    return (int)cdiv(T, stc_split_frames(B, T));
}

extern "C" int fgcn_stc_mean_t(const float* g, float* mt, int B, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(g && mt, FGCN_E_BADARG, "stc_mean_t: null pointer");
    if (int e = stc_check_dims("stc_mean_t", B, T, V, C)) return e;
    STC_ALIGNED("stc_mean_t", g, mt);
    StcMeanTArgs a;
    a.g = g, a.mt = mt, a.T = T, a.vc4 = (unsigned)(V * C / 4);
    hipLaunchKernelGGL(stc_mean_t_kernel, dim3((unsigned)cdiv(a.vc4, 64), (unsigned)B), dim3(64, STC_WAVES), 0, (hipStream_t)stream, a);
    return launch_status("stc_mean_t");
}

extern "C" int fgcn_stc_gate_s(const float* mt, const float* w_sa, const float* b_sa, float* s, int B, int V, int C, void* stream) {
    FGCN_REQUIRE(mt && w_sa && b_sa && s, FGCN_E_BADARG, "stc_gate_s: null pointer");
    if (int e = stc_check_dims("stc_gate_s", B, 1, V, C)) return e;
    StcGateSArgs a;
    a.mt = mt, a.w = w_sa, a.bias = b_sa, a.s = s, a.V = V, a.C = C, a.k = stc_sa_kernel(V), a.p = (a.k - 1) / 2;
    hipLaunchKernelGGL(stc_gate_s_kernel, dim3((unsigned)B), dim3(STC_SMALL_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_gate_s");
}

extern "C" int fgcn_stc_mean_v(const float* g, const float* s, float* m, int B, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(g && s && m, FGCN_E_BADARG, "stc_mean_v: null pointer");
    if (int e = stc_check_dims("stc_mean_v", B, T, V, C)) return e;
    STC_ALIGNED("stc_mean_v", g, m);
    StcMeanVArgs a;
    a.g = g, a.s = s, a.m = m, a.T = T, a.V = V, a.C4 = C / 4, a.tc4 = (unsigned)(T * (C / 4)), a.by_c4 = make_fastdiv((unsigned)(C / 4));
    hipLaunchKernelGGL(stc_mean_v_kernel, dim3((unsigned)cdiv(a.tc4, STC_THREADS), (unsigned)B), dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_mean_v");
}

extern "C" int fgcn_stc_gates_tc(const float* m, const float* w_ta, const float* b_ta, const float* w1, const float* b1, const float* w2,
                                 const float* b2, float* tg, float* cm, float* h, float* cg, int B, int T, int C, void* stream) {
    FGCN_REQUIRE(m && w_ta && b_ta && w1 && b1 && w2 && b2 && tg && cm && h && cg, FGCN_E_BADARG, "stc_gates_tc: null pointer");
    if (int e = stc_check_dims("stc_gates_tc", B, T, 1, C)) return e;
    StcGatesTCArgs a;
    a.m = m, a.w_ta = w_ta, a.b_ta = b_ta, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.tg = tg, a.cm = cm, a.h = h, a.cg = cg, a.T = T, a.C = C;
    hipLaunchKernelGGL(stc_gates_tc_kernel, dim3((unsigned)B), dim3(STC_SMALL_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_gates_tc");
}

static void stc_apply_args(StcApplyArgs& a, int T, int V, int C) {
    a.T = T, a.V = V, a.C4 = C / 4, a.per_sample = (unsigned)((long long)T * V * (C / 4));
    a.by_vc4 = make_fastdiv((unsigned)(V * (C / 4))), a.by_c4 = make_fastdiv((unsigned)(C / 4));
}

extern "C" int fgcn_stc_apply(const float* g, const float* s, const float* tg, const float* cg, float* out, int B, int T, int V, int C,
                              void* stream) {
    FGCN_REQUIRE(g && s && tg && cg && out, FGCN_E_BADARG, "stc_apply: null pointer");
    if (int e = stc_check_dims("stc_apply", B, T, V, C)) return e;
    STC_ALIGNED("stc_apply", g, cg, out);
    StcApplyArgs a;
    a.in = g, a.s = s, a.tg = tg, a.cg = cg, a.dm = nullptr, a.dmt = nullptr, a.out = out;
    stc_apply_args(a, T, V, C);
    hipLaunchKernelGGL(stc_apply_kernel<0>, dim3((unsigned)cdiv(a.per_sample, STC_THREADS), (unsigned)B), dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_apply");
}

extern "C" int fgcn_stc_bwd_qr(const float* dout, const float* g, const float* s, const float* tg, float* q, float* rpart, int B, int T, int V,
                               int C, void* stream) {
    FGCN_REQUIRE(dout && g && s && tg && q && rpart, FGCN_E_BADARG, "stc_bwd_qr: null pointer");
    if (int e = stc_check_dims("stc_bwd_qr", B, T, V, C)) return e;
    StcBwdQRArgs a;
    a.dout = dout, a.g = g, a.s = s, a.tg = tg, a.q = q, a.rpart = rpart, a.T = T, a.V = V, a.C = C;
    a.fps = stc_split_frames(B, T), a.nsplit = (int)cdiv(T, a.fps), a.TC = V <= 32 ? 4 : 2;
    const dim3 grid((unsigned)(C / 64), (unsigned)a.nsplit, (unsigned)B);
    FGCN_REQUIRE(a.nsplit <= 65535, FGCN_E_BADARG, "stc_bwd_qr: %d frame splits are more than one grid holds", a.nsplit);
    if (V <= 32) hipLaunchKernelGGL(stc_bwd_qr_kernel<8>, grid, dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(stc_bwd_qr_kernel<16>, grid, dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_bwd_qr");
}

extern "C" int fgcn_stc_bwd_tc(const float* q, const float* m, const float* tg, const float* cg, const float* cm, const float* h,
                               const float* w_ta, const float* w1, const float* w2, float* dzc, float* dhpre, float* dcm, float* dzt, float* dm,
                               float* dwta_part, float* dbta_part, int B, int T, int C, void* stream) {
    FGCN_REQUIRE(q && m && tg && cg && cm && h && w_ta && w1 && w2 && dzc && dhpre && dcm && dzt && dm && dwta_part && dbta_part, FGCN_E_BADARG,
                 "stc_bwd_tc: null pointer");
    if (int e = stc_check_dims("stc_bwd_tc", B, T, 1, C)) return e;
    StcBwdTCArgs a;
    a.q = q, a.m = m, a.tg = tg, a.cg = cg, a.cm = cm, a.h = h, a.w_ta = w_ta, a.w1 = w1, a.w2 = w2;
    a.dzc = dzc, a.dhpre = dhpre, a.dcm = dcm, a.dzt = dzt, a.dm = dm, a.dwta_part = dwta_part, a.dbta_part = dbta_part, a.T = T, a.C = C;
    hipLaunchKernelGGL(stc_bwd_tc_kernel, dim3((unsigned)B), dim3(STC_SMALL_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_bwd_tc");
}

extern "C" int fgcn_stc_bwd_ds(const float* dm, const float* g, float* dspart, int B, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(dm && g && dspart, FGCN_E_BADARG, "stc_bwd_ds: null pointer");
    if (int e = stc_check_dims("stc_bwd_ds", B, T, V, C)) return e;
    StcBwdDsArgs a;
    a.dm = dm, a.g = g, a.dspart = dspart, a.T = T, a.V = V, a.C = C, a.fps = stc_split_frames(B, T), a.nsplit = (int)cdiv(T, a.fps);
    const dim3 grid((unsigned)a.nsplit, (unsigned)B);
    if (V <= 32) hipLaunchKernelGGL(stc_bwd_ds_kernel<8>, grid, dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(stc_bwd_ds_kernel<16>, grid, dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_bwd_ds");
}

extern "C" int fgcn_stc_bwd_s(const float* rpart, const float* dspart, const float* cg, const float* s, const float* mt, const float* w_sa,
                              float* dzs, float* dmt, float* dwsa_part, float* dbsa_part, int B, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(rpart && dspart && cg && s && mt && w_sa && dzs && dmt && dwsa_part && dbsa_part, FGCN_E_BADARG, "stc_bwd_s: null pointer");
    if (int e = stc_check_dims("stc_bwd_s", B, T, V, C)) return e;
    StcBwdSArgs a;
    a.rpart = rpart, a.dspart = dspart, a.cg = cg, a.s = s, a.mt = mt, a.w_sa = w_sa, a.dzs = dzs, a.dmt = dmt, a.dwsa_part = dwsa_part;
    a.dbsa_part = dbsa_part, a.V = V, a.C = C, a.k = stc_sa_kernel(V), a.p = (a.k - 1) / 2, a.nsplit = fgcn_stc_splits(B, T);
    hipLaunchKernelGGL(stc_bwd_s_kernel, dim3((unsigned)B), dim3(STC_SMALL_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_bwd_s");
}

extern "C" int fgcn_stc_bwd_apply(const float* dout, const float* s, const float* tg, const float* cg, const float* dm, const float* dmt,
                                  float* dg, int B, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(dout && s && tg && cg && dm && dmt && dg, FGCN_E_BADARG, "stc_bwd_apply: null pointer");
    if (int e = stc_check_dims("stc_bwd_apply", B, T, V, C)) return e;
    STC_ALIGNED("stc_bwd_apply", dout, cg, dm, dmt, dg);
    StcApplyArgs a;
    a.in = dout, a.s = s, a.tg = tg, a.cg = cg, a.dm = dm, a.dmt = dmt, a.out = dg;
    stc_apply_args(a, T, V, C);
    hipLaunchKernelGGL(stc_apply_kernel<1>, dim3((unsigned)cdiv(a.per_sample, STC_THREADS), (unsigned)B), dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_bwd_apply");
}

extern "C" int fgcn_stc_param_grads(const float* dzc, const float* dhpre, const float* cm, const float* h, const float* dwta_part,
                                    const float* dbta_part, const float* dwsa_part, const float* dbsa_part, float* d_wsa, float* d_bsa,
                                    float* d_wta, float* d_bta, float* d_w1, float* d_b1, float* d_w2, float* d_b2, int B, int V, int C,
                                    void* stream) {
    FGCN_REQUIRE(dzc && dhpre && cm && h && dwta_part && dbta_part && dwsa_part && dbsa_part, FGCN_E_BADARG, "stc_param_grads: null pointer");
    FGCN_REQUIRE(d_wsa && d_bsa && d_wta && d_bta && d_w1 && d_b1 && d_w2 && d_b2, FGCN_E_BADARG, "stc_param_grads: null pointer (a gradient)");
    if (int e = stc_check_dims("stc_param_grads", B, 1, V, C)) return e;
    StcParamGradArgs a;
    a.dzc = dzc, a.dhpre = dhpre, a.cm = cm, a.h = h, a.dwta_part = dwta_part, a.dbta_part = dbta_part, a.dwsa_part = dwsa_part;
    a.dbsa_part = dbsa_part, a.d_wsa = d_wsa, a.d_bsa = d_bsa, a.d_wta = d_wta, a.d_bta = d_bta, a.d_w1 = d_w1, a.d_b1 = d_b1, a.d_w2 = d_w2;
    a.d_b2 = d_b2, a.B = B, a.C = C, a.k = stc_sa_kernel(V);
    const long long n = (long long)C * C + C + C / 2 + (long long)C * (STC_TA_TAPS + a.k) + 2;      // C * C: the two (C, C / 2) matrices
    hipLaunchKernelGGL(stc_param_grads_kernel, dim3((unsigned)cdiv(n, STC_THREADS)), dim3(STC_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("stc_param_grads");
}
