// The channel-wise topology refinement graph convolution of CTR-GCN (Chen et al., ICCV 2021; contract in include/fgcn.h, "CTR graph
// convolution").  All tensors float32 channels-last; K = 3 subsets, C = Cout in 64s, V <= 32, R in 4s.
//
//   forward    ctr_mean_t         xm[b, v, :] = mean_t x                                        one pass over x
//              ctr_tanh           th[b, k, u, v, r] = tanh(x1_k[b, u, r] - x2_k[b, v, r])       once per sample, shared by every channel
//              ctr_aggregate      y[b, t, u, c] = sum_k sum_v A'_k[b, u, v, c] x3[b, t, v, kC + c]
//   backward   ctr_bwd_dx3        dx3[b, t, v, kC + c] = sum_u A'_k[b, u, v, c] dy[b, t, u, c]
//              ctr_bwd_da         dA'_k[b, u, v, c] = sum_t dy[b, t, u, c] x3[b, t, v, kC + c]    (written out: DESIGN.md 8r has its bytes)
//              ctr_bwd_small      one workgroup per (sample, subset): the sample's terms of dPA, dW4, db4, dalpha, and dx1 | dx2
//              ctr_param_grads    the four parameter gradients: sums over the samples in sample order
//              ctr_mean_t_bwd     dx (+)= dxm / T
//
// A'_k[b, u, v, c] = alpha (b4_k[c] + sum_r W4_k[c, r] th[b, k, u, v, r]) + PA[k, u, v] never reaches memory: a thread of the three
// activation-sized kernels owns (joint, channel) -- lane = channel of a 64-channel tile, wave = joint -- and holds its 3 V values of A' in
// registers for all the frames its workgroup walks; the frames' other operand goes through LDS in chunks of CTR_FC frames.  A thread owns
// two joints (8 waves x 2 = 16 joints per workgroup), so one LDS read feeds two FMAs.
//
// Every sum has one order fixed by the sizes alone: r, v, u, k and t ascending in a thread, lanes by the xor butterfly, waves in wave order,
// samples in sample order.  No atomics.  No forward kernel reads another sample.  Nothing is skipped on a value: alpha == 0 still multiplies.
#include <cmath>

#include "fgcn_common.hpp"

namespace fgcn {

constexpr int CTR_K = 3, CTR_MAX_V = 32;
constexpr int CTR_THREADS = 512, CTR_WAVES = CTR_THREADS / 64, CTR_NU = 2, CTR_UG = CTR_WAVES * CTR_NU;
constexpr int CTR_FC = 2;                // frames per LDS stage: 2 x 3 x 32 rows of 64 floats = 48 KiB at most
constexpr int CTR_SMALL_THREADS = 256, CTR_SMALL_WAVES = CTR_SMALL_THREADS / 64;

__device__ __forceinline__ float ctr_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- xm = mean_t x and its backward ----------------------------------------------------------------------------------------------------
struct CtrMeanArgs {
    const float* in;     // x (forward), dxm (backward)
    float* out;          // xm (forward), dx (backward)
    int T, accumulate;
    unsigned vc4;        // V * C / 4
};

// grid (ceil(vc4 / 64), B), block (64, 4): thread (x, y) adds frames y, y + 4, .. of 16-byte group x
__global__ __launch_bounds__(256) void ctr_mean_t_kernel(CtrMeanArgs a) {
    __shared__ f32x4 part[4][64];
    const unsigned e = blockIdx.x * 64u + threadIdx.x;
    const int y = threadIdx.y;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (e < a.vc4) {
        const f32x4* base = reinterpret_cast<const f32x4*>(a.in) + (long long)blockIdx.y * a.T * a.vc4 + e;
        for (int t = y; t < a.T; t += 4) acc += base[(long long)t * a.vc4];
    }
    part[y][threadIdx.x] = acc;
    __syncthreads();
    if (y == 0 && e < a.vc4) {
        const f32x4 s = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        reinterpret_cast<f32x4*>(a.out)[(long long)blockIdx.y * a.vc4 + e] = s / (float)a.T;
    }
}

// grid (ceil(vc4 / 256), B): dx[b, t, e] (+)= dxm[b, e] / T
__global__ __launch_bounds__(256) void ctr_mean_t_bwd_kernel(CtrMeanArgs a) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.vc4) return;
    const f32x4 d = reinterpret_cast<const f32x4*>(a.in)[(long long)blockIdx.y * a.vc4 + e] / (float)a.T;
    f32x4* out = reinterpret_cast<f32x4*>(a.out) + (long long)blockIdx.y * a.T * a.vc4 + e;
    for (int t = 0; t < a.T; ++t) {
        if (a.accumulate) out[(long long)t * a.vc4] += d;
        else out[(long long)t * a.vc4] = d;
    }
}

// ---- th = tanh(x1[u] - x2[v]) ----------------------------------------------------------------------------------------------------------
struct CtrTanhArgs {
    const float* x12;    // (B, V, 2 K R): x1_k at k R, x2_k at (K + k) R
    float* th;           // (B, K, V, V, R)
    int V, R;
    unsigned per_sample; // K V V R
};

// grid (ceil(per_sample / 256), B)
__global__ __launch_bounds__(256) void ctr_tanh_kernel(CtrTanhArgs a) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.per_sample) return;
    const int V = a.V, R = a.R;
    const unsigned r = e % R, uv = (e / R) % (V * V), k = e / ((unsigned)R * V * V);
    const unsigned u = uv / V, v = uv - u * V;
    const float* x = a.x12 + (long long)blockIdx.y * V * 2 * CTR_K * R;
    a.th[(long long)blockIdx.y * a.per_sample + e] = tanhf(x[u * 2 * CTR_K * R + k * R + r] - x[v * 2 * CTR_K * R + (CTR_K + k) * R + r]);
}

// ---- the three activation-sized kernels ------------------------------------------------------------------------------------------------
struct CtrAggArgs {
    const float *x3, *dy, *th, *w4, *b4, *alpha, *pa;
    float* out;          // y (forward), dx3, dA'
    int T, V, C, R, fps; // C = Cout; fps: frames per split (T in ctr_bwd_da)
};

// A[i][k][j] = alpha (b4_k[c] + sum_r W4_k[c, r] th[k, u, v, r]) + PA[k, u, v] with (u, v) = (own[i], j), or (j, own[i]) when TRANS.
// th is read in wave-uniform 16-byte groups, W4's row of the lane's channel in 16-byte groups; j >= V: zero.
template <int VT, int TRANS>
__device__ __forceinline__ void ctr_form(float (&A)[CTR_NU][CTR_K][VT], const CtrAggArgs& a, int b, int c, const int (&own)[CTR_NU]) {
    const int V = a.V, R = a.R;
    const float alpha = a.alpha[0];
#pragma unroll
    for (int i = 0; i < CTR_NU; ++i) {
#pragma unroll
        for (int k = 0; k < CTR_K; ++k) {
            const float* th = a.th + ((long long)b * CTR_K + k) * V * V * R;
            const float* w = a.w4 + ((long long)k * a.C + c) * R;
            float acc[VT];
#pragma unroll
            for (int j = 0; j < VT; ++j) acc[j] = 0.f;
            for (int r = 0; r < R; r += 4) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + r);
#pragma unroll
                for (int j = 0; j < VT; ++j) {
                    if (j < V) {
                        const int uv = TRANS ? j * V + own[i] : own[i] * V + j;
                        const f32x4 t = *reinterpret_cast<const f32x4*>(th + (long long)uv * R + r);
                        acc[j] = fmaf(wv[0], t[0], acc[j]);
                        acc[j] = fmaf(wv[1], t[1], acc[j]);
                        acc[j] = fmaf(wv[2], t[2], acc[j]);
                        acc[j] = fmaf(wv[3], t[3], acc[j]);
                    }
                }
            }
            const float bias = a.b4[k * a.C + c];
#pragma unroll
            for (int j = 0; j < VT; ++j) {
                const int uv = TRANS ? j * V + own[i] : own[i] * V + j;
                A[i][k][j] = j < V ? fmaf(alpha, bias + acc[j], a.pa[k * V * V + uv]) : 0.f;
            }
        }
    }
}

// rows (f, q) -> stage[(f * rows + q) * 16 + 16-byte group]: `rows` rows of the tile's 64 channels per frame, n frames from frame t.
// X3: the rows are (k, v) of x3 (row stride K C, subset k at k C); else the rows are the joints of dy (row stride C).
template <int X3>
__device__ __forceinline__ void ctr_stage(f32x4* stage, const CtrAggArgs& a, int b, int t, int n, int tile) {
    const int V = a.V, C = a.C, rows = X3 ? CTR_K * V : V;
    const int g = threadIdx.x & 15;
    for (int q = threadIdx.x >> 4; q < n * rows; q += CTR_THREADS / 16) {
        const int f = q / rows, row = q - f * rows;
        const float* src;
        if constexpr (X3) {
            const int k = row / V, v = row - k * V;
            src = a.x3 + (((long long)b * a.T + t + f) * V + v) * CTR_K * C + k * C + tile * 64;
        } else {
            src = a.dy + (((long long)b * a.T + t + f) * V + row) * C + tile * 64;
        }
        stage[q * 16 + g] = reinterpret_cast<const f32x4*>(src)[g];
    }
}

struct CtrWho {
    int tile, b, lane, c, own[CTR_NU];
    bool valid[CTR_NU];
};

// grid x = (C / 64) * ceil(V / 16): the tile and the group of 16 joints; thread (wave w, lane) owns joints group * 16 + w + 8 i of channel
// tile * 64 + lane.  A joint beyond V is clamped for the arithmetic (uniform control flow) and stores nothing.
__device__ __forceinline__ CtrWho ctr_who(const CtrAggArgs& a) {
    CtrWho o;
    const int tiles = a.C / 64, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    o.tile = blockIdx.x % tiles;
    o.b = blockIdx.z;
    o.lane = threadIdx.x & 63;
    o.c = o.tile * 64 + o.lane;
#pragma unroll
    for (int i = 0; i < CTR_NU; ++i) {
        const int j = (blockIdx.x / tiles) * CTR_UG + w + CTR_WAVES * i;
        o.valid[i] = j < a.V;
        o.own[i] = j < a.V ? j : a.V - 1;
    }
    return o;
}

// grid ((C / 64) * ceil(V / 16), splits, B)
template <int VT>
__global__ __launch_bounds__(CTR_THREADS) void ctr_fwd_kernel(CtrAggArgs a) {
    __shared__ f32x4 stage[CTR_FC * CTR_K * CTR_MAX_V * 16];
    const CtrWho o = ctr_who(a);
    const int V = a.V, C = a.C;
    float A[CTR_NU][CTR_K][VT];
    ctr_form<VT, 0>(A, a, o.b, o.c, o.own);
    const float* sf = reinterpret_cast<const float*>(stage);
    const int t0 = blockIdx.y * a.fps, t1 = min(a.T, t0 + a.fps);
    for (int tc = t0; tc < t1; tc += CTR_FC) {
        const int n = min(CTR_FC, t1 - tc);
        __syncthreads();
        ctr_stage<1>(stage, a, o.b, tc, n, o.tile);
        __syncthreads();
        for (int f = 0; f < n; ++f) {
            float y[CTR_NU];
#pragma unroll
            for (int i = 0; i < CTR_NU; ++i) y[i] = 0.f;
#pragma unroll
            for (int k = 0; k < CTR_K; ++k) {
#pragma unroll
                for (int j = 0; j < VT; ++j) {
                    if (j < V) {
                        const float x = sf[((f * CTR_K + k) * V + j) * 64 + o.lane];
#pragma unroll
                        for (int i = 0; i < CTR_NU; ++i) y[i] = fmaf(A[i][k][j], x, y[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < CTR_NU; ++i)
                if (o.valid[i]) a.out[(((long long)o.b * a.T + tc + f) * V + o.own[i]) * C + o.c] = y[i];
        }
    }
}

// grid as ctr_fwd_kernel; the thread's joints are the v of dx3[b, t, v, k C + c] = sum_u A'_k[u, v, c] dy[b, t, u, c]
template <int VT>
__global__ __launch_bounds__(CTR_THREADS) void ctr_bwd_dx3_kernel(CtrAggArgs a) {
    __shared__ f32x4 stage[CTR_FC * CTR_MAX_V * 16];
    const CtrWho o = ctr_who(a);
    const int V = a.V, C = a.C;
    float A[CTR_NU][CTR_K][VT];
    ctr_form<VT, 1>(A, a, o.b, o.c, o.own);
    const float* sf = reinterpret_cast<const float*>(stage);
    const int t0 = blockIdx.y * a.fps, t1 = min(a.T, t0 + a.fps);
    for (int tc = t0; tc < t1; tc += CTR_FC) {
        const int n = min(CTR_FC, t1 - tc);
        __syncthreads();
        ctr_stage<0>(stage, a, o.b, tc, n, o.tile);
        __syncthreads();
        for (int f = 0; f < n; ++f) {
            float d[CTR_NU][CTR_K];
#pragma unroll
            for (int i = 0; i < CTR_NU; ++i)
#pragma unroll
                for (int k = 0; k < CTR_K; ++k) d[i][k] = 0.f;
#pragma unroll
            for (int j = 0; j < VT; ++j) {
                if (j < V) {
                    const float g = sf[(f * V + j) * 64 + o.lane];
#pragma unroll
                    for (int i = 0; i < CTR_NU; ++i)
#pragma unroll
                        for (int k = 0; k < CTR_K; ++k) d[i][k] = fmaf(A[i][k][j], g, d[i][k]);
                }
            }
#pragma unroll
            for (int i = 0; i < CTR_NU; ++i)
                if (o.valid[i]) {
                    float* dst = a.out + (((long long)o.b * a.T + tc + f) * V + o.own[i]) * CTR_K * C + o.c;
#pragma unroll
                    for (int k = 0; k < CTR_K; ++k) dst[k * C] = d[i][k];
                }
        }
    }
}

// grid ((C / 64) * ceil(V / 16), 1, B): all T frames in frame order; the thread's joints are the u of dA'_k[b, u, v, c]
template <int VT>
__global__ __launch_bounds__(CTR_THREADS) void ctr_bwd_da_kernel(CtrAggArgs a) {
    __shared__ f32x4 stage[CTR_FC * CTR_K * CTR_MAX_V * 16];
    const CtrWho o = ctr_who(a);
    const int V = a.V, C = a.C;
    float acc[CTR_NU][CTR_K][VT];
#pragma unroll
    for (int i = 0; i < CTR_NU; ++i)
#pragma unroll
        for (int k = 0; k < CTR_K; ++k)
#pragma unroll
            for (int j = 0; j < VT; ++j) acc[i][k][j] = 0.f;
    const float* sf = reinterpret_cast<const float*>(stage);
    for (int tc = 0; tc < a.T; tc += CTR_FC) {
        const int n = min(CTR_FC, a.T - tc);
        __syncthreads();
        ctr_stage<1>(stage, a, o.b, tc, n, o.tile);
        __syncthreads();
        for (int f = 0; f < n; ++f) {
            float g[CTR_NU];
#pragma unroll
            for (int i = 0; i < CTR_NU; ++i) g[i] = a.dy[(((long long)o.b * a.T + tc + f) * V + o.own[i]) * C + o.c];
#pragma unroll
            for (int k = 0; k < CTR_K; ++k) {
#pragma unroll
                for (int j = 0; j < VT; ++j) {
                    if (j < V) {
                        const float x = sf[((f * CTR_K + k) * V + j) * 64 + o.lane];
#pragma unroll
                        for (int i = 0; i < CTR_NU; ++i) acc[i][k][j] = fmaf(g[i], x, acc[i][k][j]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CTR_NU; ++i)
        if (o.valid[i]) {
#pragma unroll
            for (int k = 0; k < CTR_K; ++k) {
                float* dst = a.out + ((((long long)o.b * CTR_K + k) * V + o.own[i]) * V) * C + o.c;
#pragma unroll
                for (int j = 0; j < VT; ++j)
                    if (j < V) dst[(long long)j * C] = acc[i][k][j];
            }
        }
}

// ---- one workgroup per (sample, subset): everything that follows from dA' ---------------------------------------------------------------
struct CtrSmallArgs {
    const float *da, *th, *w4, *b4, *alpha;
    float *dz;                   // (B, K, V, V, R) scratch: alpha dth (1 - th^2)
    float *dx12;                 // (B, V, 2 K R)
    float *s2_part, *s1_part;    // (B, K, C, R) = sum_{u, v} dA' th, (B, K, C) = sum_{u, v} dA'    (not yet times alpha)
    float *dpa_part;             // (B, K, V, V) = sum_c dA'
    float *dalpha_part;          // (B, K) = <b4_k, s1> + <W4_k, s2>
    int V, C, R;
};

// grid (K, B)
__global__ __launch_bounds__(CTR_SMALL_THREADS) void ctr_bwd_small_kernel(CtrSmallArgs a) {
    __shared__ float part[CTR_SMALL_WAVES];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int V = a.V, C = a.C, R = a.R, VV = V * V;
    const long long bk = (long long)b * CTR_K + k;
    const float* da = a.da + bk * VV * C;
    const float* th = a.th + bk * VV * R;
    const float* w4 = a.w4 + (long long)k * C * R;
    const float alpha = a.alpha[0];
    float dal = 0.f;
    for (int e = tid; e < C * R; e += CTR_SMALL_THREADS) {              // s2[c, r] = sum_{uv} dA'[uv, c] th[uv, r]
        const int c = e / R, r = e - c * R;
        float s = 0.f;
        for (int uv = 0; uv < VV; ++uv) s = fmaf(da[(long long)uv * C + c], th[uv * R + r], s);
        a.s2_part[bk * C * R + e] = s;
        dal = fmaf(w4[e], s, dal);
    }
    for (int c = tid; c < C; c += CTR_SMALL_THREADS) {                  // s1[c] = sum_{uv} dA'[uv, c]
        float s = 0.f;
        for (int uv = 0; uv < VV; ++uv) s += da[(long long)uv * C + c];
        a.s1_part[bk * C + c] = s;
        dal = fmaf(a.b4[k * C + c], s, dal);
    }
    for (int uv = w; uv < VV; uv += CTR_SMALL_WAVES) {                  // sum_c dA'[uv, c]
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += da[(long long)uv * C + c];
        s = ctr_wave_sum(s);
        if (lane == 0) a.dpa_part[bk * VV + uv] = s;
    }
    float* dz = a.dz + bk * VV * R;
    for (int e = tid; e < VV * R; e += CTR_SMALL_THREADS) {             // dz[uv, r] = alpha (sum_c dA'[uv, c] W4[c, r]) (1 - th^2)
        const int uv = e / R, r = e - uv * R;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(da[(long long)uv * C + c], w4[c * R + r], s);
        const float t = th[e];
        dz[e] = (alpha * s) * (1.0f - t * t);
    }
    dal = ctr_wave_sum(dal);
    if (lane == 0) part[w] = dal;
    __syncthreads();                                                   // (dz is visible to the workgroup behind this barrier too)
    if (tid == 0) a.dalpha_part[bk] = ((part[0] + part[1]) + part[2]) + part[3];
    float* dx12 = a.dx12 + (long long)b * V * 2 * CTR_K * R;
    for (int e = tid; e < V * R; e += CTR_SMALL_THREADS) {              // dx1[u] = sum_v dz[u, v], dx2[v] = -sum_u dz[u, v]
        const int j = e / R, r = e - j * R;
        float s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < V; ++i) {
            s1 += dz[(j * V + i) * R + r];
            s2 += dz[(i * V + j) * R + r];
        }
        dx12[j * 2 * CTR_K * R + k * R + r] = s1;
        dx12[j * 2 * CTR_K * R + (CTR_K + k) * R + r] = -s2;
    }
}

// ---- the cross-sample sums ----------------------------------------------------------------------------------------------------------
struct CtrParamGradArgs {
    const float *s2_part, *s1_part, *dpa_part, *dalpha_part, *alpha;
    float *d_w4, *d_b4, *d_pa, *d_alpha;
    int B, n_pa, n_w4, n_b4;     // K V V, K C R, K C
};

// one thread per output element; each adds its B terms in sample order
__global__ __launch_bounds__(256) void ctr_param_grads_kernel(CtrParamGradArgs a) {
    long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const float alpha = a.alpha[0];
    float s = 0.f;
    if (e < a.n_pa) {
        for (int b = 0; b < a.B; ++b) s += a.dpa_part[(long long)b * a.n_pa + e];
        a.d_pa[e] = s;
        return;
    }
    e -= a.n_pa;
    if (e < a.n_w4) {
        for (int b = 0; b < a.B; ++b) s += a.s2_part[(long long)b * a.n_w4 + e];
        a.d_w4[e] = alpha * s;
        return;
    }
    e -= a.n_w4;
    if (e < a.n_b4) {
        for (int b = 0; b < a.B; ++b) s += a.s1_part[(long long)b * a.n_b4 + e];
        a.d_b4[e] = alpha * s;
        return;
    }
    if (e == a.n_b4) {
        for (int i = 0; i < a.B * CTR_K; ++i) s += a.dalpha_part[i];
        a.d_alpha[0] = s;
    }
}

static int ctr_check_dims(const char* what, int B, int T, int V, int C, int R) {
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0 && V > 0 && V <= CTR_MAX_V, FGCN_E_BADARG, "%s: bad B/T/V %d/%d/%d (V <= %d, B <= 65535)", what, B, T,
                 V, CTR_MAX_V);
    FGCN_REQUIRE(C > 0 && C % 64 == 0 && C <= 512, FGCN_E_BADARG, "%s: Cout=%d is not a multiple of 64 up to 512", what, C);
    FGCN_REQUIRE(R > 0 && R % 4 == 0 && R <= 64, FGCN_E_BADARG, "%s: R=%d is not a multiple of 4 up to 64", what, R);
    FGCN_REQUIRE((long long)T * V * CTR_K * C < (1ll << 31), FGCN_E_BADARG, "%s: T * V * 3 * Cout = %lld does not fit 31 bits", what,
                 (long long)T * V * CTR_K * C);
    return FGCN_OK;
}

static int ctr_split_frames(int B, int T, int V, int C) {     // frames per split: about 1024 workgroups, at least 16 frames each (A' is formed per split)
    const long long wgs = (long long)B * (C / 64) * cdiv(V, CTR_UG), want = cdiv(1024, wgs), most = T / 16 > 1 ? T / 16 : 1;
    return (int)cdiv(T, want < 1 ? 1 : (want > most ? most : want));
}

template <template <int> class Launch>
static bool ctr_by_joints(int V, dim3 grid, hipStream_t s, const CtrAggArgs& a) {
    return dispatch([&](auto vt) { Launch<decltype(vt)::value>::run(grid, s, a); return true; }, one_of<8, 16, 24, 32>{(V + 7) / 8 * 8});
}
template <int VT> struct CtrLaunchFwd { static void run(dim3 g, hipStream_t s, const CtrAggArgs& a) { hipLaunchKernelGGL(ctr_fwd_kernel<VT>, g, dim3(CTR_THREADS), 0, s, a); } };
template <int VT> struct CtrLaunchDx3 { static void run(dim3 g, hipStream_t s, const CtrAggArgs& a) { hipLaunchKernelGGL(ctr_bwd_dx3_kernel<VT>, g, dim3(CTR_THREADS), 0, s, a); } };
template <int VT> struct CtrLaunchDa { static void run(dim3 g, hipStream_t s, const CtrAggArgs& a) { hipLaunchKernelGGL(ctr_bwd_da_kernel<VT>, g, dim3(CTR_THREADS), 0, s, a); } };

}  // namespace fgcn

using namespace fgcn;

#define CTR_ALIGNED(what, ...)                                                                                   \
    do {                                                                                                         \
        const void* ptrs_[] = {__VA_ARGS__};                                                                     \
        for (const void* p_ : ptrs_) FGCN_REQUIRE(aligned16(p_), FGCN_E_ALIGN, what ": a tensor is not 16-byte aligned"); \
    } while (0)

extern "C" int fgcn_ctr_chunk(void) { return CTR_FC; }

extern "C" int fgcn_ctr_split_frames(int B, int T, int V, int Cout) {
    if (B <= 0 || B > 65535 || T <= 0 || V <= 0 || V > CTR_MAX_V || Cout < 64 || Cout % 64 || Cout > 512) return 0;
    if ((long long)T * V * CTR_K * Cout >= (1ll << 31)) return 0;
    return ctr_split_frames(B, T, V, Cout);
}

extern "C" int fgcn_ctr_mean_t(const float* x, float* xm, int B, int T, int V, int C, void* stream) {
    FGCN_REQUIRE(x && xm, FGCN_E_BADARG, "ctr_mean_t: null pointer");
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0 && V > 0 && V <= CTR_MAX_V, FGCN_E_BADARG, "ctr_mean_t: bad B/T/V %d/%d/%d", B, T, V);
    FGCN_REQUIRE(C > 0 && C % 4 == 0 && (long long)T * V * C < (1ll << 31), FGCN_E_BADARG, "ctr_mean_t: C=%d is not a multiple of 4, or T * V * C does not fit 31 bits", C);
    CTR_ALIGNED("ctr_mean_t", x, xm);
    CtrMeanArgs a;
    a.in = x, a.out = xm, a.T = T, a.accumulate = 0, a.vc4 = (unsigned)(V * C / 4);
    hipLaunchKernelGGL(ctr_mean_t_kernel, dim3((unsigned)cdiv(a.vc4, 64), (unsigned)B), dim3(64, 4), 0, (hipStream_t)stream, a);
    return launch_status("ctr_mean_t");
}

extern "C" int fgcn_ctr_mean_t_bwd(const float* dxm, float* dx, int B, int T, int V, int C, int accumulate, void* stream) {
    FGCN_REQUIRE(dxm && dx, FGCN_E_BADARG, "ctr_mean_t_bwd: null pointer");
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0 && V > 0 && V <= CTR_MAX_V, FGCN_E_BADARG, "ctr_mean_t_bwd: bad B/T/V %d/%d/%d", B, T, V);
    FGCN_REQUIRE(C > 0 && C % 4 == 0 && (long long)T * V * C < (1ll << 31), FGCN_E_BADARG, "ctr_mean_t_bwd: C=%d is not a multiple of 4, or T * V * C does not fit 31 bits", C);
    CTR_ALIGNED("ctr_mean_t_bwd", dxm, dx);
    CtrMeanArgs a;
    a.in = dxm, a.out = dx, a.T = T, a.accumulate = accumulate != 0, a.vc4 = (unsigned)(V * C / 4);
    hipLaunchKernelGGL(ctr_mean_t_bwd_kernel, dim3((unsigned)cdiv(a.vc4, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("ctr_mean_t_bwd");
}

extern "C" int fgcn_ctr_tanh(const float* x12, float* th, int B, int V, int R, void* stream) {
    FGCN_REQUIRE(x12 && th, FGCN_E_BADARG, "ctr_tanh: null pointer");
    if (int e = ctr_check_dims("ctr_tanh", B, 1, V, 64, R)) return e;
    CtrTanhArgs a;
    a.x12 = x12, a.th = th, a.V = V, a.R = R, a.per_sample = (unsigned)(CTR_K * V * V * R);
    hipLaunchKernelGGL(ctr_tanh_kernel, dim3((unsigned)cdiv(a.per_sample, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("ctr_tanh");
}

static void ctr_agg_args(CtrAggArgs& a, const float* x3, const float* dy, const float* th, const float* w4, const float* b4, const float* alpha,
                         const float* pa, float* out, int T, int V, int C, int R, int fps) {
    a.x3 = x3, a.dy = dy, a.th = th, a.w4 = w4, a.b4 = b4, a.alpha = alpha, a.pa = pa, a.out = out, a.T = T, a.V = V, a.C = C, a.R = R, a.fps = fps;
}

extern "C" int fgcn_ctr_aggregate(const float* x3, const float* th, const float* w4, const float* b4, const float* alpha, const float* pa, float* y,
                                  int B, int T, int V, int Cout, int R, void* stream) {
    FGCN_REQUIRE(x3 && th && w4 && b4 && alpha && pa && y, FGCN_E_BADARG, "ctr_aggregate: null pointer");
    if (int e = ctr_check_dims("ctr_aggregate", B, T, V, Cout, R)) return e;
    CTR_ALIGNED("ctr_aggregate", x3, th, w4);
    CtrAggArgs a;
    ctr_agg_args(a, x3, nullptr, th, w4, b4, alpha, pa, y, T, V, Cout, R, ctr_split_frames(B, T, V, Cout));
    const dim3 grid((unsigned)((Cout / 64) * cdiv(V, CTR_UG)), (unsigned)cdiv(T, a.fps), (unsigned)B);
    FGCN_REQUIRE(ctr_by_joints<CtrLaunchFwd>(V, grid, (hipStream_t)stream, a), FGCN_E_BADARG, "ctr_aggregate: no kernel for V=%d", V);
    return launch_status("ctr_aggregate");
}

extern "C" int fgcn_ctr_bwd_dx3(const float* dy, const float* th, const float* w4, const float* b4, const float* alpha, const float* pa, float* dx3,
                                int B, int T, int V, int Cout, int R, void* stream) {
    FGCN_REQUIRE(dy && th && w4 && b4 && alpha && pa && dx3, FGCN_E_BADARG, "ctr_bwd_dx3: null pointer");
    if (int e = ctr_check_dims("ctr_bwd_dx3", B, T, V, Cout, R)) return e;
    CTR_ALIGNED("ctr_bwd_dx3", dy, th, w4);
    CtrAggArgs a;
    ctr_agg_args(a, nullptr, dy, th, w4, b4, alpha, pa, dx3, T, V, Cout, R, ctr_split_frames(B, T, V, Cout));
    const dim3 grid((unsigned)((Cout / 64) * cdiv(V, CTR_UG)), (unsigned)cdiv(T, a.fps), (unsigned)B);
    FGCN_REQUIRE(ctr_by_joints<CtrLaunchDx3>(V, grid, (hipStream_t)stream, a), FGCN_E_BADARG, "ctr_bwd_dx3: no kernel for V=%d", V);
    return launch_status("ctr_bwd_dx3");
}

extern "C" int fgcn_ctr_bwd_da(const float* dy, const float* x3, float* da, int B, int T, int V, int Cout, void* stream) {
    FGCN_REQUIRE(dy && x3 && da, FGCN_E_BADARG, "ctr_bwd_da: null pointer");
    if (int e = ctr_check_dims("ctr_bwd_da", B, T, V, Cout, 4)) return e;
    CTR_ALIGNED("ctr_bwd_da", x3);
    CtrAggArgs a;
    ctr_agg_args(a, x3, dy, nullptr, nullptr, nullptr, nullptr, nullptr, da, T, V, Cout, 0, T);
    const dim3 grid((unsigned)((Cout / 64) * cdiv(V, CTR_UG)), 1, (unsigned)B);
    FGCN_REQUIRE(ctr_by_joints<CtrLaunchDa>(V, grid, (hipStream_t)stream, a), FGCN_E_BADARG, "ctr_bwd_da: no kernel for V=%d", V);
    return launch_status("ctr_bwd_da");
}

extern "C" int fgcn_ctr_bwd_small(const float* da, const float* th, const float* w4, const float* b4, const float* alpha, float* dz, float* dx12,
                                  float* s2_part, float* s1_part, float* dpa_part, float* dalpha_part, int B, int V, int Cout, int R, void* stream) {
    FGCN_REQUIRE(da && th && w4 && b4 && alpha && dz && dx12 && s2_part && s1_part && dpa_part && dalpha_part, FGCN_E_BADARG,
                 "ctr_bwd_small: null pointer");
    if (int e = ctr_check_dims("ctr_bwd_small", B, 1, V, Cout, R)) return e;
    CtrSmallArgs a;
    a.da = da, a.th = th, a.w4 = w4, a.b4 = b4, a.alpha = alpha, a.dz = dz, a.dx12 = dx12, a.s2_part = s2_part, a.s1_part = s1_part;
    a.dpa_part = dpa_part, a.dalpha_part = dalpha_part, a.V = V, a.C = Cout, a.R = R;
    hipLaunchKernelGGL(ctr_bwd_small_kernel, dim3(CTR_K, (unsigned)B), dim3(CTR_SMALL_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("ctr_bwd_small");
}

extern "C" int fgcn_ctr_param_grads(const float* s2_part, const float* s1_part, const float* dpa_part, const float* dalpha_part, const float* alpha,
                                    float* d_w4, float* d_b4, float* d_pa, float* d_alpha, int B, int V, int Cout, int R, void* stream) {
    FGCN_REQUIRE(s2_part && s1_part && dpa_part && dalpha_part && alpha && d_w4 && d_b4 && d_pa && d_alpha, FGCN_E_BADARG,
                 "ctr_param_grads: null pointer");
    if (int e = ctr_check_dims("ctr_param_grads", B, 1, V, Cout, R)) return e;
    CtrParamGradArgs a;
    a.s2_part = s2_part, a.s1_part = s1_part, a.dpa_part = dpa_part, a.dalpha_part = dalpha_part, a.alpha = alpha;
    a.d_w4 = d_w4, a.d_b4 = d_b4, a.d_pa = d_pa, a.d_alpha = d_alpha, a.B = B, a.n_pa = CTR_K * V * V, a.n_w4 = CTR_K * Cout * R, a.n_b4 = CTR_K * Cout;
    const long long n = (long long)a.n_pa + a.n_w4 + a.n_b4 + 1;
    hipLaunchKernelGGL(ctr_param_grads_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("ctr_param_grads");
}
