// The two shift operations of Shift-GCN (Cheng et al., CVPR 2020; contract in include/fgcn.h, "Shift graph convolution"; DESIGN.md
// section 8s).  All tensors float32 channels-last, rows r = (b, t), activations (B, T, V, C).
//
//   joint shift   shift_joint_kernel   out[r, v, c] = in[r, (v + dir c) mod V, c] * g       forward (g at the output joint) and dx (g at the
//                                      source joint, dir negated) are one template; the dx form also leaves the per-workgroup terms of dmask
//                 shift_joint4_kernel  the 3-channel input that travels as 4: lane = joint, the pad channel is written as zero
//                 shift_dmask_kernel   dmask[v, c] = (1 - tanh(mask)^2) * (summed terms at the joint the forward read)
//   frame shift   shift_frame_kernel       out[b, to, v, c] = (1 - f) tap(to s + k) + f tap(to s + k + 1), optionally with the BatchNorm partial
//                                          sums of out from the same pass
//                 shift_frame_bwd_kernel   dx in its gather form, and the per-workgroup terms of dpos
//
// A thread that owns channel c and reads joint (v + c) mod V from memory puts a wave on 64 cache lines, so the joint shift stages whole
// frames of a 64-channel tile in LDS with coalesced 16-byte loads and reads LDS at the shifted joint: the bank is c mod 64 whatever the
// joint, 64 banks of 4 bytes, no conflict.  The frame shift needs no staging: lane = channel, both taps are rows of the same tensor.
//
// Every sum has one order fixed by the sizes alone: frames and joints ascending in a thread, waves in wave order, workgroups by
// fgcn_reduce_sum.  No atomics.  Nothing is skipped on a value: a gate of 1 still multiplies, f == 0 still multiplies its tap.
#include <cmath>

#include "fgcn_common.hpp"

namespace fgcn {

constexpr int SH_MAX_V = 64, SH_MAX_C = 512;
constexpr int SH_THREADS = 512, SH_WAVES = SH_THREADS / 64, SH_JPT = SH_MAX_V / SH_WAVES;     // joints per thread: 8
constexpr int SH_STAGE = 128;                  // joint rows (of 64 channels) per LDS stage: 32 KiB, at least two frames
constexpr int SH_TARGET_WGS = 2048;            // workgroups a launch aims at (8 per CU)
constexpr int SH_MIN_ROWS = 8;                 // rows a workgroup of the joint shift walks at least (the gate tile costs one row's work)
constexpr int SHF_MIN_FRAMES = 4;              // output frames a workgroup of the frame shift walks at least
constexpr int SHF_THREADS = 256, SHF_WAVES = SHF_THREADS / 64;
constexpr float SH_K_LIMIT = 67108864.f;       // 2^26: |k| beyond every clip, and to s + k + 1 stays inside an int

// ---- joint shift -----------------------------------------------------------------------------------------------------------------------
struct ShiftJointArgs {
    const float *in, *x, *mask;
    float *out, *part;       // part (chunks, V, C): sum_r in[r, src, c] x[r, v, c] at the thread's OWN joint v
    long long rows;
    int V, C, dir, rpw, mask_ld;
};

// (dir c) mod V in [0, V)
__device__ __forceinline__ int shift_of(int c, int V, int dir) {
    const int m = c % V;
    return (dir < 0 && m) ? V - m : m;
}

// grid (C / 64, chunks).  GATE: 0 none, 1 g[v, c] of the output joint (forward), 2 g[src, c] of the source joint (dx).  DMASK: 1 with GATE 2
template <int GATE, int DMASK>
__global__ __launch_bounds__(SH_THREADS) void shift_joint_kernel(ShiftJointArgs a) {
    __shared__ f32x4 stage[SH_STAGE * 16];
    __shared__ float gate[GATE ? SH_MAX_V * 64 : 1];
    const int V = a.V, C = a.C, tile = blockIdx.x, lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = tile * 64 + lane, sh = shift_of(c, V, a.dir);
    if constexpr (GATE != 0) {
        for (int e = threadIdx.x; e < V * 64; e += SH_THREADS) gate[e] = tanhf(a.mask[(long long)(e >> 6) * C + tile * 64 + (e & 63)]) + 1.0f;
    }
    float acc[SH_JPT];
#pragma unroll
    for (int j = 0; j < SH_JPT; ++j) acc[j] = 0.f;
    const float* sf = reinterpret_cast<const float*>(stage);
    const long long r0 = (long long)blockIdx.y * a.rpw, r1 = min(a.rows, r0 + a.rpw);
    const int fr = SH_STAGE / V, c4 = C / 4;
    for (long long rc = r0; rc < r1; rc += fr) {
        const int n = (int)min((long long)fr, r1 - rc);
        __syncthreads();                                    // (the gate is visible behind the first one)
        const f32x4* src = reinterpret_cast<const f32x4*>(a.in + rc * V * C + tile * 64);
        for (int q = threadIdx.x; q < n * V * 16; q += SH_THREADS) stage[q] = src[(long long)(q >> 4) * c4 + (q & 15)];
        __syncthreads();
        for (int f = 0; f < n; ++f) {
#pragma unroll
            for (int j = 0; j < SH_JPT; ++j) {
                const int v = w + SH_WAVES * j;
                if (v < V) {                                // (wave-uniform)
                    int s = v + sh;
                    s = s >= V ? s - V : s;
                    const float raw = sf[(f * V + s) * 64 + lane];
                    const long long o = ((rc + f) * V + v) * C + c;
                    if constexpr (DMASK != 0) acc[j] = fmaf(raw, a.x[o], acc[j]);
                    float val = raw;
                    if constexpr (GATE != 0) val = raw * gate[(GATE == 1 ? v : s) * 64 + lane];
                    a.out[o] = val;
                }
            }
        }
    }
    if constexpr (DMASK != 0) {
#pragma unroll
        for (int j = 0; j < SH_JPT; ++j) {
            const int v = w + SH_WAVES * j;
            if (v < V) a.part[((long long)blockIdx.y * V + v) * C + c] = acc[j];
        }
    }
}

// C = 4 (three channels and a zero pad): grid (chunks), one wave, lane = joint; the mask row stride is mask_ld (3 or 4)
template <int GATE, int DMASK>
__global__ __launch_bounds__(64) void shift_joint4_kernel(ShiftJointArgs a) {
    const int V = a.V, v = threadIdx.x;
    if (v >= V) return;
    int s[3];
    float g[3], acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s[c] = v + shift_of(c, V, a.dir);
        s[c] = s[c] >= V ? s[c] - V : s[c];
        g[c] = 1.0f;
        if constexpr (GATE != 0) g[c] = tanhf(a.mask[(GATE == 1 ? v : s[c]) * a.mask_ld + c]) + 1.0f;
        acc[c] = 0.f;
    }
    const long long r0 = (long long)blockIdx.x * a.rpw, r1 = min(a.rows, r0 + a.rpw);
    for (long long r = r0; r < r1; ++r) {
        const float* row = a.in + r * V * 4;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float raw = row[s[c] * 4 + c];
            if constexpr (DMASK != 0) acc[c] = fmaf(raw, a.x[(r * V + v) * 4 + c], acc[c]);
            o[c] = GATE != 0 ? raw * g[c] : raw;
        }
        *reinterpret_cast<f32x4*>(a.out + (r * V + v) * 4) = o;
    }
    if constexpr (DMASK != 0)
        *reinterpret_cast<f32x4*>(a.part + ((long long)blockIdx.x * V + v) * 4) = f32x4{acc[0], acc[1], acc[2], 0.f};
}

// sums (V, C): the terms summed over the workgroups, at the joint u = (v + dir c) mod V that owned them; dir: the FORWARD's
__global__ __launch_bounds__(256) void shift_dmask_kernel(const float* sums, const float* mask, float* dmask, int V, int C, int mask_ld, int dir) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= V * mask_ld) return;
    const int v = e / mask_ld, c = e - v * mask_ld;
    if (C == 4 && c == 3) {
        dmask[e] = 0.f;
        return;
    }
    int u = v + shift_of(c, V, dir);
    u = u >= V ? u - V : u;
    const float th = tanhf(mask[e]);
    dmask[e] = (1.0f - th * th) * sums[u * C + c];
}

// ---- frame shift -----------------------------------------------------------------------------------------------------------------------
struct ShiftFrameArgs {
    const float *x, *dout, *pos;
    float *out, *part;       // forward: out, BatchNorm partials (B nsplit, 2, C); backward: dx, dpos terms (B nsplit, C)
    int T, T_out, V, C, fps, nsplit;
};

struct ShiftPos {
    int k;
    float f;
};

__device__ __forceinline__ ShiftPos shift_pos(float p) {
    const float kf = floorf(p);
    ShiftPos o;
    o.f = p - kf;                                                       // (a non-finite position: NaN, through every output of its channel)
    o.k = (int)fminf(fmaxf(kf, -SH_K_LIMIT), SH_K_LIMIT);               // clamped as a float; NaN -> -2^26
    return o;
}

// phi(x[t]) inside the clip, 0 (and no read) outside; `col` points at frame 0 of the thread's (sample, joint, channel)
template <int RELU>
__device__ __forceinline__ float shift_tap(const float* col, int t, int T, long long stride) {
    if ((unsigned)t >= (unsigned)T) return 0.f;
    const float v = col[(long long)t * stride];
    return RELU ? relu_nan(v) : v;
}

// the waves' values of one channel added in wave order -> wave 0 returns the sum
__device__ __forceinline__ float shift_wave_order_sum(float (*red)[64], float v, int w, int lane) {
    __syncthreads();
    red[w][lane] = v;
    __syncthreads();
    float s = red[0][lane];
#pragma unroll
    for (int i = 1; i < SHF_WAVES; ++i) s += red[i][lane];
    return s;
}

// grid (C / 64, nsplit, B), block 256: lane = channel, wave w walks the joints w, w + 4, .. over the split's output frames
template <int S, int RELU, int STATS>
__global__ __launch_bounds__(SHF_THREADS) void shift_frame_kernel(ShiftFrameArgs a) {
    __shared__ float red[SHF_WAVES][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int V = a.V, C = a.C, T = a.T, b = blockIdx.z, c = blockIdx.x * 64 + lane;
    const ShiftPos p = shift_pos(a.pos[c]);
    const int to0 = blockIdx.y * a.fps, to1 = min(a.T_out, to0 + a.fps);
    const long long fs = (long long)V * C;
    float s1 = 0.f, s2 = 0.f;
    for (int v = w; v < V; v += SHF_WAVES) {
        const float* col = a.x + ((long long)b * T * V + v) * C + c;
        float* dst = a.out + ((long long)b * a.T_out * V + v) * C + c;
        for (int to = to0; to < to1; ++to) {
            const int t = to * S + p.k;
            const float lo = shift_tap<RELU>(col, t, T, fs), hi = shift_tap<RELU>(col, t + 1, T, fs);
            const float o = (1.0f - p.f) * lo + p.f * hi;
            dst[(long long)to * fs] = o;
            if constexpr (STATS != 0) {
                s1 += o;
                s2 = fmaf(o, o, s2);
            }
        }
    }
    if constexpr (STATS != 0) {
        const float t1 = shift_wave_order_sum(red, s1, w, lane), t2 = shift_wave_order_sum(red, s2, w, lane);
        if (w == 0) {
            float* row = a.part + ((long long)b * a.nsplit + blockIdx.y) * 2 * C + c;
            row[0] = t1;
            row[C] = t2;
        }
    }
}

// the same grid; the split's input frames are [to0 s, to1 s) cut at T
template <int S, int RELU>
__global__ __launch_bounds__(SHF_THREADS) void shift_frame_bwd_kernel(ShiftFrameArgs a) {
    __shared__ float red[SHF_WAVES][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int V = a.V, C = a.C, T = a.T, T_out = a.T_out, b = blockIdx.z, c = blockIdx.x * 64 + lane;
    const ShiftPos p = shift_pos(a.pos[c]);
    const int to0 = blockIdx.y * a.fps, to1 = min(T_out, to0 + a.fps);
    const int t0 = to0 * S, t1 = min(T, to1 * S);
    const long long fs = (long long)V * C;
    float acc = 0.f;
    for (int v = w; v < V; v += SHF_WAVES) {
        const float* col = a.x + ((long long)b * T * V + v) * C + c;
        const float* dcol = a.dout + ((long long)b * T_out * V + v) * C + c;
        float* dst = a.out + ((long long)b * T * V + v) * C + c;
        for (int t = t0; t < t1; ++t) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 2; ++e) {                   // e = 0: the (1 - f) tap, output frame (t - k) / s; e = 1: the f tap, (t - k - 1) / s
                const int n = t - p.k - e;
                if (n >= 0 && (S == 1 || (n & 1) == 0)) {
                    const int q = S == 1 ? n : n >> 1;
                    if (q < T_out) d = fmaf(e ? p.f : 1.0f - p.f, dcol[(long long)q * fs], d);
                }
            }
            if constexpr (RELU != 0) d = relu_open(col[(long long)t * fs]) ? d : 0.f;
            dst[(long long)t * fs] = d;
        }
        for (int to = to0; to < to1; ++to) {
            const int t = to * S + p.k;
            const float lo = shift_tap<RELU>(col, t, T, fs), hi = shift_tap<RELU>(col, t + 1, T, fs);
            acc = fmaf(dcol[(long long)to * fs], hi - lo, acc);
        }
    }
    const float s = shift_wave_order_sum(red, acc, w, lane);
    if (w == 0) a.part[((long long)b * a.nsplit + blockIdx.y) * C + c] = s;
}

static bool shift_wide_c(int C) { return C >= 64 && C % 64 == 0 && C <= SH_MAX_C; }

static int shift_joint_rows(long long rows, int C) {     // rows per workgroup: about SH_TARGET_WGS workgroups, SH_MIN_ROWS rows at least
    const long long tiles = C == 4 ? 1 : C / 64, want = cdiv(rows * tiles, SH_TARGET_WGS);
    const long long rpw = want < SH_MIN_ROWS ? SH_MIN_ROWS : want;
    return (int)(rpw < rows ? rpw : rows);
}

static int shift_frame_split(int B, int T_out, int C) {  // output frames per workgroup
    const long long splits = cdiv(SH_TARGET_WGS, (long long)B * (C / 64)), want = cdiv(T_out, splits);
    const long long fps = want < SHF_MIN_FRAMES ? SHF_MIN_FRAMES : want;
    return (int)(fps < T_out ? fps : T_out);
}

static int shift_check_joint(const char* what, long long rows, int V, int C, int mask_ld) {
    FGCN_REQUIRE(rows > 0 && V > 0 && V <= SH_MAX_V, FGCN_E_BADARG, "%s: bad rows/V %lld/%d (V <= %d)", what, rows, V, SH_MAX_V);
    FGCN_REQUIRE(C == 4 || shift_wide_c(C), FGCN_E_BADARG, "%s: C=%d is neither 4 nor a multiple of 64 up to %d", what, C, SH_MAX_C);
    FGCN_REQUIRE(rows < (1ll << 31) / ((long long)V * C), FGCN_E_BADARG, "%s: rows * V * C = %lld * %d * %d does not fit 31 bits", what, rows, V, C);
    FGCN_REQUIRE(mask_ld == C || (C == 4 && mask_ld == 3), FGCN_E_BADARG, "%s: mask row stride %d for C=%d", what, mask_ld, C);
    return FGCN_OK;
}

static int shift_check_frame(const char* what, int B, int T, int V, int C, int stride) {
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0 && V > 0 && V <= SH_MAX_V, FGCN_E_BADARG, "%s: bad B/T/V %d/%d/%d (V <= %d, B <= 65535)", what, B, T, V,
                 SH_MAX_V);
    FGCN_REQUIRE(shift_wide_c(C), FGCN_E_BADARG, "%s: C=%d is not a multiple of 64 up to %d", what, C, SH_MAX_C);
    FGCN_REQUIRE(stride == 1 || stride == 2, FGCN_E_BADARG, "%s: stride=%d is neither 1 nor 2", what, stride);
    FGCN_REQUIRE((long long)B * T < (1ll << 31) / ((long long)V * C), FGCN_E_BADARG, "%s: B * T * V * C does not fit 31 bits", what);
    return FGCN_OK;
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_shift_joint_rows(long long rows, int V, int C) {
    if (rows <= 0 || V <= 0 || V > SH_MAX_V || !(C == 4 || shift_wide_c(C)) || rows >= (1ll << 31) / ((long long)V * C)) return 0;
    return shift_joint_rows(rows, C);
}

extern "C" int fgcn_shift_joint_stage(int V) { return (V <= 0 || V > SH_MAX_V) ? 0 : SH_STAGE / V; }

extern "C" int fgcn_shift_frame_split(int B, int T, int V, int C, int stride) {
    if (B <= 0 || B > 65535 || T <= 0 || V <= 0 || V > SH_MAX_V || !shift_wide_c(C) || (stride != 1 && stride != 2)) return 0;
    if ((long long)B * T >= (1ll << 31) / ((long long)V * C)) return 0;
    return shift_frame_split(B, (T - 1) / stride + 1, C);
}

extern "C" int fgcn_shift_joint(const float* in, const float* mask, const float* x, float* out, float* part, long long rows, int V, int C,
                                int mask_ld, int dir, int source_gate, void* stream) {
    FGCN_REQUIRE(in && out, FGCN_E_BADARG, "shift_joint: null pointer");
    FGCN_REQUIRE(dir == 1 || dir == -1, FGCN_E_BADARG, "shift_joint: dir=%d is neither +1 nor -1", dir);
    FGCN_REQUIRE(!x == !part && (!part || (mask && source_gate)), FGCN_E_BADARG,
                 "shift_joint: the mask-gradient terms need x, part, the mask and the gate at the source joint together");
    if (int e = shift_check_joint("shift_joint", rows, V, C, mask ? mask_ld : C)) return e;
    FGCN_REQUIRE(aligned16(in) && aligned16(out) && (!part || aligned16(part)), FGCN_E_ALIGN, "shift_joint: a tensor is not 16-byte aligned");
    ShiftJointArgs a;
    a.in = in, a.x = x, a.mask = mask, a.out = out, a.part = part, a.rows = rows, a.V = V, a.C = C, a.dir = dir, a.mask_ld = mask_ld;
    a.rpw = shift_joint_rows(rows, C);
    const unsigned chunks = (unsigned)cdiv(rows, a.rpw);
    const int gate = !mask ? 0 : (source_gate ? 2 : 1);
    const bool built = dispatch(
        [&](auto G, auto D) {
            constexpr bool ok = D == 0 || G == 2;
            if constexpr (ok) {
                if (C == 4) hipLaunchKernelGGL((shift_joint4_kernel<G, D>), dim3(chunks), dim3(64), 0, (hipStream_t)stream, a);
                else hipLaunchKernelGGL((shift_joint_kernel<G, D>), dim3((unsigned)(C / 64), chunks), dim3(SH_THREADS), 0, (hipStream_t)stream, a);
            }
            return ok;
        },
        one_of<0, 1, 2>{gate}, one_of<0, 1>{part != nullptr});
    FGCN_REQUIRE(built, FGCN_E_BADARG, "shift_joint: no such kernel form");
    return launch_status("shift_joint");
}

extern "C" int fgcn_shift_dmask(const float* sums, const float* mask, float* dmask, int V, int C, int mask_ld, int dir, void* stream) {
    FGCN_REQUIRE(sums && mask && dmask, FGCN_E_BADARG, "shift_dmask: null pointer");
    FGCN_REQUIRE(dir == 1 || dir == -1, FGCN_E_BADARG, "shift_dmask: dir=%d is neither +1 nor -1", dir);
    if (int e = shift_check_joint("shift_dmask", 1, V, C, mask_ld)) return e;
    hipLaunchKernelGGL(shift_dmask_kernel, dim3((unsigned)cdiv((long long)V * mask_ld, 256)), dim3(256), 0, (hipStream_t)stream, sums, mask, dmask, V, C,
                       mask_ld, dir);
    return launch_status("shift_dmask");
}

static void shift_frame_args(ShiftFrameArgs& a, const float* x, const float* dout, const float* pos, float* out, float* part, int B, int T, int V,
                             int C, int stride) {
    a.x = x, a.dout = dout, a.pos = pos, a.out = out, a.part = part, a.T = T, a.T_out = (T - 1) / stride + 1, a.V = V, a.C = C;
    a.fps = shift_frame_split(B, a.T_out, C);
    a.nsplit = (int)cdiv(a.T_out, a.fps);
}

extern "C" int fgcn_shift_frame(const float* x, const float* pos, float* out, float* part, int B, int T, int V, int C, int stride, int relu,
                                void* stream) {
    FGCN_REQUIRE(x && pos && out, FGCN_E_BADARG, "shift_frame: null pointer");
    if (int e = shift_check_frame("shift_frame", B, T, V, C, stride)) return e;
    ShiftFrameArgs a;
    shift_frame_args(a, x, nullptr, pos, out, part, B, T, V, C, stride);
    const dim3 grid((unsigned)(C / 64), (unsigned)a.nsplit, (unsigned)B);
    const bool built = dispatch(
        [&](auto S, auto R, auto ST) {
            hipLaunchKernelGGL((shift_frame_kernel<S, R, ST>), grid, dim3(SHF_THREADS), 0, (hipStream_t)stream, a);
            return true;
        },
        one_of<1, 2>{stride}, one_of<0, 1>{relu != 0}, one_of<0, 1>{part != nullptr});
    FGCN_REQUIRE(built, FGCN_E_BADARG, "shift_frame: no such kernel form");
    return launch_status("shift_frame");
}

extern "C" int fgcn_shift_frame_bwd(const float* dout, const float* x, const float* pos, float* dx, float* dpos_part, int B, int T, int V, int C,
                                    int stride, int relu, void* stream) {
    FGCN_REQUIRE(dout && x && pos && dx && dpos_part, FGCN_E_BADARG, "shift_frame_bwd: null pointer");
    if (int e = shift_check_frame("shift_frame_bwd", B, T, V, C, stride)) return e;
    ShiftFrameArgs a;
    shift_frame_args(a, x, dout, pos, dx, dpos_part, B, T, V, C, stride);
    const dim3 grid((unsigned)(C / 64), (unsigned)a.nsplit, (unsigned)B);
    const bool built = dispatch(
        [&](auto S, auto R) {
            hipLaunchKernelGGL((shift_frame_bwd_kernel<S, R>), grid, dim3(SHF_THREADS), 0, (hipStream_t)stream, a);
            return true;
        },
        one_of<1, 2>{stride}, one_of<0, 1>{relu != 0});
    FGCN_REQUIRE(built, FGCN_E_BADARG, "shift_frame_bwd: no such kernel form");
    return launch_status("shift_frame_bwd");
}
