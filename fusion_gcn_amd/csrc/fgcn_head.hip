// The two ends of the step around the ten blocks: the BatchNorm of the network input (`data_bn`, reference
// torch_src/models/mmargcn/agcn.py:150,186-188) and the CrossEntropy loss (session/session.py:53, step.py:38-46).
// Both are tiny (11.5 MB of input, a 64 x 60 logit matrix) -- they are here so that EVERY gradient of the step is a fixed-order
// libfgcn sum (MIOpen's BatchNorm backward was the one gradient of 274 that was not bitwise reproducible).
//
// data_bn = nn.BatchNorm1d(M*V*C) over x (N, M, T, V, C) viewed as (N, M*V*C, T): channel ch = (m*V + v)*C + c, statistics over
// (n, t).  x is already the blocks' (B = N*M, T, V, C) layout, so the apply pass writes the block input (B, T, V, Cp) directly,
// zero pad channels included; no permute / view / pad launches.
#include "fgcn_common.hpp"

namespace fgcn {

constexpr int DBN_T_CHUNK = 32;     // frames per tile: N * ceil(T / 32) tiles (640 at the headline shape)

// partials[tile][0][ch] = sum x, [tile][1][ch] = sum x^2 over the tile's frames of clip n.  `centered`: a tile has four rows, and
// [tile][2][ch] = sum (x - p), [tile][3][ch] = sum (x - p)^2 about p[ch] = x[n = 0][m][t = 0][v][c], a sample of the channel itself
// (data, not a statistic: every tile reads it from the input, no launch or host read in front), so those sums carry the channel's
// spread and not its offset -- raw sensor units (metres, pixels, gravity) enter here, and a float32 sum of x^2 loses var to mean^2;
// fgcn_bn_finalize chooses per channel (pivot = x, inner = V*C, outer = T*V*C).  The differences are exact in double and the <= 32
// terms of a tile are summed in double: the one rounding per tile is the float32 store, and a constant channel gives exact zeros
// about its pivot.  thread <-> channel, so consecutive threads of one body m read consecutive floats of a frame row
__global__ __launch_bounds__(256) void data_bn_stats_kernel(const float* x, float* partials, int M, int T, int VC, int chunks,
                                                            int centered) {
    const int n = blockIdx.x / chunks, t0 = (blockIdx.x % chunks) * DBN_T_CHUNK;
    const int t1 = min(t0 + DBN_T_CHUNK, T), MVC = M * VC, R = centered ? 4 : 2;
    for (int ch = threadIdx.x; ch < MVC; ch += blockDim.x) {
        const int m = ch / VC, vc = ch - m * VC;
        const double pivot = centered ? (double)x[(long long)m * T * VC + vc] : 0.0;
        const float* p = x + ((long long)(n * M + m) * T + t0) * VC + vc;
        float s1 = 0.f, s2 = 0.f;
        double c1 = 0.0, c2 = 0.0;
        for (int t = t0; t < t1; ++t, p += VC) {
            const float v = *p;
            s1 += v;
            s2 += v * v;
            const double d = (double)v - pivot;
            c1 += d;
            c2 += d * d;
        }
        partials[((long long)blockIdx.x * R + 0) * MVC + ch] = s1;
        partials[((long long)blockIdx.x * R + 1) * MVC + ch] = s2;
        if (centered) {
            partials[((long long)blockIdx.x * R + 2) * MVC + ch] = (float)c1;
            partials[((long long)blockIdx.x * R + 3) * MVC + ch] = (float)c2;
        }
    }
}

// one thread per (b, t, v) row: out[row][0..C) = x[row][c] * scale[ch] + shift[ch], out[row][C..Cp) = 0
__global__ __launch_bounds__(256) void data_bn_apply_kernel(const float* x, const float* vec, float* out, long long rows, int M,
                                                            int T, int V, int C, int Cp) {
    const int MVC = M * V * C;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(r % V);
        const int m = (int)((r / ((long long)T * V)) % M);
        const int ch0 = (m * V + v) * C;
        for (int c = 0; c < Cp; ++c)
            out[r * Cp + c] = c < C ? x[r * C + c] * vec[2 * MVC + ch0 + c] + vec[3 * MVC + ch0 + c] : 0.f;
    }
}

// partials[tile][0][ch] = sum dout, [tile][1][ch] = sum dout * (x - mean) * rstd  (d beta, d gamma)
__global__ __launch_bounds__(256) void data_bn_bwd_reduce_kernel(const float* dout, const float* x, const float* vec, float* partials,
                                                                 int M, int T, int V, int C, int Cp, int chunks) {
    const int VC = V * C, MVC = M * VC;
    const int n = blockIdx.x / chunks, t0 = (blockIdx.x % chunks) * DBN_T_CHUNK;
    const int t1 = min(t0 + DBN_T_CHUNK, T);
    for (int ch = threadIdx.x; ch < MVC; ch += blockDim.x) {
        const int m = ch / VC, vc = ch - m * VC, v = vc / C, c = vc - v * C;
        const float mean = vec[ch], rstd = vec[MVC + ch];
        float s1 = 0.f, s2 = 0.f;
        for (int t = t0; t < t1; ++t) {
            const long long row = ((long long)(n * M + m) * T + t) * V + v;
            const float d = dout[row * Cp + c];
            s1 += d;
            s2 += d * ((x[row * C + c] - mean) * rstd);
        }
        partials[((long long)blockIdx.x * 2 + 0) * MVC + ch] = s1;
        partials[((long long)blockIdx.x * 2 + 1) * MVC + ch] = s2;
    }
}

// dx = scale * (dout - sum_d / m - xhat * sum_dxhat / m)  (train)  |  scale * dout  (eval)
__global__ __launch_bounds__(256) void data_bn_bwd_apply_kernel(const float* dout, const float* x, const float* vec, const float* sums,
                                                                float* dx, long long rows, int M, int T, int V, int C, int Cp,
                                                                int train, float inv_m) {
    const int MVC = M * V * C;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(r % V);
        const int m = (int)((r / ((long long)T * V)) % M);
        const int ch0 = (m * V + v) * C;
        for (int c = 0; c < C; ++c) {
            const int ch = ch0 + c;
            float g = dout[r * Cp + c];
            if (train) {
                const float xh = (x[r * C + c] - vec[ch]) * vec[MVC + ch];
                g = g - sums[ch] * inv_m - xh * (sums[MVC + ch] * inv_m);
            }
            dx[r * C + c] = g * vec[2 * MVC + ch];
        }
    }
}

// ---- CrossEntropyLoss, mean reduction -------------------------------------------------------------------------------------------
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ONE workgroup (the row count is the clip batch): wave w takes rows w, w + 4, ...; probs = softmax(logits) is kept for the
// backward, row_loss[i] = logsumexp - logit[label]; rows labelled -100 (torch's ignore_index) do not count; any OTHER label outside
// [0, classes) -- torch raises a device assert there -- makes the row's loss, hence the batch loss and every gradient, NaN: a corrupt
// label fails loudly instead of being dropped from the mean;
// loss[0] = sum row_loss / n_valid, loss[1] = n_valid -- summed by wave 0 in a fixed order (lane l: rows l, l + 64, ...; then the
// butterfly): bitwise reproducible.
__global__ __launch_bounds__(256) void cross_entropy_fwd_kernel(const float* logits, const long long* labels, float* probs,
                                                                float* row_loss, float* loss, int rows, int classes, int ld) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = wave; i < rows; i += 4) {
        const float* z = logits + (long long)i * ld;
        float mx = -INFINITY;
        for (int c = lane; c < classes; c += 64) mx = fmaxf(mx, z[c]);
        mx = wmax(mx);
        float s = 0.f;
        for (int c = lane; c < classes; c += 64) s += expf(z[c] - mx);
        s = wsum(s);
        const float inv = 1.f / s;
        for (int c = lane; c < classes; c += 64) probs[(long long)i * classes + c] = expf(z[c] - mx) * inv;
        if (lane == 0) {
            const long long y = labels[i];
            row_loss[i] = (y >= 0 && y < classes) ? (mx + logf(s)) - z[y] : (y == -100 ? 0.f : NAN);
        }
    }
    __syncthreads();
    if (wave == 0) {
        float a = 0.f, cnt = 0.f;
        for (int i = lane; i < rows; i += 64) {
            const long long y = labels[i];
            const bool ok = y != -100;
            a += ok ? row_loss[i] : 0.f;
            cnt += ok ? 1.f : 0.f;
        }
        a = wsum(a);
        cnt = wsum(cnt);
        if (lane == 0) {
            loss[0] = cnt > 0.f ? a / cnt : NAN;      // torch: mean over no rows is NaN
            loss[1] = cnt;
        }
    }
}

// dlogits[i][c] = (probs[i][c] - [c == label_i]) * dloss / n_valid   (0 for ignored rows); columns [classes, ld_out) zero
__global__ __launch_bounds__(256) void cross_entropy_bwd_kernel(const float* probs, const long long* labels, const float* loss,
                                                                const float* dloss, float* dlogits, int rows, int classes,
                                                                int ld_out) {
    const float g = dloss[0] / loss[1];
    const long long n = (long long)rows * ld_out;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(e / ld_out), c = (int)(e - (long long)i * ld_out);
        const long long y = labels[i];
        float d = 0.f;
        if (c < classes && y >= 0 && y < classes) d = (probs[(long long)i * classes + c] - (c == y ? 1.f : 0.f)) * g;
        else if (c < classes && y != -100) d = NAN;             // a label outside [0, classes) that is not ignore_index
        dlogits[e] = d;
    }
}

// ---- CrossEntropyLoss with torch's arguments: weight, ignore_index, reduction, label_smoothing, class-probability targets ---------
// (include/fgcn.h, fgcn_ce_fwd; the two kernels above are the plain path and stay as they are.)
constexpr int CE_ROWS = 16;         // rows per workgroup: wave w takes rows 4 w .. 4 w + 3 of the group, one after the other

// PROB selects WHAT is loaded as the target (labels[i] | target[i][c]), HAS_W whether weight[] is loaded at all: template
// parameters, not branches around each load.  Per row i, lse = logsumexp(z_i):
//   index targets:  keep = y != ignore_index;  y in [0, classes) (checked BEFORE weight[y] / z[y] are addressed):
//                   row_loss = (1 - eps) w[y] (lse - z[y]) + eps/C sum_c w[c] (lse - z[c]),  row_scale = (1 - eps) w[y] + eps/C sum_c w[c],
//                   denominator term w[y];  ignored: all three 0;  any other y: row_loss = row_scale = NaN, denominator term 0.
//   probabilities:  t' = (1 - eps) t + eps/C;  row_loss = sum_c w[c] t'[c] (lse - z[c]),  row_scale = sum_c w[c] t'[c],  denominator term 1.
// partials[block] = {sum row_loss, sum denominator terms} over the block's <= 16 rows in row order, in float64, by one thread.
template <bool PROB, bool HAS_W>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* logits, const long long* labels, const float* target,
                                                     const float* weight, float* probs, float* row_loss, float* row_scale,
                                                     double* partials, int rows, int classes, int ld, int ld_t, long long ignore_index,
                                                     float eps) {
    __shared__ float sh_loss[CE_ROWS], sh_den[CE_ROWS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float smooth = eps / (float)classes, sharp = 1.f - eps;
    for (int k = 0; k < CE_ROWS / 4; ++k) {
        const int slot = wave * (CE_ROWS / 4) + k, i = blockIdx.x * CE_ROWS + slot;
        float rl = 0.f, den = 0.f;                                   // a row past the end adds nothing
        if (i < rows) {                                              // wave-uniform
            const float* z = logits + (long long)i * ld;
            float mx = -INFINITY;
            for (int c = lane; c < classes; c += 64) mx = fmaxf(mx, z[c]);
            mx = wmax(mx);
            float s = 0.f;
            for (int c = lane; c < classes; c += 64) s += expf(z[c] - mx);
            s = wsum(s);
            const float inv = 1.f / s, lse = mx + logf(s);
            if (probs)
                for (int c = lane; c < classes; c += 64) probs[(long long)i * classes + c] = expf(z[c] - mx) * inv;
            float rs;
            if constexpr (PROB) {
                const float* t = target + (long long)i * ld_t;
                float a = 0.f, b = 0.f;
                for (int c = lane; c < classes; c += 64) {
                    const float q = (HAS_W ? weight[c] : 1.f) * (sharp * t[c] + smooth);
                    a += q * (lse - z[c]);
                    b += q;
                }
                rl = wsum(a);
                rs = wsum(b);
                den = 1.f;
            } else {
                float a = 0.f, b = 0.f;                              // sum_c w[c] (lse - z[c]), sum_c w[c]: the smoothing term only
                if (eps > 0.f) {
                    for (int c = lane; c < classes; c += 64) {
                        const float w = HAS_W ? weight[c] : 1.f;
                        a += w * (lse - z[c]);
                        b += w;
                    }
                    a = wsum(a);
                    b = wsum(b);
                }
                const long long y = labels[i];
                if (y == ignore_index) {
                    rs = 0.f;
                } else if (y >= 0 && y < classes) {
                    const float wy = HAS_W ? weight[y] : 1.f;
                    rl = sharp * wy * (lse - z[y]) + smooth * a;
                    rs = sharp * wy + smooth * b;
                    den = wy;
                } else {
                    rl = rs = NAN;
                }
            }
            if (lane == 0) {
                row_loss[i] = rl;
                row_scale[i] = rs;
            }
        }
        if (lane == 0) {
            sh_loss[slot] = rl;
            sh_den[slot] = den;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, d = 0.0;
        for (int r = 0; r < CE_ROWS; ++r) {
            a += (double)sh_loss[r];
            d += (double)sh_den[r];
        }
        partials[2 * blockIdx.x] = a;
        partials[2 * blockIdx.x + 1] = d;
    }
}

// One workgroup: the partials are staged through LDS 256 at a time and added by ONE thread in index order, in float64 -- the
// order of the additions is the order of the rows, whatever order the workgroups of ce_fwd_kernel ran in.
// loss[0] = mean ? sum / denominator (NaN for a zero denominator: every row ignored, every present weight zero) : sum; loss[1] = denominator.
__global__ __launch_bounds__(256) void ce_finish_kernel(const double* partials, float* loss, int nparts, int mean) {
    __shared__ double sh[2 * 256];
    double a = 0.0, d = 0.0;
    for (int p0 = 0; p0 < nparts; p0 += 256) {
        const int n = min(256, nparts - p0);
        if ((int)threadIdx.x < n) {
            sh[2 * threadIdx.x] = partials[2 * (p0 + threadIdx.x)];
            sh[2 * threadIdx.x + 1] = partials[2 * (p0 + threadIdx.x) + 1];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int p = 0; p < n; ++p) {
                a += sh[2 * p];
                d += sh[2 * p + 1];
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = mean ? (d != 0.0 ? (float)(a / d) : NAN) : (float)a;
        loss[1] = (float)d;
    }
}

// dlogits[i][c] = g_i (probs[i][c] row_scale[i] - a_ic), a_ic = w[c] q_ic (q: the smoothed one-hot | t'); g_i = dloss[0] / loss[1]
// (mean; NaN for a zero denominator), dloss[0] (sum), dloss[i] (none).  An ignored row is written as 0 whatever g is; a label outside [0, classes) that is not
// ignore_index has row_scale = NaN, hence a NaN row; columns [classes, ld_out) zero.
template <bool PROB, bool HAS_W>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* probs, const long long* labels, const float* target,
                                                     const float* weight, const float* row_scale, const float* loss,
                                                     const float* dloss, float* dlogits, int rows, int classes, int ld_t, int ld_out,
                                                     long long ignore_index, float eps, int reduction) {
    const float smooth = eps / (float)classes, sharp = 1.f - eps;
    // (mean over a zero denominator: torch's gradient of a row that is not ignored is NaN -- 0/0 -- there, also where g * (...) would be inf)
    const float g_all = reduction == FGCN_CE_MEAN ? (loss[1] != 0.f ? dloss[0] / loss[1] : NAN) : dloss[0];
    const long long n = (long long)rows * ld_out;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(e / ld_out), c = (int)(e - (long long)i * ld_out);
        float d = 0.f;
        if (c < classes) {
            const float g = reduction == FGCN_CE_NONE ? dloss[i] : g_all;
            const float w = HAS_W ? weight[c] : 1.f;
            const float ps = probs[(long long)i * classes + c] * row_scale[i];
            if constexpr (PROB) {
                d = g * (ps - w * (sharp * target[(long long)i * ld_t + c] + smooth));
            } else {
                const long long y = labels[i];
                if (y != ignore_index) d = g * (ps - w * ((c == y ? sharp : 0.f) + smooth));
            }
        }
        dlogits[e] = d;
    }
}

}  // namespace fgcn

using namespace fgcn;

static unsigned stream_blocks(long long n) {
    const long long b = cdiv(n, 256);
    return (unsigned)(b < 4096 ? b : 4096);
}

extern "C" int fgcn_data_bn_tiles(int N, int T) { return N * (int)cdiv(T, DBN_T_CHUNK); }

static int check_dbn(const char* what, int N, int M, int T, int V, int C, int Cp) {
    FGCN_REQUIRE(N > 0 && M > 0 && T > 0 && V > 0 && C > 0 && Cp >= C, FGCN_E_BADARG, "%s: bad shape N=%d M=%d T=%d V=%d C=%d Cp=%d", what,
                 N, M, T, V, C, Cp);
    FGCN_REQUIRE((long long)N * M * T * V * Cp < (1ll << 31) && (long long)N * cdiv(T, DBN_T_CHUNK) < (1ll << 31), FGCN_E_BADARG,
                 "%s: tensor too large", what);
    return FGCN_OK;
}

extern "C" int fgcn_data_bn_stats(const float* x, float* partials, int N, int M, int T, int V, int C, int centered, void* stream) {
    FGCN_REQUIRE(x && partials, FGCN_E_BADARG, "data_bn_stats: null pointer");
    if (int e = check_dbn("data_bn_stats", N, M, T, V, C, C)) return e;
    const int chunks = (int)cdiv(T, DBN_T_CHUNK);
    hipLaunchKernelGGL(data_bn_stats_kernel, dim3((unsigned)(N * chunks)), dim3(256), 0, (hipStream_t)stream, x, partials, M, T, V * C,
                       chunks, centered);
    return launch_status("data_bn_stats");
}

extern "C" int fgcn_data_bn_apply(const float* x, const float* vec, float* out, int N, int M, int T, int V, int C, int Cp,
                                  void* stream) {
    FGCN_REQUIRE(x && vec && out, FGCN_E_BADARG, "data_bn_apply: null pointer");
    if (int e = check_dbn("data_bn_apply", N, M, T, V, C, Cp)) return e;
    const long long rows = (long long)N * M * T * V;
    hipLaunchKernelGGL(data_bn_apply_kernel, dim3(stream_blocks(rows)), dim3(256), 0, (hipStream_t)stream, x, vec, out, rows, M, T, V, C,
                       Cp);
    return launch_status("data_bn_apply");
}

extern "C" int fgcn_data_bn_bwd_reduce(const float* dout, const float* x, const float* vec, float* partials, int N, int M, int T,
                                       int V, int C, int Cp, void* stream) {
    FGCN_REQUIRE(dout && x && vec && partials, FGCN_E_BADARG, "data_bn_bwd_reduce: null pointer");
    if (int e = check_dbn("data_bn_bwd_reduce", N, M, T, V, C, Cp)) return e;
    const int chunks = (int)cdiv(T, DBN_T_CHUNK);
    hipLaunchKernelGGL(data_bn_bwd_reduce_kernel, dim3((unsigned)(N * chunks)), dim3(256), 0, (hipStream_t)stream, dout, x, vec, partials,
                       M, T, V, C, Cp, chunks);
    return launch_status("data_bn_bwd_reduce");
}

extern "C" int fgcn_data_bn_bwd_apply(const float* dout, const float* x, const float* vec, const float* sums, float* dx, int N, int M,
                                      int T, int V, int C, int Cp, int train, void* stream) {
    FGCN_REQUIRE(dout && vec && dx && (!train || (x && sums)), FGCN_E_BADARG, "data_bn_bwd_apply: null pointer");
    if (int e = check_dbn("data_bn_bwd_apply", N, M, T, V, C, Cp)) return e;
    const long long rows = (long long)N * M * T * V;
    hipLaunchKernelGGL(data_bn_bwd_apply_kernel, dim3(stream_blocks(rows)), dim3(256), 0, (hipStream_t)stream, dout, x, vec, sums, dx,
                       rows, M, T, V, C, Cp, train, 1.f / (float)((long long)N * T));
    return launch_status("data_bn_bwd_apply");
}

extern "C" int fgcn_cross_entropy_fwd(const float* logits, const long long* labels, float* probs, float* row_loss, float* loss,
                                      int rows, int classes, int ld, void* stream) {
    FGCN_REQUIRE(logits && labels && probs && row_loss && loss && rows > 0 && classes > 0 && ld >= classes, FGCN_E_BADARG,
                 "cross_entropy_fwd: bad argument (rows=%d classes=%d ld=%d)", rows, classes, ld);
    hipLaunchKernelGGL(cross_entropy_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, probs, row_loss, loss, rows,
                       classes, ld);
    return launch_status("cross_entropy_fwd");
}

extern "C" int fgcn_cross_entropy_bwd(const float* probs, const long long* labels, const float* loss, const float* dloss,
                                      float* dlogits, int rows, int classes, int ld_out, void* stream) {
    FGCN_REQUIRE(probs && labels && loss && dloss && dlogits && rows > 0 && classes > 0 && ld_out >= classes, FGCN_E_BADARG,
                 "cross_entropy_bwd: bad argument (rows=%d classes=%d ld_out=%d)", rows, classes, ld_out);
    hipLaunchKernelGGL(cross_entropy_bwd_kernel, dim3(stream_blocks((long long)rows * ld_out)), dim3(256), 0, (hipStream_t)stream, probs,
                       labels, loss, dloss, dlogits, rows, classes, ld_out);
    return launch_status("cross_entropy_bwd");
}

extern "C" long long fgcn_ce_workspace_bytes(int rows) { return rows > 0 ? cdiv(rows, CE_ROWS) * 2 * (long long)sizeof(double) : 0; }

// the checks fgcn_ce_fwd and fgcn_ce_bwd share: one kind of target, the shape, eps in [0, 1] (a NaN fails the comparison), the reduction
static int check_ce(const char* what, const long long* labels, const float* target, int rows, int classes, int ld_t, float eps,
                    int reduction) {
    FGCN_REQUIRE((labels != nullptr) != (target != nullptr), FGCN_E_BADARG, "%s: exactly one of labels / target", what);
    FGCN_REQUIRE(rows > 0 && classes > 0 && (!target || ld_t >= classes), FGCN_E_BADARG, "%s: bad shape (rows=%d classes=%d ld_target=%d)",
                 what, rows, classes, ld_t);
    FGCN_REQUIRE(eps >= 0.f && eps <= 1.f, FGCN_E_BADARG, "%s: label_smoothing %g outside [0, 1]", what, (double)eps);
    FGCN_REQUIRE(reduction == FGCN_CE_MEAN || reduction == FGCN_CE_SUM || reduction == FGCN_CE_NONE, FGCN_E_BADARG,
                 "%s: unknown reduction %d", what, reduction);
    return FGCN_OK;
}

extern "C" int fgcn_ce_fwd(const float* logits, const long long* labels, const float* target, const float* weight, float* probs,
                           float* row_loss, float* row_scale, float* loss, void* workspace, int rows, int classes, int ld,
                           int ld_target, long long ignore_index, float label_smoothing, int reduction, void* stream) {
    FGCN_REQUIRE(logits && row_loss && row_scale && loss && workspace, FGCN_E_BADARG, "ce_fwd: null pointer");
    if (int e = check_ce("ce_fwd", labels, target, rows, classes, ld_target, label_smoothing, reduction)) return e;
    FGCN_REQUIRE(ld >= classes, FGCN_E_BADARG, "ce_fwd: ld=%d < classes=%d", ld, classes);
    FGCN_REQUIRE((uintptr_t)workspace % 8 == 0, FGCN_E_ALIGN, "ce_fwd: workspace not 8-byte aligned");
    const int nparts = (int)cdiv(rows, CE_ROWS);
    auto kernel = target ? (weight ? ce_fwd_kernel<true, true> : ce_fwd_kernel<true, false>)
                         : (weight ? ce_fwd_kernel<false, true> : ce_fwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, logits, labels, target, weight, probs, row_loss,
                       row_scale, (double*)workspace, rows, classes, ld, ld_target, ignore_index, label_smoothing);
    if (int e = launch_status("ce_fwd")) return e;
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, loss, nparts,
                       (int)(reduction == FGCN_CE_MEAN));
    return launch_status("ce_fwd (finish)");
}

extern "C" int fgcn_ce_bwd(const float* probs, const long long* labels, const float* target, const float* weight,
                           const float* row_scale, const float* loss, const float* dloss, float* dlogits, int rows, int classes,
                           int ld_target, int ld_out, long long ignore_index, float label_smoothing, int reduction, void* stream) {
    FGCN_REQUIRE(probs && row_scale && loss && dloss && dlogits, FGCN_E_BADARG, "ce_bwd: null pointer");
    if (int e = check_ce("ce_bwd", labels, target, rows, classes, ld_target, label_smoothing, reduction)) return e;
    FGCN_REQUIRE(ld_out >= classes, FGCN_E_BADARG, "ce_bwd: ld_out=%d < classes=%d", ld_out, classes);
    auto kernel = target ? (weight ? ce_bwd_kernel<true, true> : ce_bwd_kernel<true, false>)
                         : (weight ? ce_bwd_kernel<false, true> : ce_bwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(stream_blocks((long long)rows * ld_out)), dim3(256), 0, (hipStream_t)stream, probs, labels, target,
                       weight, row_scale, loss, dloss, dlogits, rows, classes, ld_target, ld_out, ignore_index, label_smoothing,
                       reduction);
    return launch_status("ce_bwd");
}
