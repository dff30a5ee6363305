// Joint-contracting kernels of the AGCN block for skeleton graphs of 33 .. 64 joints (FGCN_MAX_V_WIDE).
//   joint_mix_wide     : out_t (V x ch) (+)= M (V x V) . in_t (V x ch)      per sample n and frame t   (MFMA 32x32x2 f32)
//   joint_gram_wide    : G (V x V) += in1_t (V x ch) . in2_t^T (ch x V)      summed over frames and channels
//   adj_softmax_*_wide : the column softmax of the data-dependent adjacency on 64 x 64 matrices.
// The 32-joint kernels (fgcn_joint.hip) put the joint index on one 32-wide MFMA dimension; here a 64-joint matrix is a 2 x 2 grid of
// 32 x 32 MFMA blocks.  The graph sizes up to 32 joints never reach this file: the host picks it only for V > FGCN_MAX_V.
// Same formulas, same operand precision (f32 products, f32 accumulation) in every math mode, like the 32-joint forms.
#include "fgcn_tile.hpp"

namespace fgcn {

constexpr int WV = 64;          // joints of a wide matrix
constexpr int WS = WV + 1;      // LDS row stride of a staged 64 x 64 matrix (both orientations read conflict-free)
constexpr int WIMG = WV * WS;   // floats per staged matrix
constexpr int WIDE_MAX_MATS = 3;

struct MixWP {
    const float* in;
    float* out;
    const float* mats;
    int B, T, V, ld_in, ld_out, n_mats, mats_batched, n_items, t_chunk;
    unsigned in_bytes, out_bytes;
    struct Item {  // dword fields: scalar loads
        int out_c, nch, nterms, mat[3], tr[3], in_c[3];
    } items[FGCN_MIX_MAX_ITEMS];
};

// One workgroup = (sample n, chunk of frames); wave w takes frames t0 + w, t0 + w + 4, ...  Lane (l31, h): channel l31 of the item's
// group and k-half h.  Per term: KS k-steps of two joints each; the input rows k = 2s + h are loaded once (buffer loads, joints >= V and
// absent channels through the out-of-range sentinel, i.e. zeros) and feed both 32-row output blocks.  The matrices sit in LDS untransposed
// with row stride 65: A[u][k] = M[u][k] (transpose 0) or M[k][u] (transpose 1) is one ds_read_b32 per lane, conflict-free either way.
// KS (compile time: branch-free MFMA chains) = 24 for V <= 48, else 32; the padding steps multiply zeros.
template <bool ACC, int KS>
__global__ __launch_bounds__(256) void joint_mix_wide_kernel(MixWP p) {
    __shared__ float img[WIDE_MAX_MATS * WIMG];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int n = blockIdx.y;
    const int t0 = blockIdx.x * p.t_chunk;
    const int t1 = min(t0 + p.t_chunk, p.T);
    const int V = p.V;

    const float* msrc = p.mats + (p.mats_batched ? (long long)n * p.n_mats * V * V : 0);
    for (int e = tid; e < p.n_mats * WV * WV; e += 256) {
        const int m = e >> 12, r = (e >> 6) & 63, c = e & 63;
        img[m * WIMG + r * WS + c] = (r < V && c < V) ? msrc[((long long)m * V + r) * V + c] : 0.f;
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rin = buffer_rsrc(p.in, p.in_bytes);
    const __amdgpu_buffer_rsrc_t rout = buffer_rsrc(p.out, p.out_bytes);
    constexpr unsigned OOB = 0x80000000u;

    for (int t = t0 + wave; t < t1; t += 4) {
        const unsigned frame = (unsigned)(n * p.T + t) * (unsigned)V;
        const unsigned fin = frame * (unsigned)p.ld_in * 4u, fout = frame * (unsigned)p.ld_out * 4u;
        for (int it = 0; it < p.n_items; ++it) {
            const int nch = __builtin_amdgcn_readfirstlane(p.items[it].nch);
            const bool lane_ok = l31 < nch;
            const unsigned so_out = __builtin_amdgcn_readfirstlane(fout + (unsigned)p.items[it].out_c * 4u);
            f32x16 acc[2] = {zero16(), zero16()};
            const int nterms = __builtin_amdgcn_readfirstlane(p.items[it].nterms);
            for (int tr = 0; tr < nterms; ++tr) {
                const unsigned so_in = __builtin_amdgcn_readfirstlane(fin + (unsigned)p.items[it].in_c[tr] * 4u);
                float bv[KS];
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const int k = 2 * s + h;
                    const unsigned off = (lane_ok && k < V) ? (unsigned)(k * p.ld_in + l31) * 4u : OOB;
                    bv[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, off, so_in, 0));
                }
                // A[u = 32 ub + l31][k = 2 s + h]: (su, sk) = strides of u and k in the staged image
                const int trn = __builtin_amdgcn_readfirstlane(p.items[it].tr[tr]);
                const int su = trn ? 1 : WS, sk = trn ? WS : 1;
                const float* a = &img[__builtin_amdgcn_readfirstlane(p.items[it].mat[tr]) * WIMG + l31 * su + h * sk];
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    acc[0] = mfma32(a[2 * s * sk], bv[s], acc[0]);
                    acc[1] = mfma32(a[32 * su + 2 * s * sk], bv[s], acc[1]);
                }
            }
#pragma unroll
            for (int ub = 0; ub < 2; ++ub) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int u = 32 * ub + acc_row(r, lane);
                    const unsigned off = (lane_ok && u < V) ? (unsigned)(u * p.ld_out + l31) * 4u : OOB;
                    float v = acc[ub][r];
                    if constexpr (ACC) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rout, off, so_out, 0));
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, off, so_out, 0);
                }
            }
        }
    }
}

struct GramWP {
    const float* in1;
    const float* in2;
    float* partial;
    int B, T, V, ld1, ld2, t_chunk, n_items;
    unsigned in1_bytes, in2_bytes;
    struct Item {
        int c1, c2, width;
    } items[3];
};

// One workgroup = (sample n, chunk of frames, item); wave w takes every fourth frame of the chunk.  Lane (l31, h) holds 4 consecutive
// channels 8 q + 4 h .. + 3 of joint row 32 vb + l31 of both operands (16-byte buffer loads); the 2 x 2 output blocks accumulate in
// 64 registers.  The four waves' sums are added in a fixed order through LDS, one block at a time: bitwise reproducible.
__global__ __launch_bounds__(256, 2) void joint_gram_wide_kernel(GramWP p) {
    __shared__ float red[4 * 1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int n = blockIdx.y, chunk = blockIdx.x, it = blockIdx.z;
    const int t0 = chunk * p.t_chunk;
    const int t1 = min(t0 + p.t_chunk, p.T);
    const int V = p.V;
    const int c1 = __builtin_amdgcn_readfirstlane(p.items[it].c1), c2 = __builtin_amdgcn_readfirstlane(p.items[it].c2);
    const int width = __builtin_amdgcn_readfirstlane(p.items[it].width);
    const __amdgpu_buffer_rsrc_t r1 = buffer_rsrc(p.in1, p.in1_bytes);
    const __amdgpu_buffer_rsrc_t r2 = buffer_rsrc(p.in2, p.in2_bytes);
    constexpr unsigned OOB = 0x80000000u;
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    const int nq = (width + 7) >> 3;
    for (int t = t0 + wave; t < t1; t += 4) {
        const unsigned row0 = (unsigned)(n * p.T + t) * (unsigned)V;
        for (int q = 0; q < nq; ++q) {
            const bool ch_ok = 8 * q + 4 * h < width;   // widths are multiples of 4
            f32x4 a[2], b[2];
#pragma unroll
            for (int vb = 0; vb < 2; ++vb) {
                const int v = 32 * vb + l31;
                const bool ok = ch_ok && v < V;
                const unsigned o1 = ok ? ((row0 + v) * (unsigned)p.ld1 + c1 + 8 * q + 4 * h) * 4u : OOB;
                const unsigned o2 = ok ? ((row0 + v) * (unsigned)p.ld2 + c2 + 8 * q + 4 * h) * 4u : OOB;
                a[vb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r1, o1, 0, 0));
                b[vb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r2, o2, 0, 0));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int vb = 0; vb < 2; ++vb)
#pragma unroll
                    for (int wb = 0; wb < 2; ++wb) acc[vb][wb] = mfma32(a[vb][e], b[wb][e], acc[vb][wb]);
        }
    }
    float* dst = p.partial + (((long long)n * gridDim.x + chunk) * p.n_items + it) * (WV * WV);
#pragma unroll
    for (int vb = 0; vb < 2; ++vb) {
#pragma unroll
        for (int wb = 0; wb < 2; ++wb) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[vb][wb][r];
            __syncthreads();
            for (int e = tid; e < 1024; e += 256) {
                const float s = red[e] + red[1024 + e] + red[2048 + e] + red[3072 + e];
                const int r = e >> 6, l = e & 63;
                dst[(32 * vb + acc_row(r, l)) * WV + 32 * wb + (l & 31)] = s;
            }
        }
    }
}

// sum of the nchunk per-chunk partial matrices at one element, fixed order (as fgcn_joint.hip's sum_chunk_partials)
__device__ __forceinline__ float sum_chunks_wide(const float* src, int nchunk, long long stride) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int c = 0;
    for (; c + 8 <= nchunk; c += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = src[(long long)(c + u) * stride];
        s0 += x[0] + x[4];
        s1 += x[1] + x[5];
        s2 += x[2] + x[6];
        s3 += x[3] + x[7];
    }
    for (; c < nchunk; ++c) s0 += src[(long long)c * stride];
    return (s0 + s1) + (s2 + s3);
}

// One 1024-thread workgroup per (sample, subset): thread e owns entries e, e + 1024, e + 2048, e + 3072 of the 64 x 64 matrix
// (row v = entry / 64, column w = entry % 64); the column statistics (softmax over v = dim -2) are formed once per column by 64 threads.
__global__ __launch_bounds__(1024) void adj_softmax_fwd_wide_kernel(const float* partial, int nchunk, float scale, const float* adj_a,
                                                                    const float* adj_b, float* c_out, float* a_hat, int K, int V,
                                                                    int use_softmax) {
    __shared__ float S[WV][WS];
    __shared__ float cmax[WV], cden[WV];
    const int n = blockIdx.x / K, k = blockIdx.x - n * K;
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = threadIdx.x + 1024 * j, v = e >> 6, w = e & 63;
        const bool in = v < V && w < V;
        const long long o = ((long long)(n * K + k) * V + v) * V + w;
        if (!use_softmax) {
            if (in) a_hat[o] = adj_a[((long long)k * V + v) * V + w] + (adj_b ? adj_b[((long long)k * V + v) * V + w] : 0.f);
            continue;
        }
        s[j] = scale * sum_chunks_wide(partial + ((long long)n * nchunk * K + k) * (WV * WV) + e, nchunk, (long long)K * WV * WV);
        S[v][w] = in ? s[j] : -INFINITY;
    }
    if (!use_softmax) return;
    __syncthreads();
    if (threadIdx.x < WV) {
        const int w = threadIdx.x;
        float mx = -INFINITY;
        for (int u = 0; u < V; ++u) mx = fmaxf(mx, S[u][w]);
        float den = 0.f;
        for (int u = 0; u < V; ++u) den += expf(S[u][w] - mx);
        cmax[w] = mx;
        cden[w] = den;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = threadIdx.x + 1024 * j, v = e >> 6, w = e & 63;
        if (v < V && w < V) {
            const long long o = ((long long)(n * K + k) * V + v) * V + w;
            const float ab = adj_a[((long long)k * V + v) * V + w] + (adj_b ? adj_b[((long long)k * V + v) * V + w] : 0.f);
            const float c = expf(s[j] - cmax[w]) / cden[w];
            c_out[o] = c;
            a_hat[o] = c + ab;
        }
    }
}

__global__ __launch_bounds__(1024) void adj_softmax_bwd_wide_kernel(const float* partial, int nchunk, float scale, const float* c_in,
                                                                    float* d_a_hat, float* d_s, int K, int V) {
    __shared__ float P[WV][WS];
    __shared__ float cdot[WV];
    const int n = blockIdx.x / K, k = blockIdx.x - n * K;
    float dc[4], cv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = threadIdx.x + 1024 * j, v = e >> 6, w = e & 63;
        const bool in = v < V && w < V;
        const long long o = ((long long)(n * K + k) * V + v) * V + w;
        dc[j] = sum_chunks_wide(partial + ((long long)n * nchunk * K + k) * (WV * WV) + e, nchunk, (long long)K * WV * WV);
        if (in) d_a_hat[o] = dc[j];
        cv[j] = (in && c_in) ? c_in[o] : 0.f;
        P[v][w] = cv[j] * dc[j];
    }
    if (!c_in || !d_s) return;
    __syncthreads();
    if (threadIdx.x < WV) {
        const int w = threadIdx.x;
        float dot = 0.f;
        for (int u = 0; u < V; ++u) dot += P[u][w];
        cdot[w] = dot;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = threadIdx.x + 1024 * j, v = e >> 6, w = e & 63;
        if (v < V && w < V) d_s[((long long)(n * K + k) * V + v) * V + w] = scale * cv[j] * (dc[j] - cdot[w]);
    }
}

}  // namespace fgcn

using namespace fgcn;

static int wide_t_chunk(int B, int T) {
    // as the 32-joint mix: enough workgroups to fill the CUs a few times over, at least 4 frames (one per wave) per workgroup
    int chunk = 32;
    while (chunk > 4 && (long long)B * cdiv(T, chunk) < 1024) chunk >>= 1;
    return chunk;
}

#define FGCN_WIDE_V_CHECK(what, V)                                                                                                  \
    FGCN_REQUIRE((V) > 0 && (V) <= FGCN_MAX_V_WIDE, FGCN_E_BADARG, "%s: V=%d joints outside 1..%d (FGCN_MAX_V_WIDE, the joint limit of " \
                 "the AGCN block)", what, (int)(V), FGCN_MAX_V_WIDE)

extern "C" int fgcn_joint_mix_wide(const float* in, float* out, const float* mats, int B, int T, int V, int ld_in, int ld_out,
                                   int n_mats, int mats_batched, const fgcn_mixv_item* items, int n_items, int accumulate,
                                   void* stream) {
    FGCN_REQUIRE(in && out && mats && items, FGCN_E_BADARG, "joint_mix_wide: null pointer");
    FGCN_WIDE_V_CHECK("joint_mix_wide", V);
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0, FGCN_E_BADARG, "joint_mix_wide: bad B/T (%d,%d)", B, T);
    FGCN_REQUIRE(n_mats >= 1 && n_mats <= WIDE_MAX_MATS && n_items >= 1 && n_items <= FGCN_MIX_MAX_ITEMS, FGCN_E_BADARG,
                 "joint_mix_wide: n_mats=%d n_items=%d out of range", n_mats, n_items);
    FGCN_REQUIRE(ld_in > 0 && ld_out > 0 && aligned16(in) && aligned16(out), FGCN_E_ALIGN, "joint_mix_wide: 16-byte alignment");
    const long long in_bytes = (long long)B * T * V * ld_in * 4, out_bytes = (long long)B * T * V * ld_out * 4;
    FGCN_REQUIRE(fits_buffer(in_bytes) && fits_buffer(out_bytes), FGCN_E_BADARG, "joint_mix_wide: tensors must be smaller than 2 GiB");
    MixWP p;
    p.in = in; p.out = out; p.mats = mats;
    p.in_bytes = (unsigned)in_bytes; p.out_bytes = (unsigned)out_bytes;
    p.B = B; p.T = T; p.V = V; p.ld_in = ld_in; p.ld_out = ld_out;
    p.n_mats = n_mats; p.mats_batched = mats_batched; p.n_items = n_items;
    p.t_chunk = wide_t_chunk(B, T);
    for (int i = 0; i < n_items; ++i) {
        const fgcn_mixv_item& it = items[i];
        FGCN_REQUIRE(it.nterms >= 1 && it.nterms <= 3 && it.nch >= 1 && it.nch <= 32 && it.out_c >= 0 && it.out_c + it.nch <= ld_out,
                     FGCN_E_BADARG, "joint_mix_wide: item %d malformed (1..32 channels inside the output row)", i);
        p.items[i].out_c = it.out_c;
        p.items[i].nch = it.nch;
        p.items[i].nterms = it.nterms;
        for (int t = 0; t < 3; ++t) {
            if (t < it.nterms)
                FGCN_REQUIRE(it.term[t].mat >= 0 && it.term[t].mat < n_mats && it.term[t].in_c >= 0 && it.term[t].in_c + it.nch <= ld_in,
                             FGCN_E_BADARG, "joint_mix_wide: item %d term %d malformed", i, t);
            p.items[i].mat[t] = t < it.nterms ? it.term[t].mat : 0;
            p.items[i].tr[t] = t < it.nterms ? (it.term[t].transpose ? 1 : 0) : 0;
            p.items[i].in_c[t] = t < it.nterms ? it.term[t].in_c : 0;
        }
    }
    dim3 grid((unsigned)cdiv(T, p.t_chunk), (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
    const bool short_k = V <= 48;
    if (accumulate) {
        if (short_k) hipLaunchKernelGGL((joint_mix_wide_kernel<true, 24>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((joint_mix_wide_kernel<true, 32>), grid, dim3(256), 0, st, p);
    } else {
        if (short_k) hipLaunchKernelGGL((joint_mix_wide_kernel<false, 24>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((joint_mix_wide_kernel<false, 32>), grid, dim3(256), 0, st, p);
    }
    return launch_status("joint_mix_wide");
}

extern "C" int fgcn_joint_gram_wide(const float* in1, const float* in2, float* partial, int B, int T, int V, int ld1, int ld2,
                                    int t_chunk, const fgcn_gram_item* items, int n_items, void* stream) {
    FGCN_REQUIRE(in1 && in2 && partial && items, FGCN_E_BADARG, "joint_gram_wide: null pointer");
    FGCN_WIDE_V_CHECK("joint_gram_wide", V);
    FGCN_REQUIRE(B > 0 && B <= 65535 && T > 0 && t_chunk > 0, FGCN_E_BADARG, "joint_gram_wide: bad sizes B=%d T=%d t_chunk=%d", B, T,
                 t_chunk);
    FGCN_REQUIRE(n_items >= 1 && n_items <= 3, FGCN_E_BADARG, "joint_gram_wide: needs 1..3 items (n_items=%d)", n_items);
    FGCN_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && aligned16(in1) && aligned16(in2), FGCN_E_ALIGN,
                 "joint_gram_wide: strides/pointers must be 16-byte aligned");
    const long long b1 = (long long)B * T * V * ld1 * 4, b2 = (long long)B * T * V * ld2 * 4;
    FGCN_REQUIRE(fits_buffer(b1) && fits_buffer(b2), FGCN_E_BADARG, "joint_gram_wide: operands must be smaller than 2 GiB");
    GramWP p;
    p.in1 = in1; p.in2 = in2; p.partial = partial;
    p.in1_bytes = (unsigned)b1; p.in2_bytes = (unsigned)b2;
    p.B = B; p.T = T; p.V = V; p.ld1 = ld1; p.ld2 = ld2; p.t_chunk = t_chunk; p.n_items = n_items;
    for (int i = 0; i < n_items; ++i) {
        FGCN_REQUIRE(items[i].mat == i && items[i].width > 0 && items[i].width % 4 == 0 && items[i].c1 >= 0 && items[i].c2 >= 0 &&
                         items[i].c1 % 4 == 0 && items[i].c2 % 4 == 0 && items[i].c1 + items[i].width <= ld1 &&
                         items[i].c2 + items[i].width <= ld2,
                     FGCN_E_BADARG, "joint_gram_wide: item %d malformed", i);
        p.items[i].c1 = items[i].c1; p.items[i].c2 = items[i].c2; p.items[i].width = items[i].width;
    }
    dim3 grid((unsigned)cdiv(T, t_chunk), (unsigned)B, (unsigned)n_items);
    hipLaunchKernelGGL(joint_gram_wide_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return launch_status("joint_gram_wide");
}

extern "C" int fgcn_adj_softmax_fwd_wide(const float* partial, int nchunk, float scale, const float* adj_a, const float* adj_b,
                                         float* c_out, float* a_hat, int B, int K, int V, int use_softmax, void* stream) {
    FGCN_REQUIRE(adj_a && a_hat && B > 0 && K > 0, FGCN_E_BADARG, "adj_softmax_fwd_wide: bad argument");
    FGCN_WIDE_V_CHECK("adj_softmax_fwd_wide", V);
    FGCN_REQUIRE(!use_softmax || (partial && c_out && nchunk > 0), FGCN_E_BADARG, "adj_softmax_fwd_wide: missing partials");
    hipLaunchKernelGGL(adj_softmax_fwd_wide_kernel, dim3((unsigned)(B * K)), dim3(1024), 0, (hipStream_t)stream, partial, nchunk, scale,
                       adj_a, adj_b, c_out, a_hat, K, V, use_softmax);
    return launch_status("adj_softmax_fwd_wide");
}

extern "C" int fgcn_adj_softmax_bwd_wide(const float* partial, int nchunk, float scale, const float* c_in, float* d_a_hat, float* d_s,
                                         int B, int K, int V, void* stream) {
    FGCN_REQUIRE(partial && d_a_hat && nchunk > 0 && B > 0 && K > 0, FGCN_E_BADARG, "adj_softmax_bwd_wide: bad argument");
    FGCN_WIDE_V_CHECK("adj_softmax_bwd_wide", V);
    hipLaunchKernelGGL(adj_softmax_bwd_wide_kernel, dim3((unsigned)(B * K)), dim3(1024), 0, (hipStream_t)stream, partial, nchunk, scale,
                       c_in, d_a_hat, d_s, K, V);
    return launch_status("adj_softmax_bwd_wide");
}
