// The input stage of the RGB patch-feature modes (reference torch_src/models/mmargcn/early_fusion_models.py:48-90, 163-210):
// per joint row p (P floats of precomputed CNN features) the reducer q = W2 . (W1 . p + b1) + b2 (two nn.Linear, no activation
// between), zeros for the joints v >= Vp that have no patch (the skeleton + IMU graph's IMU joints), then the early fusion with the
// skeleton row s: concatenate [s | q], sum s + q, product s * q, average (s + q) / 2.  The result z (N, M, T, V, C) is what data_bn
// reads; the statistics partials of data_bn are formed over it by fgcn_data_bn_stats itself, so they are the same tiles, in the same
// summation order, as the composed route's.
//
// Forward: one workgroup per 32 patch rows.  The rows are staged once into LDS; the four waves take the H / 32 hidden chunks in turn,
// form h^T (32 hidden x 32 rows) on the f32 MFMA, add b1 and feed h^T straight from the accumulator registers into q^T += W2 . h^T
// (the accumulator layout of h^T is the B-operand layout of the second product).  The hidden tensor never leaves the registers.
// The four waves' q^T are summed in a fixed order through LDS.
//
// Backward: workgroup (hidden chunk, slab of row blocks); the chunk index runs fastest, so the H / 32 workgroups that read one slab's
// patch rows are adjacent in launch order and share them through L2.  Per 32-row block: dq from dz through the fusion's derivative
// (v < Vp only), dh = dq . W2[:, chunk] (its accumulator layout is the A-operand layout of dh^T), dW1[chunk] += dh^T . p (each wave a
// quarter of P), h^T recomputed (each wave a quarter of the contraction, summed through LDS), dW2[:, chunk] += dq^T . h, db1, db2.
// Every workgroup writes its slab's partials; fgcn_reduce_multi sums the slabs in a fixed order.
//
// Arithmetic: every MFMA is v_mfma_f32_32x32x2_f32 with four consecutive contraction indices per 16-byte fragment read (lane half h holds
// k = 8q + 4h + e).  FGCN_MATH_F32, FGCN_MATH_BF16X3 and its f16x2 products: exact float32 operands (this stage is a few percent of
// the step's matrix work; the split forms would only add passes).  FGCN_MATH_BF16: every operand rounded to bfloat16 (RNE) once, as it
// is staged or as its fragment is formed; products of two bfloat16 values are exact in the float32 accumulator, so this is the
// arithmetic of the bf16 MFMA with float32 accumulation.  Bias terms and every sum stay float32.
#include "fgcn_common.hpp"

namespace fgcn {

constexpr int PI_ROWS = 32;     // patch rows per block
constexpr int PI_PAD = 8;       // floats of LDS padding per staged patch row (the two lane halves of a B read land 32 banks apart)
constexpr int PI_LD = 36;       // row stride of the 32 x 32 LDS tiles
constexpr int PI_MAX_P = 1024;
constexpr int PI_MAX_H = 1024;
constexpr int PI_SLAB_TARGET = 256;   // backward workgroups to aim for (chunks x slabs)

enum { PI_CONCAT = 0, PI_SUM = 1, PI_PRODUCT = 2, PI_AVERAGE = 3 };

__device__ __forceinline__ float round_bf16(float x) {      // to the nearest bfloat16 (ties to even), returned as a float
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return __uint_as_float(u & 0xffff0000u);
}
template <bool BF>
__device__ __forceinline__ float opnd(float x) { return BF ? round_bf16(x) : x; }

__device__ __forceinline__ float fuse(int fusion, float s, float q) {
    if (fusion == PI_SUM) return s + q;
    if (fusion == PI_PRODUCT) return s * q;
    return (s + q) * 0.5f;                                   // PI_AVERAGE: torch.stack((s, q), -1).mean(-1)
}

struct PatchArgs {
    const float *s, *p, *w1, *b1, *w2, *b2, *dz;
    float *z, *pw1, *pb1, *pw2, *pb2;
    long long R;            // patch rows N * M * T * Vp
    long long pad_rows;     // rows without a patch: N * M * T * (V - Vp)
    int V, Vp, Cs, P, H, Q, C, fusion, nblocks, bps;
};

// patch row pr = (frame, v < Vp) -> its row of z (frame, v) with V joints per frame
__device__ __forceinline__ long long z_row(long long pr, int Vp, int V) { return (pr / Vp) * V + pr % Vp; }

// stage rows [r0, r0 + 32) of p into LDS (zeros past the last row), rounded to bfloat16 in math mode bf16
template <bool BF>
__device__ __forceinline__ void stage_patch_rows(const PatchArgs& a, long long r0, float* ps, int ldp) {
    const int P4 = a.P >> 2;
    for (int i = threadIdx.x; i < PI_ROWS * P4; i += 256) {
        const int r = i / P4, c4 = i - r * P4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < a.R) v = *reinterpret_cast<const f32x4*>(a.p + (r0 + r) * a.P + 4 * c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = opnd<BF>(v[e]);
        *reinterpret_cast<f32x4*>(ps + r * ldp + 4 * c4) = v;
    }
}

// h^T (32 hidden k of chunk h0 x 32 staged rows) over contraction indices [j_lo, j_hi): A lane (k, h) = W1[h0 + k][j], B lane
// (row, h) = p[row][j].  Accumulator: lane (row, g), register 4q + e holds k = 8q + 4g + e.
template <bool BF>
__device__ __forceinline__ f32x16 hidden_t(const PatchArgs& a, const float* ps, int ldp, int h0, int j_lo, int j_hi) {
    const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
    const float* wrow = a.w1 + (long long)(h0 + li) * a.P + 4 * hh;
    const float* prow = ps + li * ldp + 4 * hh;
    f32x16 acc = {};
    for (int j8 = j_lo; j8 < j_hi; j8 += 8) {
        const f32x4 wa = *reinterpret_cast<const f32x4*>(wrow + j8);
        const f32x4 pb = *reinterpret_cast<const f32x4*>(prow + j8);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma32(opnd<BF>(wa[e]), pb[e], acc);
    }
    return acc;
}

template <bool BF>
__global__ __launch_bounds__(256) void patch_input_fwd_kernel(PatchArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, hh = lane >> 5;
    if ((int)blockIdx.x >= a.nblocks) {                       // rows without a patch: q = 0
        const long long u = (long long)(blockIdx.x - a.nblocks) * 256 + tid;
        if (u >= a.pad_rows) return;
        const int np = a.V - a.Vp;
        const long long row = (u / np) * a.V + a.Vp + u % np;
        float* zr = a.z + row * a.C;
        const float* sr = a.s ? a.s + row * a.Cs : nullptr;
        for (int c = 0; c < a.C; ++c) {
            float v = 0.f;
            if (sr) v = a.fusion == PI_CONCAT ? (c < a.Cs ? sr[c] : 0.f) : fuse(a.fusion, sr[c], 0.f);
            zr[c] = v;
        }
        return;
    }
    const long long r0 = (long long)blockIdx.x * PI_ROWS;
    const int ldp = a.P + PI_PAD;
    float* ps = lds;                                        // [32][P + PAD]
    float* qs = lds + PI_ROWS * ldp;                        // [4 waves][32 outputs c][PI_LD] : q^T partials
    if (a.w1) {
        stage_patch_rows<BF>(a, r0, ps, ldp);
        __syncthreads();
        f32x16 qacc = {};
        for (int hc = wave; hc < (a.H >> 5); hc += 4) {
            const int h0 = hc * 32;
            const f32x16 h = hidden_t<BF>(a, ps, ldp, h0, 0, a.P);
            // q^T[c][row] += sum_k W2[c][h0 + k] h^T[k][row]: A lane (c, hh) = W2 row c, B = the accumulator of h^T as it is
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k0 = h0 + 8 * q + 4 * hh;
                f32x4 w2 = {0.f, 0.f, 0.f, 0.f};
                if (li < a.Q) w2 = *reinterpret_cast<const f32x4*>(a.w2 + (long long)li * a.H + k0);
#pragma unroll
                for (int e = 0; e < 4; ++e) qacc = mfma32(opnd<BF>(w2[e]), opnd<BF>(h[4 * q + e] + a.b1[k0 + e]), qacc);
            }
        }
        // accumulator: lane (row = li, g = hh), register r holds c = (r & 3) + 8 (r >> 2) + 4 g
#pragma unroll
        for (int r = 0; r < 16; ++r) qs[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * PI_LD + li] = qacc[r];
        __syncthreads();
    }
    for (int i = tid; i < PI_ROWS * a.C; i += 256) {
        const int row = i / a.C, c = i - row * a.C;
        const long long pr = r0 + row;
        if (pr >= a.R) continue;
        const long long zr = z_row(pr, a.Vp, a.V);
        const int qc = a.fusion == PI_CONCAT ? c - a.Cs : c;
        float q = 0.f;
        if (qc >= 0) {
            if (a.w1) {
                const float* t = qs + qc * PI_LD + row;
                q = t[0] + t[32 * PI_LD] + t[64 * PI_LD] + t[96 * PI_LD] + a.b2[qc];
            } else {
                q = a.p[pr * a.P + qc];                     // identity reducer
            }
        }
        float v;
        if (a.fusion == PI_CONCAT) v = qc < 0 ? a.s[zr * a.Cs + c] : q;
        else v = fuse(a.fusion, a.s[zr * a.Cs + c], q);
        a.z[zr * a.C + c] = v;
    }
}

template <bool BF>
__global__ __launch_bounds__(256) void patch_input_bwd_kernel(PatchArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, hh = lane >> 5;
    const int h0 = blockIdx.x * 32, slab = blockIdx.y;
    const int ldp = a.P + PI_PAD;
    float* ps = lds;                                        // [32 rows][P + PAD]
    float* dqs = ps + PI_ROWS * ldp;                        // [32 rows][PI_LD]: dq, float32
    float* hs = dqs + PI_ROWS * PI_LD;                      // [4 waves][32 k][PI_LD rows]: partial h^T
    const int ntw = a.P >> 7;                               // 32-wide dW1 column tiles per wave (P / 128 <= 8)
    const int jq = a.P >> 2;                                // each wave's quarter of the contraction of h^T
    const int qoff = a.fusion == PI_CONCAT ? a.Cs : 0;
    f32x16 w1acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) w1acc[t] = f32x16{};
    f32x16 w2acc = {};
    float db1 = 0.f, db2 = 0.f;
    const int b_lo = slab * a.bps, b_hi = min(b_lo + a.bps, a.nblocks);
    for (int b = b_lo; b < b_hi; ++b) {
        const long long r0 = (long long)b * PI_ROWS;
        __syncthreads();                                    // the previous block's LDS reads are done
        stage_patch_rows<BF>(a, r0, ps, ldp);
        for (int i = tid; i < PI_ROWS * 32; i += 256) {
            const int row = i >> 5, c = i & 31;
            const long long pr = r0 + row;
            float g = 0.f;
            if (pr < a.R && c < a.Q) {
                const long long zr = z_row(pr, a.Vp, a.V);
                g = a.dz[zr * a.C + qoff + c];
                if (a.fusion == PI_PRODUCT) g *= a.s[zr * a.Cs + c];
                else if (a.fusion == PI_AVERAGE) g *= 0.5f;
            }
            dqs[row * PI_LD + c] = g;
        }
        __syncthreads();
        // partial h^T over this wave's quarter of P -> LDS
        {
            const f32x16 h = hidden_t<BF>(a, ps, ldp, h0, wave * jq, (wave + 1) * jq);
#pragma unroll
            for (int r = 0; r < 16; ++r) hs[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * PI_LD + li] = h[r];
        }
        // dh[row][k] = sum_c dq[row][c] W2[c][h0 + k]: A lane (row, hh) = dq row, B lane (k, hh) = W2 column h0 + k.
        // Accumulator: lane (k, g), register 4q + e holds row 8q + 4g + e -- the A operand of dh^T below.
        f32x16 dh = {};
        for (int q = 0; q < ((a.Q + 7) >> 3); ++q) {
            const int c0 = 8 * q + 4 * hh;
            const f32x4 dq = *reinterpret_cast<const f32x4*>(dqs + li * PI_LD + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w = c0 + e < a.Q ? a.w2[(long long)(c0 + e) * a.H + h0 + li] : 0.f;
                dh = mfma32(opnd<BF>(dq[e]), opnd<BF>(w), dh);
            }
        }
        // dW1[h0 + k][j] += sum_row dh[row][k] p[row][j]: B lane (j, hh) = p[8q + 4hh + e][j0 + j]
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t < ntw) {
                const float* pcol = ps + (wave * ntw + t) * 32 + li;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        w1acc[t] = mfma32(opnd<BF>(dh[4 * q + e]), pcol[(8 * q + 4 * hh + e) * ldp], w1acc[t]);
            }
        }
        if (wave == 0) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s += dh[r];
            db1 += s + __shfl_xor(s, 32);
        }
        __syncthreads();                                    // every wave's partial h^T is in LDS
        if (wave == 0) {
            // dW2[c][h0 + k] += sum_row dq[row][c] h[row][k]: A lane (c, hh) = dq column c, B lane (k, hh) = h^T row k (+ b1)
            const float b1k = a.b1[h0 + li];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rw = 8 * q + 4 * hh;
                f32x4 h = *reinterpret_cast<const f32x4*>(hs + li * PI_LD + rw);
#pragma unroll
                for (int w = 1; w < 4; ++w) h += *reinterpret_cast<const f32x4*>(hs + (w * 32 + li) * PI_LD + rw);
#pragma unroll
                for (int e = 0; e < 4; ++e) w2acc = mfma32(opnd<BF>(dqs[(rw + e) * PI_LD + li]), opnd<BF>(h[e] + b1k), w2acc);
            }
            if (blockIdx.x == 0 && hh == 0) {
                float s = 0.f;
                for (int row = 0; row < PI_ROWS; ++row) s += dqs[row * PI_LD + li];
                db2 += s;
            }
        }
    }
    // slab partials.  dW1 tile t: lane (j, g), register r holds k = (r & 3) + 8 (r >> 2) + 4 g
    float* pw1 = a.pw1 + (long long)slab * a.H * a.P;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < ntw) {
            const int j = (wave * ntw + t) * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) pw1[(long long)(h0 + (r & 3) + 8 * (r >> 2) + 4 * hh) * a.P + j] = w1acc[t][r];
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (c < a.Q) a.pw2[((long long)slab * a.Q + c) * a.H + h0 + li] = w2acc[r];
        }
        if (hh == 0) {
            a.pb1[(long long)slab * a.H + h0 + li] = db1;
            if (blockIdx.x == 0 && li < a.Q) a.pb2[(long long)slab * a.Q + li] = db2;
        }
    }
}

}  // namespace fgcn

using namespace fgcn;

static size_t patch_lds(int P, bool bwd) {
    return sizeof(float) * ((size_t)PI_ROWS * (P + PI_PAD) + (bwd ? PI_ROWS * PI_LD : 0) + 4 * 32 * PI_LD);
}

static int check_patch(const char* what, const float* s, const float* p, const float* w1, const float* b1, const float* w2,
                       const float* b2, int N, int M, int T, int V, int Vp, int Cs, int P, int H, int Q, int fusion, bool bwd) {
    FGCN_REQUIRE(p, FGCN_E_BADARG, "%s: null patch rows", what);
    FGCN_REQUIRE(N > 0 && M > 0 && T > 0 && Vp > 0 && Vp <= V && Cs >= 0 && P > 0 && P % 4 == 0, FGCN_E_BADARG,
                 "%s: bad shape N=%d M=%d T=%d V=%d Vp=%d Cs=%d P=%d", what, N, M, T, V, Vp, Cs, P);
    FGCN_REQUIRE(fusion >= PI_CONCAT && fusion <= PI_AVERAGE, FGCN_E_BADARG, "%s: unknown fusion type %d", what, fusion);
    FGCN_REQUIRE((s != nullptr) == (Cs > 0), FGCN_E_BADARG, "%s: skeleton rows and Cs=%d disagree", what, Cs);
    FGCN_REQUIRE(fusion == PI_CONCAT || (s && Q == Cs), FGCN_E_BADARG,
                 "%s: fusion type %d combines channel by channel and needs Q == Cs (Q=%d Cs=%d)", what, fusion, Q, Cs);
    if (w1) {
        FGCN_REQUIRE(b1 && w2 && (b2 || bwd), FGCN_E_BADARG, "%s: the reducer needs W1, b1, W2 and b2", what);
        FGCN_REQUIRE(P % 128 == 0 && P <= PI_MAX_P && H % 32 == 0 && H > 0 && H <= PI_MAX_H && Q >= 1 && Q <= 32, FGCN_E_BADARG,
                     "%s: unsupported reducer P=%d H=%d Q=%d (P a multiple of 128 up to %d, H a multiple of 32 up to %d, Q <= 32)",
                     what, P, H, Q, PI_MAX_P, PI_MAX_H);
        FGCN_REQUIRE(aligned16(p) && aligned16(w1) && aligned16(w2), FGCN_E_ALIGN, "%s: patch rows / weights not 16-byte aligned", what);
    } else {
        FGCN_REQUIRE(Q == P, FGCN_E_BADARG, "%s: the identity reducer has Q == P (Q=%d P=%d)", what, Q, P);
    }
    FGCN_REQUIRE((long long)N * M * T * V * (Cs + Q) < (1ll << 31) && (long long)N * M * T * Vp * P < (1ll << 40), FGCN_E_BADARG,
                 "%s: tensor too large", what);
    return FGCN_OK;
}

static PatchArgs patch_args(const float* s, const float* p, const float* w1, const float* b1, const float* w2, const float* b2, int N,
                            int M, int T, int V, int Vp, int Cs, int P, int H, int Q, int fusion) {
    PatchArgs a{};
    a.s = s, a.p = p, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2;
    a.R = (long long)N * M * T * Vp;
    a.pad_rows = (long long)N * M * T * (V - Vp);
    a.V = V, a.Vp = Vp, a.Cs = Cs, a.P = P, a.H = H, a.Q = Q, a.fusion = fusion;
    a.C = fusion == PI_CONCAT ? Cs + Q : Cs;
    a.nblocks = (int)cdiv(a.R, PI_ROWS);
    return a;
}

constexpr int PI_MAX_LDS = 160 * 1024;

static int patch_bps(long long R, int H) {
    const long long nblocks = cdiv(R, PI_ROWS);
    const long long want = H >= 32 ? PI_SLAB_TARGET / (H / 32) : PI_SLAB_TARGET;
    const long long slabs = want < 1 ? 1 : (want < nblocks ? want : nblocks);
    return (int)cdiv(nblocks, slabs);
}

extern "C" int fgcn_patch_input_slabs(int N, int M, int T, int Vp, int H) {
    FGCN_REQUIRE(N > 0 && M > 0 && T > 0 && Vp > 0 && H > 0, FGCN_E_BADARG, "patch_input_slabs: bad shape");
    const long long R = (long long)N * M * T * Vp;
    return (int)cdiv(cdiv(R, PI_ROWS), patch_bps(R, H));
}

extern "C" int fgcn_patch_input_fwd(const float* s, const float* p, const float* w1, const float* b1, const float* w2, const float* b2,
                                    float* z, float* stat_partials, int N, int M, int T, int V, int Vp, int Cs, int P, int H, int Q,
                                    int fusion, int stat_centered, void* stream) {
    FGCN_REQUIRE(z, FGCN_E_BADARG, "patch_input_fwd: null output");
    if (int e = check_patch("patch_input_fwd", s, p, w1, b1, w2, b2, N, M, T, V, Vp, Cs, P, H, Q, fusion, false)) return e;
    PatchArgs a = patch_args(s, p, w1, b1, w2, b2, N, M, T, V, Vp, Cs, P, H, Q, fusion);
    a.z = z;
    const bool bf = w1 && math_mode() == FGCN_MATH_BF16;
    const unsigned grid = (unsigned)(a.nblocks + cdiv(a.pad_rows, 256));
    const size_t lds = w1 ? patch_lds(P, false) : 0;
    if (bf) launch_lds<patch_input_fwd_kernel<true>>(dim3(grid), dim3(256), PI_MAX_LDS, lds, (hipStream_t)stream, a);
    else launch_lds<patch_input_fwd_kernel<false>>(dim3(grid), dim3(256), PI_MAX_LDS, lds, (hipStream_t)stream, a);
    if (int e = launch_status("patch_input_fwd")) return e;
    return stat_partials ? fgcn_data_bn_stats(z, stat_partials, N, M, T, V, a.C, stat_centered, stream) : FGCN_OK;
}

extern "C" int fgcn_patch_input_bwd(const float* dz, const float* s, const float* p, const float* w1, const float* b1, const float* w2,
                                    float* pw1, float* pb1, float* pw2, float* pb2, int N, int M, int T, int V, int Vp, int Cs, int P,
                                    int H, int Q, int fusion, void* stream) {
    FGCN_REQUIRE(dz && w1 && pw1 && pb1 && pw2 && pb2, FGCN_E_BADARG, "patch_input_bwd: null pointer (the identity reducer has no gradient)");
    if (int e = check_patch("patch_input_bwd", s, p, w1, b1, w2, nullptr, N, M, T, V, Vp, Cs, P, H, Q, fusion, true)) return e;
    PatchArgs a = patch_args(s, p, w1, b1, w2, nullptr, N, M, T, V, Vp, Cs, P, H, Q, fusion);
    a.dz = dz, a.pw1 = pw1, a.pb1 = pb1, a.pw2 = pw2, a.pb2 = pb2;
    a.bps = patch_bps(a.R, H);
    const dim3 grid((unsigned)(H / 32), (unsigned)cdiv(a.nblocks, a.bps));
    if (math_mode() == FGCN_MATH_BF16)
        launch_lds<patch_input_bwd_kernel<true>>(grid, dim3(256), PI_MAX_LDS, patch_lds(P, true), (hipStream_t)stream, a);
    else
        launch_lds<patch_input_bwd_kernel<false>>(grid, dim3(256), PI_MAX_LDS, patch_lds(P, true), (hipStream_t)stream, a);
    return launch_status("patch_input_bwd");
}
