// Sparse aggregation of the static-adjacency IMU graph convolution (include/fgcn.h, fgcn_graph_spmm):
//
//     out[b, v, c] = act( sum_{j in row v} val[j] * in[b, col[j], c]  +  residual term ),     node-major (B, V, C) tensors, CSR matrix.
//
// The IMU graph's adjacency has 8 .. 30 non-zeros in a row of ~2000 (a node, the other values of its time step, one or six values
// of the steps around it), so the product is a GATHER of a handful of rows: no matrix pipe, no transpose, no padding.  Called with
// the CSR form of adj it is the forward aggregation, with that of adj^T the data gradient -- both gathers, no atomics.
//
// Work split: a wave owns one node at a time and 256 consecutive channels (16 bytes per lane); the four waves of a workgroup take
// nodes n0 + wave, n0 + wave + 4, ... of a run of RUN consecutive nodes.  Neighbours of consecutive nodes are consecutive nodes, so
// at any moment the workgroup reads a window of a few dozen rows x 1 KB: every row but the first touch of the run comes from the
// CU's vector cache or L2, and HBM sees `in` once.  Node runs are the fastest grid axis: workgroups resident together share halos.
//
// The CSR entries of a row are wave-uniform: they live in SGPRs (scalar loads / readfirstlane) and a gathered row's byte offset is
// the scalar offset of the buffer load.  Entries are taken eight at a time and two such groups are in flight; the entries of
// the last group that do not exist get the out-of-range lane offset (the load returns zeros) and the weight 0.  A group is read as
// eight consecutive entries whatever the row's length, hence the seven padding entries behind col and val (include/fgcn.h).
//
// Arithmetic: float32 FMAs in ascending column order in EVERY math mode -- two launches agree bit for bit and the math mode changes
// nothing (the rule of the joint kernels).
#include "fgcn_tile.hpp"

namespace fgcn {

struct SpmmP {
    const float* in;
    const float* b;
    const float* vec_b;
    float* out;
    unsigned char* mask;
    unsigned in_bytes, b_bytes, out_bytes, mask_bytes;
    int V, C, ld_in, ld_b, ld_out, relu;
};

constexpr int SPMM_RUN = 32;      // nodes per workgroup (eight per wave)
constexpr int SPMM_U = 8;         // CSR entries (row loads) in flight per wave

// RES: 0 none, 1 `+ b`, 2 `+ b * scale + shift` (selects the loads of the epilogue); MASK: the sign image is written; STR: streamed stores
template <int RES, bool MASK, bool STR>
__global__ __launch_bounds__(256) void graph_spmm_kernel(SpmmP p, const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                         const float* __restrict__ val) {
    constexpr unsigned OOB = 0x80000000u;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = ((int)blockIdx.y * 64 + lane) * 4;
    const unsigned lane_off = c < p.C ? (unsigned)c * 4u : OOB;           // channels past C: loads return zeros, stores are dropped
    const int row0 = (int)blockIdx.z * p.V;                                // first row of this sample (B * V < 2^29: host check)
    const int n0 = (int)blockIdx.x * SPMM_RUN;

    const __amdgpu_buffer_rsrc_t rin = buffer_rsrc(p.in, p.in_bytes);
    const __amdgpu_buffer_rsrc_t rout = buffer_rsrc(p.out, p.out_bytes);
    const __amdgpu_buffer_rsrc_t rb = buffer_rsrc((RES ? p.b : p.in), RES ? p.b_bytes : 0u);
    const __amdgpu_buffer_rsrc_t rm = buffer_rsrc((MASK ? (void*)p.mask : (void*)p.out), MASK ? p.mask_bytes : 0u);
    f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if constexpr (RES == 2) {
        const __amdgpu_buffer_rsrc_t rv = buffer_rsrc(p.vec_b, (unsigned)p.C * 16u);
        sc = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, lane_off, (unsigned)p.C * 8u, 0));
        sh = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, lane_off, (unsigned)p.C * 12u, 0));
    }
    const unsigned in_row_b = (unsigned)p.ld_in * 4u;

    // A cursor names one group of SPMM_U entries of one node's row (all scalar).  An empty row is one group without entries: its node still
    // gets its epilogue and its store.  `ok` false: behind the last node of this wave -- such a group is still "issued" (every load out of
    // range, no traffic) so that the number of loads between a group's request and its use does not depend on a branch.
    struct Cur {
        int i, v, j, je;
        bool ok;
    };
    auto open = [&](int i) -> Cur {
        Cur q;
        q.i = i, q.v = __builtin_amdgcn_readfirstlane(n0 + wave + 4 * i);
        q.ok = i < SPMM_RUN / 4 && q.v < p.V;
        const int vv = q.ok ? q.v : 0;                                     // (row_ptr[0 .. 1] exist for every V)
        q.j = __builtin_amdgcn_readfirstlane(row_ptr[vv]), q.je = __builtin_amdgcn_readfirstlane(row_ptr[vv + 1]);
        return q;
    };
    auto advance = [&](Cur& q) {
        if (q.j + SPMM_U < q.je) q.j += SPMM_U;
        else q = open(q.i + 1);
    };
    auto last_group = [&](const Cur& q) -> bool { return q.ok && q.j + SPMM_U >= q.je; };
    // request a group's rows (and, with its node's last group, the node's residual row)
    auto issue = [&](const Cur& q, f32x4 (&x)[SPMM_U], float (&w)[SPMM_U], f32x4& res) {
        const int j = q.ok ? q.j : 0;                                      // (entries 0 .. 7 of col / val exist for every matrix: the padding)
#pragma unroll
        for (int u = 0; u < SPMM_U; ++u) {
            const bool there = q.ok && j + u < q.je;                       // scalar: the entry exists
            // (j + u may pass the row's end by up to seven entries: the next rows' entries or the arrays' padding, read and ignored --
            // eight consecutive dwords are one scalar load)
            const int cu = __builtin_amdgcn_readfirstlane(col[j + u]);
            const float wu = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, val[j + u])));
            w[u] = there ? wu : 0.f;
            x[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rin, there ? lane_off : OOB,
                                                                                   there ? (unsigned)(row0 + cu) * in_row_b : 0u, 0));
        }
        if constexpr (RES != 0) {
            const bool l = last_group(q);
            res = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, l ? lane_off : OOB,
                                                                                  l ? (unsigned)(row0 + q.v) * ((unsigned)p.ld_b * 4u) : 0u, 0));
        }
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // a group's FMAs in ascending column order; behind a node's last group its epilogue and stores
    auto consume = [&](const Cur& q, const f32x4 (&x)[SPMM_U], const float (&w)[SPMM_U], const f32x4& res) {
#pragma unroll
        for (int u = 0; u < SPMM_U; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w[u], x[u][e], acc[e]);
        }
        if (!last_group(q)) return;
        const int row = __builtin_amdgcn_readfirstlane(row0 + q.v);        // (scalar offsets of the stores)
        const unsigned out_off = (unsigned)row * ((unsigned)p.ld_out * 4u);
        if constexpr (RES == 1) {
            acc += res;
        } else if constexpr (RES == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __builtin_fmaf(res[e], sc[e], sh[e]);
        }
        if (p.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = relu_nan(acc[e]);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, acc), rout, lane_off, out_off,
                                               STR ? FGCN_STORE_AUX : 0);
        // A 16-byte store reads its data registers over several cycles; hipcc assumes that a store with a scalar offset needs no wait
        // states before a VALU write of them and placed `acc = 0` directly behind it: on the MI355X the last dword then left as 0.0
        // (seen in the first GPU run of tests/test_imu_sparse_gpu.py, one element per lane and row).  Two wait states, kept in place.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 1");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MASK) {
            // fgcn_bn_act's image: bit e % 8 of byte e / 8 = [!(out[e] <= 0)], e the element index in the contiguous (B, V, C) tensor; C % 8 == 0
            // (host check), so a lane pair shares a byte and a row owns C / 8 whole bytes
            const int nib = (relu_open(acc[0]) ? 1 : 0) | (relu_open(acc[1]) ? 2 : 0) | (relu_open(acc[2]) ? 4 : 0) | (relu_open(acc[3]) ? 8 : 0);
            const int other = __shfl_xor(nib, 1);
            const unsigned moff = (lane & 1) || c >= p.C ? OOB : (unsigned)c >> 3;
            __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(nib | (other << 4)), rm, moff, (unsigned)row * ((unsigned)p.C >> 3), 0);
        }
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // Two groups in flight: the next group's rows are requested BEFORE the present group is waited for, and a node's stores are
    // issued behind them -- no wait in this loop drains the stores (vmcnt counts loads and stores in issue order).
    Cur cur = open(0);
    if (!cur.ok) return;
    f32x4 xa[SPMM_U], xb[SPMM_U], ra = {0.f, 0.f, 0.f, 0.f}, rb2 = {0.f, 0.f, 0.f, 0.f};
    float wa[SPMM_U], wb[SPMM_U];
    issue(cur, xa, wa, ra);
    Cur nxt = cur;
    advance(nxt);
    while (true) {
        issue(nxt, xb, wb, rb2);
        consume(cur, xa, wa, ra);
        if (!nxt.ok) break;
        cur = nxt;
        advance(nxt);
        issue(nxt, xa, wa, ra);
        consume(cur, xb, wb, rb2);
        if (!nxt.ok) break;
        cur = nxt;
        advance(nxt);
    }
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_graph_spmm(const float* in, const int* row_ptr, const int* col, const float* val, const float* b, const float* vec_b,
                               float* out, unsigned char* sign_mask, int B, int V, int C, int ld_in, int ld_b, int ld_out, int res_mode,
                               int relu, void* stream) {
    FGCN_REQUIRE(in && out, FGCN_E_BADARG, "graph_spmm: null tensor");
    FGCN_REQUIRE(row_ptr && col && val, FGCN_E_BADARG, "graph_spmm: null CSR array (row_ptr, col and val are all required)");
    FGCN_REQUIRE(B > 0 && V > 0 && C > 0 && C % 4 == 0, FGCN_E_BADARG, "graph_spmm: B=%d V=%d C=%d (C must be a multiple of 4)", B, V, C);
    FGCN_REQUIRE(res_mode >= 0 && res_mode <= 2, FGCN_E_BADARG, "graph_spmm: res_mode=%d", res_mode);
    FGCN_REQUIRE(res_mode == 0 || b, FGCN_E_BADARG, "graph_spmm: residual operand missing");
    FGCN_REQUIRE(res_mode != 2 || vec_b, FGCN_E_BADARG, "graph_spmm: residual coefficient vector missing");
    FGCN_REQUIRE(ld_in >= C && ld_in % 4 == 0 && ld_out >= C && ld_out % 4 == 0 && (res_mode == 0 || (ld_b >= C && ld_b % 4 == 0)), FGCN_E_BADARG,
                 "graph_spmm: row strides must cover C and be multiples of 4 (ld_in=%d ld_b=%d ld_out=%d C=%d)", ld_in, ld_b, ld_out, C);
    FGCN_REQUIRE(!sign_mask || C % 8 == 0, FGCN_E_BADARG, "graph_spmm: a sign mask needs C %% 8 == 0 (C=%d)", C);
    // 32-bit row math: row indices below 2^29, byte offsets below 2^31 (bit 31 of a lane offset marks an absent row)
    const long long rows = (long long)B * V;
    const long long ld_max = ld_in > ld_out ? (ld_in > ld_b ? ld_in : ld_b) : (ld_out > ld_b ? ld_out : ld_b);
    FGCN_REQUIRE(rows < (1ll << 29), FGCN_E_BADARG, "graph_spmm: B * V = %lld rows overflow the kernel's 32-bit row math (< 2^29)", rows);
    FGCN_REQUIRE(((rows - 1) * ld_max + C) * 4 < (1ll << 31), FGCN_E_BADARG,
                 "graph_spmm: %lld rows of stride %lld overflow the kernel's 32-bit byte offsets (< 2^31 bytes per tensor)", rows, ld_max);
    const int cw = (int)cdiv(C, 256);
    FGCN_REQUIRE(B <= 65535 && cw <= 65535, FGCN_E_BADARG, "graph_spmm: B=%d samples / %d channel windows exceed the grid (65535)", B, cw);
    FGCN_REQUIRE(aligned16(in) && aligned16(out) && (!b || aligned16(b)) && (!vec_b || aligned16(vec_b)), FGCN_E_ALIGN,
                 "graph_spmm: 16-byte alignment");
    SpmmP p;
    p.in = in, p.b = b, p.vec_b = vec_b, p.out = out, p.mask = sign_mask;
    p.in_bytes = (unsigned)(((rows - 1) * ld_in + C) * 4);
    p.b_bytes = res_mode ? (unsigned)(((rows - 1) * ld_b + C) * 4) : 0u;
    p.out_bytes = (unsigned)(((rows - 1) * ld_out + C) * 4);
    p.mask_bytes = sign_mask ? (unsigned)(rows * C / 8) : 0u;
    p.V = V, p.C = C, p.ld_in = ld_in, p.ld_b = ld_b, p.ld_out = ld_out, p.relu = relu;
    const dim3 grid((unsigned)cdiv(V, SPMM_RUN), (unsigned)cw, (unsigned)B), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const bool str = stream_out(rows * C * 4);
#define FGCN_SPMM3(RES_, M_, S_) hipLaunchKernelGGL((graph_spmm_kernel<RES_, M_, S_>), grid, blk, 0, s, p, row_ptr, col, val)
#define FGCN_SPMM2(RES_, M_)             \
    do {                                 \
        if (str) FGCN_SPMM3(RES_, M_, true); \
        else FGCN_SPMM3(RES_, M_, false);    \
    } while (0)
#define FGCN_SPMM(RES_)                        \
    do {                                       \
        if (sign_mask) FGCN_SPMM2(RES_, true); \
        else FGCN_SPMM2(RES_, false);          \
    } while (0)
    if (res_mode == 0) FGCN_SPMM(0);
    else if (res_mode == 1) FGCN_SPMM(1);
    else FGCN_SPMM(2);
#undef FGCN_SPMM
#undef FGCN_SPMM2
#undef FGCN_SPMM3
    return launch_status("graph_spmm");
}
