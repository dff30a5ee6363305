/*
 * fgcn.h — C ABI of libfgcn.so: the MI355X (gfx950) kernels behind fusion-gcn's AGCN / ST-GCN block.
 *
 * The reference (mduhme/fusion-gcn) has no FFI of its own: its hot path is the op sequence of
 * torch_src/models/mmargcn/agcn.py (SpatialGraphConv :96-115, TemporalConv :49-51, SpatialTemporalConv
 * :134-136), dispatched to ATen.  Each entry point below names the reference lines whose arithmetic it
 * replaces.  The Python host (fusion_gcn_amd/ops.py) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, a hipStream_t passed as void*.
 *   - activations are float32 (bfloat16 where a `half_mask` says so, see "storage types and half_mask"), channels-last: element (n, t, v, c) of a tensor with row stride `ld`
 *     lives at base[((n*T + t)*V + v)*ld + c].  `ld` and every channel offset are multiples of 4 floats
 *     and every base pointer is 16-byte aligned.
 *   - the caller owns every buffer (outputs, workspaces, partial-sum scratch); the library allocates nothing,
 *     never synchronises and only enqueues work on `stream`.
 *   - return value: 0 = ok, <0 = error (FGCN_E_*); text via fgcn_last_error() (thread-local).  Never throws
 *     or exits.  Shapes are validated on the host before any launch.
 */
#ifndef FGCN_H
#define FGCN_H

#ifdef __cplusplus
extern "C" {
#endif

#define FGCN_OK 0
#define FGCN_E_BADARG (-1)   /* null pointer / inconsistent or unsupported shape */
#define FGCN_E_ALIGN (-2)    /* pointer or stride not aligned as required */
#define FGCN_E_LAUNCH (-3)   /* hipLaunchKernel reported an error */
#define FGCN_E_ARCH (-4)     /* device is not gfx950 */

#define FGCN_MAX_V 32        /* joints per skeleton graph (reference graphs: 18..27) */
#define FGCN_MAX_V_WIDE 64   /* joints per graph of the wide joint kernels (fgcn_*_wide), the AGCN block's limit; 33..64 take them */
#define FGCN_MIX_MAX_ITEMS 24
#define FGCN_GRAM_MAX_ITEMS 4

int fgcn_version(void);
const char* fgcn_last_error(void);
/* 0 if the current HIP device is gfx950, FGCN_E_ARCH otherwise (message names the arch found). */
int fgcn_check_device(void);

/* Non-finite values in the inputs.  Classify every output element as finite, NaN, +inf or -inf.  "The reference" is the float64 restatement
 * of an entry point (torch's composition of the same operation) run on the same float32 input with the same non-finite element in it.
 * tests/test_nonfinite_gpu.py asserts exactly these rules (tests/nonfinite_ref.py counts swallowed / corrupted / spilled elements):
 *   1. Elementwise kernels and epilogues reproduce the reference's class at every position: NaN stays NaN, +-inf keeps its sign, wherever
 *      the value enters -- the pre-activation, the residual, the per-channel scale or shift.  fgcn_bn_act (every res_mode, with and without
 *      the sign image, every half_mask, the four- and the eight-wide forms), fgcn_bn_act_pool, the add + ReLU built on fgcn_bn_act, the
 *      BatchNorm + shortcut + ReLU epilogues of fgcn_tconv_halo_bn_relu and fgcn_spatial_fwd_tile_bn_relu, fgcn_graph_spmm's epilogue.
 *      The ReLU is max(v, 0) that KEEPS a NaN (torch.relu; fmaxf(NaN, 0) is 0).  The two fused epilogues add the conv bias to the accumulator
 *      before the scale: (acc + bias) * scale + shift, as the reference does, not acc * scale + (bias * scale + shift), which is inf - inf for an
 *      inf scale.
 *   2. The ReLU gate of the backward is torch's: grad if !(y <= 0) else 0.  A NaN output PASSES its gradient.  The sign image bit is
 *      [!(out[e] <= 0)] (equal to [out[e] > 0] on every number; set for a NaN), and a gate read from `out` decides the same way.
 *   3. Contractions never swallow and never corrupt silently (the row GEMMs, fgcn_pw_gemm, fgcn_tconv_halo, fgcn_joint_mix*, the spatial,
 *      embedding and weight-gradient tile kernels, fgcn_row_softmax_*, the cross-entropy kernels): where the reference is non-finite the
 *      result is non-finite -- NaN against +-inf need not match: an inf that went through a bf16 or f16 split is inf - inf = NaN in its second
 *      part, and everything behind it is what the reference computes from a NaN there (ReLUs the reference closes at -inf are open at the
 *      NaN) -- and where the reference is finite the result is within the tolerance of the same call on finite data, or non-finite.  A finite
 *      wrong value is the failure.
 *   4. Containment: with running-statistics BatchNorm (eval) a non-finite element of one sample leaves the other samples finite and within
 *      that tolerance -- for a NaN in every math mode, for +-inf in f32, bf16x3 and bf16.  FGCN_PRODUCTS_F16X2 with an inf: rule 3 alone.  That
 *      mode scales each staged block (a K chunk of a row tile, a frame pair, a sample's adjacency images, a whole tensor in the weight
 *      gradient) by its largest magnitude; the maxima are taken with fmaxf, so a NaN does not move the scale but an inf does, and an inf's
 *      scale would flush every other value of the block to an f16 zero.  A block whose maximum is an inf is scaled by NaN instead: every
 *      accumulator it reaches is NaN, which may include rows of neighbouring samples in the same tile.
 *   5. Structural zeros: fgcn_graph_spmm multiplies the STORED entries of its CSR matrix only, so its reference is torch's sparse product
 *      over the same entries: a NaN in node u reaches the nodes with a stored entry in column u, not every node.  No other route skips a
 *      product: the mixing matrices of fgcn_joint_mix* are dense operands, and 0 * NaN = NaN there.
 * The conv-bias gradients in front of a batch-statistics BatchNorm, which the host of the AGCN block hands out as exact zeros
 * (fusion_gcn_amd/block.py, _BiasGrads), are under rule 3 too: they are s - s of that BatchNorm backward's channel sums (fgcn_bn_act_bwd_reduce's
 * row 1, the shortcut BatchNorm's row 2), 0 for a number and NaN otherwise.  The MS-G3D op wrappers (fusion_gcn_amd/fops.py, zero_bias_grad) still
 * hand out plain zeros: not under these rules, and not tested.
 * The earlier NaN rules stand beside these: fgcn_tmaxpool3_fwd (a NaN tap wins), fgcn_classify_update and the fused scores' ranking (NaN sorts
 * above every number), fgcn_signal_prepare's min / max (a NaN in the array makes every output NaN). */

/* Contexts: where the settings live that the launchers read on the host at call time -- the math mode, the product form that belongs to
 * it and the kernel-variant table below.  Every thread has a CURRENT context; a thread that never made one current reads (and, through the
 * setters below, writes) the process-wide defaults.  fgcn_ctx_create copies the calling thread's current settings into a new
 * context; fgcn_ctx_set_current(ctx) makes it current for the CALLING THREAD ONLY (NULL: back to the process-wide defaults);
 * fgcn_set_math_mode / fgcn_set_products / fgcn_set_tuning then change that context and nothing else.  NO KERNEL ENTRY POINT MODIFIES A
 * CONTEXT: the setters are the only writers, so what fgcn_get_math_mode / fgcn_get_products / fgcn_get_tuning return is the same before
 * and after any launch (tests/test_weight_form_gpu.py), and nothing a launcher needs to know about one of its ARGUMENTS is read from
 * here -- the layout of a weight argument is stated by the caller (w_form, below).  Two threads with two contexts
 * -- two models in two math modes on two streams -- therefore never see each other's settings (tests/test_context_gpu.py).  A caller
 * whose work continues on another thread (an autograd backward) makes the same context current there for the duration of its calls:
 * fusion_gcn_amd.ops.context_bound does that for every autograd Function of the host.  A context must not be destroyed while it is
 * current on the destroying thread, and not while another thread still uses it. */
typedef struct fgcn_ctx fgcn_ctx;
int fgcn_ctx_create(fgcn_ctx** out);
int fgcn_ctx_destroy(fgcn_ctx* ctx);
int fgcn_ctx_set_current(fgcn_ctx* ctx);
fgcn_ctx* fgcn_ctx_get_current(void);

/* Select a kernel variant in the calling thread's current context (for tuning tools and same-box A/B runs -- value 0 of every key is the
 * measured-best default, every other form computes the same result in another summation order at most: tests/variants.py lists every
 * (key, value) with the launcher's condition for it and the test that runs it).  Keys 0..31 (others: FGCN_E_BADARG); a key that is not
 * listed is stored and read by nothing:
 *   0  row-GEMM tile when N <= 64: 0 = 128x(32*nt) rows per workgroup, 1 = 256-row tile (default), 2 = 256-row, double-buffered LDS
 *      (launches of fewer than 256 workgroups run the 128-row tile whatever the key says, unless key 24 = 1)
 *   1  row GEMM, wider N: 0 = two barriers per K chunk, 1 = double-buffered LDS
 *   4  f32 halo conv: 0 = three workgroups per CU, 1 = two
 *   5  workgroup orders (bits): 1 row GEMM XCD-aware order on; 8 row GEMM column-tile-fastest off; 4 generic weight gradient (rows_wgrad) XCD-aware off;
 *      16 spatial forward XCD-aware off; 32 split-bf16 halo conv XCD-aware off; 2 f32 halo conv XCD-aware on; 64 split weight gradient XCD-aware off
 *   6  (bits) 1: 1x1 weight gradients of the bf16 modes on the 256-thread kernel that splits fragments as it reads them;
 *      8: joint_dagg at two workgroups per CU; 16: joint_dagg's gram on the f32 MFMA in every mode;
 *      32: 1x1 weight gradients on ONE 8-wave workgroup per CU (default: two 4-wave ones); 64: all-taps kernels above 64 output
 *      columns on 8 waves (default 4); 256: at 64 columns on 4 waves (default 8); 128: all-taps weight gradient without the circular tap window;
 *      512: fgcn_spatial_wgrad on exact-f32 MFMAs in math mode bf16x3 (default there: the split-bf16 form)
 *      1024: joint_dagg with its subset count / accumulate flag as run-time values (the form before the end of round 3); 2048: both at compile time,
 *      three workgroups per CU, one tile register set (default: one set per subset refilled a chunk ahead, two workgroups per CU)
 *   7  split-bf16 kernels (bits) 1: spatial forward, one frame per wave (older form; FGCN_PACK_SPLIT3_ACC weights only -- it has no f16x2
 *      form, and for FGCN_PACK_SPLIT2H_ACC weights the bit selects nothing); 8: split-bf16 halo conv as 2 x 2 waves over 128-row tiles at every width (default:
 *      4 x 1 waves over 192-row tiles up to 128 columns, see 64); 16: the 4 x 1 form with a 128-column tile for every N > 64 (default: 64 < N <= 128 only), and in
 *      FGCN_MATH_BF16 the 4 x 1 forms at all (default there: 2 x 2); 32: never the 128-column 4 x 1 form; 64: the 4 x 1 forms whatever the
 *      tile count (default: from 1536 192-row tiles on; tests)
 *   8  fgcn_pw_gemm: 1 = one tile per workgroup (default: persistent workgroups that walk their XCD's tiles; same bits)
 *   10 output stores of the activation-writing kernels: 0 = non-temporal (streamed past L2) when the call writes 96 MiB or more, plain below;
 *      1 = always plain; 2 = always non-temporal (same results in every setting: tests/test_block_model_gpu.py)
 *   12 joint gram of three equal-width items: 1 = the generic kernel (default: joint_gram3_kernel)
 *   13 fgcn_spatial_wgrad: workgroups to aim for (0 = 512 up to 32 samples, 1024 above)
 *   15 fgcn_spatial_bwd_tile: workgroups to aim for (0 = 256, one per CU; sets the segment count, i.e. the shape of `partial`)
 *   16 fgcn_spatial_wgrad_tile: workgroups to aim for (0 = 256; sets the slab count)
 *   17 fgcn_emb_wgrad_tile: workgroups to aim for (0 = 256; sets the slab count)
 *   18 fgcn_emb_dx_tile: 1 = 128-column tiles with a two-slot weight ring (default four)
 *   19 fgcn_emb_wgrad_tile: 1 = emb values requested one frame slot ahead (default: two)
 *   21 fgcn_spatial_wgrad_tile / fgcn_emb_wgrad_tile: 2 = 64 x 64 tiles (default: the widest tiles the channels allow)
 *   22 fgcn_emb_fwd_tile: resident workgroups to aim for (0 = 512; sets the segment count)
 *   24 fgcn_rows_gemm*: 1 = the large-problem tiles (256 / 128 rows x the widest column tile) also where they leave fewer than 256
 *      workgroups (small problems otherwise take the smallest tiles that pad no extra column)
 *   25 bfloat16 outputs (FGCN_MATH_BF16, half_mask) are stored plainly whatever key 10 says; (bits) 1: fgcn_tconv_halo, 2: fgcn_spatial_fwd_tile
 *      follow key 10's rule for them too (non-temporal stores of the 32-byte pieces)
 *   26 (bits) 1: fgcn_bn_act_bwd_reduce on bfloat16 operands (the eight-channels-per-thread kernel) with 256 threads per workgroup instead of
 *      128 and twice the LDS (a thread then sums other rows: the partial sums differ in their last bits) */
int fgcn_set_tuning(int key, int value);
int fgcn_get_tuning(int key);

/* Arithmetic of the convolution / GEMM kernels, a setting of the calling thread's current context (the reference's counterpart is its
 * mixed-precision step, session/procedures/step.py:55-78, which wraps model(x) in autocast).  The process-wide default is
 * FGCN_MATH_BF16X3: the arithmetic bench.py reports (float32-accurate, 1.57x the step rate of FGCN_MATH_F32 on MI355X).
 *   FGCN_MATH_F32  v_mfma_f32_32x32x2_f32 on float32 operands -- the exact-f32 parity path (<= 1e-3 rel);
 *   FGCN_MATH_BF16 (BASELINE config 5) operands rounded to bfloat16 (round-to-nearest-even) once -- as a tile is staged,
 *                  as a fragment is formed, or (weights of fgcn_tconv_halo) by fgcn_pack_split3 -- bf16 MFMAs with float32
 *                  accumulation; tensors in HBM, BatchNorm statistics, softmax, the joint mixing and every reduction
 *                  stay float32.  Different tolerance contract: logits <= 1e-2 rel, gradient cosine >= 0.98 against the
 *                  f32 path.
 *   FGCN_MATH_BF16X3 float32-accurate products on the bf16 matrix pipe: both operand fragments are split exactly into
 *                  three bfloat16 terms (x = x_h + x_m + x_l, 24 significand bits) and the six partial products down
 *                  to 2^-16 of the leading one are accumulated in float32 (the dropped ones are below 2^-23 |a.b|, the
 *                  rounding of a float32 product).  Six bf16 MFMAs replace four f32 MFMAs (2.67x the f32 matrix
 *                  rate); same tolerance contract as FGCN_MATH_F32 (the parity tests run in both).  The default. */
#define FGCN_MATH_F32 0
#define FGCN_MATH_BF16 1
#define FGCN_MATH_BF16X3 2
int fgcn_set_math_mode(int mode);
int fgcn_get_math_mode(void);
/* Product form: the second half of the math-mode setting inside FGCN_MATH_BF16X3 (FGCN_MATH_BF16X3 + FGCN_PRODUCTS_F16X2 is the mode
 * the host calls "f16x2").  It is a MODE-LEVEL setting: it says which weight forms the owner of the model keeps (FGCN_PACK_SPLIT2H[_ACC]
 * instead of FGCN_PACK_SPLIT3[_ACC]) and is read by mode-level decisions only -- fgcn_spatial_fwd_tile_available, and
 * fgcn_tconv_halo_bn_relu / fgcn_spatial_fwd_tile_bn_relu, which take fgcn_pack_split3 forms and refuse with FGCN_PRODUCTS_F16X2 selected.
 * No launcher derives the layout of a weight argument from it.
 *
 * THE FORM OF A WEIGHT ARGUMENT IS STATED BY THE CALLER.  The entry points that accept weights in more than one layout --
 * fgcn_tconv_halo, fgcn_pw_gemm, fgcn_spatial_fwd -- take `int w_form`, a FGCN_PACK_* constant (below), as the argument DIRECTLY AFTER
 * THE WEIGHT POINTER.  It is checked against the math mode (and, for fgcn_spatial_fwd, Cin) before anything else; a pair outside this
 * table is FGCN_E_BADARG with a message that names the form and the mode:
 *     fgcn_tconv_halo, fgcn_pw_gemm    FGCN_MATH_F32                        FGCN_PACK_K4
 *                                      FGCN_MATH_BF16                       FGCN_PACK_SPLIT3
 *                                      FGCN_MATH_BF16X3                     FGCN_PACK_SPLIT3 or FGCN_PACK_SPLIT2H
 *     fgcn_spatial_fwd                 FGCN_MATH_BF16X3 and Cin % 32 == 0   FGCN_PACK_SPLIT3_ACC or FGCN_PACK_SPLIT2H_ACC
 *                                      anything else                        FGCN_PACK_K4
 * (fgcn_pw_gemm runs in the split modes only: fgcn_pw_gemm_available.)  The byte bound of the weight buffer, the kernel instantiation and
 * whether in_amax is recorded all follow w_form: a FGCN_PACK_SPLIT2H form runs the f16x2 products whatever fgcn_get_products says, a
 * FGCN_PACK_SPLIT3 form the bf16x3 ones.  The weight gradients have no weight argument: they run their f16x2 form in FGCN_MATH_BF16X3
 * when both operand scales are given (a_amax / g_amax, below).
 *   FGCN_PRODUCTS_BF16X3  six bf16 partial products from exact three-way bf16 splits (above);
 *   FGCN_PRODUCTS_F16X2   three f16 products from two-way f16 splits: x 2^s = h + l (11 + 11 significand bits + the sign of l: within
 *                         2^-24 |x| while l is a normal f16), l.l dropped (<= 2^-24 |a.b|) -- half the matrix work at float32-class
 *                         accuracy.  f16 has 5 exponent bits, so every operand BLOCK is scaled by an exact power of two that puts its
 *                         largest magnitude into [2^14, 2^15): activations per staged (row tile, channel chunk) inside the kernels
 *                         (the accumulator carries the scale, only ever towards larger magnitudes), weights per packed form
 *                         (FGCN_PACK_SPLIT2H).  Error model per operand element: max(2^-24 |x|, 2^-40 * block maximum). */
#define FGCN_PRODUCTS_BF16X3 0
#define FGCN_PRODUCTS_F16X2 1
int fgcn_set_products(int products);
int fgcn_get_products(void);

/* Temporal index map shared by the row GEMMs: for output frame `to` and tap `j`
 *     num = to*ta + j*tb + tc ;  valid iff num >= 0, num % td == 0 and num/td < T_in ;  ti = num/td.
 * forward conv (kernel kt, stride s, pad p): ta=s tb=1 tc=-p td=1 ; its data gradient: ta=1 tb=-1 tc=p td=s. */
typedef struct {
    int taps, ta, tb, tc, td;
} fgcn_tmap;

/* out[(n,to,v), 0:N] (+)= bias + sum_j sum_k in[(n,ti(to,j),v), k] * w[j][k][n]      (implicit GEMM over rows)
 *   replaces nn.Conv2d 1x1 / (kt,1) forward and data-gradient: agcn.py:41-42 (tcn conv), :71-73 (conv_a/b/d),
 *   :77 (down), :125-132 (residual conv) and their autograd backward w.r.t. the input.
 *   w is packed [taps][K][N] (N contiguous, N % 4 == 0).  bias may be NULL.
 *   stat_partials (may be NULL): float[ceil(M/128)][2][N] receives per-row-tile sum and sum of squares of the
 *   values written (the BatchNorm batch statistics of agcn.py:44,78,83 come from these).  accumulate: out += .
 *   At most 2^29 rows (B * T_out * V) per call.  half_mask: "storage types and half_mask" below. */
int fgcn_rows_gemm(const void* in, void* out, const float* w, const float* bias, float* stat_partials,
                   int B, int T_in, int T_out, int V, int K, int N, int ld_in, int ld_out,
                   fgcn_tmap map, int accumulate, int half_mask, void* stream);
/* `batch` independent problems out_b[rows x N] (+)= in_b[rows x K] . w_b[K x N] in one launch (one per blockIdx.z): problem b
 * reads in + b*in_bstride, w + b*w_bstride and writes out + b*out_bstride (strides in floats, multiples of 4; row strides
 * ld_in / ld_out as above).  The per-sample V x V products of AGCNGraphConvolution on IMU graphs
 * (torch_src/models/mmargcn/graph_convolution.py:96-101 and their backward): one sample's matrix is the weight. */
int fgcn_rows_gemm_batched(const float* in, float* out, const float* w, int batch, long long in_bstride,
                           long long out_bstride, long long w_bstride, int rows, int K, int N, int ld_in, int ld_out,
                           int accumulate, void* stream);
/* The same with two batch levels, batch * inner problems per launch: problem (o, i) reads in + o*in_bstride + i*in_bstride2 (w, out
 * alike) -- the three subsets of one sample in one launch (o = sample, i = subset) where a tensor is laid out (sample, subset, ...)
 * and another (subset, sample, ...). */
int fgcn_rows_gemm_batched2(const float* in, float* out, const float* w, int batch, long long in_bstride,
                            long long out_bstride, long long w_bstride, int inner, long long in_bstride2,
                            long long out_bstride2, long long w_bstride2, int rows, int K, int N, int ld_in, int ld_out,
                            int accumulate, void* stream);
/* number of row tiles = leading dimension of stat_partials for M = B*T_out*V rows */
int fgcn_rows_gemm_tiles(long long M);

/* Temporal (kt x 1) convolution / its data gradient as a halo-tile implicit GEMM (agcn.py:41-42 and its backward):
 *   out[(n, fo(th), v), 0:N] (+)= bias + sum_j sum_k in[(n, fi(th + d_j), v), k] * W[j][k][n],   d_j = j*tb + tc,
 * over "virtual" frames th in [0, Th): fi(t) = t*in_s + in_o (valid for t in [0, Th_in)), fo(t) = t*out_s + out_o.
 * A stride-1 conv is one call with identity views; a stride-2 conv (or its data gradient) is two calls, one per frame
 * parity of the strided side, so no tap meets a structurally empty row.  The input tile plus its temporal halo is
 * staged in LDS once per 32 input channels and all taps run from it.
 *   w4 (FGCN_MATH_F32): k-interleaved packed weights float[taps][K/4][N][4]  (w4[j][k/4][n][k%4] = W[j][k][n]);
 *   w4 (FGCN_MATH_BF16X3 and FGCN_MATH_BF16): the fgcn_pack_split3 form (the bf16 mode reads its part 0 only);  K % 32 == 0.
 *   stat_partials: float[fgcn_tconv_halo_tiles(B, Th, Th_in, V)][2][N] or NULL (sums of the values written, after
 *   accumulation).  Tensors must be smaller than 2 GiB (32-bit buffer offsets). */
int fgcn_tconv_halo_tiles(int B, int Th_out, int Th_in, int V);

/* ---- INFERENCE forms of the two north-star kernels (round 6): with eval-mode BatchNorm the statistics are constants, so BatchNorm +
 * shortcut + ReLU are the producing kernel's epilogue and a block is two kernels + the attention, as SURVEY.md Appendix A.3 states it.
 * (A TRAINING step cannot do this: train-mode BatchNorm needs the statistics of the whole batch before it can be applied, so there the
 * kernels emit the partial sums and fgcn_bn_act applies them.)  Split kernels only: FGCN_MATH_BF16X3 with the bf16x3 products, or
 * FGCN_MATH_BF16.  bn_vec / res_vec: float[4][N] of fgcn_bn_eval_coeffs; res: the shortcut operand or NULL; nothing is kept for a backward.
 *
 * fgcn_tconv_halo_bn_relu -- "temporal 9x1 conv + BN + ReLU" (reference torch_src/models/mmargcn/agcn.py:49-51,134-136):
 *   out = relu(BN(conv_{taps x 1, stride 1}(in) + bias) + [res | BN_res(res)]), res laid out like out.
 * fgcn_spatial_fwd_tile_bn_relu -- aggregation + 1x1 feature contraction + BN + shortcut + ReLU (agcn.py:103-115):
 *   g = relu(BN(sum_k conv_d[k](x . A^_k) + bias_sum) + [res | BN_res(res)]), res rows of ld_res floats (x, or the down conv's output). */
int fgcn_tconv_halo_bn_relu(const float* in, float* out, const float* w4, const float* bias, const float* bn_vec,
                            const float* res, const float* res_vec, int B, int T, int V, int K, int N, int ld_in, int ld_out,
                            int taps, int tb, int tc, void* stream);
int fgcn_spatial_fwd_tile_bn_relu(const float* x, const float* a_hat, const void* w3, const float* bias_sum, float* g,
                                  const float* bn_vec, const float* res, int ld_res, const float* res_vec,
                                  int B, int T, int V, int Cin, int Cout, int ld_x, int ld_g, int a_hat_batched, void* stream);

/* ---- storage types and `half_mask` (bfloat16 tensors: math mode FGCN_MATH_BF16 only; round 6) ------------------------------------------------
 * The reference's MixedPrecisionStep (torch_src/session/procedures/step.py:55-78: torch.cuda.amp.autocast around model(x)) keeps activations in
 * half precision: every convolution / matmul OUTPUT is a half-precision tensor and BatchNorm / ReLU / the residual adds read and write half
 * precision too; only statistics, softmax and accumulators are float32.  The fifteen entry points of the table take `half_mask`, immediately
 * before `stream`: one bit per activation-sized tensor argument, in argument order (set = the tensor is bfloat16, `unsigned short` bit patterns,
 * contiguous, strides in elements; those arguments are `void*`).  Mask 0 = all float32, valid in every math mode; any other mask needs
 * FGCN_MATH_BF16.  Accumulation, BatchNorm statistics (summed from the float32 accumulators, before the rounding of the stored value) and
 * every small tensor stay float32.
 *   A bfloat16 INPUT of a matrix kernel changes nothing: the FGCN_MATH_BF16 kernels round their f32 operands to bfloat16 (to nearest even) as
 *   they stage them, so a producer that writes the bfloat16 values directly -- G, the temporal conv's input (fgcn_bn_act, mask 4); dU, the
 *   gradient of its output, and dY, that of the spatial stage's (fgcn_bn_act_bwd_apply, mask 8); emb, the attention embeddings
 *   (fgcn_emb_fwd_tile, mask 2) -- leaves every result BIT-IDENTICAL to the f32-storage form (one rounding per value either way) while the
 *   consumers copy instead of convert and move half the bytes.
 *   A bfloat16 OUTPUT is the float32 result rounded to nearest even once.  Contract of the mode with half-precision activations: SURVEY.md
 *   section 7 (logits <= 1e-2, loss <= 1e-3 abs ..., gradient cosine >= 0.98).
 * Masks a kernel is not built for are refused with FGCN_E_BADARG before any launch.
 *   fgcn_bn_act             bit 0 a, 1 b (shortcut), 2 out
 *   fgcn_bn_act_pool        bit 0 a, 1 b
 *   fgcn_bn_act_bwd_reduce  bit 0 dout, 1 a, 2 b          (grp_rows > 0: dout is the float32 per-group form; the ReLU gate is the sign image)
 *   fgcn_bn_act_bwd_apply   bit 0 dout, 1 a, 2 b, 3 da, 4 db  (a bfloat16 db: C % 8 == 0, not accumulating)
 *   fgcn_tconv_halo         bit 0 in, 1 out               masks 0, 1, 3; a bfloat16 in: the tap form, no fused input stage; a bfloat16 out: the
 *                                                         plain store epilogue (no accumulation / BatchNorm-backward sums)
 *   fgcn_tconv_wgrad        bit 0 a, 1 g                  masks 0, 3 (mask 3: a_amax = g_amax = NULL)
 *   fgcn_pw_wgrad           bit 0 a, 1 g                  masks 0, 3 (mask 3: a_amax = g_amax = NULL)
 *   fgcn_spatial_fwd_tile   bit 0 x, 1 y                  masks 0, 2, 3
 *   fgcn_emb_fwd_tile       bit 0 x, 1 emb                (bit 1: emb is not NULL)
 *   fgcn_spatial_bwd_tile   bit 0 dy, 1 x, 2 dx + gated addends (a per-group extra1 stays float32)     masks 0, 1, 3, 7
 *   fgcn_spatial_wgrad_tile bit 0 x, 1 dy                 masks 0, 2, 3
 *   fgcn_emb_dx_tile        bit 0 emb, 1 dx               masks 0, 1, 3
 *   fgcn_emb_wgrad_tile     bit 0 emb, 1 x                masks 0, 1, 3
 *   fgcn_rows_gemm          bit 0 in, 1 out               (a bfloat16 tensor: a single problem, taken whole; a bfloat16 out: no accumulation)
 *   fgcn_pw_gemm            bit 0 in, 1 out               (a bfloat16 out: no accumulation) */

/* bn_a / bn_mask / bn_vec (all NULL, or all given where fgcn_tconv_halo_bn_sums() == 1: the split-bf16 kernel of the bf16 math
 * modes): the call is the data gradient that produces dG, the gradient of G = relu(BatchNorm(a) + shortcut) (agcn.py:113-115), and
 * stat_partials receives the BatchNorm-backward sums instead of the forward moments -- per row tile and channel
 *   [0] sum dp,  [1] sum dp * (a - mean) * rstd,   dp = (value written) * [bit of bn_mask],
 * bn_a = the BatchNorm's input (same shape as out, contiguous: ld_out == N), bn_mask = fgcn_bn_act's sign image of G, bn_vec =
 * fgcn_bn_finalize's vector (mean at [0, N), rstd at [N, 2N)): what fgcn_bn_act_bwd_reduce computes in a pass of its own over dG
 * and a (two activation reads and two launches less per identity block). */
int fgcn_tconv_halo_bn_sums(void);
/* fin_vec / fin_res / fin_out / fin_mask (all NULL, or all given where fgcn_tconv_halo_bn_sums() == 1; taps > 1, a plain contiguous
 * input view with ld_in == K, V <= 32): the INPUT STAGE of the temporal conv fused into its image fill -- the north star's "temporal
 * 9x1 conv + BN + ReLU as one kernel", consumer side.  `in` is then y, the input of the graph convolution's BatchNorm, and the conv
 * runs on G = relu(y * scale + shift + fin_res) (agcn.py:113-115; fin_vec = fgcn_bn_finalize's float[4][K], fin_res = the identity
 * shortcut x, laid out like `in`), formed as the rows are staged; G (fin_out, like `in`) and its sign image (fin_mask, fgcn_bn_act's
 * layout, rows*K/8 bytes) are written once as by-products (the backward's weight gradient and ReLU gate read them): what an
 * fgcn_bn_act(res_mode = 1, relu = 1) pass in front of this call computes, without that pass. */
int fgcn_tconv_halo(const void* in, void* out, const float* w4, int w_form, const float* bias, float* stat_partials,
                    int B, int Th, int V, int K, int N, int ld_in, int ld_out,
                    int T_in_full, int in_s, int in_o, int Th_in,
                    int T_out_full, int out_s, int out_o,
                    int taps, int tb, int tc, int accumulate, const float* bn_a, const unsigned char* bn_mask,
                    const float* bn_vec, const float* fin_vec, const float* fin_res, float* fin_out, unsigned char* fin_mask,
                    unsigned* in_amax, int half_mask, void* stream);
/* w_form: the layout of w4 ("Product form" above: FGCN_PACK_K4, FGCN_PACK_SPLIT3 or FGCN_PACK_SPLIT2H).
 * in_amax (may be NULL; written with FGCN_PACK_SPLIT2H weights only): a device word that receives, by integer atomic maximum (order-independent), the
 * float bits of max |in| over everything this call stages -- zero it before the first call that should count; the weight gradient of
 * the same tensor takes it as its operand scale (fgcn_tconv_wgrad). */

/* partial[s][j][k][n] = sum over the s-th slice of rows m=(n,tg,v) of a[(n,ti(tg,j),v), k] * g[m, n]
 *   (weight gradient of the same convolutions; autograd backward of agcn.py:41-42,71-73,77).
 *   partial: float[nsplit][taps][K][N]; reduce with fgcn_reduce_sum.  nsplit >= 1. */
int fgcn_rows_wgrad(const float* a, const float* g, float* partial,
                    int B, int T_a, int T_g, int V, int K, int N, int ld_a, int ld_g,
                    fgcn_tmap map, int nsplit, void* stream);

/* Weight gradient of the (taps x 1) temporal convolution, all taps of one call in a single pass over the rows
 * (backward of agcn.py:41-51 w.r.t. conv.weight):
 *     partial[slab][tap0 + i*tap_step][k][n] = sum over the slab's rows (b, t, v) of
 *                                              a[(b, (t + shift0 + i)*a_s + a_o, v), k] * g[(b, t, v), n],  i < ntaps
 *   a: float[B][T_a_full][V][ld_a] seen through the frame view f -> f*a_s + a_o (Th_a frames; frames outside the view
 *   contribute zeros), g: float[B][T_g][V][ld_g].  A stride-s convolution is s calls (one per residue of the tap offset).
 *   partial: float[fgcn_tconv_wgrad_slabs(N, nsplit)][taps_total][K][N]; every slab of the taps of this call is written;
 *   the caller sums the slabs (fgcn_reduce_sum).  ntaps in {1..5, 9}; K, N, ld_a, ld_g multiples of 4; tensors < 2 GiB. */
int fgcn_tconv_wgrad_slabs(int N, int nsplit);
/* slabs of fgcn_pw_wgrad's partial buffer, and the number of workgroups of a fgcn_tconv_wgrad launch that are resident
 * at once in the current math mode (choose nsplit so that tiles * nsplit stays within it) */
int fgcn_pw_wgrad_slabs(int N, int nsplit);
int fgcn_tconv_wgrad_resident(int N);
int fgcn_pw_wgrad_resident(int N);
int fgcn_tconv_wgrad(const void* a, const void* g, float* partial, int B, int T_g, int V, int K, int N,
                     int ld_a, int ld_g, int T_a_full, int a_s, int a_o, int Th_a,
                     int ntaps, int shift0, int tap0, int tap_step, int taps_total, int nsplit,
                     const unsigned* a_amax, const unsigned* g_amax, int half_mask, void* stream);

/* Weight gradient of a 1x1 convolution (theta|phi embedding, conv_d on the stacked agg, down, residual): the same
 * kernel with one accumulator per 32-channel chunk of a instead of per tap (each g fragment feeds up to 6 MFMAs):
 *     partial[slab][k][n] = sum over the slab's rows (b, t, v) of a[(b, t*a_s + a_o, v), k] * g[(b, t, v), n]
 *   partial: float[fgcn_tconv_wgrad_slabs(N, nsplit)][K][N].  Same alignment / size rules as fgcn_tconv_wgrad. */
int fgcn_pw_wgrad_chunks(int K, int N);
int fgcn_pw_wgrad(const void* a, const void* g, float* partial, int B, int T_g, int V, int K, int N,
                  int ld_a, int ld_g, int T_a_full, int a_s, int a_o, int nsplit,
                  const unsigned* a_amax, const unsigned* g_amax, int half_mask, void* stream);
/* a_amax / g_amax (both weight-gradient entry points; may be NULL): device words holding the float bits of max |a| / max |g| over
 * the whole tensors, as fgcn_tconv_halo / fgcn_pw_gemm leave them in `in_amax`.  With both given in FGCN_MATH_BF16X3 (whatever the
 * product form of the context: the call states its form by what it passes) the split kernel runs its f16x2 form (operands scaled by the exact powers of two that put those maxima into [2^14, 2^15)); without
 * them it runs the bf16x3 form.  A bfloat16 operand pair (half_mask 3) takes neither: FGCN_E_BADARG. */

/* dst[i] (+)= sum_s src[s*count + i]   (deterministic tree-free column sum; also bias / adj_b gradients) */
int fgcn_reduce_sum(float* dst, const float* src, int S, long long count, int accumulate, void* stream);

/* The same slab sum written through strides: element (tap, k, n) of the [taps][K][N] slabs lands at
 * dst[tap*st_tap + k*st_k + n*st_n] for k < K_dst (input channels beyond K_dst are padding) -- i.e. directly in a conv
 * parameter's own (out, in, taps, 1) layout, so the gradient needs no transposing copy. */
int fgcn_reduce_sum_strided(float* dst, const float* src, int S, int taps, int K, int N, int K_dst,
                            long long st_tap, long long st_k, long long st_n, int accumulate, void* stream);

/* Up to FGCN_REDUCE_MAX_ITEMS of those slab sums in one launch (the leaf reductions of a block's backward -- weight-gradient
 * slabs, adj_b, bias partials -- collected and issued together; same arithmetic and summation order as the single calls;
 * a plain fgcn_reduce_sum over `count` elements is the item taps = K = K_dst = 1, N = count, st_n = 1). */
#define FGCN_REDUCE_MAX_ITEMS 8
typedef struct {
    float* dst;
    const float* src;
    long long st_tap, st_k, st_n;
    int S, taps, K, N, K_dst, accumulate;
} fgcn_reduce_item;
int fgcn_reduce_multi(const fgcn_reduce_item* items, int n_items, void* stream);

/* FGCN_MATH_BF16X3 form of a packed (taps, K, N) weight: dst = unsigned short[3][taps][ceil(K/8)][N][8], part 0/1/2 the
 * high / middle / low bfloat16 term of the exact split w = w_h + w_m + w_l (channels beyond K are zeros; part 0 alone is the
 * round-to-nearest-even bfloat16 of w).  This is what fgcn_tconv_halo takes as `w4` in both bf16 math modes.  acc_order = 1 (fgcn_spatial_fwd's `wd` in that
 * mode; ceil(K/16)*2 groups): group 2*k16 + h holds k = 16*k16 + 4h + (j & 3) + 8*(j >> 2), the order in which a 32x32
 * MFMA accumulator enumerates its rows. */
int fgcn_pack_split3(unsigned short* dst, const float* src, int taps, int K, int N, int acc_order, void* stream);

/* All packed / split weight forms of a model in ONE launch (the step after an optimizer update re-lays-out ~250 small
 * matrices; as separate launches they sit on the critical path of a small-batch step).  An item describes one form: the
 * logical matrix W[tap][k][n] (taps x K x N) as the SUM of up to FGCN_PACK_MAX_SEG source segments -- segment s covers
 * taps [t0, t0+tlen), rows [k0, k0+klen), columns [n0, n0+nlen) and reads
 *     src[((tap-t0)*tap_step + tap0)*st_tap + (k-k0)*st_k + (n-n0)*st_n]
 * (disjoint segments = concatenation of parameters along k or n; overlapping = their sum, e.g. conv_d's three biases; an
 * uncovered range = zero padding of the channel count) -- and the layout written to dst:
 *   FGCN_PACK_PLAIN       float[taps][K][N]
 *   FGCN_PACK_K4          float[taps][ceil(K/4)][N][4]        (k-interleaved: fgcn_tconv_halo / fgcn_spatial_fwd, f32 mode)
 *   FGCN_PACK_SPLIT3      the fgcn_pack_split3 form, acc_order 0   (unsigned short[3][taps][ceil(K/8)][N][8])
 *   FGCN_PACK_SPLIT3_ACC  the fgcn_pack_split3 form, acc_order 1
 * `kgroups` must equal fgcn_pack_kgroups(mode, K).  items_dev: the item table in DEVICE memory; blockmap_dev: int[2] per
 * workgroup = (item index, index of the workgroup's first 256 units within the item), fgcn_pack_units(...) units per item
 * (one unit = one element, float4, or 8-value split group).  The reference's counterpart is nothing: its Conv2d weights are
 * consumed in place by ATen (agcn.py:41-42,71-73,77). */
#define FGCN_PACK_MAX_SEG 6
#define FGCN_PACK_PLAIN 0
#define FGCN_PACK_K4 1
#define FGCN_PACK_SPLIT3 2
#define FGCN_PACK_SPLIT3_ACC 3
/*   FGCN_PACK_SPLIT2H     FGCN_PRODUCTS_F16X2 weights: a 16-byte header whose first word holds the float bits of max |W| over the
 *                         form, then _Float16[2][taps][ceil(K/8)][N][8] = the high / low f16 parts of W * 2^s, s = 141 - biased
 *                         exponent of that maximum (scaled maximum in [2^14, 2^15); s = 0 for an all-zero form).  Needs
 *                         fgcn_pack_run_scaled (the maximum is a pass of its own). */
#define FGCN_PACK_SPLIT2H 4
/*   FGCN_PACK_SPLIT2H_ACC the same with the k order of FGCN_PACK_SPLIT3_ACC (fgcn_spatial_fwd's weights for the f16x2 products) */
#define FGCN_PACK_SPLIT2H_ACC 5
typedef struct {
    const float* src;
    long long st_tap, st_k, st_n;
    int t0, tlen, k0, klen, n0, nlen, tap0, tap_step;
} fgcn_pack_seg;
typedef struct {
    void* dst;
    int mode, taps, K, N, kgroups, nseg;
    fgcn_pack_seg seg[FGCN_PACK_MAX_SEG];
} fgcn_pack_item;
int fgcn_pack_kgroups(int mode, int K);
long long fgcn_pack_units(int mode, int taps, int K, int N);
int fgcn_pack_run(const fgcn_pack_item* items_dev, const int* blockmap_dev, int n_workgroups, void* stream);
/* the same for tables that hold FGCN_PACK_SPLIT2H items: three launches -- headers zeroed, per-form maxima (integer atomic max over
 * the float bits: order-independent, so reproducible), then the pack proper */
int fgcn_pack_run_scaled(const fgcn_pack_item* items_dev, const int* blockmap_dev, int n_workgroups, int n_items, void* stream);

/* dst[j][k][n] = src[n*st_n + k*st_k + jj*st_tap], jj = flip ? taps-1-j : j ; n >= N_src zero-filled up to N_dst
 * (weight re-layout into the packed [taps][K][N] form; N_dst % 4 == 0). */
int fgcn_pack_weight(float* dst, const float* src, int taps, int K, int N_src, int N_dst,
                     long long st_tap, long long st_k, long long st_n, int flip, void* stream);

/* Global average pooling in front of the classifier (agcn.py:196-197: mean over frames and joints, then persons):
 * out[g][c] = mean over the `rows` consecutive rows of group g of x[(g*rows + r)*ld + c].  Two fixed-order stages;
 * partial: float[groups * fgcn_group_mean_splits(groups, rows)][C]. */
int fgcn_group_mean_splits(int groups, int rows);
int fgcn_group_mean(const float* x, float* partial, float* out, int groups, int rows, int C, int ld, void* stream);

/* ---- joint-mixing kernels (the "graph" part: A.X over the K=3 partition adjacencies) ------------------ */
typedef struct {
    short mat;        /* which V x V matrix of the sample (0..n_mats-1) */
    short transpose;  /* 0: out_joint = row index of mat;  1: out_joint = column index */
    short in_c_lo;    /* input channel of lane 0  (lanes 0..15 read in_c_lo + lane) */
    short in_c_hi;    /* input channel of lane 16 (lanes 16..31 read in_c_hi + lane-16) */
    short mask;       /* bit0: lanes 0..15 take this term, bit1: lanes 16..31 take it */
} fgcn_mix_term;
typedef struct {
    short out_c;      /* first of the (up to 32) output channels of this tile */
    short width;      /* lanes (channels) of the tile that exist: 1..32 */
    short nterms;     /* 1..3 */
    fgcn_mix_term term[3];
} fgcn_mix_item;

/* For every sample n, frame t and item: out[(n,t,u), out_c + l] (+)= sum_terms sum_v M[u][v] * in[(n,t,v), in_c(l)]
 *   with M = mats[n][term.mat] (or its transpose).  One kernel serves
 *     agg_k = x . A^_k                (agcn.py:109-110, torch.matmul(A2, A1))        and the two backward mixes
 *     dx += sum_k dagg_k . A^_k^T ,   dtheta_k = dS_k . phi_k ,  dphi_k = dS_k^T . theta_k.
 *   mats: float[B or 1][n_mats][V][V]; mats_batched = 0 shares one set across the batch (static-adjacency ST-GCN).
 *   Channels >= in_channels / out_channels are treated as absent. */
int fgcn_joint_mix(const float* in, float* out, const float* mats, int B, int T, int V,
                   int ld_in, int ld_out, int in_channels, int out_channels, int n_mats, int mats_batched,
                   const fgcn_mix_item* items, int n_items, int accumulate, void* stream);

/* Channel-group variant (no 16-lane masks): lane j of a group owns `vw` (1 or 2) consecutive channels, one item
 * covers up to 32*vw channels with 4/8-byte buffer loads and stores; all items of a call have the same `nch`.
 * Same formula as fgcn_joint_mix; used for the agg recompute, dx and the embedding gradients of the backward pass.
 * Both tensors must be smaller than 2 GiB. */
typedef struct {
    short mat;
    short transpose;
    short in_c;       /* first input channel of the group (multiple of vw) */
} fgcn_mixv_term;
typedef struct {
    short out_c;      /* first output channel of the group (multiple of vw) */
    short nch;        /* channels in the group: vw .. 32*vw, multiple of vw */
    short nterms;     /* 1..3 */
    fgcn_mixv_term term[3];
} fgcn_mixv_item;
int fgcn_joint_mix_vec(const float* in, float* out, const float* mats, int B, int T, int V,
                       int ld_in, int ld_out, int n_mats, int mats_batched,
                       const fgcn_mixv_item* items, int n_items, int vw, int accumulate,
                       float* colsum_partial, unsigned* out_amax, void* stream);
/* colsum_partial (optional, only without accumulation): float[B * fgcn_joint_mix_chunks(B, T)][ld_out]; row i receives the
 * column sums of everything workgroup i wrote (the theta|phi bias gradient falls out of the embedding-gradient mix
 * instead of a separate pass over its output); channels no item writes receive 0.
 * out_amax (optional): a device word that receives, by integer atomic maximum, the float bits of the largest magnitude written -- the
 * operand scale of the f16x2 weight gradient that reads `out` (fgcn_pw_wgrad); zero it before the launches that should count. */
int fgcn_joint_mix_chunks(int B, int T);

typedef struct {
    short c1;     /* first channel of in1 */
    short c2;     /* first channel of in2 */
    short width;  /* channels contracted */
    short mat;    /* output matrix index */
} fgcn_gram_item;

/* partial[n][chunk][mat][u][w] = sum_{t in chunk} sum_c in1[(n,t,u), c1+c] * in2[(n,t,w), c2+c]   (32x32 padded)
 *   joint affinity  theta^T phi  (agcn.py:104-106, torch.matmul(A1, A2)) and dA^_k = x^T dagg_k in backward.
 *   partial: float[B][nchunk][n_mats][32][32], nchunk = ceil(T / t_chunk). */
int fgcn_joint_gram(const float* in1, const float* in2, float* partial, int B, int T, int V,
                    int ld1, int ld2, int t_chunk, int n_mats, const fgcn_gram_item* items, int n_items,
                    void* stream);

/* Weight gradient of conv_d with the aggregation recomputed on chip (backward of agcn.py:109-110 w.r.t. conv_d[k].weight):
 *     partial[slab][k*Cin + c][o] = sum over the slab's frames of (n, t) and joints w of
 *                                   (sum_v x[(n,t,v), c] * A^_k[n][v][w]) * dy[(n,t,w), o]
 *   replaces fgcn_joint_mix_vec (agg = x . A^, 3 activations wide, written to HBM) + the row weight-gradient GEMM over it.
 *   partial: float[B * fgcn_spatial_wgrad_chunks(B, T, Cin, Cout)][n_subsets * Cin][Cout]; the caller sums the slabs.
 *   Honors fgcn_set_math_mode for the Cin x Cout contraction (the joint mixing stays f32). */
int fgcn_spatial_wgrad_chunks(int B, int T, int Cin, int Cout);
int fgcn_spatial_wgrad(const float* x, const float* dy, const float* mats, float* partial,
                       int B, int T, int V, int Cin, int Cout, int ld_x, int ld_dy, int n_subsets,
                       int mats_batched, void* stream);

/* Both consumers of dagg = dY . Wd in one pass over it (backward of agcn.py:109-110):
 *     dx[(n,t,v), c]        (+)= sum_k sum_w A^_k[n][v][w] * dagg[(n,t,w), k*C + c]
 *     partial[n][chunk][k][v][w] = sum_{t in chunk} sum_c x[(n,t,v), c] * dagg[(n,t,w), k*C + c]      (32x32 padded)
 *   i.e. fgcn_joint_mix_vec (dx) and fgcn_joint_gram (dA^_k = x^T dagg_k) without reading the 3*C-wide dagg twice.
 *   mats: float[B or 1][n_subsets][V][V]; partial: float[B][ceil(T/t_chunk)][n_subsets][32][32].  C % 4 == 0.
 *   extra1/mask1, extra2/mask2 (NULL or both of a pair): gated addends of dx,
 *     dx[(n,t,v), c] += extra_i[(n,t,v), c] * [bit ((n,t,v)*C + c) of mask_i]
 *   -- the gradients that reach x through the block's identity shortcuts (y += x before the ReLU of the graph convolution,
 *   agcn.py:114, and + residual(x) before the block's output ReLU, agcn.py:135): extra = incoming gradient of that ReLU,
 *   mask = fgcn_bn_act's sign image of its output; contiguous float[B][T][V][C], C % 8 == 0.  Writing them here saves the
 *   BatchNorm-backward kernels a read-modify-write of dx each. */
int fgcn_joint_dagg(const float* x, const float* dagg, const float* mats, float* dx, float* partial,
                    int B, int T, int V, int C, int ld_x, int ld_dagg, int ld_dx, int n_subsets,
                    int mats_batched, int t_chunk, int accumulate, const float* extra1, const unsigned char* mask1,
                    const float* extra2, const unsigned char* mask2, void* stream);

/* S = scale * sum_chunks partial ; C[n,k,:,w] = softmax over v ; a_hat = C + adj_a[k] + adj_b[k]   (agcn.py:84,100,106-108)
 *   c_out, a_hat: float[B][K][V][V]; adj_a (constant partition adjacency), adj_b (learned, may be NULL): float[K][V][V].
 *   use_softmax = 0 gives the static-adjacency case a_hat = adj_a + adj_b (c_out untouched). */
int fgcn_adj_softmax_fwd(const float* partial, int nchunk, float scale, const float* adj_a, const float* adj_b,
                         float* c_out, float* a_hat, int B, int K, int V, int use_softmax, void* stream);
/* d_a_hat[n,k] = sum_chunks partial ; dS = scale * C .* (dC - colsum(C .* dC))  with dC = d_a_hat (softmax backward) */
int fgcn_adj_softmax_bwd(const float* partial, int nchunk, float scale, const float* c_in,
                         float* d_a_hat, float* d_s, int B, int K, int V, void* stream);

/* ---- wide graphs: 33 .. FGCN_MAX_V_WIDE joints ------------------------------------------------------------ */
/* The joint-contracting kernels above hold a joint index on one 32-wide MFMA dimension (V <= FGCN_MAX_V).  These take graphs up to
 * FGCN_MAX_V_WIDE joints (64 x 64 matrices as 2 x 2 blocks of 32 x 32); the host uses them only for V > FGCN_MAX_V.  Same formulas,
 * f32 products and accumulation in every math mode.  V > FGCN_MAX_V_WIDE: FGCN_E_BADARG, the message names the limit.
 *
 * fgcn_joint_mix_wide: fgcn_joint_mix_vec's formula with its item table, one channel per lane: every item covers 1..32 channels
 *   (its own nch; in_c / out_c need no alignment), no column sums, no amax.  mats: float[B or 1][n_mats][V][V], n_mats <= 3. */
int fgcn_joint_mix_wide(const float* in, float* out, const float* mats, int B, int T, int V, int ld_in, int ld_out,
                        int n_mats, int mats_batched, const fgcn_mixv_item* items, int n_items, int accumulate, void* stream);
/* fgcn_joint_gram_wide: fgcn_joint_gram's formula, matrix i from item i (1..3 items; channels, widths and strides multiples of 4),
 *   partial: float[B][ceil(T / t_chunk)][n_items][64][64] (rows / columns >= V are zeros). */
int fgcn_joint_gram_wide(const float* in1, const float* in2, float* partial, int B, int T, int V, int ld1, int ld2, int t_chunk,
                         const fgcn_gram_item* items, int n_items, void* stream);
/* fgcn_adj_softmax_{fwd,bwd}_wide: fgcn_adj_softmax_{fwd,bwd} on partials of 64 x 64 matrices (fgcn_joint_gram_wide's layout, n_items = K). */
int fgcn_adj_softmax_fwd_wide(const float* partial, int nchunk, float scale, const float* adj_a, const float* adj_b,
                              float* c_out, float* a_hat, int B, int K, int V, int use_softmax, void* stream);
int fgcn_adj_softmax_bwd_wide(const float* partial, int nchunk, float scale, const float* c_in,
                              float* d_a_hat, float* d_s, int B, int K, int V, void* stream);

/* ---- BatchNorm / activation epilogues ------------------------------------------------------------------ */
/* mean/var from row-tile partials -> scale = gamma*rstd, shift = beta - mean*scale, and the running-stat update
 * (momentum, unbiased variance) of nn.BatchNorm2d in train mode (agcn.py:44,78,83; torch defaults eps 1e-5, 0.1).
 * out_vec: float[4][C] = {mean, rstd, scale, shift}.  running_* may be NULL.
 * pivot (may be NULL: partials float[n_partials][2][C], pivot_inner / pivot_outer ignored): the partials are
 * fgcn_data_bn_stats(centered != 0)'s, float[n_partials][4][C] = per tile the sums of x, x^2, x - p and (x - p)^2 about the per-channel
 * pivot p[c] = pivot[(c / pivot_inner) * pivot_outer + c % pivot_inner].  A channel whose offset is no larger than its spread
 * (mean^2 <= var) is finalised from the first two rows, exactly as without a pivot; any other channel from the centred rows,
 * mean = p + a / n, var = b / n - (a / n)^2, so its variance does not lose digits to its offset and a constant channel gets 0. */
int fgcn_bn_finalize(const float* partials, int n_partials, long long count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps,
                     float* out_vec, int C, const float* pivot, int pivot_inner, long long pivot_outer, void* stream);
/* eval mode: scale/shift from running statistics; out_vec as above (mean = running_mean, rstd = 1/sqrt(var+eps)) */
int fgcn_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, float* out_vec, int C, void* stream);

/* out = act( a*scale_a + shift_a + r ),  r = 0 | b | b*scale_b + shift_b          (agcn.py:113-115, :135-136)
 *   res_mode: 0 none, 1 identity, 2 batch-normalised.  vec_a / vec_b: the float[4][C] of fgcn_bn_finalize.
 *   rows x C elements, all tensors share row stride ld (== C). relu: 0/1. */
/*   sign_mask (may be NULL; needs rows*C % 8 == 0): also stores bit e%8 of byte e/8 = [!(out[e] <= 0)] (set for a NaN: rule 2 above) -- rows*C/8 bytes the
 *   backward passes can read instead of the whole of `out` (the ReLU gate of the reference's autograd). */
int fgcn_bn_act(const void* a, const float* vec_a, const void* b, const float* vec_b, void* out, unsigned char* sign_mask,
                long long rows, int C, int res_mode, int relu, int half_mask, void* stream);

/* The last block's epilogue and the pooling behind it in one pass (agcn.py:135-136 then :196-197):
 *     pooled[g][c] = mean over the grp_rows consecutive rows r of group g of relu( a*scale_a + shift_a + r-term )[(g*grp_rows + r), c]
 *   -- fgcn_bn_act (relu = 1) followed by fgcn_group_mean, but `out` is never written: only its sign image (sign_mask, rows*C/8 bytes,
 *   what the backward reads) and the sums.  C % 8 == 0; partial: float[groups * fgcn_bn_act_pool_splits(groups, grp_rows)][C].
 *   Fixed summation order (another one than fgcn_group_mean's). */
int fgcn_bn_act_pool_splits(int groups, int grp_rows);
int fgcn_bn_act_pool(const void* a, const float* vec_a, const void* b, const float* vec_b, unsigned char* sign_mask,
                     float* partial, float* pooled, int groups, int grp_rows, int C, int res_mode, int half_mask, void* stream);

/* Backward of the above, pass 1 (reductions): with dP = dout .* [!(out <= 0)] (or dout when relu = 0)
 *   partials[tile][0][c] = sum dP, [1] = sum dP * a_hat, [2] = sum dP * b_hat   (a_hat = (a-mean_a)*rstd_a).
 *   The gate comes from sign_mask when it is given (then `out` may be NULL), else from `out`.
 *   grp_rows (both passes; 0: dout is (rows, C)) > 0: the gradient of a POOLED output (fgcn_bn_act_pool) -- dout is float[rows / grp_rows][C],
 *   one row per group of grp_rows consecutive rows (the pooled gradient already divided by the group size); every row reads its group's row
 *   instead of a rows x C broadcast of it. */
int fgcn_bn_act_bwd_reduce(const void* dout, int grp_rows, const float* out, const unsigned char* sign_mask, const void* a,
                           const float* vec_a, const void* b, const float* vec_b, float* partials, int n_tiles, long long rows,
                           int C, int res_mode, int relu, int half_mask, void* stream);
/* pass 2: da = scale_a * (dP - s1/m - a_hat*s2a/m) (train) or scale_a*dP (eval);
 *         db = dP (identity) or scale_b*(dP - s1/m - b_hat*s2b/m);  sums: float[3][C] reduced partials.
 *   db may be NULL (res_mode 0); db_accumulate adds into db instead of storing. */
int fgcn_bn_act_bwd_apply(const void* dout, int grp_rows, const float* out, const unsigned char* sign_mask, const void* a,
                          const float* vec_a, const void* b, const float* vec_b, const float* sums, void* da, void* db,
                          long long rows, int C, int res_mode, int relu, int train, int db_accumulate, int half_mask, void* stream);
/* number of row tiles the reduce kernel uses for `rows` rows (leading dim of its partials) */
int fgcn_elem_tiles(long long rows);
/* The same three passes for a plain BatchNorm (no residual, no activation) whose result is a CHANNEL WINDOW of a wider tensor: one of the
 * six branches of MS-G3D's multi-scale temporal convolution, concatenated on the channel axis (reference torch_src/models/msg3d/ms_tcn.py:88-109).
 *   fgcn_bn_apply_ld:      out[r * ld_out + c] = a[r * C + c] * scale[c] + shift[c]     (out = window base; ld_out >= C, both multiples of 4)
 *   fgcn_bn_bwd_reduce_ld: partials as fgcn_bn_act_bwd_reduce with res_mode = relu = 0, dout read as dout[r * ld_dout + c] (dout = window base)
 *   fgcn_bn_bwd_apply_ld:  da (contiguous, float[rows][C]) as fgcn_bn_act_bwd_apply with res_mode = relu = 0, dout read the same way
 * -- no torch.cat of the branches and no contiguous copies of its backward slices. */
int fgcn_bn_apply_ld(const float* a, const float* vec_a, float* out, long long rows, int C, int ld_out, void* stream);
int fgcn_bn_bwd_reduce_ld(const float* dout, int ld_dout, const float* a, const float* vec_a, float* partials, int n_tiles,
                          long long rows, int C, void* stream);
int fgcn_bn_bwd_apply_ld(const float* dout, int ld_dout, const float* a, const float* vec_a, const float* sums, float* da,
                         long long rows, int C, int train, void* stream);

/* partials[tile][c] = sum over the tile's rows of x[row][c]   (bias gradients); n_tiles = fgcn_elem_tiles(rows) */
int fgcn_col_sum(const float* x, float* partials, long long rows, int C, int ld, void* stream);

/* ---- fused spatial block forward (north-star kernel 1) -------------------------------------------------- */
/* y[(n,t,w), o] = sum_k bd_k[o] + sum_c Wd_k[o][c] * sum_v x[(n,t,v), c] * a_hat[n][k][v][w]
 *   = conv_d[k](x . A^_k) summed over the K subsets (agcn.py:103-111) in ONE kernel: A^ staged in LDS, the joint
 *   aggregation and the Cin x Cout contraction chained on MFMA without materialising agg.
 *   wd: k-interleaved packed float[K*Cin/4][Cout][4] with wd[(k*Cin+c)/4][o][(k*Cin+c)%4] = Wd_k[o][c] (Cin % 4 == 0; FGCN_PACK_K4), or in
 *   FGCN_MATH_BF16X3 with Cin % 32 == 0 the accumulator-ordered split of the same matrix (FGCN_PACK_SPLIT3_ACC / FGCN_PACK_SPLIT2H_ACC);
 *   w_form says which ("Product form" above);
 *   bias_sum: float[Cout] (= sum_k bd_k) or NULL.
 *   stat_partials: float[fgcn_spatial_tiles(B,T)][2][Cout] or NULL. */
int fgcn_spatial_fwd(const float* x, const float* a_hat, const float* wd, int w_form, const float* bias_sum, float* y,
                     float* stat_partials, int B, int T, int V, int Cin, int Cout, int ld_x, int ld_y,
                     int n_subsets, int a_hat_batched, void* stream);
int fgcn_spatial_tiles(int B, int T);
/* The same product in its TILE form (split-bf16 math mode, bf16x3 products; fgcn_spatial_tile.hip): a workgroup owns 128 / V whole
 *   frames of one sample (125 of 128 matrix rows at V = 25 instead of 25 of 32 columns per frame) times 64 / 128 output columns; the
 *   aggregation x . A^_k of a (32-channel tile, subset) pair is formed once per workgroup on the matrix pipe and written to an LDS
 *   image, from which the feature contraction runs like one tap of fgcn_tconv_halo.
 *   w3: fgcn_pack_split3 form (acc_order 0) of the (3 Cin) x Cout matrix [k * Cin + c][o] = Wd_k[o][c] (one tap, K = 3 Cin); three
 *   subsets; Cin % 64 == 0; 16 <= V <= 32.  stat_partials: float[fgcn_spatial_fwd_tile_tiles(B, T, V)][2][Cout] or NULL.
 *   fgcn_spatial_fwd_tile_available: 1 when the current math mode / products and these sizes run on this kernel. */
int fgcn_spatial_fwd_tile(const void* x, const float* a_hat, const void* w3, const float* bias_sum, void* y,
                          float* stat_partials, int B, int T, int V, int Cin, int Cout, int ld_x, int ld_y,
                          int a_hat_batched, int half_mask, void* stream);
int fgcn_spatial_fwd_tile_tiles(int B, int T, int V);
int fgcn_spatial_fwd_tile_available(int V, int Cin, int Cout);

/* The backward of the same stage in tile form (fgcn_spatial_bwd_tile.hip; reference: the autograd backward of agcn.py:103-111,
 * SURVEY.md Appendix A.2) -- ONE launch for what fgcn_pw_gemm (dagg = dy . Wd) + fgcn_joint_dagg did through a three-activation-wide
 * tensor in HBM:
 *     dagg_k = dy . Wd_k (on chip only);  dx (+)= sum_k dagg_k . A^_k^T;  partial = per-workgroup sums of dA^_k = x^T . dagg_k.
 *   dy (B,T,V,>=Cout), x (B,T,V,>=Cin), a_hat (B or 1, 3, V, V), dx (B,T,V,>=Cin);
 *   w3: fgcn_pack_split3 form (acc_order 0) of the Cout x (3 Cin) matrix [o][k * Cin + c] = Wd_k[o][c] (one tap, K = Cout);
 *   partial: float[B][fgcn_spatial_bwd_tile_segments(B, T, V)][3][32][32] (rows v, columns w; entries beyond V are zero) -- the layout
 *   fgcn_adj_softmax_bwd sums.  Three subsets; Cin % 64 == 0, Cout % 64 == 0; 16 <= V <= 32; math mode bf16x3 with either product form (the
 *   kernel always multiplies three-way bf16 splits: fgcn_spatial_bwd_tile_available).  accumulate != 0: dx += (load, add, store); every sum has a fixed order.
 *   extra1 / mask1, extra2 / mask2 (all four or none; not with accumulate; ld_x == Cin): dx = ... + extra_i * [bit of mask_i] -- contiguous
 *   (B, T, V, Cin) tensors with fgcn_bn_act's one-bit sign images: the ReLU-gated gradients of the block's two identity shortcuts
 *   (agcn.py:114,135), as in fgcn_joint_dagg.
 *   extra1_group (0: the form above) > 0: the first gated addend is given per GROUP of extra1_group consecutive samples, extra1 =
 *   float[B / extra1_group][Cin]; every row of a group's samples adds its group's row (gated by mask1's bits as before) -- the gradient of the
 *   pooled output of the model's last block (fgcn_bn_act_pool) without its (B, T, V, Cin) broadcast.  Not accumulating. */
int fgcn_spatial_bwd_tile(const void* dy, const void* x, const float* a_hat, const void* w3, void* dx, float* partial,
                          int B, int T, int V, int Cin, int Cout, int ld_dy, int ld_x, int ld_dx, int a_hat_batched, int accumulate,
                          const void* extra1, int extra1_group, const unsigned char* mask1, const void* extra2,
                          const unsigned char* mask2, int half_mask, void* stream);
int fgcn_spatial_bwd_tile_segments(int B, int T, int V);
int fgcn_spatial_bwd_tile_available(int V, int Cin, int Cout);

/* conv_d's weight gradient of the same stage in tile form (fgcn_spatial_wgrad_tile.hip; reference: the autograd backward of
 * agcn.py:103-111 with respect to conv_d[k].weight): fgcn_spatial_wgrad's sum,
 *     partial[slab][k*Cin + c][o] = sum over the slab's (n, t) and joints w of (sum_v x[(n,t,v), c] * A^_k[n][v][w]) * dy[(n,t,w), o],
 *   for every channel count in 64s: a workgroup owns a (64 or 128) x (64 or 128) tile of all three subsets and walks whole frame
 *   tiles, so x and dy are read Cout/128 and Cin/128 times instead of Cout/64 and Cin/32 times, and the 3-wide aggregation that
 *   wider layers wrote with fgcn_joint_mix_vec and read back in the row weight-gradient GEMM never exists.
 *   a_hat: float[B or 1][3][V][V] (a_hat_batched: one per sample).  partial: float[fgcn_spatial_wgrad_tile_slabs(B, T, V, Cin, Cout)]
 *   [3 * Cin][Cout]; the caller sums the slabs (fgcn_reduce_multi).  Math mode FGCN_MATH_BF16X3 only (either product form; the kernel
 *   always multiplies three-way bf16 splits, the mixing included): fgcn_spatial_wgrad_tile_available.  Every sum has a fixed order.
 *   Tuning key 16: workgroups to aim for (0 = 256, one per CU; sets the slab count). */
int fgcn_spatial_wgrad_tile(const void* x, const void* dy, const float* a_hat, float* partial, int B, int T, int V, int Cin,
                            int Cout, int ld_x, int ld_dy, int a_hat_batched, int half_mask, void* stream);
int fgcn_spatial_wgrad_tile_slabs(int B, int T, int V, int Cin, int Cout);
int fgcn_spatial_wgrad_tile_available(int V, int Cin, int Cout);

/* Forward of the attention embeddings with the affinity gram on chip (fgcn_emb_fwd_tile.hip; reference: A1 = conv_a[k](x), A2 = conv_b[k](x),
 * torch.matmul(A1, A2) of SpatialGraphConv.forward, torch_src/models/mmargcn/agcn.py:104-106):
 *     emb[(n,t,v), j] = sum_c x[(n,t,v), c] Wemb[c][j] + bias[j]     (B, T, V, ld_e) rows [th0 ph0 th1 ph1 th2 ph2], each `ic` wide: written
 *     partial[n][s][k][v][w] = sum over the frames t of row segment s and the channels e of emb[(n,t,v), th_k + e] emb[(n,t,w), ph_k + e]
 * w3 = fgcn_pack_split3 of the (1, Cin, 6 ic) matrix, bias: float[6 ic].  partial: float[B][fgcn_emb_fwd_tile_segments(B, T, V, ic)][3][32][32]
 * (rows / columns >= V are zeros), the input format of fgcn_adj_softmax_fwd (nchunk = segments), which applies the 1 / (ic T) scale.
 * Replaces fgcn_pw_gemm / fgcn_rows_gemm (emb) + fgcn_joint_gram and the gram's read of the 1.5-activation-wide emb.  Sizes: 16 <= V <=
 * FGCN_MAX_V, ic 16 / 32 / 64, Cin a multiple of 32; math modes FGCN_MATH_BF16X3 (either product form: exact three-way bf16 splits) and
 * FGCN_MATH_BF16: fgcn_emb_fwd_tile_available.  Tuning key 22: resident workgroups to aim for (0 = 512; sets the segment count).
 * emb == NULL (inference: only the backward reads the embeddings): emb is not written, `partial` is all the call produces. */
int fgcn_emb_fwd_tile(const void* x, const void* w3, const float* bias, void* emb, float* partial, int B, int T, int V, int Cin, int ic,
                      int ld_x, int ld_e, int half_mask, void* stream);
int fgcn_emb_fwd_tile_segments(int B, int T, int V, int ic);
int fgcn_emb_fwd_tile_available(int V, int ic, int Cin);

/* Backward of the attention embeddings with the embedding gradient on chip (fgcn_emb_tile.hip; reference: the autograd backward of
 * SpatialGraphConv.forward through A1 = conv_a[k](x), A2 = conv_b[k](x), softmax(A1^T A2 / (ic T)), torch_src/models/mmargcn/agcn.py:104-106).
 *   emb: (B, T, V, ld_e) rows [th0 ph0 th1 ph1 th2 ph2], each `ic` channels wide (the 6 ic outputs of the stacked 1x1 embedding);
 *   d_s: float[B or 1][3][V][V], the gradient in front of the column softmax (fgcn_adj_softmax_bwd's dS, scale folded in);
 *   demb[(n,t,v), th_k + e] = sum_w dS_k[v][w] emb[(n,t,w), ph_k + e],  demb[(n,t,w), ph_k + e] = sum_v dS_k[v][w] emb[(n,t,v), th_k + e]
 * is formed per frame on the matrix pipe inside both kernels and never written:
 *   fgcn_emb_dx_tile     dx[(n,t,v), 0:Cx] (+)= demb[(n,t,v), :] . Wemb^T, w3 = fgcn_pack_split3 of the (1, 6 ic, Cx) matrix [j][c] = Wemb[j][c]
 *                        (accumulate: dx += ...; dx_old -- half_mask 3 with accumulate, or NULL -- is the float32 tensor that holds the values
 *                        to add to: dx = bfloat16(dx_old + term) is then only written);
 *   fgcn_emb_wgrad_tile  partial[s][j][c] = sum over the rows of slab s of demb[row, j] x[row, c]  (float[slabs][6 ic][Cx]: already the
 *                        parameters' (out, in) order) and bias_partial[s][j] = sum of demb[row, j] (float[slabs][6 ic]); the caller adds the
 *                        fgcn_emb_wgrad_tile_slabs(B, T, V, ic, Cx) slabs (fgcn_reduce_multi).
 * Sizes: 16 <= V <= FGCN_MAX_V, ic a multiple of 16, Cx a multiple of 64; math modes FGCN_MATH_BF16X3 (either product form: the kernels
 * always multiply exact three-way bf16 splits, the mixing included) and FGCN_MATH_BF16 (operands rounded to bfloat16 once):
 * fgcn_emb_tile_available.  Replaces fgcn_joint_mix_vec(demb) + fgcn_pw_gemm / fgcn_rows_gemm(demb . W) + fgcn_pw_wgrad(x, demb) and the
 * 1.5-activation-wide demb tensor between them.  Every sum has a fixed order.
 * Tuning key 17: fgcn_emb_wgrad_tile workgroups to aim for (0 = 256; sets the slab count). */
int fgcn_emb_dx_tile(const void* emb, const float* d_s, const void* w3, void* dx, void* workspace, int B, int T, int V, int ic, int Cx, int ld_e,
                     int ld_dx, int d_s_batched, int accumulate, const float* dx_old, int half_mask, void* stream);
/* bytes of fgcn_emb_dx_tile's caller-owned workspace (16-byte aligned; the split bf16 planes of dS and dS^T of every sample, written by a
 * small first launch and read by every workgroup of the main one) in the current math mode */
long long fgcn_emb_dx_tile_workspace(int B, int d_s_batched);
int fgcn_emb_wgrad_tile(const void* emb, const void* x, const float* d_s, float* partial, float* bias_partial, int B, int T, int V, int ic,
                        int Cx, int ld_e, int ld_x, int d_s_batched, int half_mask, void* stream);
int fgcn_emb_wgrad_tile_slabs(int B, int T, int V, int ic, int Cx);
int fgcn_emb_tile_available(int V, int ic, int Cx);

/* ---- 1-D graph convolutions on IMU graphs --------------------------------------------------- */
/* Batched transpose between the node-major (B, V, F) and feature-major (B, F, V) images of an activation:
 *     out[b][c][r] = in[b][r][c]  (r < R, c < C);  out rows have stride ld_out >= R, their columns [R, ld_out) are zero-filled.
 * STGCNGraphConvolution (torch_src/models/mmargcn/graph_convolution.py:12-52) is then three existing entry points: the 1x1
 * Conv1d = fgcn_rows_gemm over node-major rows, `torch.matmul(support, adj.t())` = fgcn_rows_gemm / fgcn_tconv_halo (taps = 1)
 * over feature-major rows with the V x V adjacency as the shared weight, residual + ReLU = fgcn_bn_act. */
int fgcn_transpose(const float* in, float* out, int B, int R, int C, int ld_in, int ld_out, void* stream);

/* Sparse form of that adjacency product (the reference's `sparse: true`, graph_convolution.py:36-43): the IMU graph's adjacency has
 * 8 .. 30 non-zeros in a row of ~2000, so `support . adj^T` is a gather of a few node rows -- no transpose, no padding, no matrix pipe:
 *     out[b][v][c] = act( sum_{j in [row_ptr[v], row_ptr[v+1])} val[j] * in[b][col[j]][c]  +  r ),   r = 0 | b | b*scale_b + shift_b
 *   in / b / out: float32 node-major (B, V, C) with row strides ld_in / ld_b / ld_out >= C (multiples of 4, 16-byte aligned bases),
 *   C % 4 == 0.  The matrix is CSR in device memory: row_ptr int[V + 1], col int[nnz], val float[nnz], columns ascending inside a row;
 *   col and val must be followed by SEVEN more readable entries (the kernel fetches entries in groups of eight and ignores those
 *   past a row's end).  Column indices are not checked on the device.
 *   res_mode / vec_b / relu / sign_mask: the epilogue of fgcn_bn_act (0 none, 1 identity, 2 `b*scale + shift` from vec_b's float[4][C]);
 *   sign_mask (may be NULL; needs C % 8 == 0): bit e%8 of byte e/8 = [!(out[e] <= 0)], e = (b*V + v)*C + c -- fgcn_bn_act's image.
 *   With the CSR form of adj this is the layer's forward (no separate fgcn_bn_act pass), with that of adj^T and no epilogue its data
 *   gradient d_support = d_main . adj: both gathers, no atomics.  float32 FMAs in ascending column order in EVERY math mode: launches
 *   agree bit for bit and the math mode changes nothing.  FGCN_E_BADARG: C % 4 != 0, a null CSR array, B*V >= 2^29 rows or a tensor
 *   of 2^31 bytes or more (the kernel's 32-bit row math). */
int fgcn_graph_spmm(const float* in, const int* row_ptr, const int* col, const float* val, const float* b, const float* vec_b,
                    float* out, unsigned char* sign_mask, int B, int V, int C, int ld_in, int ld_b, int ld_out, int res_mode,
                    int relu, void* stream);

/* Softmax of AGCNGraphConvolution's attention (graph_convolution.py:95-100: softmax over dim -2 of theta^T phi / ic, then
 * + adj[i]) on the TRANSPOSED scores st[row = (b, k, w)][v], so that it runs along the contiguous axis (V up to thousands):
 *     c = softmax_v(scale * st[row][0:V]);   a = c + adj_t[row % KV][0:V]   (adj_t: float[K*V][ld] = (adj_a + adj_b)^T per subset)
 *     backward: ds = scale * c .* (da - sum_v c .* da).
 * Rows have stride ld >= V; the columns [V, ld) of every output row are zero-filled. */
int fgcn_row_softmax_fwd(const float* st, const float* adj_t, float* c_out, float* a_out, long long rows, int V, int ld,
                         int KV, float scale, void* stream);
int fgcn_row_softmax_bwd(const float* da, const float* c, float* ds, long long rows, int V, int ld, float scale, void* stream);

/* ---- the step after the path: parameter update over flat buffers ------------------- */
/* fgcn_optim_step: one launch applies torch.optim's update to every trainable value of the model (reference: create_optimizer,
 * torch_src/session_helper.py:80-84, optimizer.step() in session/session.py:176-183):
 *   FGCN_OPT_SGD    d = g + wd*p;  buf = first step ? d : momentum*buf + (1-dampening)*d;  d = nesterov ? d + momentum*buf : buf;
 *                   p -= lr*d                                                        (state1 = buf, NULL when momentum == 0)
 *   FGCN_OPT_ADAM   g += wd*p;  m += (g-m)(1-beta1);  v = beta2*v + (1-beta2) g*g;
 *                   p -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)   (state1 = exp_avg, state2 = exp_avg_sq)
 *   FGCN_OPT_ADAMW  p *= 1 - lr*wd first, g untouched, then the same moments and update.
 *   FGCN_OPT_ASGD   g += wd*p;  p *= (float)(1 - (double)lambd*eta);  p += -eta*g;  ax = mu == 1 ? p : ax + (p - ax)*mu
 *                   (torch 2.10's _single_tensor_asgd, non-capturable path; state1 = ax, the averaged iterate; state2 must be NULL)
 * g is read as grad_scale * grads (the 1/world of the data-parallel average).  params, grads, state*: float[n], 16-byte
 * aligned, n % 4 == 0 (padding elements must hold zeros in all buffers); step counts from 1.  amsgrad / maximize: not built.
 *
 * Limit: n / 4 < 2^31 (a 34 GB parameter buffer): the tile table addresses 16-byte groups with an int.
 *
 * Parameter groups and the tile table.  The scalars come per group (torch.optim's param_groups: one optimizer kind, per-group scalars;
 * groups[g] travels by value in the kernel arguments, a new learning rate costs nothing), and which group an element belongs to comes
 * from a device-resident tile table the caller builds once:
 *   tiles[3*t + 0] = start4   first 16-byte group (float4) of the tile inside the flat buffers
 *   tiles[3*t + 1] = count4   16-byte groups in the tile, 1 .. FGCN_OPT_TILE4
 *   tiles[3*t + 2] = group    0 .. ngroups-1
 * all int (ntiles rows); one workgroup per tile.  A tile never holds values of two groups; the tiles together cover every 16-byte
 * group of the buffers exactly once (the <= 3 padding floats behind a tensor ride in that tensor's last 16-byte group and keep their
 * zeros).  The table is always given: one group is ngroups == 1 and a table whose rows all name group 0.  How the rows cut the buffer
 * does not change a bit of the result.  The library cannot read the table on the host: a tile that reaches past n / 4 or names a group
 * outside [0, ngroups) is ignored by the kernel, everything else about the table is the caller's contract.
 * Adam's step size is (float)((double)lr_g / (1 - beta1_g^step)) and sqrt(1 - beta2_g^step) per group.  state1 may be NULL only when no
 * SGD group has a momentum.
 *
 * The guard (guard != NULL; NULL: the plain update above, `step` >= 1 the host-side count) is decided on the device: clip by the
 * global gradient norm (torch.nn.utils.clip_grad_norm_ in front of optimizer.step()) and skip a step whose gradients are not finite
 * (what GradScaler.step does in the reference's MixedPrecisionStep, torch_src/session/procedures/step.py:55-78).  The step count lives
 * in guard->state and `step` must be 0.  Three stream-ordered launches, nothing is read back:
 *   1. partials[w] = sum over workgroup w's elements of ((double)grad_scale * grads[i])^2, float64, plain stores.  Elements are
 *      assigned to threads and workgroups by index alone and every sum has a fixed order: the same buffer gives the same bits on
 *      every call.  n_partials must be fgcn_grad_norm_tiles(n) (>= 1, monotone in n, at most FGCN_GRAD_NORM_MAX_TILES).  The square of
 *      a float32 fits a float64 exactly, so no finite input overflows the sum (1e30 per element has a finite norm here).
 *   2. one workgroup adds the partials in index order and writes the decision into `state`, one decision and one count for all groups:
 *        norm  = sqrt(sum)                                                                   (float64)
 *        coef  = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1       (clip_grad_norm_'s formula in float64; NaN propagates)
 *        apply = isfinite(norm) || !skip_nonfinite
 *      apply:  ++STEP; ++CLIPPED when coef < 1; SGD's first step is STEP == 1; Adam / AdamW: group_sched[2g], [2g + 1] =
 *              lr_g / (1 - beta1_g^STEP), sqrt(1 - beta2_g^STEP) in float64 from the NEW device-side step count (what the plain
 *              update computes on the host); ASGD: see below.
 *      !apply: ++SKIPPED; STEP, CLIPPED and group_sched keep their values.  NORM, COEF and APPLY are written on every call.
 *   3. the update with g = (float)(grad_scale * coef) * grads -- scaled before weight decay is added, which is where clip_grad_norm_
 *      sits relative to optimizer.step() -- and the step's scalars taken from `state` and `group_sched`; it stores nothing when APPLY
 *      is 0: params, state1 and state2 keep their bits.
 * state: fgcn_optim_guard_bytes() bytes, 8-byte aligned, FGCN_GUARD_WORDS words of 8 bytes indexed by the enum below; the caller
 * zeroes it to reset (STEP = 0: the next applied step is the first).  group_sched: 2 (ASGD: 4) * FGCN_OPT_MAX_GROUPS doubles, 8-byte
 * aligned.  All of it is caller-owned device memory; the library allocates nothing and keeps no state.
 *
 * ASGD's scalars.  eta and mu are float32 STATE of a parameter group, not functions of the current lr: torch computes them after a
 * step, from that step's lr, and uses them in the next one (an LR scheduler shows up one step late in eta):
 *   first step: eta = (float)lr, mu = 1;
 *   after the step that made the count STEP:  eta = (float)(lr / pow(1 + lambd*lr*STEP, alpha)),  mu = (float)(1 / max(1, STEP - t0)),
 *   both in double arithmetic.
 * The fields beta1, beta2, eps of fgcn_optim_group carry lambd, alpha, t0.  Without a guard momentum, dampening carry the CURRENT
 * eta, mu; the caller owns that state and computes the next values after the call (lr and `step` are not used by the update itself).
 * With a guard eta / mu live in group_sched, {eta_use, mu_use, eta_next, mu_next} per group.  The caller initialises eta_next = lr_g,
 * mu_next = 1 once (zeroing is NOT a reset for this kind).  Launch 2, when the step applies, copies next -> use and then computes the
 * new next from the new STEP and the group's current lr; launch 3 reads use; the momentum / dampening fields are ignored.
 *
 * FGCN_E_BADARG: a null or empty buffer, n / 4 >= 2^31, an unknown kind, step < 1 without a guard or != 0 with one, ngroups outside
 * [1, FGCN_OPT_MAX_GROUPS], a null groups / tiles, ntiles < 1, a missing state buffer (ASGD: also a non-null state2), a group's lr /
 * weight_decay / betas / eps / momentum out of range, Nesterov without momentum or with dampening, ASGD's lambd < 0, alpha or t0 not
 * finite and without a guard an eta < 0 or a mu outside (0, 1] (the message names the group); a null partials / state / group_sched,
 * a wrong n_partials, max_norm negative or NaN (0 switches clipping off).  FGCN_E_ALIGN: buffers not 16-byte aligned or n % 4 != 0,
 * tiles not 4-byte, partials / state / group_sched not 8-byte aligned.  Every check precedes the first launch. */
#define FGCN_OPT_SGD 0
#define FGCN_OPT_ADAM 1
#define FGCN_OPT_ADAMW 2
#define FGCN_OPT_ASGD 3
#define FGCN_OPT_MAX_GROUPS 8
#define FGCN_OPT_TILE4 1024
#define FGCN_GRAD_NORM_MAX_TILES 512
typedef struct fgcn_optim_group {
    float lr, weight_decay;
    float beta1, beta2, eps;       /* Adam / AdamW; ASGD: lambd, alpha, t0 */
    float momentum, dampening;     /* SGD; ASGD (no guard): the step's eta, mu */
    int nesterov;
} fgcn_optim_group;
enum fgcn_guard_word {
    FGCN_GUARD_STEP = 0,       /* int64: updates applied */
    FGCN_GUARD_SKIPPED = 1,    /* int64: calls that applied nothing (norm not finite, skip_nonfinite set) */
    FGCN_GUARD_CLIPPED = 2,    /* int64: applied updates with coef < 1 */
    FGCN_GUARD_NORM = 3,       /* float64: the last call's norm of grad_scale * grads */
    FGCN_GUARD_COEF = 4,       /* float64: the last call's clip coefficient */
    FGCN_GUARD_APPLY = 5,      /* int64 0 / 1: the last call's decision -- this and the next one are what launch 3 reads */
    FGCN_GUARD_FIRST_STEP = 6, /* int64 0 / 1: STEP == 1 (SGD: the momentum buffer starts as the gradient) */
    FGCN_GUARD_WORDS = 7
};
typedef struct fgcn_optim_guard {   /* NULL in the call: the plain update */
    double max_norm;                /* 0: no clipping */
    int skip_nonfinite, n_partials; /* n_partials == fgcn_grad_norm_tiles(n) */
    double* partials;
    void* state;                    /* fgcn_optim_guard_bytes() bytes, the words of enum fgcn_guard_word */
    double* group_sched;            /* 2 (Adam/AdamW) or 4 (ASGD) doubles per group, FGCN_OPT_MAX_GROUPS groups */
} fgcn_optim_guard;
int fgcn_grad_norm_tiles(long long n);      /* partial sums launch 1 writes for a buffer of n floats */
long long fgcn_optim_guard_bytes(void);
int fgcn_optim_step(float* params, const float* grads, float* state1, float* state2, long long n, int kind,
                    const fgcn_optim_group* groups, int ngroups, const int* tiles, int ntiles, float grad_scale,
                    long long step, const fgcn_optim_guard* guard, void* stream);

/* ---- MS-G3D data movement ------------------------------------------------------------------
 * (3 x 1) temporal max pooling with padding 1 and stride `stride` (nn.MaxPool2d((3,1), (stride,1), (1,0)) of
 * MultiScale_TemporalConv's pooling branch, models/msg3d/ms_tcn.py:72-78):
 *   out[(b, to, v), c] = max_j in[(b, to*stride + j - 1, v), c], j = 0..2 inside [0, T_in); idx = the winning tap (first maximum,
 *   as torch keeps it).  `in` may be a channel window of a wider tensor (row stride ld_in); out / idx / dout are contiguous
 *   (B, T_out, V, C), T_out = (T_in - 1) / stride + 1.  The backward is a gather: din[(b, ti, v), c] (+)= the dout of every
 *   window that holds ti and whose winning tap is ti. */
int fgcn_tmaxpool3_fwd(const float* in, float* out, unsigned char* idx, int B, int T_in, int T_out, int V, int C, int ld_in,
                       int stride, void* stream);
int fgcn_tmaxpool3_bwd(const float* dout, const unsigned char* idx, float* din, int B, int T_in, int T_out, int V, int C,
                       int ld_in, int stride, int accumulate, void* stream);

/* Temporal-window unfold (UnfoldTemporalWindows.forward, models/msg3d/ms_gtcn.py:37-45): the `window` frames around every
 * stride-th frame become `window * V` nodes of one spatial-temporal graph,
 *   out[(b, to, j*V + v), c] = x[(b, to*stride + j*dilation - pad, v), c]   (zeros outside [0, T)),
 *   pad = (window + (window-1)*(dilation-1) - 1) / 2,  T_out = (T + 2 pad - dilation (window-1) - 1) / stride + 1.
 * backward != 0: `in` is d(out) (B, T_out, window*V, C) and `out` receives dx (B, T, V, C) (a gather over the windows). */
int fgcn_unfold_windows(const float* in, float* out, int B, int T, int T_out, int V, int C, int window, int stride,
                        int dilation, int backward, void* stream);

/* ---- 1x1 convolutions in the split-bf16 math modes: persistent row GEMM (fgcn_pw.hip) ---------------------------------------------
 * out[m][n] (+)= sum_k in[m][k] * W[k][n] + bias[n] over `rows` contiguous rows (row strides ld_in / ld_out): the theta|phi embedding,
 * dY.Wd, down and dEmb.W products of the block (agcn.py:71-73,77,104-111) where the row GEMM above has no temporal map.  w3 = the
 * fgcn_pack_split3 form of the (1, K, N) matrix; K % 32 == 0, N % 4 == 0; stat_partials: float[fgcn_pw_gemm_tiles(rows)][2][N] or NULL
 * (sum and sum of squares of the values written, per 128-row tile).  A workgroup walks a list of (128 rows x 64 | 128 columns) tiles
 * and requests the next chunk's -- or the next tile's -- rows before the current MFMAs: the tiles of a 1x1 convolution are too short
 * (K = 64..384) to hide their own staging latency and store tail.  fgcn_pw_gemm_available() = 1 in FGCN_MATH_BF16X3 / FGCN_MATH_BF16. */
int fgcn_pw_gemm_available(void);
int fgcn_pw_gemm_tiles(long long rows);
int fgcn_pw_gemm(const void* in, void* out, const void* w3, int w_form, const float* bias, float* stat_partials, long long rows,
                 int K, int N, int ld_in, int ld_out, int accumulate, unsigned* in_amax, int half_mask, void* stream);
/* (w_form: FGCN_PACK_SPLIT3, or in FGCN_MATH_BF16X3 FGCN_PACK_SPLIT2H -- "Product form" above; in_amax as for fgcn_tconv_halo) */

/* ---- the two ends of the step: input BatchNorm and loss (fgcn_head.hip) ------------------------------------------------------
 * `data_bn` = nn.BatchNorm1d(M*V*C) over the network input x (N, M, T, V, C) viewed as (N, M*V*C, T)
 * (torch_src/models/mmargcn/agcn.py:150,186-188; msg3d.py:93,152-154): channel ch = (m*V + v)*C + c, statistics over (n, t).
 *   stats:      partials float[fgcn_data_bn_tiles(N, T)][2][M*V*C] (sum x, sum x^2 per tile) -> fgcn_bn_finalize(count = N*T)
 *               gives vec float[4][M*V*C] and updates the running statistics.  centered != 0 (what block.data_bn runs): partials
 *               float[tiles][4][M*V*C], rows 2 and 3 = the sums of x - p and (x - p)^2 about the channel's pivot
 *               p[ch] = x[0][m][0][v][c], a sample of the channel -- raw sensor units enter here, and sums about a sample carry
 *               the channel's spread, not its offset -> fgcn_bn_finalize(count = N*T, pivot = x, pivot_inner = V*C,
 *               pivot_outer = T*V*C);
 *   apply:      out (N*M, T, V, Cp) = x * scale[ch] + shift[ch], channels [C, Cp) zero -- the blocks' input layout, written directly;
 *   bwd_reduce: partials float[tiles][2][M*V*C] = (sum dout, sum dout * xhat) -> fgcn_reduce_sum -> (d beta, d gamma);
 *   bwd_apply:  dx (N, M, T, V, C) = scale * (dout - sum0/m - xhat * sum1/m), m = N*T (train) | scale * dout (eval). */
int fgcn_data_bn_tiles(int N, int T);
int fgcn_data_bn_stats(const float* x, float* partials, int N, int M, int T, int V, int C, int centered, void* stream);
int fgcn_data_bn_apply(const float* x, const float* vec, float* out, int N, int M, int T, int V, int C, int Cp, void* stream);
int fgcn_data_bn_bwd_reduce(const float* dout, const float* x, const float* vec, float* partials, int N, int M, int T, int V,
                            int C, int Cp, void* stream);
int fgcn_data_bn_bwd_apply(const float* dout, const float* x, const float* vec, const float* sums, float* dx, int N, int M, int T,
                           int V, int C, int Cp, int train, void* stream);
/* ---- the input stage of the RGB patch-feature modes (fgcn_patch.hip) --------------------------------------------------------------
 * Replaces, in front of data_bn, the reducer / zero-pad / fusion of reference torch_src/models/mmargcn/early_fusion_models.py:48-90
 * (SkeletonRgbPatchFeaturesEarlyFusion: `patch_feature_dim_reducer` = nn.Sequential(nn.Linear(P, H), nn.Linear(H, Q)), no activation,
 * then Fusion.combine(skeleton, rgb)) and :163-210 (SkeletonImuRgbPatchFeaturesEarlyFusion: the same, with the reduced rows zero-padded
 * from Vp patch joints to the V joints of the skeleton + IMU graph AFTER the reducer, so the IMU joints get 0, not b2).
 *   s  (N, M, T, V, Cs) skeleton rows, or NULL with Cs = 0 (concatenate only);  p (N, M, T, Vp, P) patch rows, Vp <= V;
 *   w1 (H, P), b1 (H), w2 (Q, H), b2 (Q): the two nn.Linear in their own layout, or w1 = b1 = w2 = b2 = NULL: the identity (Q = P);
 *   fusion: 0 concatenate z = [s | q] (C = Cs + Q), 1 sum s + q, 2 product s * q, 3 average (s + q) / 2 (1..3: C = Cs = Q);
 *   z  (N, M, T, V, C): the fused network input, q = 0 for v >= Vp;  stat_partials (may be NULL): what
 *      fgcn_data_bn_stats(z, ..., stat_centered) writes, float[fgcn_data_bn_tiles(N, T)][2 or 4][M*V*C] (it is that kernel, run over z)
 *      -> fgcn_bn_finalize (stat_centered: with pivot = z) / fgcn_data_bn_apply unchanged.
 * The hidden (rows, H) tensor stays in registers.  Sizes with a reducer: P a multiple of 128 up to 1024, H a multiple of 32 up to 1024,
 * 1 <= Q <= 32; others are FGCN_E_BADARG.  Math mode: FGCN_MATH_BF16 rounds every operand to bfloat16 once; every other mode (and
 * product form) multiplies exact float32 operands on v_mfma_f32_32x32x2_f32.
 * bwd: dz (N, M, T, V, C) = data_bn's dx -> slab partials pw1 float[S][H][P], pb1 [S][H], pw2 [S][Q][H], pb2 [S][Q] of dW1, db1, dW2,
 *      db2, S = fgcn_patch_input_slabs(N, M, T, Vp, H); sum them with fgcn_reduce_multi (fixed order: bitwise reproducible).  h is
 *      recomputed from p; s is read for the product's derivative; s and p get no gradient (data).  Identity reducer: nothing to do. */
int fgcn_patch_input_slabs(int N, int M, int T, int Vp, int H);
int fgcn_patch_input_fwd(const float* s, const float* p, const float* w1, const float* b1, const float* w2, const float* b2, float* z,
                         float* stat_partials, int N, int M, int T, int V, int Vp, int Cs, int P, int H, int Q, int fusion,
                         int stat_centered, void* stream);
int fgcn_patch_input_bwd(const float* dz, const float* s, const float* p, const float* w1, const float* b1, const float* w2, float* pw1,
                         float* pb1, float* pw2, float* pb2, int N, int M, int T, int V, int Vp, int Cs, int P, int H, int Q, int fusion,
                         void* stream);
/* nn.CrossEntropyLoss() (mean reduction; session/session.py:53, procedures/step.py:38-46) over logits (rows, classes) with row
 * stride ld and int64 labels: probs float[rows][classes] = softmax (kept for the backward), row_loss float[rows], loss float[2] =
 * {mean over the rows whose label is not -100 (torch's ignore_index rows do not count), that row count}; any OTHER label outside
 * [0, classes) -- a device assert in torch -- makes the loss and, in the backward, its row's gradient NaN; one workgroup, fixed
 * summation order.  bwd: dlogits (rows, ld_out) = (probs - onehot) * dloss[0] / loss[1], columns [classes, ld_out) zero. */
int fgcn_cross_entropy_fwd(const float* logits, const long long* labels, float* probs, float* row_loss, float* loss, int rows,
                           int classes, int ld, void* stream);
int fgcn_cross_entropy_bwd(const float* probs, const long long* labels, const float* loss, const float* dloss, float* dlogits,
                           int rows, int classes, int ld_out, void* stream);
/* The same loss with torch.nn.CrossEntropyLoss's arguments (weight, ignore_index, reduction, label_smoothing, class-probability
 * targets); the two calls above are the path of the default arguments and are untouched.  DESIGN.md section 8d.
 *   logits (rows, classes) float32, row stride ld >= classes;  EXACTLY ONE of labels int64[rows] | target float32 (rows, classes)
 *   class probabilities with row stride ld_target >= classes (ld_target is not read with labels);  weight float32[classes] or NULL
 *   = all ones;  ignore_index applies to labels only (a value inside [0, classes) is legal);  label_smoothing eps in [0, 1].
 * Per row i, lp = log_softmax(z_i), C = classes:
 *   labels:  keep = (y != ignore_index);  row_loss = keep [(1 - eps) w[y] (-lp[y]) + eps/C sum_c w[c] (-lp[c])],
 *            row_scale = keep [(1 - eps) w[y] + eps/C sum_c w[c]],  denominator = sum_i keep w[y_i] (it does not depend on eps).
 *            A label outside [0, classes) that is not ignore_index: row_loss = row_scale = NaN (so are the mean and the sum, and
 *            that row's gradient); no address is ever formed from a label before it is range-checked.
 *   target:  t' = (1 - eps) t + eps/C;  row_loss = -sum_c w[c] t'[c] lp[c],  row_scale = sum_c w[c] t'[c],  denominator = rows.
 * fwd writes row_loss float[rows] (the result of FGCN_CE_NONE), row_scale float[rows] (for the backward), probs float[rows][classes]
 * = softmax (NULL when no backward follows) and loss float[2] = {value, denominator}: value = sum row_loss (FGCN_CE_SUM, FGCN_CE_NONE)
 * or that sum / denominator (FGCN_CE_MEAN; NaN for a zero denominator, as in torch: every row ignored, every present weight zero).
 * workspace: fgcn_ce_workspace_bytes(rows) bytes, 8-byte aligned, caller-owned (0 for rows <= 0): one float64 pair {sum row_loss,
 * sum denominator} per workgroup of 16 rows (one wave per row), added in index order in float64 by a second one-workgroup launch --
 * the order of the additions does not depend on the order the workgroups ran in: the same call leaves the same bits.
 * bwd: dlogits (rows, ld_out) = g_i (probs[i][c] row_scale[i] - a_ic), a_ic = keep w[c] q_ic (q: the smoothed one-hot | t'),
 *   g_i = dloss[0] / loss[1] (MEAN; NaN for a zero denominator, as torch's 0/0), dloss[0] (SUM), dloss[i] (NONE: dloss is float[rows]); an ignored row's gradient is exactly 0;
 *   columns [classes, ld_out) zero.  It takes the labels / target / weight / ignore_index / label_smoothing / reduction of its fwd.
 * FGCN_E_BADARG before any launch: a null required pointer (workspace included), both or neither of labels / target, rows <= 0,
 * classes <= 0, ld / ld_target / ld_out < classes, eps outside [0, 1] or NaN, an unknown reduction; FGCN_E_ALIGN: workspace. */
enum fgcn_ce_reduction { FGCN_CE_MEAN = 0, FGCN_CE_SUM = 1, FGCN_CE_NONE = 2 };
long long fgcn_ce_workspace_bytes(int rows);
int fgcn_ce_fwd(const float* logits, const long long* labels, const float* target, const float* weight, float* probs, float* row_loss,
                float* row_scale, float* loss, void* workspace, int rows, int classes, int ld, int ld_target, long long ignore_index,
                float label_smoothing, int reduction, void* stream);
int fgcn_ce_bwd(const float* probs, const long long* labels, const float* target, const float* weight, const float* row_scale,
                const float* loss, const float* dloss, float* dlogits, int rows, int classes, int ld_target, int ld_out,
                long long ignore_index, float label_smoothing, int reduction, void* stream);

/* Classification metrics accumulated on the device (metrics.py; reference torch_src/metrics.py Mean / MultiClassAccuracy /
 * TopKAccuracy / ConfusionMatrix / MisclassifiedSamplesList): ONE launch per batch adds everything those classes derive their values
 * from to a caller-owned state buffer; the host reads it when it wants a value, not once per batch.
 *
 * state (8-byte aligned, fgcn_classify_state_bytes(classes) bytes; the caller zeroes it to reset; the library allocates nothing
 * and keeps no state):
 *     bytes [0, 64)                    FGCN_CLS_WORDS = 8 words of 8 bytes, indexed by the enum below: int64 counters, except
 *                                      word FGCN_CLS_LOSS_SUM, which is one float64
 *     bytes [64, 64 + 4*classes^2)     int32 confusion[classes][classes], row = label, column = prediction
 *     (+ 4 bytes of padding when classes is odd: the size is a multiple of 8)
 *
 * Per row r < rows of logits (float32, row stride ld >= classes) with label y = labels[r] (int64).  Logits compare in torch's
 * order: NaN is greater than every number and equal to NaN; for rows without NaN that is plain > and ==.
 *     pred    = the FIRST index of the row's maximum (torch.argmax; a NaN is the maximum).
 *     rank(y) = #{j : logit_j > logit_y} + #{j < y : logit_j == logit_y}; the row is a top-k hit when rank(y) < k.  torch.topk
 *               leaves the order of equal logits unspecified; this rule resolves ties towards the lower class index and makes a
 *               top-1 hit the same thing as pred == y.
 *     y == -100 (torch's ignore_index, as in fgcn_cross_entropy_fwd): ++IGNORED, nothing else.
 *     any other y outside [0, classes): ++INVALID, nothing else; no address is ever formed from such a label.
 *     otherwise: ++EXAMPLES, ++TOP1 if pred == y, ++TOPK on a hit, ++confusion[y][pred].
 *     pred_out (may be NULL; int32[pred_capacity]): pred_out[pred_offset + r] = pred, or -1 for an ignored / invalid row, when
 *               pred_offset + r < pred_capacity; a row past the capacity is not stored and counted in DROPPED.
 * loss (may be NULL; device pointer to ONE float32, the step's loss): LOSS_SUM += (double)loss[0] * rows, LOSS_ITEMS += rows, by a
 * single thread -- the reference's Mean.update(loss, num_items=len(label)), gradient-accumulation quotient included.
 * Integer sums are exact in any order and the loss term is one addition per call: the same calls leave bit-identical state.
 * FGCN_E_BADARG: a null logits / labels / state, rows <= 0, classes outside [1, FGCN_CLS_MAX_CLASSES], ld < classes, k outside
 * [1, classes] (torch.topk raises there too), a negative pred_offset or pred_capacity; FGCN_E_ALIGN: state not 8-byte aligned. */
enum fgcn_cls_word {
    FGCN_CLS_EXAMPLES = 0,   /* rows with a label in [0, classes) */
    FGCN_CLS_TOP1 = 1,       /* of those, pred == label */
    FGCN_CLS_TOPK = 2,       /* of those, rank(label) < k */
    FGCN_CLS_IGNORED = 3,    /* rows labelled -100 */
    FGCN_CLS_INVALID = 4,    /* rows with any other label outside [0, classes) */
    FGCN_CLS_DROPPED = 5,    /* rows whose prediction did not fit into pred_out */
    FGCN_CLS_LOSS_ITEMS = 6, /* sum of `rows` over the calls that passed a loss */
    FGCN_CLS_LOSS_SUM = 7,   /* float64: sum of loss[0] * rows over those calls */
    FGCN_CLS_WORDS = 8
};
#define FGCN_CLS_MAX_CLASSES 1024
long long fgcn_classify_state_bytes(int classes);   /* 0 for classes outside [1, FGCN_CLS_MAX_CLASSES] */
int fgcn_classify_update(const float* logits, const long long* labels, const float* loss, void* state, int* pred_out,
                         long long pred_offset, long long pred_capacity, int rows, int classes, int ld, int k, void* stream);

/* Dropout with masks from a counter-based generator (fops.dropout / FusedDropout: the IMU graph convolution's and the MS-G3D MLP's
 * `dropout=`).  The masks are a pure function of (seed, site, *step, element index): a test recomputes them on
 * the host bit for bit, two runs from one state draw the same masks, and a recorded HIP graph draws new ones on every replay
 * without the host, because the step counter is a word in device memory.
 *
 * Philox4x32-10 (Salmon et al., SC'11): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten
 * rounds; one round maps (c0, c1, c2, c3), (k0, k1) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) and the key
 * is bumped after each round.  fgcn_philox4x32_10 is the HOST copy of the function the kernel calls (no device is touched);
 * ctr = key = 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  FGCN_E_BADARG: a null pointer.
 *
 * fgcn_dropout_fwd, float32 x -> y, n elements: element i belongs to group g = i >> 2 and uses word i & 3 of
 *     philox(ctr = {(unsigned)g, site, lo32(*step), hi32(*step)}, key = {lo32(seed), hi32(seed)});
 * it is kept iff word >= thr, thr = (unsigned)((double)p * 4294967296.0); y[i] = kept ? x[i] * s : 0.0f with
 * s = 1.0f / (1.0f - p) formed in float32 on the host.  keep_mask (ceil(n / 8) bytes) receives bit i & 7 of byte i >> 3 = kept,
 * unused tail bits zero: the bit layout of fgcn_bn_act's sign image.  `step` is a device pointer to one 8-byte word that the call
 * reads and does not change.  FGCN_E_BADARG before any launch: n <= 0, n % 4 != 0, n >= 2^34, p < 0, p >= 1 or not finite, a null
 * pointer, x / y not 16-byte aligned (step: 8-byte).  Float32 storage only.
 *
 * fgcn_dropout_bwd: dx[i] = kept ? dy[i] * s : 0.0f from the bit image; dx == dy (in place) is allowed.  Same refusals.
 *
 * fgcn_rng_advance: *step += 1 by one lane, in a launch of its own: stream-ordered behind the forward that read the word, so no
 * workgroup of that forward sees the new value, and the pair captures into a HIP graph as a straight line. */
int fgcn_philox4x32_10(const unsigned ctr[4], const unsigned key[2], unsigned out[4]);
int fgcn_dropout_fwd(const float* x, float* y, unsigned char* keep_mask, long long n, float p, unsigned long long seed, unsigned site,
                     const unsigned long long* step, void* stream);
int fgcn_dropout_bwd(const float* dy, const unsigned char* keep_mask, float* dx, long long n, float p, void* stream);
int fgcn_rng_advance(unsigned long long* step, void* stream);

/* Augmentation of clips as the batch is gathered (data.ClipBatches(augment=...)).  Row k of `out` is source row
 * idx[k] of `src`, resampled in time and -- joints with three coordinates -- rotated and scaled, with random numbers that are a pure
 * function of (seed, site, epoch, sample_ids[k]): the same bits in any batch order, on any number of ranks, on the resident and the
 * streaming path, and in a second run.  A sample is (outer, T, inner) float32: a skeleton (M, T, V, C) is (M, T, V * C), an inertial
 * signal (T, S) is (1, T, S), patch features (M, T, V, F) are (M, T, V * F).
 *
 * Random words: two Philox blocks per sample, philox(ctr = {(unsigned)sample, site, epoch, j}, key = {lo32(seed), hi32(seed)}), j = 0, 1.
 * A word w gives the uniform u = (float)(w >> 8) * 2^-24, exact in float32, in [0, 1).  All arithmetic below is float32, every product
 * and sum rounded on its own unless an fma is named.
 *
 * Parameters (the table row of the sample, 12 floats): with u0..u3 the words of block 0 and u4, u5 words 0, 1 of block 1,
 *     theta_a = (2 u_a - 1) * max_angle[a], a = x, y, z (2u - 1 is exact);   s = 1 + (2 u3 - 1) * scale;
 *     A = s * Rz(theta_z) * Ry(theta_y) * Rx(theta_x), each entry formed as s * (the sum of its one or two products of sinf / cosf values);
 *     r = min_window + u4 * (1 - min_window);   o = u5 * (1 - r), formed as u5 * ((1 - u4) * (1 - min_window)) (1 - u4 is exact);
 *     row = {A row-major (9), o, r, 0}.
 * Zero angles and scale and min_window = 1 give exactly the identity matrix, o = 0 and r = 1.
 *
 * Temporal part, all of `inner`: v = valid[idx[k]] (valid == NULL: T; a value outside [1, T] is clamped into it), output frame t reads
 *     pos = (o + r * t / (T - 1)) * (v - 1), formed as fma(r * t, (v - 1) / (T - 1), o * (v - 1)) (the quotient counts as 0 for T == 1);
 *     f0 = floor(pos) clamped to [0, v - 1], f1 = min(f0 + 1, v - 1), w = pos - f0, y = fma(w, x[f1] - x[f0], x[f0]).
 * Spatial part, after the interpolation, joints [joint_lo, joint_hi) of a sample with C == 3 (inner = V * 3):
 *     y'_c = fma(A[c][2], y_2, fma(A[c][1], y_1, A[c][0] * y_0)).  No translation: a zero joint stays zero.
 * Identity: with zero angles and scale, min_window = 1 and valid == NULL (or T), pos == t and w == 0 exactly and `out` equals the gathered
 * rows (x[f0] + 0 * (x[f0] - x[f0]), then 1 * y_0 + 0 * y_1 + 0 * y_2).
 *
 * fgcn_clip_augment: src (rows, outer, T, inner), idx / sample_ids (b) 8-byte integers on the device (idx may repeat and need not be sorted;
 * every idx[k] must be a row of src -- the caller's duty; the streaming path passes idx = 0..b-1 and the real ids), valid NULL or 4-byte
 * integers indexed by SOURCE row, out (b, outer, T, inner), params (b, 12) receives the table.  Two launches: one lane per row forms the
 * table, then one lane per (row, outer, frame, joint) -- per element when no joint is rotated -- reads it back.  Rows need 4-byte alignment only.
 * FGCN_E_BADARG before any launch: a null pointer (valid excepted); b, outer, T or inner <= 0; C <= 0 or inner % C != 0; a joint range
 * outside 0 <= joint_lo <= joint_hi <= inner / C; joint_hi > joint_lo with C != 3; min_window outside (0, 1]; scale outside [0, 1); an
 * angle that is not finite; out == src.
 *
 * fgcn_augment_params: the HOST copy of the table row (no device is touched), computed by the function the kernel calls; the device's row
 * differs from it by the two sinf / cosf implementations alone.  The same refusals for its arguments. */
int fgcn_clip_augment(const float* src, const long long* idx, const long long* sample_ids, const int* valid, float* out, float* params, int b,
                      int outer, int T, int inner, int C, int joint_lo, int joint_hi, const float max_angle[3], float scale, float min_window,
                      unsigned long long seed, unsigned site, unsigned epoch, void* stream);
int fgcn_augment_params(unsigned sample, unsigned site, unsigned epoch, unsigned long long seed, const float max_angle[3], float scale,
                        float min_window, float out12[12]);

/* Normalisation of raw skeleton clips as the batch is gathered (data.ClipBatches(normalize=...)): the reference's
 * normalize_skeleton(skeleton, origin_joint, z_axis_joints, x_axis_joints) (util/preprocessing/skeleton.py) on source row idx[k].  A clip
 * is (M, T, V, C) float32, C = 2 or 3; the result is a pure function of the clip and the joint numbers.
 *
 * Definitions.  A frame of a body is NULL when all its V * C values are zero (-0 counts as zero, a NaN as a value); a body is INVALID when
 * all its frames are null; a joint of a frame is MISSING when its C values are zero.  (The reference tests sum() == 0 instead: the two
 * differ only where non-zero values cancel exactly, and there this definition is the one that holds.)
 *
 * Stage 1, the frame map of every body (pad_null_frames): output frame t is source frame map[t].  If frame 0 is null, base = the non-null
 * frames in order and f = their number; otherwise f = the last non-null frame + 1 and base = 0 .. f-1 (null frames inside [0, f) stay).
 * map[t] = base[t] for t < f, base[(t - f) mod f] for t >= f.  An invalid body has the identity map and comes out as zeros.
 * Stage 2 (move_skeleton_origin): centre[t] = joint `origin` of body 0 at ITS mapped frame t (zero when body 0 is invalid or the joint
 * is missing there); every joint becomes x - centre[t], a missing joint stays zero.
 * Stage 3 (parallelize_joints_to_axis, twice; C == 3): the pass for the pair (j0, j1) and a unit axis takes bone = p[j1] - p[j0] from body
 * 0, output frame 0, of the clip as it stands -- after stage 2 for the z pass (z0, z1) -> (0, 0, 1), after the z pass for the x pass
 * (x0, x1) -> (1, 0, 0).  The pass is skipped if sum|bone| < 1e-6; with k = bone x axis and theta = acos(bone . axis / |bone|) it is
 * skipped if sum|k| < 1e-6 or |theta| < 1e-6 (so a bone antiparallel to the axis is left alone, as in the reference); otherwise every
 * joint is multiplied by the Rodrigues matrix I + sin(theta) K + (1 - cos(theta)) K^2 of k / |k|.  The argument of acos is clamped to
 * [-1, 1]: the reference would return NaN where a rounding takes it outside.
 * Arithmetic: float64 from the float32 input throughout -- the centred coordinates, both matrices, their product R = R_x R_z, and
 * R (x - centre) -- and ONE rounding to float32 at the store.  With no rotation applied the stored value is float32(x - centre).
 *
 * fgcn_clip_normalize: src (rows, M, T, V, C), idx (b) 8-byte integers on the device (they may repeat and need not be sorted; every idx[k]
 * must be a row of src -- the caller's duty), out (b, M, T, V, C), frame_map (b, M, T) 4-byte integers and params (b, 12) float64 receive
 * the tables: params[0..8] = R row-major, [9] = 1.0 if the z rotation was applied, [10] the same for x, [11] the number of valid bodies.
 * z0 < 0: no z pair; x0 < 0: no x pair.  Two launches: one workgroup per clip forms its tables, then one lane per (clip, body, frame,
 * joint) gathers through them (a frame number read back is clamped into [0, T)).  Rows need 4-byte alignment only.
 * FGCN_E_BADARG before any launch: a null pointer; b, M, T or V <= 0; V > 64; C not 2 or 3; T > FGCN_NORMALIZE_MAX_T; origin outside
 * [0, V); a pair whose joints are outside [0, V) or equal; a pair with C != 3; out == src (the gather reads other frames); b * M >= 2^31
 * (one grid does not hold more bodies). */
#define FGCN_NORMALIZE_MAX_T 4096
int fgcn_clip_normalize(const float* src, const long long* idx, float* out, int* frame_map, double* params, int b, int M, int T, int V, int C,
                        int origin, int z0, int z1, int x0, int x1, void* stream);

/* Selection of a clip's most energetic bodies as the batch is gathered (data.ClipBatches(bodies=...)): the
 * reference's SkeletonSample._filter_bodies (datasets/ntu_rgb_d/io.py) with body_score (util/preprocessing/skeleton.py) on source row
 * idx[k].  It runs in FRONT of fgcn_clip_normalize, which centres and rotates the clip by body 0: this stage decides what body 0 is.  A
 * clip is (Mr, T, V, C) float32, C = 2 or 3; the stage keeps M bodies, 1 <= M <= Mr <= FGCN_BODIES_MAX.
 *
 * Null frames.  A frame of a body is NULL when all its V * C values are zero (-0 counts as zero, a NaN as a value): fgcn_clip_normalize's
 * definition.  (The reference tests sum() != 0 instead: the two differ only where non-zero values cancel exactly, and there this
 * definition is the one that holds.)
 * Score.  Let F be the body's non-null frames and n = |F| * V.  n == 0: the score is +0.  Otherwise it is the sum over the channels c of
 * sqrt(sum_{t in F, v} (x[t, v, c] - mean_c)^2 / n) with mean_c = sum_{t in F, v} x[t, v, c] / n: the population standard deviation
 * (numpy's std()), two passes, the mean first and then the squared deviations.  Arithmetic: float64 from the float32 input throughout.  The
 * order of every sum is fixed and depends on (T, V, C) alone -- not on b, on the clip's place in the batch, on its address or on the number
 * of workgroups -- and there are no floating-point atomics: a clip's score has the same bits alone and in any batch, in a second call, on
 * the resident path and on the streaming path.  A body that holds a NaN or an inf has a NaN score.
 * Ranking.  Descending score; a NaN ranks above every number (where numpy's argsort()[::-1] puts it; a NaN stays visible, DESIGN.md
 * section 8l); equal scores, several NaNs included: the HIGHER source index first (what numpy's stable sort, reversed, gives for these sizes
 * -- but the rule is this contract's, not numpy's).
 * Output.  out[k, j] = src[idx[k], order[k, j]] for j < M: a copy, every value bit for bit.
 *
 * fgcn_clip_bodies: src (rows, Mr, T, V, C), idx (b) 8-byte integers on the device (they may repeat and need not be sorted; every idx[k]
 * must be a row of src -- the caller's duty), out (b, M, T, V, C), order (b, Mr) 4-byte integers, the complete ranking (order[k, 0] is the
 * source body with the highest score), scores (b, Mr) float64 indexed by SOURCE body.  M == Mr gives a pure reordering.  Two launches:
 * one workgroup per (clip, body) scores it, then the workgroups of the gather rank the clip's scores by counting and copy.  No host read
 * and no synchronising call.  Rows need 4-byte alignment only.
 * FGCN_E_BADARG before any launch: a null pointer; b, Mr, M, T or V <= 0; M > Mr; Mr > FGCN_BODIES_MAX; C not 2 or 3; T * V * C >= 2^29 (a
 * lane's index inside a body); T > FGCN_BODIES_MAX_T (the frame flags of a body stay in LDS, one bit a frame); b * Mr >= 2^31 (one grid
 * does not hold more bodies); out == src. */
#define FGCN_BODIES_MAX 16
#define FGCN_BODIES_MAX_T 524288
int fgcn_clip_bodies(const float* src, const long long* idx, float* out, int* order, double* scores, int b, int Mr, int M, int T, int V, int C,
                     void* stream);

/* Preparation of raw inertial recordings as the batch is gathered (data.ClipBatches(inertial=...)): what the
 * reference's offline preprocessing does to the accelerometer / gyroscope recording of a sample.  The recording has Li frames of S values
 * (stored in a row of L >= Li frames), the sample's skeleton recording has Ls frames, a clip has T >= Ls frames.
 *
 * Step 1, resample (NearestNeighborInterpolator, util/preprocessing/interpolator.py): frame t of the result, 0 <= t < Ls, is frame
 *     r(t) = t                                          where Li == Ls (the reference takes the recording as it is),
 *     r(t) = rint(t * ((Li - 1) / (Ls - 1)))            otherwise: the quotient first, then the product, both float64, ties to even
 * of the recording; r = 0 where Ls == 1; r is clamped into [0, Li - 1].  Step 2, pad (pad_sequence_numpy): frames Ls .. T-1 are zero.
 * Step 3a, the signal (InertialProcessor, normalize_signal): over the WHOLE padded (T, S) array -- the padding zeros take part --
 *     mn = min x, mx = fl32(max x - mn), y = fl32(fl32(x - mn) / mx), all float32, the division correctly rounded.
 * A constant array gives 0 / 0 = NaN, as in the reference; a NaN in the array makes mn, mx and every y NaN, as numpy's min and max do.
 * Step 3b, the enhanced skeleton (SkeletonProcessor("imu_enhanced")): (M, T, V + S / 3, 3); joints 0 .. V-1 of every body are the
 * skeleton's (a third coordinate of zero where it has two), joint V + j of EVERY body holds values 3j .. 3j+2 of the padded array of
 * step 2 -- not min-max normalised, and zero from frame Ls on, whatever the skeleton's normalisation repeated into those frames.
 *
 * fgcn_resample_index: r(t) on the HOST (no device is touched), by the function both kernels call.  FGCN_E_BADARG: out == NULL or a length <= 0.
 *
 * fgcn_signal_prepare: steps 1, 2, 3a.  src (rows, L, S), idx (b) 8-byte integers on the device (they may repeat and need not be sorted;
 * every idx[k] must be a row of src -- the caller's duty), src_len / dst_len 4-byte integers on the device indexed by SOURCE row (Li and
 * Ls; a value outside [1, L] / [1, T] is clamped into it), out (b, T, S), stats (b, 2) receives mn, mx.  minmax == 0: steps 1 and 2
 * alone, and stats receives 0, 1.  One launch, one workgroup per clip: minimum and maximum (order-independent, so two calls give the same
 * bits), then the values.
 * fgcn_imu_enhance: steps 1, 2, 3b.  skel (rows_s, M, T, V, C) with skel_idx (b), imu (rows_i, L, S) with imu_idx (b), src_len / dst_len
 * indexed by the row of IMU, out (b, M, T, V + S / 3, 3).  One launch, one lane per output joint.  skel may be what fgcn_clip_normalize wrote.
 * Both: rows need 4-byte alignment only.  FGCN_E_BADARG before any launch: a null pointer; a size <= 0; C not 2 or 3 and S % 3 != 0
 * (enhance); out == an input; 2^31 or more elements in out, in a clip or in a recording. */
int fgcn_resample_index(int t, int src_len, int dst_len, int* out);
int fgcn_signal_prepare(const float* src, const long long* idx, const int* src_len, const int* dst_len, float* out, float* stats, int b, int L,
                        int S, int T, int minmax, void* stream);
int fgcn_imu_enhance(const float* skel, const long long* skel_idx, const float* imu, const long long* imu_idx, const int* src_len,
                     const int* dst_len, float* out, int b, int M, int T, int V, int C, int L, int S, void* stream);

/* The input streams of the two-stream AGCN family, derived as the batch is gathered (data.ClipBatches(streams=...); DESIGN.md section
 * 8j).  A clip x is (M, T, V, C) float32, C = 2 or 3; every body and coordinate is treated alike, [t, v] below names the C values of
 * joint v in frame t.  parents[v] = p is the joint's parent; L is the valid frame count of the clip (T without a table).  Every value is
 * ONE correctly rounded float32 subtraction, a copy or a zero -- there is no product and no fused operation, so a numpy float32
 * restatement gives the same bits.
 *
 *     joint[t, v]       = x[t, v]
 *     bone[t, v]        = x[t, v] - x[t, p]                 p == v (the root, as in 2s-AGCN): x - x, exactly +0 for a finite x;
 *                       = x[t, v]                           p == -1: copied through (the sensor joints that imu_enhance appends hold
 *                                                           sensor axes, not positions)
 *     motion[t, v]      = x[t+1, v] - x[t, v]               for t < L - 1;   +0 for t >= L - 1
 *     bone_motion[t, v] = bone[t+1, v] - bone[t, v]         for t < L - 1;   +0 for t >= L - 1.  Both bones are rounded to float32 first;
 *                                                           for p == -1 it equals motion.
 * bone and joint know nothing of L: they cover all T frames.  motion and bone_motion read frame t+1 only when t+1 < L: neither frame T nor
 * any frame at or behind L is ever read for one of their values (the lanes of frames L-1 .. T-1 read frame L-1 and store the zero).
 *
 * fgcn_clip_streams: src (rows, M, T, V, C), idx (b) 8-byte integers on the device (they may repeat and need not be sorted; every idx[k]
 * must be a row of src -- the caller's duty; the streaming path passes idx = 0..b-1), parents (V) 4-byte integers on the device (a value
 * outside [-1, V) is clamped into it, so that none becomes an address: the host layer checks them once, when it builds the table), valid
 * NULL or 4-byte integers on the device indexed by SOURCE row idx[k] (a value outside [1, T] is clamped into it).  joint, bone, motion,
 * bone_motion: (b, M, T, V, C) each, or NULL = that stream is not wanted; at least one of bone, motion, bone_motion.  One launch, one lane
 * per (row, body, frame, joint); which outputs exist is uniform over the launch; no atomics; two calls give the same bits.  Rows need
 * 4-byte alignment only.
 * FGCN_E_BADARG before any launch: src, idx or parents NULL; no derived output; b, M, T or V <= 0; C not 2 or 3; an output == src; more
 * lanes than one grid holds (b * M * T * V > (2^31 - 1) * 256). */
int fgcn_clip_streams(const float* src, const long long* idx, const int* parents, const int* valid, float* joint, float* bone, float* motion,
                      float* bone_motion, int b, int M, int T, int V, int C, void* stream);

/* A clip cropped to a part of its valid frames and resized to a window of W frames as the batch is gathered (data.ClipBatches(window=...);
 * DESIGN.md section 8n): the recipe of the two-stream AGCN family's successors -- a random part when training, the centred one when
 * evaluating, and a model built for W frames instead of the stored T.  fgcn_clip_augment's conventions: a sample is (outer, T, inner)
 * float32, row k of `out` is made of source row idx[k], the random numbers are a pure function of (seed, site, epoch, sample_ids[k]), a word
 * w gives the uniform u = (float)(w >> 8) * 2^-24, all arithmetic is float32 with every product and sum rounded on its own unless an fma
 * is named.
 *
 * Parameters (the table row of the sample, 2 floats {o, r}: the part [o, o + r] of the recording, as fractions of it), with
 * interval = (lo, hi), 0 < lo <= hi <= 1:
 *     FGCN_WINDOW_RANDOM:  u0, u1 = words 0, 1 of ONE Philox block, philox(ctr = {(unsigned)sample, site, epoch, 2}, key = {lo32(seed),
 *                          hi32(seed)}) -- fgcn_clip_augment uses counter words 0 and 1 at the same (seed, site), so the crop is
 *                          independent of the rotation without a second site;
 *                          r = min(lo + u0 * (hi - lo), hi);   o = min(u1 * (1 - r), 1 - r), the first 1 - r formed as
 *                          (1 - hi) + (1 - u0) * (hi - lo) (1 - u0 is exact and no term is negative; exactly 0 for lo = hi = 1), the
 *                          second as the one subtraction.  The two min() act on the last rounding alone: lo <= r <= hi and o + r <= 1
 *                          (to the rounding of that sum) hold for every draw.
 *     FGCN_WINDOW_CENTRE:  r = hi;   o = (1 - r) * 0.5.  No random numbers: seed, site, epoch and sample_ids are ignored.
 * interval = (1, 1) gives exactly o = 0 and r = 1 in both modes.
 *
 * Output frame t, 0 <= t < W, all of `inner`: v = valid[idx[k]] (valid == NULL: T; a value outside [1, T] is clamped into it),
 *     pos = (o + r * t / (W - 1)) * (v - 1), formed as fma(r * t, (v - 1) / (W - 1), o * (v - 1)) (the quotient counts as 0 for W == 1);
 *     f0 = floor(pos) clamped to [0, v - 1], f1 = min(f0 + 1, v - 1), w = pos - f0, y = fma(w, x[f1] - x[f0], x[f0]).
 * No frame at or behind v, and so no frame T behind a row, is ever read.  W may be smaller than, equal to or larger than T.
 * Identity: with W == T, interval = (1, 1) and valid == NULL (or T), in either mode, pos == t and w == 0 exactly and `out` equals the
 * gathered rows bit for bit.
 * Non-finite inputs: rule 3 of "Non-finite values in the inputs" above -- an output that reads a non-finite value (x[f0] or x[f1], whatever
 * w is: 0 * inf and inf - inf are NaN) is non-finite, NaN against +-inf need not match; an output that reads none is what it is on finite data.
 *
 * fgcn_clip_window: src (rows, outer, T, inner), idx / sample_ids (b) 8-byte integers on the device (idx may repeat and need not be sorted;
 * every idx[k] must be a row of src -- the caller's duty; the streaming path passes idx = 0..b-1 and the real ids), valid NULL or 4-byte
 * integers indexed by SOURCE row, out (b, outer, W, inner), params (b, 2) receives the table.  Two launches: one lane per row forms the
 * table, then one lane per output element reads it back.  Rows need 4-byte alignment only.
 * FGCN_E_BADARG before any launch: a null pointer (valid excepted, and sample_ids in mode CENTRE); b, outer, T, W or inner <= 0; an
 * interval outside 0 < lo <= hi <= 1 or not finite; an unknown mode; out == src; W * inner >= 2^29 (a lane's index inside a body) or more
 * workgroups than one grid holds.
 *
 * fgcn_window_params: the HOST copy of the table row (no device is touched), computed by the function the kernel calls: there is no
 * transcendental function and contraction is off, so the device's row has the same bits.  The same refusals for its arguments.
 *
 * fgcn_clip_valid_frames: out[k] (4-byte integers on the device) = 1 + the largest t for which frame t of ANY of the `outer` bodies of
 * source row idx[k] is not null, under fgcn_clip_normalize's definition: a frame of a body is null when all its `inner` values are zero
 * (-0 counts as zero, a NaN as a value).  A null frame in front of a later frame that holds a value does not end the clip; a clip
 * without a value gives 1, so the table lies in [1, T] and is what `valid` above, fgcn_clip_augment and fgcn_clip_streams take.  One
 * launch, one workgroup per row, no atomics; 4-byte loads.  FGCN_E_BADARG before any launch: a null pointer; b, outer, T or inner <= 0;
 * T * inner >= 2^29. */
enum fgcn_window_mode { FGCN_WINDOW_RANDOM = 0, FGCN_WINDOW_CENTRE = 1 };
int fgcn_clip_window(const float* src, const long long* idx, const long long* sample_ids, const int* valid, float* out, float* params, int b,
                     int outer, int T, int W, int inner, float lo, float hi, int mode, unsigned long long seed, unsigned site, unsigned epoch,
                     void* stream);
int fgcn_window_params(unsigned sample, unsigned site, unsigned epoch, unsigned long long seed, float lo, float hi, int mode, float out2[2]);
int fgcn_clip_valid_frames(const float* src, const long long* idx, int* out, int b, int outer, int T, int inner, void* stream);

/* Augmentation of inertial recordings as the batch is gathered (data.ClipBatches(sensors=...)): the four standard
 * perturbations of wearable-sensor data -- a random rotation of the sensor frame, a random gain per sensor, a smooth magnitude warp over
 * time, additive jitter -- and the drop of a whole sensor.  fgcn_clip_augment's conventions: a sample is (outer, T, inner) float32, row k
 * of `out` is made of source row idx[k], the random numbers are a pure function of (seed, site, epoch, sample_ids[k]), a word w gives the
 * uniform u = (float)(w >> 8) * 2^-24, all arithmetic is float32 with every product and sum rounded on its own unless an fma is named.
 *
 * Sensors.  A SENSOR is a triple of values; inner = 3 * units, and the sensors are units [joint_lo, joint_hi), G = joint_hi - joint_lo of
 * them, 1 <= G <= FGCN_SENSORS_MAX.  In a (T, S) signal (outer = 1, inner = S, the range [0, S / 3)) sensor g is columns 3g .. 3g+2; in an
 * (M, T, V, 3) array (outer = M, inner = 3 V) sensor g is joint joint_lo + g of EVERY body.  The units outside the range are copied through
 * by the same gather.  Values are physical ones, zero meaning no signal.  No draw is keyed by the body: all bodies of an array receive the
 * same values for a sensor (fgcn_imu_enhance's invariant "joint V + j of every body holds the recording" is kept), and two arrays of one
 * sample that hold the same G sensors -- the signal and the enhanced skeleton -- share every draw: equal inputs give equal outputs bit for
 * bit.
 *
 * Random words: philox(ctr = {(unsigned)sample, site, epoch, j}, key = {lo32(seed), hi32(seed)}).  fgcn_clip_augment uses j = 0, 1 and
 * fgcn_clip_window j = 2 at the same (seed, site); this stage uses j = 3 for the sample, j = 16 + 4g + {0, 1, 2} for sensor g and
 * j = 2^20 + t * G + g for the jitter of frame t, sensor g: the three stages are independent without a second site.
 *
 * Parameters (the table row of the sample, 12 + 12 G floats).  Floats 0..11, from block 3:
 *     theta_a = (2 u_a - 1) * max_angle[a], a = x, y, z, from words 0..2 (2u - 1 is exact);
 *     R = Rz(theta_z) * Ry(theta_y) * Rx(theta_x), each entry the sum of its one or two products of sinf / cosf values, formed by the
 *     function fgcn_clip_augment forms its matrix with (at s = 1);   row[0..11] = {R row-major (9), 0, 0, 0}.
 * ONE rotation per sample, shared by all its sensors: they sit in one device frame.  It is independent of fgcn_clip_augment's rotation
 * of the skeleton: a change of camera view does not turn a body-worn sensor's axes.
 * Floats 12 + 12g .. 12 + 12g + 11, the group of sensor g, from blocks 16 + 4g (gain, drop), 16 + 4g + 1 (knots 0..3), 16 + 4g + 2 (knots 4..7):
 *     s_g = 1 + (2 u_0 - 1) * scale;   dropped iff word_1 < (unsigned)(drop * 2^32), an integer compare (the product in float64, as in
 *     fgcn_dropout_fwd);   d_{g,k} = (2 u - 1) * warp for k < K = warp_knots, u from word k & 3 of the knot's block;
 *     group = {s_g, 1.0 if dropped else 0.0, 0, 0, d_{g,0..7} with the knots k >= K as 0}.
 *
 * A valid frame t < v of sensor g (v = valid[idx[k]]; valid == NULL: T; a value outside [1, T] is clamped into it), x its source triple:
 *   1. y_c = s_g * fma(R[c][2], x_2, fma(R[c][1], x_1, R[c][0] * x_0)).
 *   2. Magnitude warp, K >= 2 (K == 0: this step is skipped):  q = t * ((K - 1) / (v - 1)), the quotient first (q = 0 when v == 1);
 *      i = min(floor(q), K - 2);  f = q - i;  p0 = d[max(i - 1, 0)], p1 = d[i], p2 = d[i + 1], p3 = d[min(i + 2, K - 1)] (the end knots
 *      repeated);  the Catmull-Rom value through them in Horner form, in exactly this order:
 *          ca = p2 - p0;   cb = ((2 p0 - 5 p1) + 4 p2) - p3;   cc = (3 (p1 - p2) + p3) - p0;
 *          delta = p1 + 0.5 * (f * (ca + f * (cb + f * cc)));   m = 1 + delta;   y_c = m * y_c.
 *      warp == 0 gives knots of +-0, delta = +-0 and m == 1 exactly.
 *   3. Jitter, sigma_g != 0 (sigma_g == 0: the step is skipped, there is no addition: a -0 that reaches this step leaves it as -0).  From the block {w0..w3} of (t, g):
 *      u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (w1 >> 8) * 2^-24;  rad = sqrtf(-2 * logf(u1));  n_0 = rad * cospif(2 u2),
 *      n_1 = rad * sinpif(2 u2);  n_2 = the cosine branch of (w2, w3);  y_c = y_c + sigma_g * n_c (a product, then a sum).  sigma is in the
 *      STORED units, one value per sensor: accelerometer and gyroscope units differ by orders of magnitude.
 *   4. Drop: a dropped sensor's valid frames are +0, whatever steps 1 to 3 gave (there is no rescaling of the kept sensors).
 * Frames at or behind v are copied bit for bit: the padding stays zero.
 * minmax != 0, (T, S) signals only (outer == 1): step 3a of fgcn_signal_prepare applied AFTER the augmentation, over the whole (T, inner)
 * array, the padding zeros included, by the same float32 formula: mn = min y, mx = fl32(max y - mn), out = fl32(fl32(y - mn) / mx), the
 * division correctly rounded; stats[k] = {mn, mx}.  The result equals the formula applied to the minmax == 0 output of the same call,
 * bit for bit.  minmax == 0: stats[k] = {0, 1}.  (Data prepared by fgcn_signal_prepare is prepared with ITS minmax == 0 for this.)
 * Identity: zero angles, scale = warp = drop = 0, zero jitter and minmax == 0 give the gathered rows, as VALUES: step 1 with R = I is
 * fma(0, x_2, fma(0, x_1, 1 * x_0)), which returns a -0 input as +0 where the 0 * x terms are +0 (fgcn_clip_augment's identity does the
 * same).  The sign of a zero is kept only in what is copied: frames at or behind v and units outside the sensor range.
 * Non-finite inputs: rule 3 of "Non-finite values in the inputs" above -- a triple of a kept sensor that reads a non-finite value is
 * non-finite in all three values (0 * inf and 0 * NaN are NaN), NaN against +-inf need not match; a dropped sensor is +0, it reads
 * nothing.  With minmax, a NaN in the augmented array makes mn, mx and the whole clip NaN, as numpy's min and max do.
 *
 * fgcn_clip_sensors: src (rows, outer, T, inner), idx / sample_ids (b) 8-byte integers on the device (idx may repeat and need not be sorted;
 * every idx[k] must be a row of src -- the caller's duty; the streaming path passes idx = 0..b-1 and the real ids), valid NULL or 4-byte
 * integers indexed by SOURCE row, out (b, outer, T, inner), params (b, 12 + 12 G) receives the table, stats (b, 2); jitter: G floats on the
 * HOST.  Two launches: one lane per (row, table group) forms the table, then one lane per (row, outer, frame, unit) reads it back -- with
 * minmax one workgroup per clip, which stores the augmented values, takes their minimum and maximum (order-independent, no atomics) and
 * has every lane normalise the values it stored itself.  The result does not depend on b or on a row's place in the batch.  Rows need
 * 4-byte alignment only.  No fgcn_set_tuning key is read.
 * FGCN_E_BADARG before any launch: a null pointer (valid excepted); b, outer, T or inner <= 0; inner % 3 != 0; a sensor range that is empty
 * or outside 0 <= joint_lo < joint_hi <= inner / 3; G > FGCN_SENSORS_MAX; an angle that is not finite; scale, warp or drop outside [0, 1);
 * warp_knots neither 0 nor in [2, FGCN_SENSORS_MAX_KNOTS]; a jitter value that is negative or not finite; minmax with outer != 1;
 * out == src; T * G >= 2^31 - 2^20 (the jitter's counter words); T * inner >= 2^29; more lanes than one grid holds.
 *
 * fgcn_sensors_params: the HOST copy of the table row of a sample with `sensors` = G sensors, 12 + 12 G floats (no device is touched),
 * computed by the functions the kernel calls; the device's row differs from it in R alone, by the two sinf / cosf implementations.  The
 * same refusals for its arguments. */
#define FGCN_SENSORS_MAX 16
#define FGCN_SENSORS_MAX_KNOTS 8
int fgcn_clip_sensors(const float* src, const long long* idx, const long long* sample_ids, const int* valid, float* out, float* params,
                      float* stats, int b, int outer, int T, int inner, int joint_lo, int joint_hi, const float max_angle[3], float scale,
                      float warp, int warp_knots, const float* jitter, float drop, int minmax, unsigned long long seed, unsigned site,
                      unsigned epoch, void* stream);
int fgcn_sensors_params(unsigned sample, unsigned site, unsigned epoch, unsigned long long seed, const float max_angle[3], float scale, float warp,
                        int warp_knots, float drop, int sensors, float* out);

/* Score fusion of separately trained stream models (ops.score_fuse / ops.fuse_sweep, ensemble.StreamEnsemble / ScoreStore; DESIGN.md
 * section 8k): the 2s-AGCN family reports the accuracy of the weighted sum of its stream models' class scores.
 *
 * The fused value.  Streams s = 0 .. S-1, 1 <= S <= FGCN_FUSE_MAX_STREAMS; scores z_s float32 (rows, classes) with row stride
 * ld_s >= classes; weights w_s float32.  Per row, the transformed scores t_s are
 *     FGCN_FUSE_NONE:     t_s[c] = z_s[c], the raw logits, as 2s-AGCN adds them;
 *     FGCN_FUSE_SOFTMAX:  t_s[c] = float32(exp((double)z_s[c] - (double)m) / sum), m = the row's maximum (NaN skipped; -inf for a row
 *                         of NaN), sum = the float64 sum of those exponentials over the row: formed in float64, rounded ONCE.  The
 *                         order of that sum's additions is fixed by the implementation (the same in both calls below and from call to
 *                         call); a restatement that adds in another order agrees to ~1e-16 relative before the rounding, so to one
 *                         float32 spacing after it.  A row holding a NaN or +inf, or nothing but -inf, is NaN in every element.
 *     fused[r, c] = float32(acc_S),   acc_0 = +0.0,   acc_(s+1) = acc_s + (double)w_s * (double)t_s[r, c]      in stream order.
 * A float32 times a float32 is exact in float64, so contracting the product into an fma changes no bit: in mode NONE the result is
 * defined bit for bit.  Both calls below obtain t_s and fused from ONE device function each, so they cannot disagree.
 *
 * fgcn_score_fuse: writes fused into out (rows, classes) with row stride ld_out >= classes; columns [classes, ld_out) are not touched.
 * One launch, one wave per row, no atomics; two calls give the same bits.  `in` is a HOST pointer; the struct travels by value.
 *
 * fgcn_fuse_sweep: for each of the G candidate weight vectors -- candidates (G, S) float32 ON THE DEVICE, row g = w_0 .. w_(S-1); the
 * struct's `weight` is ignored -- it ADDS to counts (8-byte aligned, 3 + 2 G words of 8 bytes on the device; the caller zeroes it):
 *     counts[FGCN_FUSE_EXAMPLES], counts[FGCN_FUSE_IGNORED], counts[FGCN_FUSE_INVALID]: the rows by label, once per call, not per candidate;
 *     counts[FGCN_FUSE_HEADER + 2 g] top-1 hits and counts[FGCN_FUSE_HEADER + 2 g + 1] top-k hits of candidate g.
 * The float32 fused values are ranked under exactly fgcn_classify_update's rules: NaN sorts above every number and equals NaN; with
 * y = labels[r], rank(y) = #{j : fused_j > fused_y} + #{j < y : fused_j == fused_y}; a top-k hit is rank(y) < k and a top-1 hit is
 * rank(y) == 0 (there: pred == y, the first index of the maximum -- the same thing); y == -100 is ignored and every other y outside
 * [0, classes) is invalid, neither counts for any candidate; the only index derived from a label is clamped first.  So counts of
 * candidate g equal what fgcn_classify_update counts on fgcn_score_fuse's output with candidate g's weights, exactly, in both transforms.
 * One workgroup per row: its waves form t_s (one stream per wave at a time) once in LDS as float32, then every lane ranks the row
 * under one candidate of its own -- the row is read from memory once per pass, not once per candidate.  A pass covers
 * FGCN_FUSE_PASS candidates, whose counters live in LDS, each owned by one lane, and are added to counts with integer atomics (exact
 * in any order) at the workgroup's end; G > FGCN_FUSE_PASS runs ceil(G / FGCN_FUSE_PASS) launches inside the call.  No float atomics;
 * two calls on zeroed counts give the same bits.
 *
 * FGCN_E_BADARG before any launch: a null in / out / candidates / labels / counts, or a null scores[s] for s < S; S outside
 * [1, FGCN_FUSE_MAX_STREAMS]; an unknown transform; rows <= 0; classes outside [1, FGCN_CLS_MAX_CLASSES]; an ld or ld_out < classes;
 * k outside [1, classes]; G <= 0 or G > FGCN_FUSE_MAX_CANDIDATES; out equal to an input.  FGCN_E_ALIGN: counts not 8-byte aligned. */
#define FGCN_FUSE_MAX_STREAMS 8
#define FGCN_FUSE_PASS 2048                  /* candidates whose counters one launch of the sweep holds */
#define FGCN_FUSE_MAX_CANDIDATES 1048576    /* 2^20: candidates of one fgcn_fuse_sweep call */
enum fgcn_fuse_transform { FGCN_FUSE_NONE = 0, FGCN_FUSE_SOFTMAX = 1 };
enum fgcn_fuse_word { FGCN_FUSE_EXAMPLES = 0, FGCN_FUSE_IGNORED = 1, FGCN_FUSE_INVALID = 2, FGCN_FUSE_HEADER = 3 };
typedef struct FgcnFuseIn {
    const float* scores[FGCN_FUSE_MAX_STREAMS];   /* device pointers; entries [S, 8) are not read */
    int ld[FGCN_FUSE_MAX_STREAMS];                /* row strides in floats */
    float weight[FGCN_FUSE_MAX_STREAMS];          /* fgcn_score_fuse only */
} FgcnFuseIn;
int fgcn_score_fuse(const FgcnFuseIn* in, int S, int transform, float* out, int ld_out, int rows, int classes, void* stream);
int fgcn_fuse_sweep(const FgcnFuseIn* in, int S, int transform, const float* candidates, int G, const long long* labels, int rows,
                    int classes, int k, unsigned long long* counts, void* stream);

/* STC attention: the spatial-temporal-channel attention module of MS-AAGCN (Shi et al., TIP 2020) between the graph convolution and the
 * temporal convolution of an AGCN block (ops.stc_*, fops.stc_attention, BlockConfig.attention).
 *
 * G (B, T, V, C) float32 channels-last, contiguous; C a multiple of 64, V <= FGCN_MAX_V_WIDE, B <= 65535, T * V * C < 2^31.  With sg =
 * the logistic sigmoid, k = V for an odd V and V - 1 otherwise, p = (k - 1) / 2, and the parameters in torch's layouts -- w_sa (1, C, k),
 * b_sa (1), w_ta (1, C, 9), b_ta (1), w1 (C / 2, C), b1 (C / 2), w2 (C, C / 2), b2 (C):
 *     mt[b, v, c] = mean_t G                      s[b, v]  = sg(b_sa + sum_{c, j} w_sa[c, j] mt[b, v + j - p, c])    (zero beyond the joints)
 *     m[b, t, c]  = mean_v G (1 + s[b, v])        tg[b, t] = sg(b_ta + sum_{c, j} w_ta[c, j] m[b, t + j - 4, c])     (zero beyond the frames)
 *     cm[b, c]    = mean_t (1 + tg[b, t]) m       h = relu(w1 cm + b1)       cg = sg(w2 h + b2)
 *     G'          = ((G (1 + s[b, v])) (1 + tg[b, t])) (1 + cg[b, c])
 * Forward: fgcn_stc_mean_t (mt), fgcn_stc_gate_s (s), fgcn_stc_mean_v (m), fgcn_stc_gates_tc (tg, cm, h, cg), fgcn_stc_apply (G'; out may
 * be g).  Three passes over G, two launches of one workgroup per sample.  No kernel reads another sample's data.
 *
 * Backward, with dG' = dout and p = dG' G:
 *     fgcn_stc_bwd_qr     q[b, t, c] = sum_v p (1 + s), and rpart (B, fgcn_stc_splits(B, T), V, C): the per-split terms of
 *                         r[b, v, c] = sum_t p (1 + tg)                                                       one pass over dout and g
 *     fgcn_stc_bwd_tc     one workgroup per sample: dzc (B, C), dhpre (B, C / 2), dcm (B, C) -- the gradients at w2 h + b2, w1 cm + b1 and
 *                         cm --, dzt (B, T) at conv_ta's output, dm (B, T, C) = dcm (1 + tg) / T + conv_ta^T dzt, and the sample's terms of
 *                         conv_ta's gradients dwta_part (B, C, 9), dbta_part (B)
 *     fgcn_stc_bwd_ds     dspart (B, fgcn_stc_splits(B, T), V): the per-split terms of sum_{t, c} dm G            one pass over g
 *     fgcn_stc_bwd_s      one workgroup per sample: dzs (B, V) at conv_sa's output from sum_c (1 + cg) r + (sum_{t, c} dm G) / V,
 *                         dmt (B, V, C) = conv_sa^T dzs, the sample's terms dwsa_part (B, C, k), dbsa_part (B)
 *     fgcn_stc_bwd_apply  dg = dout (1 + s)(1 + tg)(1 + cg) + dm (1 + s) / V + dmt / T                            (dg may be dout)
 *     fgcn_stc_param_grads  the eight parameter gradients in the parameters' layouts: sums over the samples, in sample order
 * Every sum has an order fixed by (B, T, V, C) alone; no atomics; two calls give the same bits.  Nothing is skipped on a value: a NaN
 * reaches the sums the definition gives it and no other ("Non-finite values in the inputs").  The ReLU's gate is that of relu_open.
 * FGCN_E_BADARG before any launch: a null pointer, a size outside the limits above.  FGCN_E_ALIGN: a tensor that is read or written in
 * 16-byte groups (g, out, dout, dg, mt, m, cg, dm, dmt) not 16-byte aligned.  fgcn_stc_splits: host only; 0 for B <= 0 or T <= 0. */
int fgcn_stc_splits(int B, int T);
int fgcn_stc_mean_t(const float* g, float* mt, int B, int T, int V, int C, void* stream);
int fgcn_stc_gate_s(const float* mt, const float* w_sa, const float* b_sa, float* s, int B, int V, int C, void* stream);
int fgcn_stc_mean_v(const float* g, const float* s, float* m, int B, int T, int V, int C, void* stream);
int fgcn_stc_gates_tc(const float* m, const float* w_ta, const float* b_ta, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* tg, float* cm, float* h, float* cg, int B, int T, int C, void* stream);
int fgcn_stc_apply(const float* g, const float* s, const float* tg, const float* cg, float* out, int B, int T, int V, int C, void* stream);
int fgcn_stc_bwd_qr(const float* dout, const float* g, const float* s, const float* tg, float* q, float* rpart, int B, int T, int V, int C,
                    void* stream);
int fgcn_stc_bwd_tc(const float* q, const float* m, const float* tg, const float* cg, const float* cm, const float* h, const float* w_ta,
                    const float* w1, const float* w2, float* dzc, float* dhpre, float* dcm, float* dzt, float* dm, float* dwta_part,
                    float* dbta_part, int B, int T, int C, void* stream);
int fgcn_stc_bwd_ds(const float* dm, const float* g, float* dspart, int B, int T, int V, int C, void* stream);
int fgcn_stc_bwd_s(const float* rpart, const float* dspart, const float* cg, const float* s, const float* mt, const float* w_sa, float* dzs,
                   float* dmt, float* dwsa_part, float* dbsa_part, int B, int T, int V, int C, void* stream);
int fgcn_stc_bwd_apply(const float* dout, const float* s, const float* tg, const float* cg, const float* dm, const float* dmt, float* dg, int B,
                       int T, int V, int C, void* stream);
int fgcn_stc_param_grads(const float* dzc, const float* dhpre, const float* cm, const float* h, const float* dwta_part, const float* dbta_part,
                         const float* dwsa_part, const float* dbsa_part, float* d_wsa, float* d_bsa, float* d_wta, float* d_bta, float* d_w1,
                         float* d_b1, float* d_w2, float* d_b2, int B, int V, int C, void* stream);

/* CTR graph convolution: the channel-wise topology refinement graph convolution of CTR-GCN (Chen et al., ICCV 2021) (ops.ctr_*,
 * fops.ctr_aggregate / fops.ctr_mean_t, models/ctrgcn).
 *
 * All tensors float32, channels-last, contiguous, in every math mode.  K = 3 subsets; x3 (B, T, V, K Cout) holds conv3_k(x) at channel
 * k Cout + c; x12 (B, V, 2 K R) holds x1_k = conv1_k(xm) at k R + r and x2_k = conv2_k(xm) at (K + k) R + r, xm = mean_t x; w4 (K, Cout, R),
 * b4 (K, Cout), alpha (1), pa (K, V, V):
 *     th[b, k, u, v, r]  = tanh(x1_k[b, u, r] - x2_k[b, v, r])                                         (B, K, V, V, R)
 *     A'_k[b, u, v, c]   = alpha (b4[k, c] + sum_r w4[k, c, r] th[b, k, u, v, r]) + pa[k, u, v]        never written to memory
 *     y[b, t, u, c]      = sum_k sum_v A'_k[b, u, v, c] x3[b, t, v, k Cout + c]
 * A' is not symmetric: u is the output joint, v the joint summed over.
 * Limits: V <= 32, Cout a multiple of 64 up to 512, R a multiple of 4 up to 64, B <= 65535, T V K Cout < 2^31; fgcn_ctr_mean_t(_bwd): C any
 * multiple of 4 with T V C < 2^31.
 *
 * Forward: fgcn_ctr_mean_t (xm), fgcn_ctr_tanh (th), fgcn_ctr_aggregate (y).  Backward, with dy the gradient of y:
 *     fgcn_ctr_bwd_dx3      dx3[b, t, v, k Cout + c] = sum_u A'_k[b, u, v, c] dy[b, t, u, c]
 *     fgcn_ctr_bwd_da       da (B, K, V, V, Cout): dA'_k[b, u, v, c] = sum_t dy[b, t, u, c] x3[b, t, v, k Cout + c], all frames in frame order
 *     fgcn_ctr_bwd_small    one workgroup per (sample, subset): dz (B, K, V, V, R) = alpha (sum_c dA' w4) (1 - th^2), dx12 (dx1 = sum_v dz,
 *                           dx2 = -sum_u dz), and the sample's terms s2_part (B, K, Cout, R) = sum_{u, v} dA' th, s1_part (B, K, Cout) =
 *                           sum_{u, v} dA', dpa_part (B, K, V, V) = sum_c dA', dalpha_part (B, K) = <b4, s1> + <w4, s2>
 *     fgcn_ctr_param_grads  d_pa = sum_b dpa_part, d_w4 = alpha sum_b s2_part, d_b4 = alpha sum_b s1_part, d_alpha = sum dalpha_part: one
 *                           launch, samples in sample order
 *     fgcn_ctr_mean_t_bwd   dx[b, t, v, c] = dxm[b, v, c] / T, added to dx when `accumulate`
 * fgcn_ctr_aggregate and fgcn_ctr_bwd_dx3 split the frames over workgroups, fgcn_ctr_split_frames(B, T, V, Cout) frames each (host only; 0
 * for sizes outside the limits), and every workgroup of the three walks its frames through LDS in chunks of fgcn_ctr_chunk() frames.
 * Every sum has an order fixed by the sizes alone; no atomics; two calls give the same bits.  No forward kernel reads another sample's
 * data.  Nothing is skipped on a value: alpha == 0 still multiplies ("Non-finite values in the inputs").
 * FGCN_E_BADARG before any launch: a null pointer, a size outside the limits above.  FGCN_E_ALIGN: a tensor that is read or written in
 * 16-byte groups (x, xm, dxm, dx, x3, th, w4, and dy of fgcn_ctr_bwd_dx3) not 16-byte aligned. */
int fgcn_ctr_chunk(void);
int fgcn_ctr_split_frames(int B, int T, int V, int Cout);
int fgcn_ctr_mean_t(const float* x, float* xm, int B, int T, int V, int C, void* stream);
int fgcn_ctr_mean_t_bwd(const float* dxm, float* dx, int B, int T, int V, int C, int accumulate, void* stream);
int fgcn_ctr_tanh(const float* x12, float* th, int B, int V, int R, void* stream);
int fgcn_ctr_aggregate(const float* x3, const float* th, const float* w4, const float* b4, const float* alpha, const float* pa, float* y,
                       int B, int T, int V, int Cout, int R, void* stream);
int fgcn_ctr_bwd_dx3(const float* dy, const float* th, const float* w4, const float* b4, const float* alpha, const float* pa, float* dx3,
                     int B, int T, int V, int Cout, int R, void* stream);
int fgcn_ctr_bwd_da(const float* dy, const float* x3, float* da, int B, int T, int V, int Cout, void* stream);
int fgcn_ctr_bwd_small(const float* da, const float* th, const float* w4, const float* b4, const float* alpha, float* dz, float* dx12,
                       float* s2_part, float* s1_part, float* dpa_part, float* dalpha_part, int B, int V, int Cout, int R, void* stream);
int fgcn_ctr_param_grads(const float* s2_part, const float* s1_part, const float* dpa_part, const float* dalpha_part, const float* alpha,
                         float* d_w4, float* d_b4, float* d_pa, float* d_alpha, int B, int V, int Cout, int R, void* stream);

/* Shift graph convolution: the two shift operations of Shift-GCN (Cheng et al., CVPR 2020) (ops.joint_shift_* / ops.frame_shift_*,
 * fops.joint_shift / fops.frame_shift, models/shiftgcn).
 *
 * All tensors float32, channels-last, contiguous, in every math mode.  Rows are r = (b, t); activations are (B, T, V, C).
 *
 * Joint shift (dir = +1 or -1, optional gate parameter mask (V, C)):
 *     g[v, c]      = tanh(mask[v, c]) + 1                     (1 when no mask is given)
 *     out[r, v, c] = x[r, (v + dir c) mod V, c] * g[v, c]
 *     dx[r, u, c]  = dout[r, w, c] * g[w, c],  w = (u - dir c) mod V
 *     dmask[v, c]  = (1 - tanh(mask[v, c])^2) * sum_r dout[r, v, c] x[r, (v + dir c) mod V, c]
 * The channel index runs far past V (C = 64 at V = 25 wraps twice): mod is the true modulo of a possibly negative number.  Limits: V <= 64;
 * C = 4 (the 3-channel input, which travels as 4 with a zero fourth channel) or a multiple of 64 up to 512; rows < 2^31 / (V C).  C = 4:
 * the mask and dmask have a row stride `mask_ld` of 3 or 4, and the pad channel is written as zero in out, dx and dmask.
 *     fgcn_shift_joint   out[r, v, c] = in[r, (v + dir c) mod V, c] * g, with g = g[v, c] (`source_gate` 0: the forward) or g = g[source
 *                        joint, c] (`source_gate` 1: the data gradient, called with in = dout and the forward's dir NEGATED).  With `x` and
 *                        `part` (chunks, V, C) (both or neither; they need the mask and source_gate) the same pass leaves the terms
 *                        part[chunk, v, c] = sum_{r in chunk} in[r, source joint, c] x[r, v, c]; chunk = the cdiv(rows, fgcn_shift_joint_rows)
 *                        row ranges one workgroup walks.  fgcn_reduce_sum adds them in chunk order.
 *     fgcn_shift_dmask   dmask[v, c] = (1 - tanh(mask[v, c])^2) * sums[(v + dir c) mod V, c] from the summed terms, dir the FORWARD's
 *     fgcn_shift_joint_rows   rows one workgroup walks (host only; 0 for sizes outside the limits)
 *     fgcn_shift_joint_stage  rows of a 64-channel tile one LDS stage holds, which a workgroup's rows are walked in (host only; 0 for V > 64)
 *
 * Frame shift (per-channel position pos (C), stride s in {1, 2}, optional ReLU on the input):
 *     T_out = (T - 1) / s + 1
 *     k = floor(pos[c]),  f = pos[c] - k,  phi = identity or relu
 *     tap(t)           = phi(x[b, t, v, c]) if 0 <= t < T, else 0      (not read outside the clip)
 *     out[b, to, v, c] = (1 - f) tap(to s + k) + f tap(to s + k + 1)
 *     dx[b, t, v, c]   = phi'(x[b, t, v, c]) ((1 - f) dout[b, (t - k) / s, v, c]  where s divides t - k and the quotient is in [0, T_out)
 *                                              + f dout[b, (t - k - 1) / s, v, c]  where s divides t - k - 1 and the quotient is in [0, T_out))
 *     dpos[c]          = sum_{b, to, v} dout[b, to, v, c] (tap(to s + k + 1) - tap(to s + k))
 * dx is the gather form.  dpos is the derivative with k held constant (what autograd gives for f = pos - floor(pos).detach()): at an integer
 * position the right derivative.  k is clamped to +-2^26 as a float before it becomes an integer: pos = +-1e9 gives all-zero output and a zero
 * dpos.  A non-finite pos gives NaN through f in every output of its channel and in no other.  Limits: C a multiple of 64 up to 512, V <= 64,
 * any T >= 1, B <= 65535, B T < 2^31 / (V C).
 *     fgcn_shift_frame       out, and with `part` (B nsplit, 2, C) the BatchNorm partial sums (sum, sum of squares) of out in the layout
 *                            fgcn_bn_finalize takes, summed in the pass that writes out; nsplit = cdiv(T_out, fgcn_shift_frame_split)
 *     fgcn_shift_frame_bwd   dx and dpos_part (B nsplit, C), the workgroups' terms of dpos (fgcn_reduce_sum adds them in order)
 *     fgcn_shift_frame_split output frames one workgroup walks (host only; 0 for sizes outside the limits)
 * `relu`, the stride and the partial sums select kernel instantiations, they are not run-time branches.
 *
 * Every sum has an order fixed by the sizes alone; no atomics; two calls give the same bits.  No kernel reads another row's (joint shift)
 * or another sample's (frame shift) data for out / dx.  Nothing is skipped on a value ("Non-finite values in the inputs"): a gate of 1 and
 * a weight f = 0 still multiply.  FGCN_E_BADARG before any launch: a null pointer, a size outside the limits.  FGCN_E_ALIGN: in, out or
 * part of fgcn_shift_joint (read or written in 16-byte groups) not 16-byte aligned; the frame shift reads and writes single floats. */
int fgcn_shift_joint_rows(long long rows, int V, int C);
int fgcn_shift_joint_stage(int V);
int fgcn_shift_frame_split(int B, int T, int V, int C, int stride);
int fgcn_shift_joint(const float* in, const float* mask, const float* x, float* out, float* part, long long rows, int V, int C, int mask_ld,
                     int dir, int source_gate, void* stream);
int fgcn_shift_dmask(const float* sums, const float* mask, float* dmask, int V, int C, int mask_ld, int dir, void* stream);
int fgcn_shift_frame(const float* x, const float* pos, float* out, float* part, int B, int T, int V, int C, int stride, int relu, void* stream);
int fgcn_shift_frame_bwd(const float* dout, const float* x, const float* pos, float* dx, float* dpos_part, int B, int T, int V, int C, int stride,
                         int relu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FGCN_H */
