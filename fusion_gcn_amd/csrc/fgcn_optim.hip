// Parameter update over the flat parameter / gradient buffers: the step after the hot path.
// The reference builds torch.optim.{SGD, Adam, AdamW} over model.parameters() (torch_src/session_helper.py:48-53,80-84; ADAM
// with weight_decay 0.01 in config/utd-mhad/skeleton/agcn.yaml:16-18) and calls optimizer.step() once per batch
// (session/session.py:176-183): 274 tensors, i.e. ~1000 small launches per step.  Here every trainable value of the model
// lives in one contiguous float32 buffer (fusion_gcn_amd/optim.py; the gradients already do, dp.FlatGradients), and one
// launch applies torch's update formulas element by element -- the data-parallel 1/world average rides along as
// `grad_scale`.  Pure HBM stream: 16-byte loads / stores, 28 B per parameter (Adam).
//
// With a guard (fgcn_optim_guard) two launches go in front of it: the float64 sum of squares of the scaled gradient (one more 4 B
// per parameter read) and a one-workgroup decision -- clip coefficient, apply / skip, step count and every group's step sizes --
// written into caller-owned device state that the update then reads.  The host reads nothing back.
//
// One entry point, fgcn_optim_step: the update is one workgroup per row of a device-resident tile table (start4, count4, group), the
// group's scalars (torch.optim's param_groups) selected from a by-value array in the kernel arguments.  One group is a table whose
// rows all name group 0.  The formulas exist once (optim_update4, guard_decide).
#include <cmath>

#include "fgcn_common.hpp"

namespace fgcn {

struct OptimP {
    float* p;
    const float* g;
    float* m;     // SGD: momentum buffer; Adam: exp_avg; ASGD: ax, the averaged iterate
    float* v;     // Adam: exp_avg_sq
    long long n4;
    float lr, wd, grad_scale;
    float beta1, beta2, eps, step_size, bc2_sqrt;      // Adam / AdamW
    float momentum, dampening;                         // SGD; ASGD: the step's eta, mu
    int nesterov, first_step;
    float c0;                                          // ASGD: 1 - lambd * eta (asgd_decay), set by the kernel
    const unsigned long long* guard;                   // GUARDED: enum fgcn_guard_word, written by optim_guard_decide_kernel
};

__device__ __forceinline__ double guard_f64(const unsigned long long* w, int word) { return __builtin_bit_cast(double, w[word]); }

// ASGD's decay factor as torch's Python scalars give it: the product and the difference each rounded to double, then to float32
// (beta1 carries lambd, momentum eta).  Wave-uniform.
__device__ __forceinline__ float asgd_decay(float lambd, float eta) {
#pragma clang fp contract(off)
    const double prod = (double)lambd * (double)eta;
    return (float)(1.0 - prod);
}

// kind 0: SGD (torch/optim/sgd.py), 1: Adam (L2 weight decay folded into the gradient), 2: AdamW (decoupled decay),
// 3: ASGD (torch/optim/asgd.py, _single_tensor_asgd: decay, step, then the running average ax in state1)
// One 16-byte group i of the flat buffers with the scalars of q (wave-uniform).
template <int KIND>
__device__ __forceinline__ void optim_update4(const OptimP& q, long long i) {
    f32x4 p = *reinterpret_cast<const f32x4*>(q.p + i * 4);
    f32x4 g = *reinterpret_cast<const f32x4*>(q.g + i * 4) * q.grad_scale;
    if (KIND == 0) {
        if (q.wd != 0.f) g += p * q.wd;
        if (q.momentum != 0.f) {
            f32x4 buf = g;                                           // first step: buf = clone(d_p)
            if (!q.first_step) buf = *reinterpret_cast<const f32x4*>(q.m + i * 4) * q.momentum + g * (1.f - q.dampening);
            *reinterpret_cast<f32x4*>(q.m + i * 4) = buf;
            g = q.nesterov ? g + buf * q.momentum : buf;
        }
        p -= g * q.lr;
    } else if (KIND == 3) {
#pragma clang fp contract(off)
        const float eta = q.momentum, mu = q.dampening;
        f32x4 ax = p;
        if (mu != 1.f) ax = *reinterpret_cast<const f32x4*>(q.m + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (q.wd != 0.f) g[e] = __builtin_fmaf(p[e], q.wd, g[e]);      // grad.add(param, alpha=wd): p before the decay
            p[e] = __builtin_fmaf(-eta, g[e], p[e] * q.c0);                 // param.mul_(c0); param.add_(grad, alpha=-eta)
            ax[e] = mu == 1.f ? p[e] : ax[e] + (p[e] - ax[e]) * mu;         // ax.copy_(param) / ax.add_(param.sub(ax).mul_(mu))
        }
        *reinterpret_cast<f32x4*>(q.m + i * 4) = ax;
    } else {
        if (KIND == 1 && q.wd != 0.f) g += p * q.wd;
        if (KIND == 2) p *= 1.f - q.lr * q.wd;
        f32x4 m = *reinterpret_cast<const f32x4*>(q.m + i * 4);
        f32x4 v = *reinterpret_cast<const f32x4*>(q.v + i * 4);
        m += (g - m) * (1.f - q.beta1);                              // exp_avg.lerp_(grad, 1 - beta1)
        v = v * q.beta2 + g * g * (1.f - q.beta2);                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        *reinterpret_cast<f32x4*>(q.m + i * 4) = m;
        *reinterpret_cast<f32x4*>(q.v + i * 4) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float denom = __fsqrt_rn(v[e]) / q.bc2_sqrt + q.eps;
            p[e] -= q.step_size * (m[e] / denom);
        }
    }
    *reinterpret_cast<f32x4*>(q.p + i * 4) = p;
}

// The update: workgroup t takes row t of the tile table (start4, count4, group) -- all int, read with uniform loads -- and
// runs optim_update4 over its 16-byte groups with that group's scalars.  A row that names no group or reaches past the buffers does
// nothing (the host cannot see the table).  GUARDED: the step's scalars come from the state of the launch before (uniform loads),
// nothing is stored when it says skip.
struct OptimGroupsP {
    OptimP base;                                       // buffers, n4, grad_scale, first_step (unguarded), guard
    const int* tiles;
    const double* sched;                               // GUARDED: {step_size, bc2_sqrt} per group, written by the decision launch
                                                       // (ASGD: {eta_use, mu_use, eta_next, mu_next} per group)
    int ngroups;
    fgcn_optim_group grp[FGCN_OPT_MAX_GROUPS];
    float step_size[FGCN_OPT_MAX_GROUPS], bc2_sqrt[FGCN_OPT_MAX_GROUPS];      // unguarded Adam: from the host-side step count
};

template <int KIND, bool GUARDED>
__global__ __launch_bounds__(256) void optim_step_groups_kernel(OptimGroupsP a) {
    const int* t = a.tiles + 3ll * blockIdx.x;
    const int start4 = t[0], gi = t[2];
    if ((unsigned)gi >= (unsigned)a.ngroups || start4 < 0) return;
    const long long room = a.base.n4 - start4;
    const int count4 = t[1] < room ? t[1] : (int)room;
    OptimP q = a.base;
    q.lr = a.grp[gi].lr; q.wd = a.grp[gi].weight_decay;
    q.beta1 = a.grp[gi].beta1; q.beta2 = a.grp[gi].beta2; q.eps = a.grp[gi].eps;
    q.momentum = a.grp[gi].momentum; q.dampening = a.grp[gi].dampening; q.nesterov = a.grp[gi].nesterov;
    q.step_size = a.step_size[gi]; q.bc2_sqrt = a.bc2_sqrt[gi];
    if (GUARDED) {
        if (q.guard[FGCN_GUARD_APPLY] == 0) return;
        q.grad_scale = (float)((double)q.grad_scale * guard_f64(q.guard, FGCN_GUARD_COEF));
        q.first_step = (int)q.guard[FGCN_GUARD_FIRST_STEP];
        if (KIND == 3) {
            q.momentum = (float)a.sched[4 * gi];
            q.dampening = (float)a.sched[4 * gi + 1];
        } else {
            q.step_size = (float)a.sched[2 * gi];
            q.bc2_sqrt = (float)a.sched[2 * gi + 1];
        }
    }
    if (KIND == 3) q.c0 = asgd_decay(q.beta1, q.momentum);
    for (int j = threadIdx.x; j < count4; j += 256) optim_update4<KIND>(q, (long long)start4 + j);
}

// ---- the guard: sum of squares of the scaled gradient, then the decision ---------------------------------------------------------
constexpr int GN_THREADS = 256;
constexpr int GN_UNROLL = 4;                                   // 16-byte groups per thread and chunk
constexpr long long GN_CHUNK4 = (long long)GN_THREADS * GN_UNROLL;  // 16-byte groups per chunk (4096 floats)

// Workgroup w takes the chunks w, w + gridDim.x, ...; inside a chunk thread t takes the groups t, t + 256, ...: which thread adds
// which element depends on the element's index and the grid alone, and the grid on n alone (fgcn_grad_norm_tiles).  The thread sums
// are combined by a butterfly inside the wave and in wave order across the workgroup.  float64 throughout.
__global__ __launch_bounds__(GN_THREADS) void grad_sqsum_kernel(const float* g, long long n4, float grad_scale, double* partials) {
    const double sc = (double)grad_scale;
    const long long chunks = (n4 + GN_CHUNK4 - 1) / GN_CHUNK4;
    double acc = 0.0;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long base = c * GN_CHUNK4 + threadIdx.x;
        f32x4 x[GN_UNROLL];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) {
            const long long i = base + (long long)u * GN_THREADS;
            x[u] = i < n4 ? *reinterpret_cast<const f32x4*>(g + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)x[u][e] * sc;
                acc = fma(d, d, acc);
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    __shared__ double wave_sum[GN_THREADS / 64];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
#pragma unroll
        for (int w = 1; w < GN_THREADS / 64; ++w) s += wave_sum[w];
        partials[blockIdx.x] = s;
    }
}

struct GuardP {
    const double* partials;
    unsigned long long* guard;
    double* sched;                                            // group_sched
    int n_partials, skip_nonfinite, kind, ngroups;
    double max_norm;
    fgcn_optim_group grp[FGCN_OPT_MAX_GROUPS];
};

// One workgroup: the partials go through LDS so that their loads overlap, thread 0 adds them in index order and decides.  Returns
// the new step count to thread 0 of an applied step, 0 to everyone else.
__device__ __forceinline__ unsigned long long guard_decide(const GuardP& q) {
    __shared__ double part[FGCN_GRAD_NORM_MAX_TILES];
    for (int i = threadIdx.x; i < q.n_partials; i += GN_THREADS) part[i] = q.partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return 0ull;
    double sum = 0.0;
    for (int i = 0; i < q.n_partials; ++i) sum += part[i];
    const double norm = sqrt(sum);
    double coef = 1.0;
    if (q.max_norm > 0.0) {
        const double c = q.max_norm / (norm + 1e-6);
        coef = c < 1.0 ? c : (c != c ? c : 1.0);              // torch.clamp(c, max=1.0): a NaN stays a NaN
    }
    const bool apply = isfinite(norm) || !q.skip_nonfinite;
    unsigned long long* w = q.guard;
    w[FGCN_GUARD_NORM] = __builtin_bit_cast(unsigned long long, norm);
    w[FGCN_GUARD_COEF] = __builtin_bit_cast(unsigned long long, coef);
    w[FGCN_GUARD_APPLY] = apply ? 1ull : 0ull;
    if (!apply) {
        w[FGCN_GUARD_SKIPPED] += 1ull;
        return 0ull;
    }
    const unsigned long long step = w[FGCN_GUARD_STEP] + 1ull;
    w[FGCN_GUARD_STEP] = step;
    if (coef < 1.0) w[FGCN_GUARD_CLIPPED] += 1ull;
    w[FGCN_GUARD_FIRST_STEP] = step == 1ull ? 1ull : 0ull;
    return step;
}

// The decision, then every group's scalars of an applied step into `sched`, in double as torch's Python scalars: lane i of thread 0's
// wave computes entry i.  Adam / AdamW: the step size and sqrt(1 - beta2^STEP) from the new STEP, two entries per group.  ASGD, one lane
// per group: the values torch computed after the step before become this step's, and the next step's come from the new STEP and the
// group's current lr (torch/optim/asgd.py: new_eta, new_mu, each rounded through float32; beta1, beta2, eps carry lambd, alpha, t0).
// Nothing moves when the step is skipped.
__global__ __launch_bounds__(GN_THREADS) void optim_guard_decide_kernel(GuardP q) {
#pragma clang fp contract(off)
    const unsigned long long step = __shfl(guard_decide(q), 0);
    const bool asgd = q.kind == FGCN_OPT_ASGD;
    const int per = asgd ? 1 : 2, i = threadIdx.x;
    if (!step || q.kind == FGCN_OPT_SGD || i >= per * q.ngroups) return;
    const fgcn_optim_group& h = q.grp[i / per];
    const double t = (double)step, lr = (double)h.lr, b1 = (double)h.beta1, b2 = (double)h.beta2;
    const double pw = pow(asgd ? 1.0 + b1 * lr * t : i & 1 ? b2 : b1, asgd ? b2 : t);
    if (asgd) {
        double* s = q.sched + 4 * i;
        s[0] = s[2];
        s[1] = s[3];
        const double over = t - (double)h.eps;
        s[2] = (double)(float)(lr / pw);
        s[3] = (double)(float)(1.0 / (over > 1.0 ? over : 1.0));
    } else
        q.sched[i] = i & 1 ? sqrt(1.0 - pw) : lr / (1.0 - pw);
}

}  // namespace fgcn

using namespace fgcn;

extern "C" int fgcn_grad_norm_tiles(long long n) {
    const long long t = cdiv(cdiv(n, 4), GN_CHUNK4);
    return (int)(t < 1 ? 1 : t < FGCN_GRAD_NORM_MAX_TILES ? t : FGCN_GRAD_NORM_MAX_TILES);
}

extern "C" long long fgcn_optim_guard_bytes(void) { return 8ll * FGCN_GUARD_WORDS; }

// Everything the call checks and fills in: the buffers, every group's ranges (the message names the group), then the guard.  `step` is
// the host-side count without a guard; with one the count lives in the guard state.
static int optim_prepare(OptimGroupsP& a, GuardP& d, float* params, const float* grads, float* state1, float* state2, long long n,
                         int kind, const fgcn_optim_group* groups, int ngroups, const int* tiles, int ntiles, float grad_scale,
                         long long step, const fgcn_optim_guard* guard) {
    FGCN_REQUIRE(params && grads && n > 0, FGCN_E_BADARG, "optim_step: null pointer or empty buffer");
    FGCN_REQUIRE(n % 4 == 0 && aligned16(params) && aligned16(grads), FGCN_E_ALIGN,
                 "optim_step: buffers must be 16-byte aligned and a multiple of 4 floats long (n=%lld)", n);
    FGCN_REQUIRE(n / 4 <= 0x7fffffffll, FGCN_E_BADARG, "optim_step: the tile table indexes 16-byte groups with an int (n=%lld)", n);
    FGCN_REQUIRE(kind >= FGCN_OPT_SGD && kind <= FGCN_OPT_ASGD, FGCN_E_BADARG, "optim_step: kind %d", kind);
    FGCN_REQUIRE(guard || step >= 1, FGCN_E_BADARG, "optim_step: step counts from 1 (got %lld)", step);
    FGCN_REQUIRE(!guard || step == 0, FGCN_E_BADARG, "optim_step: with a guard the count lives in its state: step must be 0 (got %lld)",
                 step);
    FGCN_REQUIRE(ngroups >= 1 && ngroups <= FGCN_OPT_MAX_GROUPS, FGCN_E_BADARG, "optim_step: 1 to %d parameter groups (got %d)",
                 FGCN_OPT_MAX_GROUPS, ngroups);
    FGCN_REQUIRE(groups, FGCN_E_BADARG, "optim_step: null groups");
    FGCN_REQUIRE(tiles && ntiles >= 1, FGCN_E_BADARG, "optim_step: null or empty tile table");
    FGCN_REQUIRE(((uintptr_t)tiles & 3) == 0, FGCN_E_ALIGN, "optim_step: the tile table must be 4-byte aligned");
    a = OptimGroupsP{};
    OptimP& q = a.base;
    q.p = params; q.g = grads; q.m = state1; q.v = state2; q.n4 = n / 4; q.grad_scale = grad_scale;
    q.first_step = kind == FGCN_OPT_SGD && step == 1;
    a.tiles = tiles; a.ngroups = ngroups;
    if (kind == FGCN_OPT_ASGD) {
        FGCN_REQUIRE(state1 && aligned16(state1), FGCN_E_BADARG, "optim_step: kind 3 (ASGD) needs ax, the averaged iterate, in state1");
        FGCN_REQUIRE(!state2, FGCN_E_BADARG, "optim_step: kind 3 (ASGD) keeps one state buffer: state2 must be NULL");
    } else if (kind != FGCN_OPT_SGD)
        FGCN_REQUIRE(state1 && state2 && aligned16(state1) && aligned16(state2), FGCN_E_BADARG,
                     "optim_step: Adam needs exp_avg and exp_avg_sq");
    for (int g = 0; g < ngroups; ++g) {
        const fgcn_optim_group& h = groups[g];
        FGCN_REQUIRE(h.lr >= 0.f && h.weight_decay >= 0.f, FGCN_E_BADARG, "optim_step: group %d: negative lr / weight_decay", g);
        if (kind == FGCN_OPT_SGD) {
            FGCN_REQUIRE(h.momentum >= 0.f && (h.momentum == 0.f || (state1 && aligned16(state1))), FGCN_E_BADARG,
                         "optim_step: group %d: SGD with momentum needs the momentum buffer", g);
            FGCN_REQUIRE(!h.nesterov || (h.momentum > 0.f && h.dampening == 0.f), FGCN_E_BADARG,
                         "optim_step: group %d: Nesterov momentum requires a momentum and zero dampening", g);
        } else if (kind == FGCN_OPT_ASGD) {      // beta1, beta2, eps carry lambd, alpha, t0
            FGCN_REQUIRE(h.beta1 >= 0.f && std::isfinite(h.beta2) && std::isfinite(h.eps), FGCN_E_BADARG,
                         "optim_step: group %d: ASGD: negative lambd or alpha / t0 not finite", g);
            // momentum, dampening carry the step's eta, mu without a guard (with one the update reads group_sched)
            FGCN_REQUIRE(guard || (h.momentum >= 0.f && h.dampening > 0.f && h.dampening <= 1.f), FGCN_E_BADARG,
                         "optim_step: group %d: ASGD: eta must be >= 0 and mu in (0, 1] (got %g, %g)", g, (double)h.momentum,
                         (double)h.dampening);
        } else {
            FGCN_REQUIRE(h.beta1 >= 0.f && h.beta1 < 1.f && h.beta2 >= 0.f && h.beta2 < 1.f && h.eps >= 0.f, FGCN_E_BADARG,
                         "optim_step: group %d: betas / eps out of range", g);
            if (!guard) {      // the bias corrections in double, as torch's Python scalars
                const double bc1 = 1.0 - std::pow((double)h.beta1, (double)step), bc2 = 1.0 - std::pow((double)h.beta2, (double)step);
                a.step_size[g] = (float)((double)h.lr / bc1);
                a.bc2_sqrt[g] = (float)std::sqrt(bc2);
            }
        }
        a.grp[g] = h;
    }
    if (!guard) return FGCN_OK;
    FGCN_REQUIRE(guard->partials && guard->state, FGCN_E_BADARG, "optim_step: null partials / guard state");
    FGCN_REQUIRE(((uintptr_t)guard->state & 7) == 0 && ((uintptr_t)guard->partials & 7) == 0, FGCN_E_ALIGN,
                 "optim_step: guard state and partials must be 8-byte aligned");
    FGCN_REQUIRE(guard->n_partials == fgcn_grad_norm_tiles(n), FGCN_E_BADARG, "optim_step: n_partials must be %d (got %d)",
                 fgcn_grad_norm_tiles(n), guard->n_partials);
    FGCN_REQUIRE(guard->max_norm >= 0.0, FGCN_E_BADARG, "optim_step: max_norm must be a number >= 0 (0: no clipping)");
    FGCN_REQUIRE(guard->group_sched, FGCN_E_BADARG, "optim_step: null group_sched");
    FGCN_REQUIRE(((uintptr_t)guard->group_sched & 7) == 0, FGCN_E_ALIGN, "optim_step: group_sched must be 8-byte aligned");
    d = GuardP{};
    d.partials = guard->partials; d.guard = static_cast<unsigned long long*>(guard->state); d.sched = guard->group_sched;
    d.n_partials = guard->n_partials; d.skip_nonfinite = guard->skip_nonfinite != 0; d.kind = kind; d.ngroups = ngroups;
    d.max_norm = guard->max_norm;
    for (int g = 0; g < ngroups; ++g) d.grp[g] = groups[g];
    q.guard = d.guard;
    a.sched = d.sched;
    return FGCN_OK;
}

template <bool GUARDED>
static void optim_launch(const OptimGroupsP& a, int kind, int ntiles, hipStream_t s) {
    const dim3 grid((unsigned)ntiles);
    if (kind == FGCN_OPT_SGD) hipLaunchKernelGGL((optim_step_groups_kernel<0, GUARDED>), grid, dim3(256), 0, s, a);
    else if (kind == FGCN_OPT_ADAM) hipLaunchKernelGGL((optim_step_groups_kernel<1, GUARDED>), grid, dim3(256), 0, s, a);
    else if (kind == FGCN_OPT_ADAMW) hipLaunchKernelGGL((optim_step_groups_kernel<2, GUARDED>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((optim_step_groups_kernel<3, GUARDED>), grid, dim3(256), 0, s, a);
}

extern "C" int fgcn_optim_step(float* params, const float* grads, float* state1, float* state2, long long n, int kind,
                               const fgcn_optim_group* groups, int ngroups, const int* tiles, int ntiles, float grad_scale,
                               long long step, const fgcn_optim_guard* guard, void* stream) {
    OptimGroupsP a;
    GuardP d;
    const int rc = optim_prepare(a, d, params, grads, state1, state2, n, kind, groups, ngroups, tiles, ntiles, grad_scale, step, guard);
    if (rc != FGCN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (guard) {      // norm -> decision -> update, stream-ordered
        hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)guard->n_partials), dim3(GN_THREADS), 0, s, grads, a.base.n4, grad_scale,
                           guard->partials);
        hipLaunchKernelGGL(optim_guard_decide_kernel, dim3(1), dim3(GN_THREADS), 0, s, d);
        optim_launch<true>(a, kind, ntiles, s);
    } else
        optim_launch<false>(a, kind, ntiles, s);
    return launch_status("optim_step");
}
