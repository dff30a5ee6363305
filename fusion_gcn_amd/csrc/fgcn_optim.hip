// Parameter update over the flat parameter / gradient buffers: the step after the hot path.
// The reference builds torch.optim.{SGD, Adam, AdamW} over model.parameters() (torch_src/session_helper.py:48-53,80-84; ADAM
// with weight_decay 0.01 in config/utd-mhad/skeleton/agcn.yaml:16-18) and calls optimizer.step() once per batch
// (session/session.py:176-183): 274 tensors, i.e. ~1000 small launches per step.  Here every trainable value of the model
// lives in one contiguous float32 buffer (fusion_gcn_amd/optim.py; the gradients already do, dp.FlatGradients), and one
// launch applies torch's update formulas element by element -- the data-parallel 1/world average rides along as
// `grad_scale`.  Pure HBM stream: 16-byte loads / stores, 28 B per parameter (Adam).
//
// The guarded form (fgcn_optim_step_guarded) puts two launches in front of it: the float64 sum of squares of the scaled gradient
// (one more 4 B per parameter read) and a one-workgroup decision -- clip coefficient, apply / skip, step count and Adam's bias
// corrections -- written into a caller-owned guard state that the update then reads.  The host reads nothing back.
//
// The grouped forms (fgcn_optim_step_groups, fgcn_optim_step_groups_guarded: torch.optim's param_groups) keep the launch counts: the
// update is still one launch, one workgroup per row of a device-resident tile table (start4, count4, group), the group's scalars
// selected from a by-value array in the kernel arguments.  The formulas exist once (optim_update4, guard_decide).
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

// GUARDED: the step's scalars come from the guard state of the launch before (uniform loads), nothing is stored when it says skip
template <int KIND, bool GUARDED>
__global__ __launch_bounds__(256) void optim_step_kernel(OptimP q) {
    if (GUARDED) {
        if (q.guard[FGCN_GUARD_APPLY] == 0) return;
        q.grad_scale = (float)((double)q.grad_scale * guard_f64(q.guard, FGCN_GUARD_COEF));
        q.first_step = (int)q.guard[FGCN_GUARD_FIRST_STEP];
        q.step_size = (float)guard_f64(q.guard, FGCN_GUARD_STEP_SIZE);
        q.bc2_sqrt = (float)guard_f64(q.guard, FGCN_GUARD_BC2_SQRT);
    }
    if (KIND == 3) q.c0 = asgd_decay(q.beta1, q.momentum);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < q.n4; i += (long long)gridDim.x * blockDim.x)
        optim_update4<KIND>(q, i);
}

// The grouped update: workgroup t takes row t of the tile table (start4, count4, group) -- all int, read with uniform loads -- and
// runs optim_update4 over its 16-byte groups with that group's scalars.  A row that names no group or reaches past the buffers does
// nothing (the host cannot see the table).
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
    int n_partials, skip_nonfinite, adam;
    double max_norm, lr, beta1, beta2;
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

__global__ __launch_bounds__(GN_THREADS) void optim_guard_decide_kernel(GuardP q) {
    const unsigned long long step = guard_decide(q);
    if (step && q.adam) {                                     // the bias corrections in double, as fgcn_optim_step's host code
        const double bc1 = 1.0 - pow(q.beta1, (double)step), bc2 = 1.0 - pow(q.beta2, (double)step);
        q.guard[FGCN_GUARD_STEP_SIZE] = __builtin_bit_cast(unsigned long long, q.lr / bc1);
        q.guard[FGCN_GUARD_BC2_SQRT] = __builtin_bit_cast(unsigned long long, sqrt(bc2));
    }
}

// The same decision for the grouped update: every group's step size and sqrt(1 - beta2^STEP) go to `sched` instead of the guard words.
struct GuardGroupsP {
    GuardP d;                                                 // (d.lr / d.beta1 / d.beta2 unused)
    double* sched;
    int ngroups;
    double lr[FGCN_OPT_MAX_GROUPS], beta1[FGCN_OPT_MAX_GROUPS], beta2[FGCN_OPT_MAX_GROUPS];
};

__global__ __launch_bounds__(GN_THREADS) void optim_guard_decide_groups_kernel(GuardGroupsP a) {
    const unsigned long long step = guard_decide(a.d);
    if (!step || !a.d.adam) return;
    for (int g = 0; g < a.ngroups; ++g) {
        const double bc1 = 1.0 - pow(a.beta1[g], (double)step), bc2 = 1.0 - pow(a.beta2[g], (double)step);
        a.sched[2 * g] = a.lr[g] / bc1;
        a.sched[2 * g + 1] = sqrt(bc2);
    }
}

// ASGD's decision: the values torch computed after the step before become this step's, and the next step's come from the new STEP and
// the groups' current lr (torch/optim/asgd.py: new_eta, new_mu, each rounded through float32).  Nothing moves when the step is skipped.
struct GuardAsgdP {
    GuardP d;                                                 // (d.lr / d.beta1 / d.beta2 unused, d.adam 0)
    double* sched;                                            // {eta_use, mu_use, eta_next, mu_next} per group
    int ngroups;
    double lr[FGCN_OPT_MAX_GROUPS], lambd[FGCN_OPT_MAX_GROUPS], alpha[FGCN_OPT_MAX_GROUPS], t0[FGCN_OPT_MAX_GROUPS];
};

__global__ __launch_bounds__(GN_THREADS) void optim_guard_decide_asgd_kernel(GuardAsgdP a) {
    const unsigned long long step = guard_decide(a.d);
    if (!step) return;
    const double t = (double)step;
    for (int g = 0; g < a.ngroups; ++g) {
#pragma clang fp contract(off)
        double* s = a.sched + 4 * g;
        s[0] = s[2];
        s[1] = s[3];
        const double over = t - a.t0[g];
        s[2] = (double)(float)(a.lr[g] / pow(1.0 + a.lambd[g] * a.lr[g] * t, a.alpha[g]));
        s[3] = (double)(float)(1.0 / (over > 1.0 ? over : 1.0));
    }
}

}  // namespace fgcn

using namespace fgcn;

// Everything both entry points check and fill in; `step` is the host-side count of the unguarded call, NULL for the guarded one
// (whose count lives in the guard state).
static int optim_prepare(OptimP& q, const char* who, float* params, const float* grads, float* state1, float* state2, long long n,
                         int kind, float lr, float weight_decay, float grad_scale, float beta1, float beta2, float eps,
                         float momentum, float dampening, int nesterov, const long long* step) {
    FGCN_REQUIRE(params && grads && n > 0, FGCN_E_BADARG, "%s: null pointer or empty buffer", who);
    FGCN_REQUIRE(n % 4 == 0 && aligned16(params) && aligned16(grads), FGCN_E_ALIGN,
                 "%s: buffers must be 16-byte aligned and a multiple of 4 floats long (n=%lld)", who, n);
    FGCN_REQUIRE(kind >= FGCN_OPT_SGD && kind <= FGCN_OPT_ASGD, FGCN_E_BADARG, "%s: kind %d", who, kind);
    FGCN_REQUIRE(!step || *step >= 1, FGCN_E_BADARG, "%s: step counts from 1 (got %lld)", who, step ? *step : 0ll);
    FGCN_REQUIRE(lr >= 0.f && weight_decay >= 0.f, FGCN_E_BADARG, "%s: negative lr / weight_decay", who);
    q = OptimP{};
    q.p = params; q.g = grads; q.m = state1; q.v = state2; q.n4 = n / 4;
    q.lr = lr; q.wd = weight_decay; q.grad_scale = grad_scale;
    if (kind == FGCN_OPT_SGD) {
        FGCN_REQUIRE(momentum >= 0.f && (momentum == 0.f || (state1 && aligned16(state1))), FGCN_E_BADARG,
                     "%s: SGD with momentum needs the momentum buffer", who);
        FGCN_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), FGCN_E_BADARG,
                     "%s: Nesterov momentum requires a momentum and zero dampening", who);
        q.momentum = momentum; q.dampening = dampening; q.nesterov = nesterov; q.first_step = step && *step == 1;
    } else if (kind == FGCN_OPT_ASGD) {      // beta1, beta2, eps carry lambd, alpha, t0; momentum, dampening the step's eta, mu
        FGCN_REQUIRE(state1 && aligned16(state1), FGCN_E_BADARG, "%s: kind 3 (ASGD) needs ax, the averaged iterate, in state1", who);
        FGCN_REQUIRE(!state2, FGCN_E_BADARG, "%s: kind 3 (ASGD) keeps one state buffer: state2 must be NULL", who);
        FGCN_REQUIRE(beta1 >= 0.f && std::isfinite(beta2) && std::isfinite(eps), FGCN_E_BADARG,
                     "%s: ASGD: negative lambd or alpha / t0 not finite", who);
        FGCN_REQUIRE(momentum >= 0.f && dampening > 0.f && dampening <= 1.f, FGCN_E_BADARG,
                     "%s: ASGD: eta must be >= 0 and mu in (0, 1] (got %g, %g)", who, (double)momentum, (double)dampening);
        q.beta1 = beta1; q.momentum = momentum; q.dampening = dampening;
    } else {
        FGCN_REQUIRE(state1 && state2 && aligned16(state1) && aligned16(state2), FGCN_E_BADARG,
                     "%s: Adam needs exp_avg and exp_avg_sq", who);
        FGCN_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, FGCN_E_BADARG,
                     "%s: betas / eps out of range", who);
        q.beta1 = beta1; q.beta2 = beta2; q.eps = eps;
        if (step) {      // the bias corrections in double, as torch's Python scalars
            const double bc1 = 1.0 - std::pow((double)beta1, (double)*step), bc2 = 1.0 - std::pow((double)beta2, (double)*step);
            q.step_size = (float)((double)lr / bc1);
            q.bc2_sqrt = (float)std::sqrt(bc2);
        }
    }
    return FGCN_OK;
}

template <bool GUARDED>
static void optim_launch(const OptimP& q, int kind, hipStream_t s) {
    const long long blocks = cdiv(q.n4, 256);
    dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (kind == FGCN_OPT_SGD) hipLaunchKernelGGL((optim_step_kernel<0, GUARDED>), grid, dim3(256), 0, s, q);
    else if (kind == FGCN_OPT_ADAM) hipLaunchKernelGGL((optim_step_kernel<1, GUARDED>), grid, dim3(256), 0, s, q);
    else if (kind == FGCN_OPT_ADAMW) hipLaunchKernelGGL((optim_step_kernel<2, GUARDED>), grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL((optim_step_kernel<3, false>), grid, dim3(256), 0, s, q);      // (ASGD has no single-group guarded form)
}

extern "C" int fgcn_optim_step(float* params, const float* grads, float* state1, float* state2, long long n, int kind,
                               float lr, float weight_decay, float grad_scale, float beta1, float beta2, float eps,
                               float momentum, float dampening, int nesterov, long long step, void* stream) {
    OptimP q;
    const int rc = optim_prepare(q, "optim_step", params, grads, state1, state2, n, kind, lr, weight_decay, grad_scale, beta1, beta2,
                                 eps, momentum, dampening, nesterov, &step);
    if (rc != FGCN_OK) return rc;
    optim_launch<false>(q, kind, (hipStream_t)stream);
    return launch_status("optim_step");
}

extern "C" int fgcn_grad_norm_tiles(long long n) {
    const long long t = cdiv(cdiv(n, 4), GN_CHUNK4);
    return (int)(t < 1 ? 1 : t < FGCN_GRAD_NORM_MAX_TILES ? t : FGCN_GRAD_NORM_MAX_TILES);
}

extern "C" long long fgcn_optim_guard_bytes(void) { return 8ll * FGCN_GUARD_WORDS; }

// What both guarded entry points check and fill in for the decision launch.
static int guard_prepare(GuardP& d, const char* who, long long n, int kind, double max_norm, int skip_nonfinite, double* partials,
                         int n_partials, void* guard) {
    FGCN_REQUIRE(partials && guard, FGCN_E_BADARG, "%s: null partials / guard state", who);
    FGCN_REQUIRE(((uintptr_t)guard & 7) == 0 && ((uintptr_t)partials & 7) == 0, FGCN_E_ALIGN,
                 "%s: guard state and partials must be 8-byte aligned", who);
    FGCN_REQUIRE(n_partials == fgcn_grad_norm_tiles(n), FGCN_E_BADARG, "%s: n_partials must be %d (got %d)", who,
                 fgcn_grad_norm_tiles(n), n_partials);
    FGCN_REQUIRE(max_norm >= 0.0, FGCN_E_BADARG, "%s: max_norm must be a number >= 0 (0: no clipping)", who);
    d = GuardP{};
    d.partials = partials; d.guard = static_cast<unsigned long long*>(guard); d.n_partials = n_partials;
    d.skip_nonfinite = skip_nonfinite != 0; d.adam = kind == FGCN_OPT_ADAM || kind == FGCN_OPT_ADAMW;
    d.max_norm = max_norm;
    return FGCN_OK;
}

extern "C" int fgcn_optim_step_guarded(float* params, const float* grads, float* state1, float* state2, long long n, int kind,
                                       float lr, float weight_decay, float grad_scale, float beta1, float beta2, float eps,
                                       float momentum, float dampening, int nesterov, double max_norm, int skip_nonfinite,
                                       double* partials, int n_partials, void* guard, void* stream) {
    FGCN_REQUIRE(kind != FGCN_OPT_ASGD, FGCN_E_BADARG,
                 "optim_step_guarded: kind 3 (ASGD) keeps eta / mu in group_sched: call fgcn_optim_step_groups_guarded with one group");
    OptimP q;
    int rc = optim_prepare(q, "optim_step_guarded", params, grads, state1, state2, n, kind, lr, weight_decay, grad_scale, beta1,
                           beta2, eps, momentum, dampening, nesterov, nullptr);
    if (rc != FGCN_OK) return rc;
    GuardP d;
    rc = guard_prepare(d, "optim_step_guarded", n, kind, max_norm, skip_nonfinite, partials, n_partials, guard);
    if (rc != FGCN_OK) return rc;
    q.guard = d.guard;
    d.lr = (double)lr; d.beta1 = (double)beta1; d.beta2 = (double)beta2;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)n_partials), dim3(GN_THREADS), 0, s, grads, q.n4, grad_scale, partials);
    hipLaunchKernelGGL(optim_guard_decide_kernel, dim3(1), dim3(GN_THREADS), 0, s, d);
    optim_launch<true>(q, kind, s);
    return launch_status("optim_step_guarded");
}

// ---- several parameter groups ----------------------------------------------------------------------------------------------------
// Everything both grouped entry points check and fill in: the buffers as optim_prepare, then every group's ranges (the message names
// the group).  `step` as in optim_prepare.
static int optim_groups_prepare(OptimGroupsP& a, const char* who, float* params, const float* grads, float* state1, float* state2,
                                long long n, int kind, const fgcn_optim_group* groups, int ngroups, const int* tiles, int ntiles,
                                float grad_scale, const long long* step) {
    FGCN_REQUIRE(params && grads && n > 0, FGCN_E_BADARG, "%s: null pointer or empty buffer", who);
    FGCN_REQUIRE(n % 4 == 0 && aligned16(params) && aligned16(grads), FGCN_E_ALIGN,
                 "%s: buffers must be 16-byte aligned and a multiple of 4 floats long (n=%lld)", who, n);
    FGCN_REQUIRE(n / 4 <= 0x7fffffffll, FGCN_E_BADARG, "%s: the tile table indexes 16-byte groups with an int (n=%lld)", who, n);
    FGCN_REQUIRE(kind >= FGCN_OPT_SGD && kind <= FGCN_OPT_ASGD, FGCN_E_BADARG, "%s: kind %d", who, kind);
    FGCN_REQUIRE(!step || *step >= 1, FGCN_E_BADARG, "%s: step counts from 1 (got %lld)", who, step ? *step : 0ll);
    FGCN_REQUIRE(ngroups >= 1 && ngroups <= FGCN_OPT_MAX_GROUPS, FGCN_E_BADARG, "%s: 1 to %d parameter groups (got %d)", who,
                 FGCN_OPT_MAX_GROUPS, ngroups);
    FGCN_REQUIRE(groups, FGCN_E_BADARG, "%s: null groups", who);
    FGCN_REQUIRE(tiles && ntiles >= 1, FGCN_E_BADARG, "%s: null or empty tile table", who);
    FGCN_REQUIRE(((uintptr_t)tiles & 3) == 0, FGCN_E_ALIGN, "%s: the tile table must be 4-byte aligned", who);
    a = OptimGroupsP{};
    OptimP& q = a.base;
    q.p = params; q.g = grads; q.m = state1; q.v = state2; q.n4 = n / 4; q.grad_scale = grad_scale;
    q.first_step = kind == FGCN_OPT_SGD && step && *step == 1;
    a.tiles = tiles; a.ngroups = ngroups;
    if (kind == FGCN_OPT_ASGD) {
        FGCN_REQUIRE(state1 && aligned16(state1), FGCN_E_BADARG, "%s: kind 3 (ASGD) needs ax, the averaged iterate, in state1", who);
        FGCN_REQUIRE(!state2, FGCN_E_BADARG, "%s: kind 3 (ASGD) keeps one state buffer: state2 must be NULL", who);
    } else if (kind != FGCN_OPT_SGD)
        FGCN_REQUIRE(state1 && state2 && aligned16(state1) && aligned16(state2), FGCN_E_BADARG, "%s: Adam needs exp_avg and exp_avg_sq",
                     who);
    for (int g = 0; g < ngroups; ++g) {
        const fgcn_optim_group& h = groups[g];
        FGCN_REQUIRE(h.lr >= 0.f && h.weight_decay >= 0.f, FGCN_E_BADARG, "%s: group %d: negative lr / weight_decay", who, g);
        if (kind == FGCN_OPT_SGD) {
            FGCN_REQUIRE(h.momentum >= 0.f && (h.momentum == 0.f || (state1 && aligned16(state1))), FGCN_E_BADARG,
                         "%s: group %d: SGD with momentum needs the momentum buffer", who, g);
            FGCN_REQUIRE(!h.nesterov || (h.momentum > 0.f && h.dampening == 0.f), FGCN_E_BADARG,
                         "%s: group %d: Nesterov momentum requires a momentum and zero dampening", who, g);
        } else if (kind == FGCN_OPT_ASGD) {      // beta1, beta2, eps carry lambd, alpha, t0
            FGCN_REQUIRE(h.beta1 >= 0.f && std::isfinite(h.beta2) && std::isfinite(h.eps), FGCN_E_BADARG,
                         "%s: group %d: ASGD: negative lambd or alpha / t0 not finite", who, g);
            // momentum, dampening carry the step's eta, mu on the unguarded path (the guarded one reads group_sched)
            FGCN_REQUIRE(!step || (h.momentum >= 0.f && h.dampening > 0.f && h.dampening <= 1.f), FGCN_E_BADARG,
                         "%s: group %d: ASGD: eta must be >= 0 and mu in (0, 1] (got %g, %g)", who, g, (double)h.momentum,
                         (double)h.dampening);
        } else {
            FGCN_REQUIRE(h.beta1 >= 0.f && h.beta1 < 1.f && h.beta2 >= 0.f && h.beta2 < 1.f && h.eps >= 0.f, FGCN_E_BADARG,
                         "%s: group %d: betas / eps out of range", who, g);
            if (step) {      // the bias corrections in double, as torch's Python scalars
                const double bc1 = 1.0 - std::pow((double)h.beta1, (double)*step), bc2 = 1.0 - std::pow((double)h.beta2, (double)*step);
                a.step_size[g] = (float)((double)h.lr / bc1);
                a.bc2_sqrt[g] = (float)std::sqrt(bc2);
            }
        }
        a.grp[g] = h;
    }
    return FGCN_OK;
}

template <bool GUARDED>
static void optim_groups_launch(const OptimGroupsP& a, int kind, int ntiles, hipStream_t s) {
    const dim3 grid((unsigned)ntiles);
    if (kind == FGCN_OPT_SGD) hipLaunchKernelGGL((optim_step_groups_kernel<0, GUARDED>), grid, dim3(256), 0, s, a);
    else if (kind == FGCN_OPT_ADAM) hipLaunchKernelGGL((optim_step_groups_kernel<1, GUARDED>), grid, dim3(256), 0, s, a);
    else if (kind == FGCN_OPT_ADAMW) hipLaunchKernelGGL((optim_step_groups_kernel<2, GUARDED>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((optim_step_groups_kernel<3, GUARDED>), grid, dim3(256), 0, s, a);
}

extern "C" int fgcn_optim_step_groups(float* params, const float* grads, float* state1, float* state2, long long n, int kind,
                                      const fgcn_optim_group* groups, int ngroups, const int* tiles, int ntiles, float grad_scale,
                                      long long step, void* stream) {
    OptimGroupsP a;
    const int rc = optim_groups_prepare(a, "optim_step_groups", params, grads, state1, state2, n, kind, groups, ngroups, tiles, ntiles,
                                        grad_scale, &step);
    if (rc != FGCN_OK) return rc;
    optim_groups_launch<false>(a, kind, ntiles, (hipStream_t)stream);
    return launch_status("optim_step_groups");
}

extern "C" int fgcn_optim_step_groups_guarded(float* params, const float* grads, float* state1, float* state2, long long n, int kind,
                                              const fgcn_optim_group* groups, int ngroups, const int* tiles, int ntiles,
                                              float grad_scale, double max_norm, int skip_nonfinite, double* partials, int n_partials,
                                              void* guard, double* group_sched, void* stream) {
    OptimGroupsP a;
    int rc = optim_groups_prepare(a, "optim_step_groups_guarded", params, grads, state1, state2, n, kind, groups, ngroups, tiles,
                                  ntiles, grad_scale, nullptr);
    if (rc != FGCN_OK) return rc;
    GuardGroupsP d{};
    rc = guard_prepare(d.d, "optim_step_groups_guarded", n, kind, max_norm, skip_nonfinite, partials, n_partials, guard);
    if (rc != FGCN_OK) return rc;
    FGCN_REQUIRE(group_sched, FGCN_E_BADARG, "optim_step_groups_guarded: null group_sched");
    FGCN_REQUIRE(((uintptr_t)group_sched & 7) == 0, FGCN_E_ALIGN, "optim_step_groups_guarded: group_sched must be 8-byte aligned");
    a.base.guard = d.d.guard;
    a.sched = group_sched;
    d.sched = group_sched; d.ngroups = ngroups;
    for (int g = 0; g < ngroups; ++g) {
        d.lr[g] = (double)groups[g].lr; d.beta1[g] = (double)groups[g].beta1; d.beta2[g] = (double)groups[g].beta2;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)n_partials), dim3(GN_THREADS), 0, s, grads, a.base.n4, grad_scale, partials);
    if (kind == FGCN_OPT_ASGD) {
        GuardAsgdP e{};
        e.d = d.d; e.sched = group_sched; e.ngroups = ngroups;
        for (int g = 0; g < ngroups; ++g) {
            e.lr[g] = (double)groups[g].lr; e.lambd[g] = (double)groups[g].beta1;
            e.alpha[g] = (double)groups[g].beta2; e.t0[g] = (double)groups[g].eps;
        }
        hipLaunchKernelGGL(optim_guard_decide_asgd_kernel, dim3(1), dim3(GN_THREADS), 0, s, e);
    } else
        hipLaunchKernelGGL(optim_guard_decide_groups_kernel, dim3(1), dim3(GN_THREADS), 0, s, d);
    optim_groups_launch<true>(a, kind, ntiles, s);
    return launch_status("optim_step_groups_guarded");
}
