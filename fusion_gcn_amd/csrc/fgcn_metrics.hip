// Classification metrics on the device (include/fgcn.h, fgcn_classify_update): per batch ONE launch adds the confusion matrix, the
// top-1 / top-k hit counts, the ignored / invalid / dropped row counts and the loss term to a caller-owned state buffer and stores
// the per-row argmax.  Rows number in the tens to hundreds and classes are at most a few hundred: a wave per row, lane-strided
// classes, wave reductions; counters are summed per wave in registers and added with integer atomics (exact in any order).
#include <climits>

#include "fgcn_common.hpp"

namespace fgcn {

constexpr int CLS_WAVES = 4;          // rows in flight per workgroup
constexpr int CLS_MAX_BLOCKS = 64;

// torch's order of floats: NaN above every number and equal to NaN
__device__ __forceinline__ bool cls_gt(float a, float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool cls_eq(float a, float b) { return a == b || (a != a && b != b); }

__global__ __launch_bounds__(64 * CLS_WAVES) void classify_update_kernel(const float* logits, const long long* labels,
                                                                         const float* loss, unsigned long long* words, int* confusion,
                                                                         int* pred_out, long long pred_offset, long long pred_capacity,
                                                                         int rows, int classes, int ld, int k) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * CLS_WAVES + (threadIdx.x >> 6), nwaves = gridDim.x * CLS_WAVES;
    unsigned examples = 0, top1 = 0, topk = 0, ignored = 0, invalid = 0, dropped = 0;      // wave-uniform
    for (int r = wave; r < rows; r += nwaves) {
        const float* z = logits + (long long)r * ld;
        const long long y = labels[r];
        const bool valid = y >= 0 && y < classes;
        const int yi = valid ? (int)y : 0;           // the only index ever derived from a label
        const float zy = z[yi];
        float bv = 0.f;
        int bi = INT_MAX, above = 0;
        for (int c = lane; c < classes; c += 64) {
            const float v = z[c];
            if (bi == INT_MAX || cls_gt(v, bv)) bv = v, bi = c;
            above += (cls_gt(v, zy) || (c < yi && cls_eq(v, zy))) ? 1 : 0;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            above += __shfl_xor(above, m);
            if (oi != INT_MAX && (bi == INT_MAX || cls_gt(ov, bv) || (cls_eq(ov, bv) && oi < bi))) bv = ov, bi = oi;
        }
        if (valid) {
            ++examples;
            top1 += bi == yi ? 1 : 0;
            topk += above < k ? 1 : 0;
            if (lane == 0) atomicAdd(&confusion[yi * classes + bi], 1);
        } else if (y == -100) {
            ++ignored;
        } else {
            ++invalid;
        }
        if (pred_out) {
            const long long slot = pred_offset + r;
            if (slot < pred_capacity) {
                if (lane == 0) pred_out[slot] = valid ? bi : -1;
            } else {
                ++dropped;
            }
        }
    }
    if (lane == 0) {
        if (examples) atomicAdd(&words[FGCN_CLS_EXAMPLES], (unsigned long long)examples);
        if (top1) atomicAdd(&words[FGCN_CLS_TOP1], (unsigned long long)top1);
        if (topk) atomicAdd(&words[FGCN_CLS_TOPK], (unsigned long long)topk);
        if (ignored) atomicAdd(&words[FGCN_CLS_IGNORED], (unsigned long long)ignored);
        if (invalid) atomicAdd(&words[FGCN_CLS_INVALID], (unsigned long long)invalid);
        if (dropped) atomicAdd(&words[FGCN_CLS_DROPPED], (unsigned long long)dropped);
    }
    if (loss && blockIdx.x == 0 && threadIdx.x == 0) {          // the one float of the state: one addition per call
        double* loss_sum = reinterpret_cast<double*>(words + FGCN_CLS_LOSS_SUM);
        *loss_sum += (double)loss[0] * (double)rows;
        words[FGCN_CLS_LOSS_ITEMS] += (unsigned long long)rows;
    }
}

}  // namespace fgcn

using namespace fgcn;

extern "C" long long fgcn_classify_state_bytes(int classes) {
    if (classes < 1 || classes > FGCN_CLS_MAX_CLASSES) return 0;
    const long long bytes = 8ll * FGCN_CLS_WORDS + 4ll * classes * classes;
    return (bytes + 7) / 8 * 8;
}

extern "C" int fgcn_classify_update(const float* logits, const long long* labels, const float* loss, void* state, int* pred_out,
                                    long long pred_offset, long long pred_capacity, int rows, int classes, int ld, int k,
                                    void* stream) {
    FGCN_REQUIRE(logits && labels && state, FGCN_E_BADARG, "classify_update: null pointer");
    FGCN_REQUIRE(rows > 0, FGCN_E_BADARG, "classify_update: bad row count rows=%d", rows);
    FGCN_REQUIRE(classes > 0 && classes <= FGCN_CLS_MAX_CLASSES, FGCN_E_BADARG, "classify_update: bad class count classes=%d (1..%d)",
                 classes, FGCN_CLS_MAX_CLASSES);
    FGCN_REQUIRE(ld >= classes, FGCN_E_BADARG, "classify_update: bad row stride ld=%d < classes=%d", ld, classes);
    FGCN_REQUIRE(k >= 1 && k <= classes, FGCN_E_BADARG, "classify_update: bad k=%d (1..classes=%d)", k, classes);
    FGCN_REQUIRE(pred_offset >= 0 && pred_capacity >= 0, FGCN_E_BADARG, "classify_update: negative pred_offset=%lld or pred_capacity=%lld",
                 pred_offset, pred_capacity);
    FGCN_REQUIRE(((uintptr_t)state & 7) == 0, FGCN_E_ALIGN, "classify_update: state must be 8-byte aligned");
    unsigned long long* words = static_cast<unsigned long long*>(state);
    int* confusion = reinterpret_cast<int*>(words + FGCN_CLS_WORDS);
    const long long blocks = cdiv(rows, CLS_WAVES);
    hipLaunchKernelGGL(classify_update_kernel, dim3((unsigned)(blocks < CLS_MAX_BLOCKS ? blocks : CLS_MAX_BLOCKS)), dim3(64 * CLS_WAVES), 0,
                       (hipStream_t)stream, logits, labels, loss, words, confusion, pred_out, pred_offset, pred_capacity, rows, classes, ld,
                       k);
    return launch_status("classify_update");
}
