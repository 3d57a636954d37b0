// Exponential average of every parameter tensor, and the exchange of averages and parameters around a validation epoch, in a
// few launches (`rave train --ema f`: scripts/train.py:81-120 -- the EMA callback's on_train_batch_end, :88-96, and
// swap_weights, :98-102).  Plumbing beside the hot path, on the pattern of adam.hip (multi_tensor.hpp): the table travels BY
// VALUE in the kernel arguments (<= 64 tensors per launch), every workgroup takes 2048 elements of one tensor with 16-byte
// accesses; 12 bytes of traffic per parameter for the update, 16 for the swap.
//
//   update:  w = w * f + p * g        f = (float)factor, g = (float)(1.0 - factor)
//
// THREE separately rounded f32 operations, as the reference's `w * factor + p * (1 - factor)` evaluates them (two tensor-by-
// Python-scalar multiplications -- the scalar is rounded to f32 once, the subtraction happens in double before that -- and
// one addition): any contraction into an FMA changes up to a quarter of the elements in the last bit.  hipcc contracts by
// default and __fmul_rn / __fadd_rn are plain operators in this toolchain, so the arithmetic sits under `fp contract(off)`.
#include <cmath>
#include "multi_tensor.hpp"

namespace {

struct PairTable {
    float* a[kMtItems];
    float* b[kMtItems];
    int blk_begin[kMtItems + 1];          // prefix of workgroups
    int n[kMtItems];
    int count;
};

__device__ __forceinline__ float ema_one(float w, float p, float f, float g) {
#pragma clang fp contract(off)
    const float wf = w * f;
    const float pg = p * g;
    return wf + pg;
}

__global__ __launch_bounds__(256) void ema_update_kernel(const PairTable tb, float f, float g) {
    RH_MT_FIND(tb, lo)
    const int n = tb.n[lo];
    const int off = ((int)blockIdx.x - tb.blk_begin[lo]) * kMtElems;
    float* __restrict__ w = tb.a[lo];
    const float* __restrict__ p = tb.b[lo];
    const bool vec = ((((uintptr_t)w | (uintptr_t)p) & 15) == 0);
#pragma unroll
    for (int j = 0; j < kMtElems / 1024; ++j) {
        const int i = off + j * 1024 + 4 * threadIdx.x;
        if (vec && i + 3 < n) {
            f32x4 ww = *reinterpret_cast<const f32x4*>(w + i);
            const f32x4 pp = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) ww[k] = ema_one(ww[k], pp[k], f, g);
            *reinterpret_cast<f32x4*>(w + i) = ww;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) w[i + k] = ema_one(w[i + k], p[i + k], f, g);
        }
    }
}

__global__ __launch_bounds__(256) void swap_kernel(const PairTable tb) {
    RH_MT_FIND(tb, lo)
    const int n = tb.n[lo];
    const int off = ((int)blockIdx.x - tb.blk_begin[lo]) * kMtElems;
    float* __restrict__ a = tb.a[lo];
    float* __restrict__ b = tb.b[lo];
    const bool vec = ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
#pragma unroll
    for (int j = 0; j < kMtElems / 1024; ++j) {
        const int i = off + j * 1024 + 4 * threadIdx.x;
        if (vec && i + 3 < n) {
            const f32x4 aa = *reinterpret_cast<const f32x4*>(a + i);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(b + i);
            *reinterpret_cast<f32x4*>(a + i) = bb;
            *reinterpret_cast<f32x4*>(b + i) = aa;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) {
                    const float x = a[i + k], y = b[i + k];
                    a[i + k] = y;
                    b[i + k] = x;
                }
        }
    }
}

// everything a table must satisfy, checked for the WHOLE table before the first launch
int pair_table_check(const char* who, const rh_pair_item* items, int32_t n_items) {
    RH_REQUIRE(n_items >= 0, RH_ERR_INVALID, "%s: negative item count %d", who, (int)n_items);
    RH_REQUIRE(n_items == 0 || items, RH_ERR_INVALID, "%s: null table", who);
    for (int i = 0; i < n_items; ++i) {
        const rh_pair_item& it = items[i];
        RH_REQUIRE(it.n >= 0 && it.n < 0x7fffffffl, RH_ERR_INVALID, "%s: item %d: bad element count %lld", who, i, (long long)it.n);
        if (it.n == 0) continue;
        RH_REQUIRE(it.a && it.b, RH_ERR_INVALID, "%s: item %d: null pointer", who, i);
        RH_REQUIRE(it.a != it.b, RH_ERR_INVALID, "%s: item %d: both sides are the same tensor", who, i);
    }
    return RH_OK;
}

template <typename Launch>
int pair_table_run(const char* what, const rh_pair_item* items, int32_t n_items, Launch launch) {
    for (int i = 0; i < n_items;) {
        PairTable tb;
        const int blk = rh_mt_fill(tb, items, n_items, i, [](PairTable& t, int c, const rh_pair_item& it, int) {
            t.a[c] = it.a; t.b[c] = it.b;
        });
        if (blk == 0) continue;
        launch(tb, dim3((unsigned)blk));
        if (int e = rh_check_launch(what)) return e;
    }
    return RH_OK;
}

}  // namespace

extern "C" int rh_ema_update_f32(const rh_pair_item* items, int32_t n_items, double factor, rh_stream_t stream) {
    if (int e = pair_table_check("ema_update", items, n_items)) return e;
    RH_REQUIRE(std::isfinite(factor) && factor >= 0.0 && factor <= 1.0, RH_ERR_INVALID, "ema_update: factor %g outside [0, 1]", factor);
    const float f = (float)factor, g = (float)(1.0 - factor);
    return pair_table_run("ema_update", items, n_items, [&](const PairTable& tb, dim3 grid) {
        hipLaunchKernelGGL(ema_update_kernel, grid, dim3(256), 0, (hipStream_t)stream, tb, f, g);
    });
}

extern "C" int rh_swap_f32(const rh_pair_item* items, int32_t n_items, rh_stream_t stream) {
    if (int e = pair_table_check("swap", items, n_items)) return e;
    return pair_table_run("swap", items, n_items, [&](const PairTable& tb, dim3 grid) {
        hipLaunchKernelGGL(swap_kernel, grid, dim3(256), 0, (hipStream_t)stream, tb);
    });
}
