// The GAN objectives of rave/core.py:151-170 (hinge_gan, ls_gan, nonsaturating_gan) summed over the discriminator heads as
// rave/model.py:354-376 accumulates them, with the logged pred_real / pred_fake of the same loop: for every head, with r a real
// and f a fake score and means over the n scores of one half,
//     hinge            dis = mean(relu(1 - r) + relu(1 + f))            adv = mean(-f)
//     least squares    dis = mean((r - 1)^2 + f^2)                      adv = mean((f - 1)^2)
//     non-saturating   p = clamp(sigmoid(s), 1e-7, 1 - 1e-7) (bounds rounded to f32)
//                      dis = mean(-(log p_r + log(1 - p_f)))            adv = mean(-log p_f)
//     pred_real = mean(r),  pred_fake = mean(f)
// and out = the four sums over the heads.  As ATen ops this is ~10 small dispatches per head each way (two 1 +- s, two relu, an
// add, the means, a negation, the scalar accumulations; backward their mirror image and the cat of the two half gradients).
// Here: all heads of a step travel in ONE table in the kernel arguments (capturable), forward = per-workgroup partials + one
// ordered finalize that also forms the four totals, backward = one launch writing d_real and d_fake of every head.  No atomics:
// every sum has one fixed order, and a thread adds the same elements in the same order whether it loads them as one 16-byte
// vector or one by one, so the bits do not depend on the alignment of the pointers either.
// The gates are ATen's: relu passes its gradient where its argument is > 0; clamp passes it where lo <= p <= hi (the bounds
// included), so the non-saturating gradient is exactly 0 wherever the clamp changed the value.
#include "common.hpp"

namespace {

constexpr int kGan = 80;                    // heads per call: the size of one kernel-argument table
constexpr int kGanChunk = 4096;             // scores of one half per workgroup
constexpr int kGanHinge = 0, kGanLs = 1, kGanNonSat = 2;

struct GanTable {
    const float* r[kGan];
    const float* f[kGan];
    float* dr[kGan];
    float* df[kGan];
    long n[kGan];
    int blk_begin[kGan + 1];
    int count;
    int mode;
};

__device__ __forceinline__ int gan_find(const GanTable& tb, int blk) {
    int lo = 0, hi = tb.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb.blk_begin[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float gan_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// up to four consecutive scores of one thread: one 16-byte load where `vec`, else `cnt` scalar loads (the rest stays 0)
__device__ __forceinline__ f32x4 gan_load(const float* __restrict__ p, int cnt, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < cnt; ++k) v[k] = p[k];
    return v;
}

__device__ __forceinline__ void gan_store(float* __restrict__ p, const f32x4 v, int cnt, bool vec) {
    if (vec) { *reinterpret_cast<f32x4*>(p) = v; return; }
    for (int k = 0; k < cnt; ++k) p[k] = v[k];
}

// clamp bounds of rave/core.py:166-167 as an f32 run takes them: the double constants rounded to f32
__device__ __forceinline__ float gan_lo() { return (float)1e-7; }
__device__ __forceinline__ float gan_hi() { return (float)(1.0 - 1e-7); }

__device__ __forceinline__ float gan_sigmoid(float s) { return 1.f / (1.f + expf(-s)); }
__device__ __forceinline__ float gan_clamp(float y) { return fminf(fmaxf(y, gan_lo()), gan_hi()); }

// part[4 blk + {0, 1, 2, 3}] = this workgroup's sums of the dis terms, the adv terms, r and f
__global__ __launch_bounds__(256) void gan_partials_kernel(const GanTable tb, float* __restrict__ part) {
    __shared__ float red[4][4];
    const int it = gan_find(tb, blockIdx.x);
    const long n = tb.n[it];
    const long e0 = (long)(blockIdx.x - tb.blk_begin[it]) * kGanChunk;
    const float* __restrict__ r = tb.r[it];
    const float* __restrict__ f = tb.f[it];
    const bool vec = (n & 3) == 0 && ((((uintptr_t)r) | ((uintptr_t)f)) & 15) == 0;
    const int mode = tb.mode;
    float sd = 0.f, sa = 0.f, sr = 0.f, sf = 0.f;
#pragma unroll
    for (int u = 0; u < kGanChunk / 1024; ++u) {
        const long e = e0 + u * 1024 + 4 * threadIdx.x;
        if (e < n) {
            const int cnt = (n - e) < 4 ? (int)(n - e) : 4;
            const f32x4 a = gan_load(r + e, cnt, vec), b = gan_load(f + e, cnt, vec);
            for (int k = 0; k < cnt; ++k) {
                const float x = a[k], y = b[k];
                if (mode == kGanHinge) {
                    sd += fmaxf(1.f - x, 0.f) + fmaxf(1.f + y, 0.f);
                    sa += -y;
                } else if (mode == kGanLs) {
                    sd += (x - 1.f) * (x - 1.f) + y * y;
                    sa += (y - 1.f) * (y - 1.f);
                } else {
                    const float pr = gan_clamp(gan_sigmoid(x)), pf = gan_clamp(gan_sigmoid(y));
                    sd += -(logf(pr) + logf(1.f - pf));
                    sa += -logf(pf);
                }
                sr += x;
                sf += y;
            }
        }
    }
    sd = gan_wave_sum(sd); sa = gan_wave_sum(sa); sr = gan_wave_sum(sr); sf = gan_wave_sum(sf);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = sd; red[wave][1] = sa; red[wave][2] = sr; red[wave][3] = sf; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[4l * blockIdx.x + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// ONE workgroup: wave w takes the heads w, w + 4, ... (their partials in order -> sums[4 i + k] = the head's four means), then
// thread k < 4 adds the heads' means in head order -> out[k]
__global__ __launch_bounds__(256) void gan_finalize_kernel(const GanTable tb, const float* __restrict__ part, float* __restrict__ sums,
                                                           float* __restrict__ out) {
    __shared__ float head[kGan][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int it = wave; it < tb.count; it += 4) {
        const int b0 = tb.blk_begin[it], b1 = tb.blk_begin[it + 1];
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = b0 + lane; b < b1; b += 64) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += part[4l * b + k];
        }
        const float fn = (float)tb.n[it];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = gan_wave_sum(s[k]);
            if (lane == 0) { const float m = t / fn; head[it][k] = m; sums[4 * it + k] = m; }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float t = 0.f;
        for (int it = 0; it < tb.count; ++it) t += head[it][threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// d_real = g_dis d dis / d r,  d_fake = g_dis d dis / d f + g_adv d adv / d f, the 1 / n of the means included
__global__ __launch_bounds__(256) void gan_bwd_kernel(const GanTable tb, const float* __restrict__ gout) {
    const int it = gan_find(tb, blockIdx.x);
    const long n = tb.n[it];
    const long e0 = (long)(blockIdx.x - tb.blk_begin[it]) * kGanChunk;
    const float* __restrict__ r = tb.r[it];
    const float* __restrict__ f = tb.f[it];
    float* __restrict__ dr = tb.dr[it];
    float* __restrict__ df = tb.df[it];
    const bool vec = (n & 3) == 0 && ((((uintptr_t)r) | ((uintptr_t)f) | ((uintptr_t)dr) | ((uintptr_t)df)) & 15) == 0;
    const int mode = tb.mode;
    const float gd = gout[0] / (float)n, ga = gout[1] / (float)n;
#pragma unroll
    for (int u = 0; u < kGanChunk / 1024; ++u) {
        const long e = e0 + u * 1024 + 4 * threadIdx.x;
        if (e < n) {
            const int cnt = (n - e) < 4 ? (int)(n - e) : 4;
            const f32x4 a = gan_load(r + e, cnt, vec), b = gan_load(f + e, cnt, vec);
            f32x4 da = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < cnt; ++k) {
                const float x = a[k], y = b[k];
                if (mode == kGanHinge) {
                    da[k] = (1.f - x) > 0.f ? -gd : 0.f;
                    db[k] = ((1.f + y) > 0.f ? gd : 0.f) - ga;
                } else if (mode == kGanLs) {
                    da[k] = gd * (2.f * (x - 1.f));
                    db[k] = gd * (2.f * y) + ga * (2.f * (y - 1.f));
                } else {
                    // with q = sigmoid(s) inside the clamp: d(-log q)/ds = -(1 - q) = -e / (1 + e), e = exp(-s) (no cancellation
                    // near q = 1), and d(-log(1 - q))/ds = q; outside the clamp (ATen's gate: lo <= q <= hi passes) exactly 0
                    const float ex = expf(-x), ey = expf(-y);
                    const float qx = 1.f / (1.f + ex), qy = 1.f / (1.f + ey);
                    const bool inx = qx >= gan_lo() && qx <= gan_hi(), iny = qy >= gan_lo() && qy <= gan_hi();
                    da[k] = inx ? -gd * (ex / (1.f + ex)) : 0.f;
                    db[k] = iny ? gd * qy - ga * (ey / (1.f + ey)) : 0.f;
                }
            }
            gan_store(dr + e, da, cnt, vec);
            gan_store(df + e, db, cnt, vec);
        }
    }
}

int gan_blocks(const rh_gan_item* items, int n, long* blocks) {
    RH_REQUIRE(items, RH_ERR_INVALID, "gan_loss: null item table");
    RH_REQUIRE(n >= 1 && n <= kGan, RH_ERR_UNSUPPORTED, "gan_loss: 1 ... %d heads per call, got %d", kGan, n);
    long blk = 0;
    for (int i = 0; i < n; ++i) {
        RH_REQUIRE(items[i].n > 0, RH_ERR_INVALID, "gan_loss: item %d has n = %lld", i, (long long)items[i].n);
        RH_REQUIRE(items[i].n < (1ll << 40), RH_ERR_UNSUPPORTED, "gan_loss: item %d is too large", i);
        blk += (items[i].n + kGanChunk - 1) / kGanChunk;
        RH_REQUIRE(blk < 0x7fffffffl, RH_ERR_UNSUPPORTED, "gan_loss: too many scores for one call");
    }
    *blocks = blk;
    return RH_OK;
}

int gan_fill(const rh_gan_item* items, int n, int mode, bool need_grad, GanTable* tb) {
    long blocks = 0;
    if (int e = gan_blocks(items, n, &blocks)) return e;
    RH_REQUIRE(mode == kGanHinge || mode == kGanLs || mode == kGanNonSat, RH_ERR_UNSUPPORTED, "gan_loss: unknown mode %d", mode);
    long blk = 0;
    for (int i = 0; i < n; ++i) {
        RH_REQUIRE(items[i].real && items[i].fake && (!need_grad || (items[i].d_real && items[i].d_fake)), RH_ERR_INVALID,
                   "gan_loss: null pointer in item %d", i);
        tb->r[i] = items[i].real; tb->f[i] = items[i].fake; tb->dr[i] = items[i].d_real; tb->df[i] = items[i].d_fake;
        tb->n[i] = items[i].n;
        tb->blk_begin[i] = (int)blk;
        blk += (items[i].n + kGanChunk - 1) / kGanChunk;
    }
    tb->blk_begin[n] = (int)blk;
    tb->count = n;
    tb->mode = mode;
    return RH_OK;
}

}  // namespace

extern "C" int rh_gan_loss_supported(int32_t mode, int32_t n_items) {
    return (mode == kGanHinge || mode == kGanLs || mode == kGanNonSat) && n_items >= 1 && n_items <= kGan;
}

extern "C" int64_t rh_gan_loss_workspace_bytes(const rh_gan_item* items, int32_t n_items) {
    long blocks = 0;
    if (gan_blocks(items, n_items, &blocks)) return -1;
    return (int64_t)blocks * 4 * (int64_t)sizeof(float);
}

extern "C" int rh_gan_loss_fwd_f32(const rh_gan_item* items, int32_t n_items, int32_t mode, void* workspace, int64_t workspace_bytes,
                                   float* sums, float* out, rh_stream_t stream) {
    GanTable tb;
    if (int e = gan_fill(items, n_items, mode, false, &tb)) return e;
    RH_REQUIRE(workspace && sums && out, RH_ERR_INVALID, "gan_loss_fwd: null pointer");
    RH_REQUIRE(workspace_bytes >= (int64_t)tb.blk_begin[n_items] * 4 * (int64_t)sizeof(float), RH_ERR_WORKSPACE,
               "gan_loss_fwd: workspace too small");
    hipLaunchKernelGGL(gan_partials_kernel, dim3((unsigned)tb.blk_begin[n_items]), dim3(256), 0, (hipStream_t)stream, tb, (float*)workspace);
    if (int e = rh_check_launch("gan_loss_partials")) return e;
    hipLaunchKernelGGL(gan_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tb, (const float*)workspace, sums, out);
    return rh_check_launch("gan_loss_finalize");
}

extern "C" int rh_gan_loss_bwd_f32(const rh_gan_item* items, int32_t n_items, int32_t mode, const float* grad_out, rh_stream_t stream) {
    GanTable tb;
    if (int e = gan_fill(items, n_items, mode, true, &tb)) return e;
    RH_REQUIRE(grad_out, RH_ERR_INVALID, "gan_loss_bwd: null pointer");
    hipLaunchKernelGGL(gan_bwd_kernel, dim3((unsigned)tb.blk_begin[n_items]), dim3(256), 0, (hipStream_t)stream, tb, grad_out);
    return rh_check_launch("gan_loss_bwd");
}
