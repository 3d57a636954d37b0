// First and second moments of the posterior mean over a validation epoch (the latent-space analysis of rave/model.py:463-481:
// `z = cat(z, 0); z = rearrange(z, "b c t -> (b t) c"); z.mean(0); PCA(...).fit(z)`).  Plumbing beside the hot path: a
// validation set is 1e4 - 1e5 rows of <= 128 channels.  What matters is that the result is exact, has one summation order and is
// read in the layout validation_step returns (batch, channels, time), time innermost: the rearrange is addressing.
//
//   acc[0]            += B * T                         (the row count, exact in f64)
//   acc[1 + i]        += sum_{b,t} z[b,i,t]
//   acc[1 + C + i*C+j] += sum_{b,t} z[b,i,t] * z[b,j,t]   (the full matrix, both triangles computed the same way)
//
// f64 throughout: the product of two f32 values is exact in f64 (24 + 24 <= 53 bits), so the only rounding is that of the
// additions.  No atomics: the (b, t) pairs are cut into chunks of kLsT time steps of one batch entry, the chunks into
// kLsMaxSlices contiguous runs -- a function of (B, T) only --, every workgroup adds one run into its own partial in the
// workspace in ascending (chunk, t) order, and a second launch adds the partials to the accumulator in slice order.
#include "common.hpp"

namespace {

constexpr int kLsMaxC = 128;
constexpr int kLsTile = 32;         // output tile: kLsTile x kLsTile entries of the outer product, 2 x 2 per thread
constexpr int kLsT = 64;            // time steps staged per chunk
constexpr int kLsMaxSlices = 64;

struct LsPlan {
    int chunks_per_b, n_chunks, slices, tiles;
    int64_t entries;                // C + C * C doubles per partial
};

LsPlan ls_plan(int B, int C, int T) {
    LsPlan p;
    p.chunks_per_b = (T + kLsT - 1) / kLsT;
    p.n_chunks = B * p.chunks_per_b;
    p.slices = p.n_chunks < kLsMaxSlices ? p.n_chunks : kLsMaxSlices;
    p.tiles = (C + kLsTile - 1) / kLsTile;
    p.entries = (int64_t)C + (int64_t)C * C;
    return p;
}

// grid = (tiles * tiles, slices); partial layout per slice: sum[C] | outer[C * C]
__global__ __launch_bounds__(256) void latent_moments_partial_kernel(const float* __restrict__ z, int C, int T, int chunks_per_b,
                                                                       int n_chunks, int tiles, double* __restrict__ part) {
    __shared__ float sa[kLsTile][kLsT + 1];
    __shared__ float sb[kLsTile][kLsT + 1];
    const int ti = (int)blockIdx.x / tiles, tj = (int)blockIdx.x % tiles;
    const int slice = blockIdx.y, slices = gridDim.y;
    const int c_begin = (int)((int64_t)slice * n_chunks / slices), c_end = (int)((int64_t)(slice + 1) * n_chunks / slices);
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, s0 = 0.0, s1 = 0.0;
    const bool sums = (tj == 0 && tx == 0);
    for (int ch = c_begin; ch < c_end; ++ch) {
        const int b = ch / chunks_per_b, t0 = (ch % chunks_per_b) * kLsT;
        const float* __restrict__ zb = z + (int64_t)b * C * T;
        for (int k = threadIdx.x; k < kLsTile * kLsT; k += 256) {
            const int r = k / kLsT, t = k % kLsT;
            const int ci = ti * kLsTile + r, cj = tj * kLsTile + r;
            const bool tin = t0 + t < T;
            sa[r][t] = (tin && ci < C) ? zb[(int64_t)ci * T + t0 + t] : 0.f;
            sb[r][t] = (tin && cj < C) ? zb[(int64_t)cj * T + t0 + t] : 0.f;
        }
        __syncthreads();
        for (int t = 0; t < kLsT; ++t) {      // rows past T are zeros: they add +0.0
            const double x0 = (double)sa[2 * ty][t], x1 = (double)sa[2 * ty + 1][t];
            const double y0 = (double)sb[2 * tx][t], y1 = (double)sb[2 * tx + 1][t];
            a00 += x0 * y0;
            a01 += x0 * y1;
            a10 += x1 * y0;
            a11 += x1 * y1;
            if (sums) {
                s0 += x0;
                s1 += x1;
            }
        }
        __syncthreads();
    }
    double* __restrict__ p = part + (int64_t)slice * ((int64_t)C + (int64_t)C * C);
    const int i0 = ti * kLsTile + 2 * ty, j0 = tj * kLsTile + 2 * tx;
    if (i0 < C) {
        if (j0 < C) p[C + (int64_t)i0 * C + j0] = a00;
        if (j0 + 1 < C) p[C + (int64_t)i0 * C + j0 + 1] = a01;
        if (sums) p[i0] = s0;
    }
    if (i0 + 1 < C) {
        if (j0 < C) p[C + (int64_t)(i0 + 1) * C + j0] = a10;
        if (j0 + 1 < C) p[C + (int64_t)(i0 + 1) * C + j0 + 1] = a11;
        if (sums) p[i0 + 1] = s1;
    }
}

__global__ __launch_bounds__(256) void latent_moments_add_kernel(const double* __restrict__ part, int slices, int64_t entries,
                                                                   double rows, double* __restrict__ acc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) acc[0] += rows;
    if (e >= entries) return;
    double v = acc[1 + e];
    for (int s = 0; s < slices; ++s) v += part[(int64_t)s * entries + e];
    acc[1 + e] = v;
}

int ls_check_sizes(const char* who, int32_t B, int32_t C, int32_t T) {
    RH_REQUIRE(B >= 1 && C >= 1 && T >= 1, RH_ERR_INVALID, "%s: batch %d x %d channels x %d steps (all must be >= 1)", who, (int)B,
               (int)C, (int)T);
    RH_REQUIRE(C <= kLsMaxC, RH_ERR_INVALID, "%s: %d channels (at most %d)", who, (int)C, kLsMaxC);
    RH_REQUIRE((int64_t)B * ((int64_t)T + kLsT) < (int64_t)0x7fffffff, RH_ERR_INVALID, "%s: batch %d x %d steps exceeds 32-bit row indexing",
               who, (int)B, (int)T);
    return RH_OK;
}

}  // namespace

extern "C" int rh_latent_moments_supported(int32_t channels) { return channels >= 1 && channels <= kLsMaxC ? 1 : 0; }

extern "C" int rh_latent_moments_workspace_bytes(int32_t batch, int32_t channels, int32_t t_len, int64_t* bytes) {
    if (int e = ls_check_sizes("latent_moments_workspace_bytes", batch, channels, t_len)) return e;
    RH_REQUIRE(bytes, RH_ERR_INVALID, "latent_moments_workspace_bytes: null result pointer");
    const LsPlan p = ls_plan(batch, channels, t_len);
    *bytes = (int64_t)sizeof(double) * p.slices * p.entries;
    return RH_OK;
}

extern "C" int rh_latent_moments_acc_f64(const float* mean, int32_t batch, int32_t channels, int32_t t_len, double* acc,
                                         void* workspace, rh_stream_t stream) {
    if (int e = ls_check_sizes("latent_moments_acc", batch, channels, t_len)) return e;
    RH_REQUIRE(mean && acc && workspace, RH_ERR_INVALID, "latent_moments_acc: null pointer");
    RH_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)workspace & 7) == 0, RH_ERR_INVALID,
               "latent_moments_acc: accumulator and workspace must be 8-byte aligned");
    const LsPlan p = ls_plan(batch, channels, t_len);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(latent_moments_partial_kernel, dim3((unsigned)(p.tiles * p.tiles), (unsigned)p.slices), dim3(256), 0,
                       (hipStream_t)stream, mean, (int)channels, (int)t_len, p.chunks_per_b, p.n_chunks, p.tiles, part);
    if (int e = rh_check_launch("latent_moments_partial")) return e;
    hipLaunchKernelGGL(latent_moments_add_kernel, dim3((unsigned)((p.entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       part, p.slices, p.entries, (double)((int64_t)batch * t_len), acc);
    return rh_check_launch("latent_moments_add");
}
