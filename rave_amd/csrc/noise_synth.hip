// Filtered-noise synthesis of the noise generators (rave/blocks.py:230-240, 282-292 over rave/core.py:23-24, 48-81): everything
// between the branch's last convolution and the (B, D, T N) signal that is added to the waveform, one launch per direction.
//
// Both transforms of the reference are linear maps of tiny fixed length, so neither needs an FFT:
//   * amp_to_impulse_response (irfft, roll, Hann, pad / crop, roll) is ir = M amp with a constant (N x nb) matrix M that depends
//     on (nb, N) only -- rh_noise_synth_table_f32 builds it in f64, the crop of a filter longer than N included;
//   * fft_convolve zero-pads both operands to 2 N, so the circular wrap never reaches the N samples it keeps:
//     out[n] = sum_{k <= n} noise[k] ir[n - k].
// Per (b, d, t):  amp_j = 2 sigmoid(h - 5)^2.3 + 1e-7,  ir = M amp,  out = noise * ir (causal, cut to N); the backward pass is
// the transpose of each step, d_ir[j] = sum_{n >= j} gout[n] noise[n - j], d_amp = M^T d_ir, gh = d_amp 4.6 s^2.3 (1 - s).
//
//   * a workgroup owns, for one b, `dt` channels x `tt` consecutive frames ("items").  h is read along t, the noise along
//     (d, n) and out / gout along (t, n): the tile makes each of these runs at least 64 bytes, the exchange between the three
//     orders goes through LDS (rows padded to an odd length), and out / gh are written by the threads in memory order.
//   * every access to global memory is one float: any 4-byte aligned pointer works.
//   * each (b, d, t) is computed by one workgroup in one fixed order -- no atomics, no workspace, the same bits every run.
#include <cmath>
#include <cstdint>
#include "common.hpp"

namespace {

constexpr int kMaxBands = 33, kMaxSize = 64;
constexpr int kThreads = 256;

struct NoiseGeom {
    int batch, d, t, nb, n;
    int dt, tt_log2;       // tile: dt channels x (1 << tt_log2) frames
    int ldm, ldn;          // LDS row lengths (odd) of the table (nb values) and of the per-item vectors (n values)
};

bool supported(int nb, int n) { return nb >= 2 && nb <= kMaxBands && n >= 1 && n <= kMaxSize; }

// Runs of >= 1 KB along out (tt n >= 256 floats) and >= 64 B along h (tt >= 16) and the noise (dt n >= 32 floats where d
// allows), at most 128 items: under 40 KB of LDS at every built size.
NoiseGeom make_geom(int batch, int d, int t, int nb, int n) {
    NoiseGeom g{batch, d, t, nb, n, 1, 4, nb | 1, n | 1};
    while ((n << g.tt_log2) < 256 && g.tt_log2 < 6) ++g.tt_log2;
    const int dt = rh_cdiv(32, n), cap = 128 >> g.tt_log2;
    g.dt = dt < cap ? dt : cap;
    if (g.dt > d) g.dt = d;
    return g;
}
int64_t grid_of(const NoiseGeom& g) {
    return (int64_t)g.batch * rh_cdiv(g.d, g.dt) * (int64_t)rh_cdiv(g.t, 1 << g.tt_log2);
}

// i = first, first + step, ... as (q, r) = (i / m, i % m) with one division at the start
struct DivStep {
    int q, r, dq, dr, m;
    __device__ DivStep(int first, int step, int m_) : q(first / m_), r(first % m_), dq(step / m_), dr(step % m_), m(m_) {}
    __device__ void next() {
        q += dq;
        r += dr;
        if (r >= m) { r -= m; ++q; }
    }
};

struct Tile {
    int b, d0, t0, tt, items;
    int nd_valid;                                   // channels of the tile inside d
    __device__ explicit Tile(const NoiseGeom& g) {
        tt = 1 << g.tt_log2;
        items = g.dt * tt;
        const int nt = (g.t + tt - 1) >> g.tt_log2, nd = (g.d + g.dt - 1) / g.dt;
        int id = blockIdx.x;
        t0 = (id % nt) << g.tt_log2;
        id /= nt;
        d0 = (id % nd) * g.dt;
        b = id / nd;
        nd_valid = g.d - d0 < g.dt ? g.d - d0 : g.dt;
    }
    // item = dl * tt + tl
    __device__ bool valid(const NoiseGeom& g, int dl, int tl) const { return dl < nd_valid && t0 + tl < g.t; }
    // offset of (b, d0 + dl, t0 + tl, 0) in out / gout (B, D, T, N)
    __device__ long out_at(const NoiseGeom& g, int dl, int tl) const {
        return (((long)b * g.d + d0 + dl) * g.t + t0 + tl) * g.n;
    }
    // offset of (b, (d0 + dl) nb + j, t0 + tl) in h / gh (B, D nb, T) for r = dl * nb + j
    __device__ long h_at(const NoiseGeom& g, int r, int tl) const {
        return (((long)b * g.d + d0) * g.nb + r) * g.t + t0 + tl;
    }
};

__device__ void load_table(const NoiseGeom& g, const float* __restrict__ table, float* s_m) {
    for (DivStep i(threadIdx.x, kThreads, g.nb); i.q < g.n; i.next()) s_m[i.q * g.ldm + i.r] = table[i.q * g.nb + i.r];
}
// noise (B, T, D, N) -> s[item][ldn]; the tile's slice of one frame is dt * n consecutive floats
__device__ void load_noise(const NoiseGeom& g, const Tile& tile, const float* __restrict__ noise, float* s) {
    for (DivStep i(threadIdx.x, kThreads, g.dt * g.n); i.q < tile.tt; i.next()) {
        const int tl = i.q, dl = i.r / g.n, k = i.r - dl * g.n;
        s[(dl * tile.tt + tl) * g.ldn + k] =
            tile.valid(g, dl, tl) ? noise[(((long)tile.b * g.t + tile.t0 + tl) * g.d + tile.d0) * g.n + i.r] : 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void noise_synth_fwd_kernel(const float* __restrict__ h, const float* __restrict__ noise,
                                                                   const float* __restrict__ table, float* __restrict__ out,
                                                                   const NoiseGeom g) {
    extern __shared__ float lds[];
    const Tile tile(g);
    const int tt = tile.tt, rows = g.dt * g.nb;
    float* s_m = lds;                               // [n][ldm]
    float* s_amp = s_m + g.n * g.ldm;               // [dl * nb + j][tt]
    float* s_noise = s_amp + rows * tt;             // [item][ldn]
    float* s_ir = s_noise + tile.items * g.ldn;     // [item][ldn]
    load_table(g, table, s_m);
    for (int i = threadIdx.x; i < rows * tt; i += kThreads) {
        const int r = i >> g.tt_log2, tl = i & (tt - 1);
        float a = 0.f;
        if (r < tile.nd_valid * g.nb && tile.t0 + tl < g.t) {
            const float s = 1.f / (1.f + expf(5.f - h[tile.h_at(g, r, tl)]));
            a = 2.f * powf(s, 2.3f) + 1e-7f;
        }
        s_amp[i] = a;
    }
    load_noise(g, tile, noise, s_noise);
    __syncthreads();
    for (DivStep i(threadIdx.x, kThreads, g.n); i.q < tile.items; i.next()) {
        const int dl = i.q >> g.tt_log2, tl = i.q & (tt - 1);
        const float* m = s_m + i.r * g.ldm;
        const float* a = s_amp + dl * g.nb * tt + tl;
        float acc = 0.f;
        for (int j = 0; j < g.nb; ++j) acc = fmaf(m[j], a[j * tt], acc);
        s_ir[i.q * g.ldn + i.r] = acc;
    }
    __syncthreads();
    for (DivStep i(threadIdx.x, kThreads, g.n); i.q < tile.items; i.next()) {
        const int dl = i.q >> g.tt_log2, tl = i.q & (tt - 1);
        if (!tile.valid(g, dl, tl)) continue;
        const float* x = s_noise + i.q * g.ldn;
        const float* ir = s_ir + i.q * g.ldn + i.r;
        float acc = 0.f;
        for (int k = 0; k <= i.r; ++k) acc = fmaf(x[k], ir[-k], acc);
        out[tile.out_at(g, dl, tl) + i.r] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void noise_synth_bwd_kernel(const float* __restrict__ h, const float* __restrict__ noise,
                                                                   const float* __restrict__ table,
                                                                   const float* __restrict__ gout, float* __restrict__ gh,
                                                                   const NoiseGeom g) {
    extern __shared__ float lds[];
    const Tile tile(g);
    const int tt = tile.tt, rows = g.dt * g.nb;
    float* s_m = lds;                               // [n][ldm]
    float* s_noise = s_m + g.n * g.ldm;             // [item][ldn]
    float* s_g = s_noise + tile.items * g.ldn;      // [item][ldn]
    float* s_dir = s_g + tile.items * g.ldn;        // [item][ldn]
    load_table(g, table, s_m);
    load_noise(g, tile, noise, s_noise);
    for (DivStep i(threadIdx.x, kThreads, g.n); i.q < tile.items; i.next()) {
        const int dl = i.q >> g.tt_log2, tl = i.q & (tt - 1);
        s_g[i.q * g.ldn + i.r] = tile.valid(g, dl, tl) ? gout[tile.out_at(g, dl, tl) + i.r] : 0.f;
    }
    __syncthreads();
    for (DivStep i(threadIdx.x, kThreads, g.n); i.q < tile.items; i.next()) {
        const float* x = s_noise + i.q * g.ldn;
        const float* go = s_g + i.q * g.ldn + i.r;
        float acc = 0.f;
        for (int k = 0; k < g.n - i.r; ++k) acc = fmaf(go[k], x[k], acc);
        s_dir[i.q * g.ldn + i.r] = acc;
    }
    __syncthreads();
    // r = dl * nb + j advances by kThreads / tt per step (tt <= 64 divides kThreads)
    DivStep rj(threadIdx.x >> g.tt_log2, kThreads >> g.tt_log2, g.nb);
    for (int i = threadIdx.x; i < rows * tt; i += kThreads, rj.next()) {
        const int tl = i & (tt - 1), dl = rj.q, j = rj.r;
        if (!tile.valid(g, dl, tl)) continue;
        const float* m = s_m + j;
        const float* di = s_dir + (dl * tt + tl) * g.ldn;
        float acc = 0.f;
        for (int n = 0; n < g.n; ++n) acc = fmaf(m[n * g.ldm], di[n], acc);
        const long at = tile.h_at(g, i >> g.tt_log2, tl);
        const float x = h[at] - 5.f;
        const float s = 1.f / (1.f + expf(-x)), c = 1.f / (1.f + expf(x));     // sigmoid and 1 - sigmoid, neither by subtraction
        gh[at] = acc * 4.6f * powf(s, 2.3f) * c;
    }
}

size_t lds_bytes(const NoiseGeom& g, bool bwd) {
    const int items = g.dt << g.tt_log2;
    const int per_item = bwd ? 3 * g.ldn : 2 * g.ldn + g.nb;
    return sizeof(float) * ((size_t)g.n * g.ldm + (size_t)items * per_item);
}

int check(const char* what, bool pointers, int32_t batch, int32_t d, int32_t t, int32_t nb, int32_t n) {
    RH_REQUIRE(pointers, RH_ERR_INVALID, "%s: null pointer", what);
    RH_REQUIRE(batch > 0 && d > 0 && t > 0, RH_ERR_INVALID, "%s: batch %d, channels %d, frames %d", what, batch, d, t);
    RH_REQUIRE(supported(nb, n), RH_ERR_UNSUPPORTED, "%s: %d noise bands, target size %d (built: 2..%d bands, size 1..%d)", what, nb,
               n, kMaxBands, kMaxSize);
    RH_REQUIRE(grid_of(make_geom(batch, d, t, nb, n)) <= 0x7fffffffll, RH_ERR_INVALID, "%s: too many tiles for one launch", what);
    return RH_OK;
}

}  // namespace

extern "C" int rh_noise_synth_supported(int32_t noise_bands, int32_t target_size) {
    return supported(noise_bands, target_size) ? 1 : 0;
}

extern "C" int rh_noise_synth_table_f32(int32_t noise_bands, int32_t target_size, float* table) {
    RH_REQUIRE(table, RH_ERR_INVALID, "noise_synth_table: null pointer");
    RH_REQUIRE(supported(noise_bands, target_size), RH_ERR_UNSUPPORTED, "noise_synth_table: %d noise bands, target size %d",
               noise_bands, target_size);
    const int nb = noise_bands, n = target_size, f = 2 * (nb - 1), half = nb - 1;      // f: length of irfft's output
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        const int m = (i + half) % n;               // the last roll, by -f / 2 on the padded / cropped length n
        for (int j = 0; j < nb; ++j) {
            double v = 0.;
            if (m < f) {                            // beyond f the pad's zeros
                const int p = (m + f - half) % f;   // the first roll, by f / 2 on length f
                const double win = 0.5 - 0.5 * cos(2. * pi * m / f);
                const double c = j == 0 ? 1. : j == nb - 1 ? (p & 1 ? -1. : 1.) : 2. * cos(2. * pi * ((j * p) % f) / f);
                v = win * c / f;
            }
            table[i * nb + j] = (float)v;
        }
    }
    return RH_OK;
}

extern "C" int rh_noise_synth_fwd_f32(const float* h, const float* noise, const float* table, int32_t batch, int32_t channels,
                                      int32_t t_len, int32_t noise_bands, int32_t target_size, float* out, rh_stream_t stream) {
    if (const int rc = check("noise_synth_fwd", h && noise && table && out, batch, channels, t_len, noise_bands, target_size)) return rc;
    const NoiseGeom g = make_geom(batch, channels, t_len, noise_bands, target_size);
    hipLaunchKernelGGL(noise_synth_fwd_kernel, dim3((unsigned)grid_of(g)), dim3(kThreads), lds_bytes(g, false), (hipStream_t)stream,
                       h, noise, table, out, g);
    return rh_check_launch("noise_synth_fwd");
}

extern "C" int rh_noise_synth_bwd_f32(const float* h, const float* noise, const float* table, const float* gout, int32_t batch,
                                      int32_t channels, int32_t t_len, int32_t noise_bands, int32_t target_size, float* gh,
                                      rh_stream_t stream) {
    if (const int rc = check("noise_synth_bwd", h && noise && table && gout && gh, batch, channels, t_len, noise_bands, target_size)) return rc;
    const NoiseGeom g = make_geom(batch, channels, t_len, noise_bands, target_size);
    hipLaunchKernelGGL(noise_synth_bwd_kernel, dim3((unsigned)grid_of(g)), dim3(kThreads), lds_bytes(g, true), (hipStream_t)stream,
                       h, noise, table, gout, gh, g);
    return rh_check_launch("noise_synth_bwd");
}
