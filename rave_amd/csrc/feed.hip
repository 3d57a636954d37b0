// GPU side of the training data feed (SURVEY.md section 8f "next" #4): one kernel per minibatch replaces the
// per-item CPU chain of rave/dataset.py:
//   int16 PCM -> float32 / (2^15 - 1)                      (AudioDataset.__getitem__, dataset.py:75-78)
//   RandomCrop(n_signal)                                   (transforms.py:96-106; crop points drawn by the host)
//   RandomApply(random_phase_mangle, p = .8)               (dataset.py:223-226,283-299: all-pass biquad with a random
//                                                           pole angle, scipy.signal.lfilter = direct form II transposed,
//                                                           evaluated in float64 like scipy does for float64 taps)
//   Dequantize(16): x += U[0,1) / 2^16, then float32       (transforms.py:109-115, dataset.py:246)
// At > 1e8 samples/s per GPU the 8-worker scipy chain cannot keep up; here a (clip, channel) row is one workgroup:
// 4096-sample chunks are staged in LDS, thread 0 advances the two-state recurrence, all threads add the noise and
// store.  The recurrence is sequential by nature (0.5 ms for 65536 samples) but rows run in parallel and the
// kernel is meant for a side stream, under the training step.
#include <algorithm>
#include "common.hpp"

namespace {

constexpr int kChunk = 4096;

__global__ __launch_bounds__(256) void feed_kernel(const int16_t* __restrict__ pcm, const int64_t* __restrict__ src_offset,
                                                   const double* __restrict__ coef, const float* __restrict__ noise,
                                                   int n_signal, double quant, float* __restrict__ out) {
    __shared__ double buf[kChunk];
    const int r = blockIdx.x;
    const int16_t* src = pcm + src_offset[r];
    const double b0 = coef[r * 5 + 0], b1 = coef[r * 5 + 1], b2 = coef[r * 5 + 2], a1 = coef[r * 5 + 3], a2 = coef[r * 5 + 4];
    const bool filt = b0 == b0;                 // NaN marks "transform not applied" (RandomApply miss)
    double z0 = 0.0, z1 = 0.0;
    for (int c0 = 0; c0 < n_signal; c0 += kChunk) {
        const int len = min(kChunk, n_signal - c0);
        for (int i = threadIdx.x; i < len; i += 256)
            buf[i] = (double)((float)src[c0 + i] / 32767.0f);          // float32 division, as the reference
        __syncthreads();
        if (filt && threadIdx.x == 0) {
            for (int i = 0; i < len; ++i) {
                const double x = buf[i];
                const double y = b0 * x + z0;
                z0 = b1 * x - a1 * y + z1;
                z1 = b2 * x - a2 * y;
                buf[i] = y;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < len; i += 256) {
            const long o = (long)r * n_signal + c0 + i;
            out[o] = (float)(buf[i] + (double)noise[o] * quant);
        }
        __syncthreads();
    }
}

// ---- the same chain with RandomPitch in front of the crop and RandomMute behind it ---------------------------------
//   RandomPitch(n_signal, [lo, hi])   (transforms.py:56-89: scipy.signal.resample_poly(item, up, down, padtype='mean') of
//                                      the WHOLE stored item, inserted at dataset.py:233-236)
//   RandomMute(prob)                  (transforms.py:168-177, configs/augmentations/mute.gin: the item times one Bernoulli draw)
// resample_poly in closed form, up / down reduced, m = max(up, down), H = 10 m, h = up * firwin(2H + 1, 1 / m, kaiser 5.0):
//   y[n] = mu + sum_k h[n down - k up + H] (x[k] - mu),   k in [ceil((n down - H) / up), floor((n down + H) / up)] and [0, L)
// with mu the mean of the whole item row.  Only the n_signal outputs inside the crop window are computed.  Per chunk the
// workgroup stages the input span those outputs reach (as float32: the reference's int16 / 32767 division, done once per
// input sample instead of once per tap) and every thread accumulates its outputs in float64, rounds once to float32 (the
// dtype the reference holds at this point) and hands the chunk to the all-pass / noise / store stages of feed_kernel.
// The taps sit in LDS phase-major -- hp[p * S + j] = h[p + j up], S odd -- so a thread walks one row with unit stride and
// the rows of a wave's <= 19 phases start on different banks (lanes on the same phase read the same address).
constexpr int kSpan = 6144;         // input samples staged per resampling pass (24 KB)
constexpr int kTapSlots = 448;      // >= up * (ceil((2H + 1) / up) | 1) for every up, down <= kMaxFactor (checked by the host)
constexpr int kMaxFactor = 19;

__host__ __device__ inline int feed_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}
__host__ __device__ inline int feed_tap_stride(int up, int H) { return ((2 * H + up) / up) | 1; }

__global__ __launch_bounds__(256) void feed_pitch_kernel(const int16_t* __restrict__ pcm, const rh_feed_pitch_row* __restrict__ rows,
                                                         const double* __restrict__ taps, const float* __restrict__ noise,
                                                         int n_signal, double quant, float* __restrict__ out) {
    __shared__ double buf[kChunk];
    __shared__ double hp[kTapSlots];
    __shared__ float span[kSpan];
    const int r = blockIdx.x;
    const rh_feed_pitch_row row = rows[r];
    if (row.mute) {                             // (x + noise) * 0
        for (int i = threadIdx.x; i < n_signal; i += 256) out[(long)r * n_signal + i] = 0.f;
        return;
    }
    const int g = feed_gcd(row.up, row.down);
    const int up = row.up / g, down = row.down / g;
    const bool pitched = up != down;
    const int H = 10 * max(up, down);
    const int S = feed_tap_stride(up, H);
    const int64_t L = row.length;
    const double mu = row.mean;
    const int16_t* src = pcm + row.base;
    const double b0 = row.coef[0], b1 = row.coef[1], b2 = row.coef[2], a1 = row.coef[3], a2 = row.coef[4];
    const bool filt = b0 == b0;                 // NaN marks "transform not applied" (RandomApply miss)
    if (pitched)
        for (int t = threadIdx.x; t <= 2 * H; t += 256) hp[(t % up) * S + t / up] = taps[row.tap_offset + t];
    // outputs per pass whose input span fits: ((nb - 1) down + 2H) / up + 1 <= kSpan
    const int nb_max = ((kSpan - 1) * up - 2 * H) / down + 1;
    double z0 = 0.0, z1 = 0.0;
    for (int c0 = 0; c0 < n_signal; c0 += kChunk) {
        const int len = min(kChunk, n_signal - c0);
        if (!pitched) {                         // ratio 1/1: the plain copy of feed_kernel
            for (int i = threadIdx.x; i < len; i += 256)
                buf[i] = (double)((float)src[row.in_point + c0 + i] / 32767.0f);
            __syncthreads();
        } else {
            for (int s0 = 0; s0 < len; s0 += nb_max) {
                const int nb = min(nb_max, len - s0);
                const int64_t n0 = row.in_point + c0 + s0;
                const int64_t lo = n0 * down - H;
                const int64_t k_lo = lo > 0 ? (lo + up - 1) / up : 0;
                const int64_t k_hi = min(((n0 + nb - 1) * down + H) / up, L - 1);
                const int cnt = (int)min(k_hi - k_lo + 1, (int64_t)kSpan);
                for (int i = threadIdx.x; i < cnt; i += 256)
                    span[i] = (float)src[k_lo + i] / 32767.0f;         // float32 division, as the reference
                __syncthreads();
                for (int i = threadIdx.x; i < nb; i += 256) {
                    const int64_t B = (n0 + i) * down + H;
                    const int64_t k_max = B / up;
                    const int p = (int)(B - k_max * up);
                    const int j_lo = k_max > L - 1 ? (int)(k_max - (L - 1)) : 0;
                    const int j_hi = (int)min((int64_t)((2 * H - p) / up), k_max - k_lo);
                    const double* hrow = hp + p * S;
                    const float* xs = span + (k_max - k_lo);
                    double acc = 0.0;
                    for (int j = j_lo; j <= j_hi; ++j) acc += hrow[j] * ((double)xs[-j] - mu);
                    buf[s0 + i] = (double)(float)(acc + mu);
                }
                __syncthreads();
            }
        }
        if (filt && threadIdx.x == 0) {
            for (int i = 0; i < len; ++i) {
                const double x = buf[i];
                const double y = b0 * x + z0;
                z0 = b1 * x - a1 * y + z1;
                z1 = b2 * x - a2 * y;
                buf[i] = y;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < len; i += 256) {
            const long o = (long)r * n_signal + c0 + i;
            out[o] = (float)(buf[i] + (double)noise[o] * quant);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int rh_feed_batch_i16_f32(const int16_t* pcm, const int64_t* src_offset, const double* coef, const float* noise,
                                     int32_t rows, int32_t n_signal, int32_t bit_depth, float* out, rh_stream_t stream) {
    RH_REQUIRE(rows >= 0 && n_signal > 0 && bit_depth > 0 && bit_depth < 32, RH_ERR_INVALID, "feed_batch: bad sizes");
    if (rows == 0) return RH_OK;
    RH_REQUIRE(pcm && src_offset && coef && noise && out, RH_ERR_INVALID, "feed_batch: null pointer");
    hipLaunchKernelGGL(feed_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, pcm, src_offset, coef, noise, n_signal,
                       1.0 / (double)(1ll << bit_depth), out);
    return rh_check_launch("feed_batch");
}

extern "C" int rh_feed_batch_pitch_i16_f32(const int16_t* pcm, int64_t pcm_samples, const rh_feed_pitch_row* rows,
                                           const rh_feed_pitch_row* rows_dev, const double* taps, int32_t n_taps,
                                           const float* noise, int32_t n_rows, int32_t n_signal, int32_t bit_depth, float* out,
                                           rh_stream_t stream) {
    RH_REQUIRE(n_rows >= 0 && n_signal > 0 && bit_depth > 0 && bit_depth < 32 && pcm_samples >= 0 && n_taps >= 0, RH_ERR_INVALID,
               "feed_batch_pitch: bad sizes");
    if (n_rows == 0) return RH_OK;
    RH_REQUIRE(pcm && rows && rows_dev && noise && out, RH_ERR_INVALID, "feed_batch_pitch: null pointer");
    for (int r = 0; r < n_rows; ++r) {
        const rh_feed_pitch_row& w = rows[r];
        RH_REQUIRE(w.up >= 1 && w.down >= 1 && w.up <= kMaxFactor && w.down <= kMaxFactor, RH_ERR_INVALID,
                   "feed_batch_pitch: row %d: ratio %d/%d outside 1..%d", r, w.up, w.down, kMaxFactor);
        RH_REQUIRE(w.length >= 1 && w.base >= 0 && w.base <= pcm_samples - w.length, RH_ERR_INVALID,
                   "feed_batch_pitch: row %d: item outside the PCM buffer", r);
        const int g = feed_gcd(w.up, w.down);
        const int up = w.up / g, down = w.down / g;
        const int64_t n_out = ((int64_t)w.length * up + down - 1) / down;
        RH_REQUIRE(w.in_point >= 0 && w.in_point <= n_out - n_signal, RH_ERR_INVALID,
                   "feed_batch_pitch: row %d: window [%lld, %lld) outside the %lld resampled samples", r, (long long)w.in_point,
                   (long long)w.in_point + n_signal, (long long)n_out);
        if (up != down && !w.mute) {
            const int H = 10 * std::max(up, down);
            RH_REQUIRE(taps && w.tap_offset >= 0 && w.tap_offset <= n_taps - (2 * H + 1), RH_ERR_INVALID,
                       "feed_batch_pitch: row %d: %d taps at offset %d outside the table of %d", r, 2 * H + 1, w.tap_offset, n_taps);
            RH_REQUIRE(up * feed_tap_stride(up, H) <= kTapSlots, RH_ERR_INVALID, "feed_batch_pitch: row %d: taps exceed the LDS table", r);
        }
    }
    hipLaunchKernelGGL(feed_pitch_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, pcm, rows_dev, taps, noise, n_signal,
                       1.0 / (double)(1ll << bit_depth), out);
    return rh_check_launch("feed_batch_pitch");
}
