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
// kernel is meant for a side stream, under the training step.  That is rh_feed_batch_i16_f32; the options below ride on a row table
// and their three entry points are one runner (feed_run): rave_amd/data.py calls the widest, rh_feed_batch_resample_i16_f32.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "common.hpp"

namespace {

constexpr int kChunk = 4096;

// thread 0's part of a staged chunk: the all-pass in place, direct form II transposed, its two states carried to the next chunk
__device__ __forceinline__ void feed_allpass(double* buf, int len, double b0, double b1, double b2, double a1, double a2,
                                             double& z0, double& z1) {
    for (int i = 0; i < len; ++i) {
        const double x = buf[i];
        const double y = b0 * x + z0;
        z0 = b1 * x - a1 * y + z1;
        z1 = b2 * x - a2 * y;
        buf[i] = y;
    }
}

// max of `v` over the 256 threads through `red` (256 doubles of LDS), stored by thread 0; max is exact, so any reduction
// order gives the same bits
__device__ __forceinline__ void feed_store_max(double* red, double v, double* dst) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = red[0];
}

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
        if (filt && threadIdx.x == 0) feed_allpass(buf, len, b0, b1, b2, a1, a2, z0, z1);
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

// kPost (normalize / derivative behind Dequantize, feed_post_kernel below): the row is not rounded and stored to `out` but kept
// in float64 in `ws` (rows x n_signal), and max |row| goes to peaks[r]; a muted row only reports the peak 0.
template <bool kPost>
__global__ __launch_bounds__(256) void feed_pitch_kernel(const int16_t* __restrict__ pcm, const rh_feed_pitch_row* __restrict__ rows,
                                                         const double* __restrict__ taps, const float* __restrict__ noise,
                                                         int n_signal, double quant, float* __restrict__ out,
                                                         double* __restrict__ ws, double* __restrict__ peaks) {
    __shared__ double buf[kChunk];
    __shared__ double hp[kTapSlots];
    __shared__ float span[kSpan];
    const int r = blockIdx.x;
    const rh_feed_pitch_row row = rows[r];
    if (row.mute) {                             // (x + noise) * 0
        if constexpr (kPost) {
            if (threadIdx.x == 0) peaks[r] = 0.0;
        } else {
            for (int i = threadIdx.x; i < n_signal; i += 256) out[(long)r * n_signal + i] = 0.f;
        }
        return;
    }
    [[maybe_unused]] double peak = 0.0;
    const int g =feed_gcd(row.up, row.down);
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
        if (filt && threadIdx.x == 0) feed_allpass(buf, len, b0, b1, b2, a1, a2, z0, z1);
        __syncthreads();
        for (int i = threadIdx.x; i < len; i += 256) {
            const long o = (long)r * n_signal + c0 + i;
            const double v = buf[i] + (double)noise[o] * quant;
            if constexpr (kPost) {
                ws[o] = v;
                peak = fmax(peak, fabs(v));
            } else {
                out[o] = (float)v;
            }
        }
        __syncthreads();
    }
    if constexpr (kPost) feed_store_max(buf, peak, peaks + r);
}

// ---- normalize_signal and the derivator behind Dequantize (`rave train --normalize / --derivative`) ---------------------
//   normalize_signal(x, max_gain_db)  (dataset.py:196-204,241-242: peak = max |x| over the WHOLE item, every channel;
//                                      peak == 0 -> x, else x * 10^(min(max_gain_db, -20 log10(peak)) / 20))
//   derivator                         (dataset.py:24-29,244-245: lfilter([.5, -.5], [1], x) per row, float64, zero state)
// Second launch of rh_feed_batch_post_i16_f32: feed_pitch_kernel<true> left the float64 rows and one peak per row; here a
// workgroup takes kPostTile samples of one row, thread 0 reduces the n_channels peaks of the row's item in channel order and
// forms the gain in float64, and every thread applies gain and difference and rounds ONCE to float32 (what the reference's
// last astype does to its float64 rows).  x[n - 1] is read from the workspace, so neither the chunk seam of the first kernel
// nor a tile seam of this one is special; only n = 0 is (zero initial state).  Scalar float stores: `out` may be 4-byte aligned.
constexpr int kPostTile = 2048;

__global__ __launch_bounds__(256) void feed_post_kernel(const double* __restrict__ ws, const double* __restrict__ peaks,
                                                        const rh_feed_pitch_row* __restrict__ rows, int n_signal, int tiles,
                                                        int n_channels, int normalize, double max_gain_db, int derivative,
                                                        float* __restrict__ out) {
    __shared__ double gain_s;
    const int r = blockIdx.x / tiles;
    const int t0 = (blockIdx.x % tiles) * kPostTile;
    const int len = min(kPostTile, n_signal - t0);
    const long base = (long)r * n_signal;
    if (rows[r].mute) {                         // RandomMute runs behind both steps: the finished item times 0
        for (int i = threadIdx.x; i < len; i += 256) out[base + t0 + i] = 0.f;
        return;
    }
    if (threadIdx.x == 0) {
        double gain = 1.0;
        if (normalize) {
            const int item = r / n_channels;
            double peak = 0.0;
            for (int c = 0; c < n_channels; ++c) peak = fmax(peak, peaks[item * n_channels + c]);
            if (peak != 0.0) gain = pow(10.0, fmin(max_gain_db, -(20.0 * log10(peak))) / 20.0);
        }
        gain_s = gain;
    }
    __syncthreads();
    const double gain = gain_s;
    for (int i = threadIdx.x; i < len; i += 256) {
        const int n = t0 + i;
        double y = ws[base + n] * gain;
        if (derivative) {
            const double prev = n > 0 ? ws[base + n - 1] * gain : 0.0;
            y = 0.5 * y - 0.5 * prev;
        }
        out[base + n] = (float)y;
    }
}

// ---- Resample behind Dequantize (a dataset stored at another rate than the run's `sr`) ---------------------------------------
//   Resample(sr_dataset, sr)          (transforms.py:31-40, dataset.py:238-239: torchaudio.functional.resample(x.float(), orig,
//                                      new), sinc_interp_hann, lowpass_filter_width 6, rolloff .99, on the CROPPED item)
// With o, n = orig, new over their gcd, width = ceil(6 o / (.99 min(o, n))), K = 2 width + o and the float32 table h (n, K) of
// the host (rave_amd/data.py: sinc_resample_kernel), torchaudio's strided convolution written out:
//   y[q n + i] = sum_{k < K} h[i][k] xpad[q o + k],   xpad[m] = float32(v[m - width]) inside [0, n_signal), 0 outside,
//   q n + i < n_res = ceil(n n_signal / o)
// Launched between feed_pitch_kernel<true>, which left the float64 rows v in the workspace, and feed_post_kernel.  A workgroup
// per row, as in the chain kernel, in passes of `nq` frames q: the input span (nq - 1) o + K of a pass is staged in LDS as
// float32 (the `.float()`; the pads are zeros and are never read from memory), work item w = i * nq + qr takes filter i at frame
// qr, so the lanes of a wave share one or two filters -- their tap loads from the (up to 1.2 MB, L2-resident) table fall on the
// same address and walk a cache line with k -- and differ in qr: their LDS reads are o apart, and the image is padded by one
// word per 32 (res_pad) so that an o that is a multiple of 32 (160 / 147) does not put them all on one bank.  float32 tap times
// float32 sample is exact in float64; the sum runs in float64 in ascending k and is rounded ONCE to float32 (what the
// reference's float32 convolution returns, up to its own rounding).  The pass's outputs meet in LDS in output order and leave
// with unit-stride scalar stores (`out` may be 4-byte aligned): kPost = false to `out`; kPost = true as doubles to the second
// region of the workspace, with max |row| behind it, for feed_post_kernel on rows of n_res samples.  A muted row is not read.
constexpr int kResSpan = 8192;      // input samples staged per pass: K <= kResSpan (checked by the host)
constexpr int kResOut = 6144;       // outputs per pass: n <= kResOut (checked by the host)

__host__ __device__ inline int res_pad(int m) { return m + (m >> 5); }

template <bool kPost>
__global__ __launch_bounds__(256) void feed_resample_kernel(const double* __restrict__ ws, const rh_feed_pitch_row* __restrict__ rows,
                                                            const float* __restrict__ taps, int n_signal, int n_res, int o, int n,
                                                            int K, int width, float* __restrict__ out, double* __restrict__ ws2,
                                                            double* __restrict__ peaks2) {
    __shared__ float span[kResSpan + kResSpan / 32 + 1];
    __shared__ float ybuf[kResOut];
    const int r = blockIdx.x;
    if (rows[r].mute) {                         // the chain kernel left nothing for this row but the peak 0
        if constexpr (kPost) {
            if (threadIdx.x == 0) peaks2[r] = 0.0;
        } else {
            for (int i = threadIdx.x; i < n_res; i += 256) out[(long)r * n_res + i] = 0.f;
        }
        return;
    }
    [[maybe_unused]] double peak = 0.0;
    const double* __restrict__ x = ws + (long)r * n_signal;
    const int frames = (n_res + n - 1) / n;
    const int qc = min((kResSpan - K) / o + 1, kResOut / n);           // frames per pass: span and outputs both fit
    for (int q0 = 0; q0 < frames; q0 += qc) {
        const int nq = min(qc, frames - q0);
        const int cnt = (nq - 1) * o + K;
        const int64_t m0 = (int64_t)q0 * o - width;                    // span[0] is v[m0]
        for (int s = threadIdx.x; s < cnt; s += 256) {
            const int64_t m = m0 + s;
            span[res_pad(s)] = m >= 0 && m < n_signal ? (float)x[m] : 0.f;
        }
        __syncthreads();
        for (int w = threadIdx.x; w < n * nq; w += 256) {
            const int i = w / nq, qr = w - i * nq;
            const float* __restrict__ h = taps + (long)i * K;
            const int s0 = qr * o;
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc += (double)h[k] * (double)span[res_pad(s0 + k)];
            ybuf[qr * n + i] = (float)acc;
        }
        __syncthreads();
        const int64_t j0 = (int64_t)q0 * n;
        const int len = (int)min((int64_t)nq * n, n_res - j0);         // the last frame is cut at n_res
        for (int j = threadIdx.x; j < len; j += 256) {
            const long at = (long)r * n_res + j0 + j;
            const float v = ybuf[j];
            if constexpr (kPost) {
                ws2[at] = (double)v;
                peak = fmax(peak, fabs((double)v));
            } else {
                out[at] = v;
            }
        }
        // no barrier: the next pass writes ybuf only behind its own first barrier, and span only after every thread is past the one above
    }
    if constexpr (kPost) {
        __shared__ double red[256];
        feed_store_max(red, peak, peaks2 + r);
    }
}

// o, n, width, K and n_res of a rate pair, or false when a length leaves int32
struct ResPlan { int o, n, width, K, n_res; };
bool feed_resample_plan(int32_t orig_freq, int32_t new_freq, int32_t n_signal, ResPlan* p) {
    const int g = feed_gcd(orig_freq, new_freq);
    p->o = orig_freq / g;
    p->n = new_freq / g;
    const double width = std::ceil(6.0 * p->o / (std::min(p->o, p->n) * 0.99));       // the IEEE expression of the host table
    const int64_t K = 2 * (int64_t)width + p->o;
    const int64_t n_res = ((int64_t)p->n * n_signal + p->o - 1) / p->o;
    if (K > 0x7fffffffll || n_res > 0x7fffffffll) return false;
    p->width = (int)width;
    p->K = (int)K;
    p->n_res = (int)n_res;
    return true;
}

// the checks of the pitched entry points on the host copy of the row table
int feed_check_rows(const char* what, int64_t pcm_samples, const rh_feed_pitch_row* rows, const double* taps, int32_t n_taps,
                    int32_t n_rows, int32_t n_signal) {
    for (int r = 0; r < n_rows; ++r) {
        const rh_feed_pitch_row& w = rows[r];
        RH_REQUIRE(w.up >= 1 && w.down >= 1 && w.up <= kMaxFactor && w.down <= kMaxFactor, RH_ERR_INVALID,
                   "%s: row %d: ratio %d/%d outside 1..%d", what, r, w.up, w.down, kMaxFactor);
        RH_REQUIRE(w.length >= 1 && w.base >= 0 && w.base <= pcm_samples - w.length, RH_ERR_INVALID,
                   "%s: row %d: item outside the PCM buffer", what, r);
        const int g = feed_gcd(w.up, w.down);
        const int up = w.up / g, down = w.down / g;
        const int64_t n_out = ((int64_t)w.length * up + down - 1) / down;
        RH_REQUIRE(w.in_point >= 0 && w.in_point <= n_out - n_signal, RH_ERR_INVALID,
                   "%s: row %d: window [%lld, %lld) outside the %lld resampled samples", what, r, (long long)w.in_point,
                   (long long)w.in_point + n_signal, (long long)n_out);
        if (up != down && !w.mute) {
            const int H = 10 * std::max(up, down);
            RH_REQUIRE(taps && w.tap_offset >= 0 && w.tap_offset <= n_taps - (2 * H + 1), RH_ERR_INVALID,
                       "%s: row %d: %d taps at offset %d outside the table of %d", what, r, 2 * H + 1, w.tap_offset, n_taps);
            RH_REQUIRE(up * feed_tap_stride(up, H) <= kTapSlots, RH_ERR_INVALID, "%s: row %d: taps exceed the LDS table", what, r);
        }
    }
    return RH_OK;
}

// The workspace of a call with a stage behind the chain kernel, as offsets in doubles: the chain's float64 rows first, one peak
// per row at `peaks`, then -- n_res > 0: Resample runs -- the resampled rows at `ws2` and their peaks at `peaks2`.
struct FeedLayout { int64_t peaks, ws2, peaks2, bytes; };
FeedLayout feed_layout(int32_t n_rows, int32_t n_signal, int32_t n_res) {
    const int64_t peaks = (int64_t)n_rows * n_signal, ws2 = peaks + n_rows, peaks2 = ws2 + (int64_t)n_rows * n_res;
    return {peaks, ws2, peaks2, (peaks2 + (n_res > 0 ? n_rows : 0)) * (int64_t)sizeof(double)};
}

// Everything a table-driven call can carry, in the argument order of rh_feed_batch_resample_i16_f32 (include/rave_hip.h); an
// entry point without the later arguments fills them with values that switch their stage off.
struct FeedChain {
    const int16_t* pcm; int64_t pcm_samples;
    const rh_feed_pitch_row *rows, *rows_dev;
    const double* taps; int32_t n_taps;
    const float* noise;
    int32_t n_rows, n_signal, bit_depth, n_channels, normalize; double max_gain_db; int32_t derivative;
    int32_t orig_freq, new_freq; const float* res_taps; int64_t n_res_taps; int32_t width;
    void* workspace; int64_t workspace_bytes;
    float* out; rh_stream_t stream;
};

// The three table-driven entry points: which stages run, the checks, the workspace, the launches.  Messages carry the name of
// the entry point the call reduces to (equal rates: feed_batch_post; both steps off as well: feed_batch_pitch), except that
// the first checks, which feed_batch_post makes before it looks at its flags and feed_batch_pitch passes, carry `entry`.
int feed_run(const char* entry, const FeedChain& c) {
    RH_REQUIRE(c.orig_freq >= 1 && c.new_freq >= 1, RH_ERR_INVALID, "feed_batch_resample: rates %d -> %d", c.orig_freq, c.new_freq);
    const bool resample = c.orig_freq != c.new_freq;        // equal rates: Resample returns its input
    const bool post = c.normalize || c.derivative, staged = resample || post;      // staged: the chain kernel writes the workspace
    const char* what = resample ? "feed_batch_resample" : post ? "feed_batch_post" : "feed_batch_pitch";
    if (resample) entry = what;
    RH_REQUIRE(c.n_rows >= 0 && c.n_signal > 0 && c.bit_depth > 0 && c.bit_depth < 32 && c.pcm_samples >= 0 && c.n_taps >= 0,
               RH_ERR_INVALID, "%s: bad sizes", entry);
    RH_REQUIRE(c.n_channels >= 1 && c.n_rows % c.n_channels == 0, RH_ERR_INVALID, "%s: %d rows are not whole items of %d channels",
               entry, c.n_rows, c.n_channels);
    RH_REQUIRE(std::isfinite(c.max_gain_db), RH_ERR_INVALID, "%s: max_gain_db is not finite", entry);
    ResPlan p = {};                                         // n_res = 0: no resampled region in the workspace
    if (resample) {
        RH_REQUIRE(feed_resample_plan(c.orig_freq, c.new_freq, c.n_signal, &p), RH_ERR_INVALID,
                   "feed_batch_resample: %d samples at %d -> %d leave int32", c.n_signal, c.orig_freq, c.new_freq);
        RH_REQUIRE(c.width == p.width, RH_ERR_INVALID, "feed_batch_resample: width %d, but %d -> %d has ceil(6 o / (.99 min(o, n))) = %d",
                   c.width, c.orig_freq, c.new_freq, p.width);
        RH_REQUIRE(c.n_res_taps == (int64_t)p.n * p.K, RH_ERR_INVALID, "feed_batch_resample: table of %lld taps, %d x %d needed",
                   (long long)c.n_res_taps, p.n, p.K);
        RH_REQUIRE(p.K <= kResSpan, RH_ERR_INVALID, "feed_batch_resample: %d taps per filter exceed kResSpan = %d", p.K, kResSpan);
        RH_REQUIRE(p.n <= kResOut, RH_ERR_INVALID, "feed_batch_resample: %d filters exceed kResOut = %d", p.n, kResOut);
    }
    if (c.n_rows == 0) return RH_OK;
    RH_REQUIRE(c.pcm && c.rows && c.rows_dev && c.noise && (c.res_taps || !resample) && c.out, RH_ERR_INVALID, "%s: null pointer", what);
    const FeedLayout l = feed_layout(c.n_rows, c.n_signal, p.n_res);
    const int n_out = resample ? p.n_res : c.n_signal;      // samples per finished row
    const int tiles = (n_out + kPostTile - 1) / kPostTile;
    if (staged) {
        RH_REQUIRE(c.workspace && c.workspace_bytes >= l.bytes, RH_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed", what,
                   (long long)c.workspace_bytes, (long long)l.bytes);
        RH_REQUIRE((uintptr_t)c.workspace % 8 == 0, RH_ERR_INVALID, "%s: workspace is not 8-byte aligned", what);
        RH_REQUIRE((int64_t)c.n_rows * tiles <= 0x7fffffffll, RH_ERR_INVALID, "%s: too many tiles for one launch", what);
    }
    if (const int rc = feed_check_rows(what, c.pcm_samples, c.rows, c.taps, c.n_taps, c.n_rows, c.n_signal)) return rc;
    double *ws = nullptr, *peaks = nullptr, *ws2 = nullptr, *peaks2 = nullptr;      // null for the stages that do not run
    if (staged) ws = (double*)c.workspace, peaks = ws + l.peaks;
    if (resample && post) ws2 = ws + l.ws2, peaks2 = ws + l.peaks2;
    hipLaunchKernelGGL(staged ? feed_pitch_kernel<true> : feed_pitch_kernel<false>, dim3(c.n_rows), dim3(256), 0, (hipStream_t)c.stream, c.pcm,
                       c.rows_dev, c.taps, c.noise, c.n_signal, 1.0 / (double)(1ll << c.bit_depth), c.out, ws, peaks);
    if (const int rc = rh_check_launch(what)) return rc;
    if (resample) {
        hipLaunchKernelGGL(post ? feed_resample_kernel<true> : feed_resample_kernel<false>, dim3(c.n_rows), dim3(256), 0, (hipStream_t)c.stream,
                           (const double*)ws, c.rows_dev, c.res_taps, c.n_signal, p.n_res, p.o, p.n, p.K, p.width, c.out, ws2, peaks2);
        if (const int rc = rh_check_launch("feed_batch_resample: resample")) return rc;
    }
    if (!post) return RH_OK;
    hipLaunchKernelGGL(feed_post_kernel, dim3(c.n_rows * tiles), dim3(256), 0, (hipStream_t)c.stream,
                       (const double*)(resample ? ws2 : ws), (const double*)(resample ? peaks2 : peaks), c.rows_dev, n_out, tiles,
                       c.n_channels, c.normalize, c.max_gain_db, c.derivative, c.out);
    return rh_check_launch(resample ? "feed_batch_resample: normalize / derivative" : "feed_batch_post: normalize / derivative");
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
    return feed_run("feed_batch_pitch", {pcm, pcm_samples, rows, rows_dev, taps, n_taps, noise, n_rows, n_signal, bit_depth,
                                         /* one channel, no step, equal rates */ 1, 0, 0.0, 0, 1, 1, nullptr, 0, 0, nullptr, 0, out, stream});
}

extern "C" int64_t rh_feed_post_workspace_bytes(int32_t n_rows, int32_t n_signal) {
    if (n_rows < 0 || n_signal <= 0) return -1;
    return feed_layout(n_rows, n_signal, 0).bytes;
}

extern "C" int rh_feed_batch_post_i16_f32(const int16_t* pcm, int64_t pcm_samples, const rh_feed_pitch_row* rows,
                                          const rh_feed_pitch_row* rows_dev, const double* taps, int32_t n_taps,
                                          const float* noise, int32_t n_rows, int32_t n_signal, int32_t bit_depth,
                                          int32_t n_channels, int32_t normalize, double max_gain_db, int32_t derivative,
                                          void* workspace, int64_t workspace_bytes, float* out, rh_stream_t stream) {
    return feed_run("feed_batch_post", {pcm, pcm_samples, rows, rows_dev, taps, n_taps, noise, n_rows, n_signal, bit_depth, n_channels,
                                        normalize, max_gain_db, derivative, /* equal rates */ 1, 1, nullptr, 0, 0, workspace,
                                        workspace_bytes, out, stream});
}

extern "C" int64_t rh_feed_resample_workspace_bytes(int32_t n_rows, int32_t n_signal, int32_t orig_freq, int32_t new_freq) {
    if (n_rows < 0 || n_signal <= 0 || orig_freq < 1 || new_freq < 1) return -1;
    ResPlan p = {};
    if (orig_freq != new_freq && !feed_resample_plan(orig_freq, new_freq, n_signal, &p)) return -1;
    return feed_layout(n_rows, n_signal, p.n_res).bytes;
}

extern "C" int rh_feed_batch_resample_i16_f32(const int16_t* pcm, int64_t pcm_samples, const rh_feed_pitch_row* rows,
                                              const rh_feed_pitch_row* rows_dev, const double* taps, int32_t n_taps,
                                              const float* noise, int32_t n_rows, int32_t n_signal, int32_t bit_depth,
                                              int32_t n_channels, int32_t normalize, double max_gain_db, int32_t derivative,
                                              int32_t orig_freq, int32_t new_freq, const float* res_taps, int64_t n_res_taps,
                                              int32_t width, void* workspace, int64_t workspace_bytes, float* out,
                                              rh_stream_t stream) {
    return feed_run("feed_batch_post", {pcm, pcm_samples, rows, rows_dev, taps, n_taps, noise, n_rows, n_signal, bit_depth, n_channels,
                                        normalize, max_gain_db, derivative, orig_freq, new_freq, res_taps, n_res_taps, width, workspace,
                                        workspace_bytes, out, stream});
}
