// FrequencyMasking of the training data feed (rave/transforms.py:180-195), behind the chain of feed.hip: per item, with
// probability `prob`, a band of `mask_size` bins starting at `freq_idx` is zeroed in scipy.signal.stft(x, nperseg = 4096)
// (periodic Hann w, hop 2048, 2048 zeros on either side, 2049 bins) and the item is rebuilt by scipy.signal.istft.  The draws
// belong to the host; this unit is handed one band per row.
//
// istft(stft(x)) is x (the window pair is normalised: the overlap-add divides by sum w^2), and masking is linear, so the result
// is x minus the band component.  With xpad_t = frame t of the zero-padded row (the original samples [2048 (t - 1), 2048 (t + 1))),
// B the indicator of the band and h_t = irfft(B . rfft(w . xpad_t)), for n = 2048 b + j, 0 <= j < 2048:
//   y[n] = x[n] - (w[j] h_{b+1}[j] + w[j + 2048] h_b[j + 2048]) / (w[j]^2 + w[j + 2048]^2)
// (the 1 / sum w of stft and the sum w of istft cancel; the denominator is never below 1/2).  The float32 transforms' rounding
// error is then a fraction of the energy REMOVED, not of the whole signal.
//
//   * a workgroup owns one hop block b of one row and transforms both frames that cover it, b and b + 1: twice the arithmetic
//     of a frame-per-workgroup scheme, but one launch, no scratch in HBM, no atomics, and every output sample has one writer and
//     one fixed order of operations, whatever the grid.
//   * the 4096-point real transform of a frame is ONE 2048-point complex transform on the packed scheme of fft_lds.inc (256
//     threads, 8 points each).  With Z, E, O, U, W and M = 2048 as there, the packed spectrum of the real signal with the
//     one-sided spectrum V = B . U is
//       Zi_k = (V_k + conj V_{M-k}) / 2 + i W^{-k} (V_k - conj V_{M-k}) / 2
//            = s Z_k + d (W^k O_k + i W^{-k} E_k),     s = (B_k + B_{M-k}) / 2,  d = (B_k - B_{M-k}) / 2
//     (B_M = 0: the band never holds the Nyquist bin), zero wherever neither k nor M - k is in the band.  Forward split and
//     inverse merge are this ONE pass over the bins that matter; the inverse transform is the same forward FFT on conj Zi,
//     conjugated and divided by M: h[2m] + i h[2m + 1].
//   * thread t ends each inverse transform with the samples m = t + 256 q, q < 8, in registers -- the very samples it loaded --
//     so windows, the two frames' contributions and x meet in registers; LDS holds nothing but the transform's image.
//   * a row with n_bins == 0 is copied: the reference returns such an item itself.
#include <cstdint>
#include "common.hpp"

namespace {

#include "fft_lds.inc"

constexpr int kMaskHop = 2048;         // hop = bins below Nyquist = points of the packed complex transform

__global__ __launch_bounds__(256) void feed_mask_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        const int32_t* __restrict__ bands, int n_signal, int n_blocks,
                                                        const c32* __restrict__ tw4) {
    typedef Fft<kMaskHop> F;
    static_assert(F::TPF == 256 && F::G == 1 && F::RF == 4 && F::NSF == 512, "one transform per workgroup, final pass of radix 4");
    __shared__ c32 z[F::ZP];
    const int t = threadIdx.x;
    const int row = blockIdx.x / n_blocks, b = blockIdx.x - row * n_blocks;
    const float* __restrict__ xr = x + (long)row * n_signal;
    float* __restrict__ yb = y + (long)row * n_signal + (long)b * kMaskHop;
    // the band, clamped to the bins below Nyquist: whatever the table holds, the bins only index the LDS image
    const long first = bands[2 * row], count = bands[2 * row + 1];
    const int lo = (int)(first > 0 ? first : 0);
    const int hi = (int)(first + count < kMaskHop ? first + count : kMaskHop);
    if (count <= 0 || hi <= lo) {               // the same for the whole workgroup: nobody is left at a barrier
        const float* __restrict__ xb = xr + (long)b * kMaskHop;
        for (int i = t; i < kMaskHop; i += 256) yb[i] = xb[i];
        return;
    }
    typename F::Tw tw;
    tw.template init<2>(t, tw4);
    c32 wk[8], wn[8];                           // W^k of the bins k = t + 256 q; the window at the samples 2m, 2m + 1, m = t + 256 r
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int m = t + 256 * q;
        wk[q] = tw4[m];
        wn[q] = mk(0.5f - 0.5f * tw4[2 * m].x, 0.5f - 0.5f * tw4[2 * m + 1].x);
    }
    c32 xs[4], acc[4];                          // the block's own samples 2m, 2m + 1, m = t + 256 q, q < 4, and what is taken off them
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = mk(0.f, 0.f);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        // frame b + s covers the blocks b + s - 1 (r < 4) and b + s (r >= 4); block b is its second half (s = 0) or its first
        const int fr = b + s;
        const long p0 = (long)(fr - 1) * kMaskHop;
        c32 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool inside = r < 4 ? fr >= 1 : fr < n_blocks;       // the 2048 zeros scipy pads on either side
            const int m = t + 256 * r;
            const c32 a = inside ? mk(xr[p0 + 2 * m], xr[p0 + 2 * m + 1]) : mk(0.f, 0.f);
            if (s == 0 && r >= 4) xs[r - 4] = a;
            v[r] = a * wn[r];
        }
        F::run(v, z, t, tw);
        F::store_natural(v, z, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = t + 256 * q, km = kMaskHop - k;              // km = 2048 (k = 0) is the Nyquist bin: never in the band
            const bool bk = k >= lo && k < hi, bm = km >= lo && km < hi;
            c32 zi = mk(0.f, 0.f);
            if (bk || bm) {
                const c32 zk = z[zpad(k)], zm = z[zpad(km & (kMaskHop - 1))];
                c32 e, o;
                pair_split(zk, zm, 0.5f, 0.5f, e, o);
                const c32 wo = cmul(o, wk[q]), we = cmul(e, mk(wk[q].x, -wk[q].y));
                const float sc = bk && bm ? 1.f : 0.5f, dc = bk && bm ? 0.f : (bk ? 0.5f : -0.5f);
                zi = zk * sc + mk(wo.x - we.y, wo.y + we.x) * dc;
            }
            v[q] = mk(zi.x, -zi.y);
        }
        F::sync();                                                     // every read of the spectrum is done
        F::run(v, z, t, tw);                                           // sample m = t + 256 (u + 2 r) in v[4 u + r], conjugated
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int qq = s == 0 ? q + 4 : q;
            const c32 h = v[(qq & 1) * 4 + (qq >> 1)];
            acc[q] = __builtin_elementwise_fma(wn[qq], mk(h.x, -h.y), acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const c32 den = wn[q] * wn[q] + wn[q + 4] * wn[q + 4];
        const c32 r = xs[q] - acc[q] * (1.f / kMaskHop) / den;
        const int m = t + 256 * q;
        yb[2 * m] = r.x;                                               // scalar stores: y may be 4-byte aligned
        yb[2 * m + 1] = r.y;
    }
}

}  // namespace

extern "C" int rh_feed_freq_mask_f32(const float* x, float* y, const int32_t* bands, int32_t n_rows, int32_t n_signal,
                                     const float* twiddle, rh_stream_t stream) {
    RH_REQUIRE(x && y && bands && twiddle, RH_ERR_INVALID, "feed_freq_mask: null pointer");
    RH_REQUIRE(n_rows > 0, RH_ERR_INVALID, "feed_freq_mask: %d rows", n_rows);
    RH_REQUIRE(n_signal >= 2 * kMaskHop && n_signal % kMaskHop == 0, RH_ERR_INVALID,
               "feed_freq_mask: n_signal %d is not a multiple of %d of at least %d (scipy.signal.stft would pad the item)", n_signal,
               kMaskHop, 2 * kMaskHop);
    if (const int rc = check_twiddle("feed_freq_mask", twiddle)) return rc;
    const int64_t n_blocks = n_signal / kMaskHop;
    RH_REQUIRE(n_rows * n_blocks <= 0x7fffffffll, RH_ERR_INVALID, "feed_freq_mask: too many hop blocks for one launch");
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
    const uint64_t bytes = (uint64_t)n_rows * (uint64_t)n_signal * sizeof(float);
    RH_REQUIRE(xa + bytes <= ya || ya + bytes <= xa, RH_ERR_INVALID,
               "feed_freq_mask: x and y overlap (a frame reads the hop blocks other workgroups write)");
    hipLaunchKernelGGL(feed_mask_kernel, dim3((unsigned)(n_rows * n_blocks)), dim3(256), 0, (hipStream_t)stream, x, y, bands,
                       n_signal, (int)n_blocks, reinterpret_cast<const c32*>(twiddle));
    return rh_check_launch("feed_freq_mask");
}
