// The mel-spectrogram encoder input of RAVE.input_mode = "mel" (rave/model.py:238-242 over torchaudio.transforms.MelSpectrogram
// as configs/hybrid.gin binds it: centred reflect-padded frames, periodic Hann window, one-sided power spectrum divided by
// sum(window^2), MelScale (htk, norm None), then log1p with the last frame dropped) in ONE launch: x (rows, t_len) ->
// y (rows, n_mels, frames), so that a plain reshape gives the encoder's (B, n_channels * n_mels, frames).  A frame lives in LDS
// from the windowed load to the mel sums: HBM traffic = the waveform read (4x-8x overlapped, from L2) + the result written.
//
//   * frames are indexed straight from x (reflect_at: no padded copy) and transformed in PAIRS, frames f and f + 1 of one row,
//     equalised by a power of two: at an onset the quiet frame of a pair would otherwise inherit the loud one's noise
//     (tests/test_gpu_mel.py pins it).  fft_lds.inc has the transform, the pair scheme and the equaliser.
//   * the power spectra of the pair go to LDS; filter m walks its own bin range [lo_m, hi_m) from a small table, weights from the
//     module's `fb` buffer (no bin feeds more than two filters: ~2 (n/2 + 1) products per frame instead of (n/2 + 1) n_mels), in
//     ascending bin order: no atomics, the same bits from run to run.
//   * a workgroup owns kMelFrames consecutive frames of a row (more where the transforms of one round cover more) and collects
//     their results in LDS, so that y is written in runs of that many consecutive floats.
//   * no backward: nothing trainable is upstream of the audio (the gradient the reference computes into x_raw is discarded).
#include "common.hpp"

namespace {

#include "fft_lds.inc"

constexpr int kMelMax = 128;           // filters (rows of the LDS result tile)
constexpr int kMelFrames = 16;         // frames per workgroup, at least

template <int N>
struct MelGeom {
    typedef Fft<N> F;
    static constexpr int FPR = 2 * F::G;                                  // frames per round (G pairs side by side)
    static constexpr int FPW = FPR > kMelFrames ? FPR : kMelFrames;       // frames per workgroup (a multiple of FPR)
    static constexpr int TS = FPW + 1;                                    // row stride of the result tile (conflict-free columns)
    static constexpr int NB = N / 2 + 1;                                  // bins
};

struct MelP {
    const float* x;
    const float* win;
    const c32* tw;
    const float* fb;         // (n / 2 + 1, n_mels)
    const int* bins;         // (n_mels, 2): lo, hi
    float* y;                // (rows, n_mels, n_frames)
    int t_len, hop, n_frames, n_mels, log1p;
    float scale;             // 1 / sum(window^2) (normalized) or 1
};

template <int N>
__global__ __launch_bounds__(256) void mel_fwd_kernel(const MelP p) {
    typedef Fft<N> F;
    typedef MelGeom<N> M;
    constexpr int TPF = F::TPF, G = F::G, NB = M::NB;
    __shared__ c32 zb[G * F::ZP];
    __shared__ float pw[G * 2 * NB];            // power spectra of the pairs of this round
    __shared__ float tile[kMelMax * M::TS];     // log-mel results: [filter][frame of the workgroup]
    __shared__ c32 fmx[4];
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int f0 = blockIdx.x * M::FPW;
    const int f1 = min(f0 + M::FPW, p.n_frames);
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    c32* z = zb + gi * F::ZP;
    float* pa = pw + gi * 2 * NB;
    float* pb = pa + NB;
    typename F::Tw tw;
    tw.init(t, p.tw);
    float wn[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
    const float scale = p.scale;
    const int n_mels = p.n_mels;
    float sc = 1.f, isc = 1.f;       // equaliser of the current pair and its inverse (frame_scale)
    auto bin = [&](int k, c32 z1, c32 z2) {
        c32 A, B;
        pair_split(z1, z2, 0.5f, 0.5f * isc, A, B);
        pa[k] = (A.x * A.x + A.y * A.y) * scale;
        pb[k] = (B.x * B.x + B.y * B.y) * scale;
    };
    c32 vn[8];
    load_pair<N>(vn, xr, p.t_len, p.hop, N / 2, f0 + 2 * gi, f0 + 2 * gi < f1, f0 + 2 * gi + 1 < f1, t);
    for (int fr = f0; fr < f0 + M::FPW; fr += M::FPR) {          // the same trip count for every thread (barriers inside)
        const int fa = fr + 2 * gi;
        c32 v[8];
        frame_scale<TPF>(vn, fmx, sc, isc, 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(vn[r].x, vn[r].y * sc) * wn[r];
        // the next round's samples fly under this one's passes
        load_pair<N>(vn, xr, p.t_len, p.hop, N / 2, fa + M::FPR, fa + M::FPR < f1, fa + M::FPR + 1 < f1, t);
        F::run(v, z, t, tw);
        F::store_natural(v, z, t);
        {
            // bins k = t + m n/8 and their mirrors n - k = (n/8 - t) + (7 - m) n/8 (t > 0; bin 0 pairs with itself)
            const c32* zk = z + zpad(t);
            const c32* zm = z + (t ? zpad(TPF - t) : 0);
#pragma unroll
            for (int m = 0; m < 4; ++m)
                bin(t + m * TPF, zk[m * TPF / 8 * 9], t ? zm[(7 - m) * TPF / 8 * 9] : (m ? z[zpad(N - m * TPF)] : z[0]));
            if (t == 0) bin(N / 2, z[zpad(N / 2)], z[zpad(N / 2)]);
        }
        F::sync();                                              // spectra complete; z is free for the next round
        // filter m of frame fa + which: the transform's own threads (one wave when TPF <= 64)
        for (int idx = t; idx < 2 * n_mels; idx += TPF) {
            const int which = idx >= n_mels ? 1 : 0;
            const int m = idx - which * n_mels;
            const int lo = max(p.bins[2 * m], 0), hi = min(p.bins[2 * m + 1], NB);
            const float* __restrict__ pwr = which ? pb : pa;
            const float* __restrict__ w = p.fb + m;
            float acc = 0.f;
            for (int k = lo; k < hi; ++k) acc = fmaf(w[(long)k * n_mels], pwr[k], acc);
            tile[m * M::TS + (fa - f0) + which] = p.log1p ? log1pf(acc) : acc;
        }
        F::sync();                                              // pw is free for the next round
    }
    __syncthreads();
    const int nf = f1 - f0;
    float* __restrict__ yr = p.y + (long)row * n_mels * p.n_frames + f0;
    for (int i = tid; i < n_mels * M::FPW; i += 256) {
        const int m = i / M::FPW, j = i - m * M::FPW;
        if (j < nf) yr[(long)m * p.n_frames + j] = tile[m * M::TS + j];
    }
}

bool mel_shape_ok(int n_fft, int hop, int n_mels, int t_len, long rows) {
    return fft_size_ok(n_fft, 2048) && hop >= 1 && hop <= n_fft && n_mels >= 1 && n_mels <= kMelMax && t_len > n_fft / 2 && t_len >= hop &&
           (long)t_len + 80l * n_fft < 0x7fffffffl && rows > 0 && rows < 65536;      // (frame index x hop stays an int one
                                                                                      // workgroup's frames past the end)
}

template <int N>
int launch_mel(const MelP& p, int rows, hipStream_t stream) {
    const int wx = (p.n_frames + MelGeom<N>::FPW - 1) / MelGeom<N>::FPW;
    hipLaunchKernelGGL(mel_fwd_kernel<N>, dim3(wx, rows), dim3(256), 0, stream, p);
    return rh_check_launch("mel_fwd");
}

}  // namespace

extern "C" int rh_mel_supported(int32_t n_fft, int32_t hop, int32_t n_mels, int32_t t_len, int64_t rows) {
    return mel_shape_ok(n_fft, hop, n_mels, t_len, rows) ? 1 : 0;
}

extern "C" int rh_mel_fwd_f32(const float* x, const float* window, const float* twiddle, const float* fb, const int32_t* bins,
                              int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_frames,
                              float scale, int32_t log1p, float* y, rh_stream_t stream) {
    RH_REQUIRE(x && window && twiddle && fb && bins && y, RH_ERR_INVALID, "mel_fwd: null pointer");
    RH_REQUIRE(mel_shape_ok(n_fft, hop, n_mels, t_len, rows), RH_ERR_UNSUPPORTED,
               "mel_fwd: unsupported geometry (n_fft %d, hop %d, n_mels %d, t %d, rows %lld)", n_fft, hop, n_mels, t_len, (long long)rows);
    RH_REQUIRE(n_frames == t_len / hop || n_frames == t_len / hop + 1, RH_ERR_INVALID,
               "mel_fwd: n_frames %d is neither t / hop nor t / hop + 1 (t %d, hop %d)", n_frames, t_len, hop);
    if (const int rc = check_twiddle("mel_fwd", twiddle)) return rc;
    if (const int rc = check_scale("mel_fwd", scale)) return rc;
    RH_REQUIRE(rows * (int64_t)n_mels * n_frames < (int64_t)1 << 40, RH_ERR_UNSUPPORTED, "mel_fwd: output too large");
    MelP p = {};
    p.x = x; p.win = window; p.tw = reinterpret_cast<const c32*>(twiddle); p.fb = fb; p.bins = bins; p.y = y;
    p.t_len = t_len; p.hop = hop; p.n_frames = n_frames; p.n_mels = n_mels; p.log1p = log1p ? 1 : 0; p.scale = scale;
    return fft_dispatch<2048>(n_fft, [&](auto n) { return launch_mel<decltype(n)::value>(p, (int)rows, (hipStream_t)stream); });
}
