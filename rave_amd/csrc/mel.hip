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
//   * no backward here: nothing trainable is upstream of the audio (the gradient the reference computes into x_raw is discarded).
//
// Beside it, the DIFFERENTIABLE mel spectrogram of the Encodec-style loss (rave/core.py:446-490: SpectralDistance(mel = n) over
// torchaudio.transforms.MelSpectrogram(center=False, power 1 or 2)): rh_mel_diff_fwd_f32 is the kernel above with DIFF = true
// (frames centred or not, |S| or |S|^2, no logarithm; DIFF = false is the encoder input's code, untouched), and
// rh_mel_diff_bwd_f32 the gradient with respect to the audio, built like spectrogram.hip's adjoint: a workgroup OWNS a span of
// dx, recomputes the spectrum of every frame pair that covers it from x, turns dmel into the spectrum's cotangent, runs the
// transposed real DFT and gathers -- one launch, no workspace, no atomics, one fixed order of additions per sample.
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
    float scale;             // 1 / sum(window^2) (normalized) or 1; DIFF: s^power, s = 1 / sqrt(sum(window^2)) or 1
    // DIFF only
    int off, power;          // n_fft / 2 (centred) or 0; 1 or 2
    const float* dmel;       // (rows, n_mels, n_frames)
    float* dx;               // (rows, t_len)
    float s;                 // 1 / sqrt(sum(window^2)) (normalized) or 1
};

// DIFF = false: the encoder input (centred, power 2); DIFF = true: frames start at f hop - p.off, |S|^p.power
template <int N, bool DIFF>
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
    const int off = DIFF ? p.off : N / 2;
    const bool mag = DIFF && p.power == 1;
    float sc = 1.f, isc = 1.f;       // equaliser of the current pair and its inverse (frame_scale)
    auto bin = [&](int k, c32 z1, c32 z2) {
        c32 A, B;
        pair_split(z1, z2, 0.5f, 0.5f * isc, A, B);
        if (mag) {
            pa[k] = sqrtf(A.x * A.x + A.y * A.y) * scale;
            pb[k] = sqrtf(B.x * B.x + B.y * B.y) * scale;
        } else {
            pa[k] = (A.x * A.x + A.y * A.y) * scale;
            pb[k] = (B.x * B.x + B.y * B.y) * scale;
        }
    };
    c32 vn[8];
    load_pair<N>(vn, xr, p.t_len, p.hop, off, f0 + 2 * gi, f0 + 2 * gi < f1, f0 + 2 * gi + 1 < f1, t);
    for (int fr = f0; fr < f0 + M::FPW; fr += M::FPR) {          // the same trip count for every thread (barriers inside)
        const int fa = fr + 2 * gi;
        c32 v[8];
        frame_scale<TPF>(vn, fmx, sc, isc, 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(vn[r].x, vn[r].y * sc) * wn[r];
        // the next round's samples fly under this one's passes
        load_pair<N>(vn, xr, p.t_len, p.hop, off, fa + M::FPR, fa + M::FPR < f1, fa + M::FPR + 1 < f1, t);
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

template <int N, bool DIFF>
int launch_mel(const MelP& p, int rows, hipStream_t stream) {
    const int wx = (p.n_frames + MelGeom<N>::FPW - 1) / MelGeom<N>::FPW;
    hipLaunchKernelGGL((mel_fwd_kernel<N, DIFF>), dim3(wx, rows), dim3(256), 0, stream, p);
    return rh_check_launch(DIFF ? "mel_diff_fwd" : "mel_fwd");
}

// ------------------------------------------------------------------------------------------------------------ backward
template <int N>
struct MelBwdGeom {
    typedef Fft<N> F;
    static constexpr int FPR = 2 * F::G;                                  // frames per round (G pairs side by side)
    static constexpr int NB = N / 2 + 1;                                  // bins
    static constexpr int DS = kMelMax + 1;                                // row stride of the staged dmel (odd: conflict-free rows)
    static constexpr int SPAN = N >= 2048 ? 8192 : (N == 1024 ? 4096 : 2048);    // samples of dx a workgroup owns
    static constexpr int SPT = SPAN / 256;                                // ... per thread
};

// dmel (rows, n_mels, frames), x -> dx (rows, t_len).  Per round the G transforms of the workgroup take G pairs (f, f + 1) of the
// SAME row (never a frame of another signal: fft_lds.inc on the equaliser): windowed load, forward transform, pair split; then
//   dP[k] = sum_m fb[k][m] dmel[m][f] over the filters whose bin range holds k (ascending m),
//   G_k = 2 s^2 S_k dP[k] (power 2)   or   s S_k / |S_k| dP[k], 0 where |S_k| = 0 (power 1: torch's abs at 0),
// the transposed real DFT of the pair as ONE complex transform (spectrogram.hip: Re FFT(conj G, zero above N / 2), two frames as
// Sa + i Sb), the window, and every thread gathers what its own samples get: frames ascending, direct before reflected.
template <int N>
__global__ __launch_bounds__(256) void mel_bwd_kernel(const MelP p) {
    typedef Fft<N> F;
    typedef MelBwdGeom<N> M;
    constexpr int TPF = F::TPF, G = F::G, NB = M::NB, FPR = M::FPR, DS = M::DS, SPT = M::SPT, RF = F::RF;
    __shared__ c32 zb[G * F::ZP];
    __shared__ float4 gbuf[G * NB];             // cotangents of the pairs' spectra: (re a, im a, re b, im b) per bin
    __shared__ float dm[FPR * DS];              // dmel of the round's frames: [frame][filter]
    __shared__ int rng[2 * kMelMax];            // the bin ranges of the filters
    __shared__ c32 fmx[4];
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int T = p.t_len, hop = p.hop, n_frames = p.n_frames, n_mels = p.n_mels, off = p.off;
    const int s0 = blockIdx.x * M::SPAN, s1 = min(s0 + M::SPAN, T);
    // the frames that can reach the span: those over [lo, hi], which holds the span and, at the edges of a centred row, its
    // mirror images (a superset is harmless: the gather tests every sample's own coverage)
    const bool left = off && s0 <= N / 2, right = off && s1 - 1 >= T - 1 - N / 2;
    const int lo = left ? -min(s1 - 1, N / 2) : s0;
    const int hi = right ? 2 * (T - 1) - max(s0, T - 1 - N / 2) : s1 - 1;
    const int num = lo + off - N + 1;
    const int fmin = num <= 0 ? 0 : (num + hop - 1) / hop;
    const int fmax = min((hi + off) / hop, n_frames - 1);
    const float* __restrict__ xr = p.x + (long)row * T;
    const float* __restrict__ dmr = p.dmel + (long)row * n_mels * n_frames;
    c32* z = zb + gi * F::ZP;
    float4* gg = gbuf + gi * NB;
    const float* zf = reinterpret_cast<const float*>(zb);
    typename F::Tw tw;
    tw.init(t, p.tw);
    // the window at the samples this thread loads (t + r TPF) and at those it holds when a transform ends (F::out_index)
    float wn[8], wo[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
#pragma unroll
    for (int u = 0; u < 8 / RF; ++u)
#pragma unroll
        for (int r = 0; r < RF; ++r) wo[u * RF + r] = p.win[F::out_index(t, u, r)];
    for (int i = tid; i < 2 * n_mels; i += 256) rng[i] = p.bins[i];
    __syncthreads();
    // this thread's bins in the pair split, k = t + j TPF (j < 4; j = 4: the Nyquist bin, thread 0's), and per bin the span
    // of filters [mlo, mhi) outside which no filter's range holds it
    int mlo[5], mhi[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int k = j < 4 ? t + j * TPF : N / 2;
        int a = n_mels, b = 0;
        for (int m = 0; m < n_mels; ++m)
            if (rng[2 * m] <= k && k < rng[2 * m + 1]) {
                a = min(a, m);
                b = m + 1;
            }
        mlo[j] = a;
        mhi[j] = b;
    }
    const bool mag = p.power == 1;
    const float cs = mag ? p.s : 2.f * p.s * p.s;
    float acc[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) acc[i] = 0.f;
    const int pt = s0 + tid;                                            // this thread's samples: pt + 256 i
    float sc = 1.f, isc = 1.f;       // equaliser of the current pair and its inverse (frame_scale)
    const float* da = dm + 2 * gi * DS;
    const float* db = da + DS;
    auto cot = [&](int mlo_k, int mhi_k, int k, c32 z1, c32 z2) {
        c32 A, B;
        pair_split(z1, z2, 0.5f, 0.5f * isc, A, B);
        const float* __restrict__ w = p.fb + (long)k * n_mels;
        float pa = 0.f, pb = 0.f;
        for (int m = mlo_k; m < mhi_k; ++m)
            if (rng[2 * m] <= k && k < rng[2 * m + 1]) {
                const float f = w[m];
                pa = fmaf(f, da[m], pa);
                pb = fmaf(f, db[m], pb);
            }
        float ca = cs * pa, cb = cs * pb;
        if (mag) {
            const float na = sqrtf(A.x * A.x + A.y * A.y), nb = sqrtf(B.x * B.x + B.y * B.y);
            ca = na > 0.f ? ca / na : 0.f;
            cb = nb > 0.f ? cb / nb : 0.f;
        }
        gg[k] = make_float4(ca * A.x, ca * A.y, cb * B.x, cb * B.y);
    };
    c32 vn[8];
    load_pair<N>(vn, xr, T, hop, off, fmin + 2 * gi, fmin + 2 * gi <= fmax, fmin + 2 * gi + 1 <= fmax, t);
    for (int fr = fmin; fr <= fmax; fr += FPR) {                        // uniform: barriers inside
        const int fa = fr + 2 * gi;
        for (int i = tid; i < n_mels * FPR; i += 256) {
            const int m = i / FPR, j = i - m * FPR;
            dm[j * DS + m] = fr + j <= fmax ? dmr[(long)m * n_frames + fr + j] : 0.f;
        }
        c32 v[8];
        frame_scale<TPF>(vn, fmx, sc, isc, 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(vn[r].x, vn[r].y * sc) * wn[r];
        // the next round's samples fly under this one's passes
        load_pair<N>(vn, xr, T, hop, off, fa + FPR, fa + FPR <= fmax, fa + FPR + 1 <= fmax, t);
        F::run(v, z, t, tw);
        F::store_natural(v, z, t);
        __syncthreads();                                                // dm is staged, the spectra lie in z
        {
            // bins k = t + j n/8 and their mirrors n - k = (n/8 - t) + (7 - j) n/8 (t > 0; bin 0 pairs with itself)
            const c32* zk = z + zpad(t);
            const c32* zm = z + (t ? zpad(TPF - t) : 0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                cot(mlo[j], mhi[j], t + j * TPF, zk[j * TPF / 8 * 9], t ? zm[(7 - j) * TPF / 8 * 9] : (j ? z[zpad(N - j * TPF)] : z[0]));
            if (t == 0) cot(mlo[4], mhi[4], N / 2, z[zpad(N / 2)], z[zpad(N / 2)]);
        }
        F::sync();                                                      // the cotangents are complete; z is free
        // the Hermitian parts of conj G of the two frames as Sa + i Sb (spectrogram.hip)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = t + r * TPF;
            if (r < 4) {
                const float4 q = gg[k];
                v[r] = k == 0 ? mk(q.x, q.z) : mk(0.5f * (q.x + q.w), 0.5f * (q.z - q.y));
            } else {
                const float4 q = gg[N - k];
                v[r] = k == N / 2 ? mk(q.x, q.z) : mk(0.5f * (q.x - q.w), 0.5f * (q.y + q.z));
            }
        }
        F::run(v, z, t, tw);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = v[r] * wo[r];
        F::store_natural(v, z, t);
        __syncthreads();                                                // every group's windowed frames are in LDS
        for (int jj = 0; jj < FPR; ++jj) {
            const int f = fr + jj;
            if (f > fmax) break;
            const int start = f * hop - off;
            // frame jj: component jj & 1 of transform jj / 2, sample n at zpad(n)
            const float* zs = zf + 2 * (jj >> 1) * F::ZP + (jj & 1);
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int n = pt + 256 * i - start;
                if ((unsigned)n < (unsigned)N) acc[i] += zs[2 * zpad(n)];
            }
            if (left) {
#pragma unroll
                for (int i = 0; i < SPT; ++i) {
                    const int pi = pt + 256 * i, n = -pi - start;
                    if (pi >= 1 && (unsigned)n < (unsigned)N) acc[i] += zs[2 * zpad(n)];
                }
            }
            if (right) {
#pragma unroll
                for (int i = 0; i < SPT; ++i) {
                    const int pi = pt + 256 * i, n = 2 * (T - 1) - pi - start;
                    if (pi <= T - 2 && (unsigned)n < (unsigned)N) acc[i] += zs[2 * zpad(n)];
                }
            }
        }
        __syncthreads();                                                // z, gbuf and dm are free for the next round
    }
    float* __restrict__ dxr = p.dx + (long)row * T;
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int pi = pt + 256 * i;
        if (pi < s1) dxr[pi] = acc[i];
    }
}

bool mel_diff_shape_ok(int n_fft, int hop, int n_mels, int t_len, long rows, int center, int power) {
    return fft_size_ok(n_fft, 2048) && hop >= 1 && hop <= n_fft && n_mels >= 1 && n_mels <= kMelMax && (power == 1 || power == 2) &&
           (center == 0 || center == 1) && (center ? t_len > n_fft / 2 : t_len >= n_fft) && t_len <= (1 << 30) && rows > 0 &&
           rows < 65536;
    // t_len <= 2^30: the backward's mirror index 2 (T - 1) and the look-ahead of either direction (under 2^18 samples past the
    // last frame at any built size) stay inside an int
}

int mel_diff_frames(int n_fft, int hop, int t_len, int center) { return center ? t_len / hop + 1 : (t_len - n_fft) / hop + 1; }

template <int N>
int launch_mel_bwd(const MelP& p, int rows, hipStream_t stream) {
    const int wx = (p.t_len + MelBwdGeom<N>::SPAN - 1) / MelBwdGeom<N>::SPAN;
    hipLaunchKernelGGL(mel_bwd_kernel<N>, dim3(wx, rows), dim3(256), 0, stream, p);
    return rh_check_launch("mel_diff_bwd");
}

// the checks both directions share, then the parameter block (y / dmel / dx are the caller's)
int mel_diff_params(const char* what, const void* a, const void* b, const float* x, const float* window, const float* twiddle,
                    const float* fb, const int32_t* bins, int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels,
                    int32_t center, int32_t power, float scale, MelP& p) {
    RH_REQUIRE(a && b && x && window && twiddle && fb && bins, RH_ERR_INVALID, "%s: null pointer", what);
    RH_REQUIRE(mel_diff_shape_ok(n_fft, hop, n_mels, t_len, rows, center, power), RH_ERR_UNSUPPORTED,
               "%s: unsupported geometry (n_fft %d, hop %d, n_mels %d, t %d, rows %lld, center %d, power %d)", what, n_fft, hop, n_mels,
               t_len, (long long)rows, center, power);
    if (const int rc = check_twiddle(what, twiddle)) return rc;
    if (const int rc = check_scale(what, scale)) return rc;
    const int n_frames = mel_diff_frames(n_fft, hop, t_len, center);
    RH_REQUIRE(rows * (int64_t)n_mels * n_frames < (int64_t)1 << 40, RH_ERR_UNSUPPORTED, "%s: output too large", what);
    p.x = x; p.win = window; p.tw = reinterpret_cast<const c32*>(twiddle); p.fb = fb; p.bins = bins;
    p.t_len = t_len; p.hop = hop; p.n_frames = n_frames; p.n_mels = n_mels; p.log1p = 0;
    p.off = center ? n_fft / 2 : 0; p.power = power; p.s = scale; p.scale = power == 2 ? scale * scale : scale;
    return check_scale(what, p.scale);                                   // (the square of a float can leave the range)
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
    return fft_dispatch<2048>(n_fft, [&](auto n) { return launch_mel<decltype(n)::value, false>(p, (int)rows, (hipStream_t)stream); });
}

extern "C" int rh_mel_diff_supported(int32_t n_fft, int32_t hop, int32_t n_mels, int32_t t_len, int64_t rows, int32_t center,
                                     int32_t power) {
    return mel_diff_shape_ok(n_fft, hop, n_mels, t_len, rows, center, power) ? 1 : 0;
}

extern "C" int rh_mel_diff_fwd_f32(const float* x, const float* window, const float* twiddle, const float* fb, const int32_t* bins,
                                   int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t center,
                                   int32_t power, float scale, float* mel, rh_stream_t stream) {
    MelP p = {};
    const int rc = mel_diff_params("mel_diff_fwd", x, mel, x, window, twiddle, fb, bins, rows, t_len, n_fft, hop, n_mels, center, power,
                                   scale, p);
    if (rc != RH_OK) return rc;
    p.y = mel;
    return fft_dispatch<2048>(n_fft, [&](auto n) { return launch_mel<decltype(n)::value, true>(p, (int)rows, (hipStream_t)stream); });
}

extern "C" int rh_mel_diff_bwd_f32(const float* dmel, const float* x, const float* window, const float* twiddle, const float* fb,
                                   const int32_t* bins, int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels,
                                   int32_t center, int32_t power, float scale, float* dx, rh_stream_t stream) {
    MelP p = {};
    const int rc = mel_diff_params("mel_diff_bwd", dmel, dx, x, window, twiddle, fb, bins, rows, t_len, n_fft, hop, n_mels, center, power,
                                   scale, p);
    if (rc != RH_OK) return rc;
    p.dmel = dmel; p.dx = dx;
    return fft_dispatch<2048>(n_fft, [&](auto n) { return launch_mel_bwd<decltype(n)::value>(p, (int)rows, (hipStream_t)stream); });
}
