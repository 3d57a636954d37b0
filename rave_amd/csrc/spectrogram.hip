// torchaudio.transforms.Spectrogram(power=None) with a gradient: the front end of the spectral discriminators
// (rave/discriminator.py:12-20,147-152: n_fft, hop n_fft / 4, normalized, center=False, then cat([s.real, s.imag], 1)) and of
// the descript MRD (rave/descript_discriminator.py:153-160: center=True, reflect).  One launch per direction, no atomics, no
// scratch in HBM.
//
// Forward, x (rows, T) -> out: framing (reflect_at for centred frames: no padded copy), window, real DFT, scale, and the
// (real, imag) planes written frame-minor.  rows = batch * channels; plane p of row (b, c) is channel p * channels + c of batch
// b in out (batch, 2 channels, bins, frames): the reference's cat([real, imag], 1) itself; with channels = 1 out is
// (rows, 2, bins, frames).
//   * n_fft <= 2048: frames f and f + 1 of a row as one equalised pair; n_fft = 4096: one frame on the packed scheme
//     (fft_lds.inc has the transform and both schemes).
//   * a workgroup owns FPW consecutive frames of a row and collects both planes in an LDS tile [plane][bin][frame]; the
//     tile leaves in runs of FPW consecutive frames per bin (float4 where `out` and the frame count allow it).
//
// Backward, dout -> dx (rows, T): the exact adjoint.  The transpose of the real DFT is
//   y[n] = sum_{k <= n/2} gr_k cos(2 pi k n / N) - gi_k sin(2 pi k n / N) = Re FFT(gr - i gi, zero above N / 2)[n]
// (no Hermitian doubling: bins 1 .. N/2 - 1 count ONCE), then the window, then overlap-add, with the reflected edges of
// centred frames folded back.  Re FFT(H) = FFT of the Hermitian part S of H (S_k = H_k / 2, S_{N-k} = conj H_k / 2,
// S_0 = Re H_0, S_{N/2} = Re H_{N/2}), which is real: two frames ride one complex transform as Sa + i Sb (n_fft <= 2048);
// at 4096 the real 4096-point result comes out of the 2048-point transform of A + i B, A_k = S_k + S_{k+M},
// B_k = W^k (S_k - S_{k+M}), as z[m] = y[2m] + i y[2m+1].
//   * decomposition: a workgroup OWNS a span of dx of one row and transforms every frame that covers the span (or, at the
//     edges of a centred row, its mirror images): (SPAN + n_fft) / hop frames for SPAN / hop frames' worth of output --
//     19 for 16 at hop = n_fft / 4 (11 for 8 at 4096) -- in exchange for one launch, no workspace and one writer per sample.
//   * dout is staged FPW frames at a time into the same LDS tile (runs of FPW frames per bin, float4 where possible);
//     after each round of transforms the windowed frames lie in LDS in natural order and every thread GATHERS what its own
//     samples (registers) get from them: frames in ascending order, direct before reflected.  One fixed order of additions:
//     the same bits on every run, whatever the grid.
#include <cstdint>
#include "common.hpp"

namespace {

#include "fft_lds.inc"

template <int N>
struct SpecGeom {
    static constexpr bool PK = N == 4096;                       // one real frame packed into a complex transform of N / 2
    static constexpr int M = PK ? N / 2 : N;                    // points of the complex transform
    typedef Fft<M> F;
    static constexpr int FPR = PK ? 1 : 2 * F::G;               // frames per round of transforms
    static constexpr int FPW = 8192 / N > FPR ? 8192 / N : FPR; // frames per tile (a multiple of FPR)
    static constexpr int TS = PK ? FPW : FPW + 1;               // row stride of the tile (odd: conflict-free columns; 4096: what fits)
    static constexpr int NB = N / 2 + 1;                        // bins
    static constexpr int SPAN = N >= 2048 ? 8192 : (N == 1024 ? 4096 : 2048);    // samples of dx a backward workgroup owns
    static constexpr int SPT = SPAN / 256;                      // ... per thread
};

struct SpecP {
    const float* x;          // forward: the signal; backward: unused
    const float* win;
    const c32* tw;           // e^{-2 pi i k / n_fft}, k < n_fft
    float* out;              // forward: the planes; backward: unused
    const float* dout;
    float* dx;
    int t_len, hop, n_frames, center, channels;
    float scale;             // 1 / sqrt(sum(window^2)) (normalized) or 1
};

// first channel (plane 0) of `row` in (batch, 2 channels, bins, frames); plane 1 is `channels` further
__device__ __forceinline__ long plane0_of(int row, int channels) {
    const int b = row / channels;
    return (long)b * 2 * channels + (row - b * channels);
}

// the tile [2 NB][TS] (frames f0 .. f0 + FPW) <-> the planes of one row; float4 where `vec` (16-byte aligned base, n_frames
// a multiple of 4; f0 is one by construction)
template <int N, bool STORE>
__device__ __forceinline__ void tile_io(float* tile, float* __restrict__ g, long ch0, int channels, int n_frames, int f0, bool vec,
                                        int tid) {
    typedef SpecGeom<N> S;
    constexpr int NB = S::NB, FPW = S::FPW, TS = S::TS;
    const int nf = min(FPW, n_frames - f0);
    if (FPW % 4 == 0 && vec) {
        constexpr int Q = FPW / 4 > 0 ? FPW / 4 : 1;
        for (int i = tid; i < 2 * NB * Q; i += 256) {
            const int pk = i / Q, j = (i - pk * Q) * 4;
            const int pl = pk >= NB ? 1 : 0, k = pk - pl * NB;
            float* gp = g + ((ch0 + (long)pl * channels) * NB + k) * n_frames + f0 + j;
            float* tp = tile + pk * TS + j;
            if (j + 4 <= nf) {
                if (STORE) {
                    *reinterpret_cast<float4*>(gp) = make_float4(tp[0], tp[1], tp[2], tp[3]);
                } else {
                    const float4 q = *reinterpret_cast<const float4*>(gp);
                    tp[0] = q.x; tp[1] = q.y; tp[2] = q.z; tp[3] = q.w;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (STORE) {
                        if (j + e < nf) gp[e] = tp[e];
                    } else {
                        tp[e] = j + e < nf ? gp[e] : 0.f;
                    }
                }
            }
        }
    } else {
        for (int i = tid; i < 2 * NB * FPW; i += 256) {
            const int pk = i / FPW, j = i - pk * FPW;
            const int pl = pk >= NB ? 1 : 0, k = pk - pl * NB;
            float* gp = g + ((ch0 + (long)pl * channels) * NB + k) * n_frames + f0 + j;
            if (STORE) {
                if (j < nf) *gp = tile[pk * TS + j];
            } else {
                tile[pk * TS + j] = j < nf ? *gp : 0.f;
            }
        }
    }
}

__device__ __forceinline__ bool vec_ok(const void* p, int n_frames) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (n_frames & 3) == 0;
}

// ------------------------------------------------------------------------------------------------------------- forward
template <int N>
__global__ __launch_bounds__(256) void spec_fwd_kernel(const SpecP p) {
    typedef SpecGeom<N> S;
    typedef typename S::F F;
    constexpr int TPF = F::TPF, G = F::G, NB = S::NB, TS = S::TS;
    __shared__ c32 zb[G * F::ZP];
    __shared__ float tile[2 * NB * TS];
    __shared__ c32 fmx[4];
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int f0 = blockIdx.x * S::FPW;
    const int f1 = min(f0 + S::FPW, p.n_frames);
    const int off = p.center ? N / 2 : 0;
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    c32* z = zb + gi * F::ZP;
    typename F::Tw tw;
    tw.init(t, p.tw);
    float wn[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
    const float scale = p.scale;
    float sc = 1.f, isc = 1.f;       // equaliser of the current pair and its inverse (frame_scale)
    float* ta = tile;
    auto bin = [&](int k, c32 z1, c32 z2) {
        c32 A, B;
        pair_split(z1, z2, 0.5f * scale, 0.5f * scale * isc, A, B);
        ta[k * TS] = A.x;
        ta[(NB + k) * TS] = A.y;
        ta[k * TS + 1] = B.x;
        ta[(NB + k) * TS + 1] = B.y;
    };
    c32 vn[8];
    load_pair<N>(vn, xr, p.t_len, p.hop, off, f0 + 2 * gi, f0 + 2 * gi < f1, f0 + 2 * gi + 1 < f1, t);
    for (int fr = f0; fr < f0 + S::FPW; fr += S::FPR) {          // the same trip count for every thread (barriers inside)
        const int fa = fr + 2 * gi;
        ta = tile + (fa - f0);
        c32 v[8];
        frame_scale<TPF>(vn, fmx, sc, isc, 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(vn[r].x, vn[r].y * sc) * wn[r];
        // the next round's samples fly under this one's passes
        load_pair<N>(vn, xr, p.t_len, p.hop, off, fa + S::FPR, fa + S::FPR < f1, fa + S::FPR + 1 < f1, t);
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
        F::sync();                                              // the spectrum is read: z is free for the next round
    }
    __syncthreads();
    tile_io<N, true>(tile, p.out, plane0_of(row, p.channels), p.channels, p.n_frames, f0, vec_ok(p.out, p.n_frames), tid);
}

// the 4096-point real frame rides the 2048-point complex transform
struct Packed {
    typedef Fft<2048> F;
    static_assert(F::TPF == 256 && F::G == 1, "one transform per workgroup");
};

__global__ __launch_bounds__(256) void spec_fwd4096_kernel(const SpecP p) {
    typedef SpecGeom<4096> S;
    typedef Packed::F F;
    constexpr int M = 2048, NB = S::NB, TS = S::TS;
    __shared__ c32 z[F::ZP];
    __shared__ float tile[2 * NB * TS];
    const int t = threadIdx.x;
    const int row = blockIdx.y;
    const int f0 = blockIdx.x * S::FPW;
    const int f1 = min(f0 + S::FPW, p.n_frames);
    const int off = p.center ? M : 0;
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    typename F::Tw tw;
    tw.template init<2>(t, p.tw);
    c32 wk[8], wn[8];                           // W^k of the bins k = t + 256 q; the window at the samples 2m, 2m + 1, m = t + 256 r
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int m = t + 256 * q;
        wk[q] = p.tw[m];
        wn[q] = mk(p.win[2 * m], p.win[2 * m + 1]);
    }
    const float scale = p.scale;
    for (int j = 0; j < S::FPW; ++j) {
        const int f = f0 + j;
        const bool valid = f < f1;
        const int p0 = f * p.hop - off;
        c32 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int q = p0 + 2 * (t + 256 * r);
            const c32 a = valid ? mk(xr[reflect_at(q, p.t_len)], xr[reflect_at(q + 1, p.t_len)]) : mk(0.f, 0.f);
            v[r] = a * wn[r];
        }
        F::run(v, z, t, tw);
        F::store_natural(v, z, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = t + 256 * q;
            const c32 zk = z[zpad(k)], zm = z[zpad((M - k) & (M - 1))];
            c32 e, o;
            pair_split(zk, zm, 0.5f, 0.5f, e, o);
            const c32 u = e + cmul(o, wk[q]);
            tile[k * TS + j] = u.x * scale;
            tile[(NB + k) * TS + j] = u.y * scale;
            if (k == 0) {                                              // the Nyquist bin: E_0 - O_0, real
                tile[M * TS + j] = (e.x - o.x) * scale;
                tile[(NB + M) * TS + j] = 0.f;
            }
        }
        F::sync();                                                     // the spectrum is read: z is free for the next frame
    }
    __syncthreads();
    tile_io<4096, true>(tile, p.out, plane0_of(row, p.channels), p.channels, p.n_frames, f0, false, t);
}

// ------------------------------------------------------------------------------------------------------------ backward
template <int N>
__global__ __launch_bounds__(256) void spec_bwd_kernel(const SpecP p) {
    typedef SpecGeom<N> S;
    typedef typename S::F F;
    constexpr bool PK = S::PK;
    constexpr int M = S::M, TPF = F::TPF, G = F::G, NB = S::NB, TS = S::TS, FPW = S::FPW, FPR = S::FPR, SPT = S::SPT, RF = F::RF;
    __shared__ c32 zb[G * F::ZP];
    __shared__ float tile[2 * NB * TS];
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int T = p.t_len, hop = p.hop, n_frames = p.n_frames;
    const int s0 = blockIdx.x * S::SPAN, s1 = min(s0 + S::SPAN, T);
    const int off = p.center ? N / 2 : 0;
    // the frames that can reach the span: those over [lo, hi], which holds the span and, at the edges of a centred row, its
    // mirror images (a superset is harmless: the gather tests every sample's own coverage)
    const bool left = p.center && s0 <= N / 2, right = p.center && s1 - 1 >= T - 1 - N / 2;
    const int lo = left ? -min(s1 - 1, N / 2) : s0;
    const int hi = right ? 2 * (T - 1) - max(s0, T - 1 - N / 2) : s1 - 1;
    const int num = lo + off - N + 1;
    int fmin = num <= 0 ? 0 : (num + hop - 1) / hop;
    const int fmax = min((hi + off) / hop, n_frames - 1);
    if (FPW % 4 == 0) fmin &= ~3;                                       // tile rows start on a 16-byte boundary of dout
    const bool vec = vec_ok(p.dout, n_frames);
    const long ch0 = plane0_of(row, p.channels);
    c32* z = zb + gi * F::ZP;
    const float* zf = reinterpret_cast<const float*>(zb);
    typename F::Tw tw;
    tw.template init<PK ? 2 : 1>(t, p.tw);
    // the window at the samples this thread holds when a transform ends (F::out_index), and W^k of its bins (4096)
    c32 wo[8], wk[PK ? 8 : 1];
#pragma unroll
    for (int u = 0; u < 8 / RF; ++u)
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int n = F::out_index(t, u, r);
            wo[u * RF + r] = PK ? mk(p.win[2 * n], p.win[2 * n + 1]) : mk(p.win[n], p.win[n]);
        }
    if (PK) {
#pragma unroll
        for (int q = 0; q < 8; ++q) wk[q] = p.tw[t + 256 * q];
    }
    float acc[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) acc[i] = 0.f;
    const int pt = s0 + tid;                                            // this thread's samples: pt + 256 i

    for (int fc = fmin; fc <= fmax; fc += FPW) {                        // uniform: barriers inside
        tile_io<N, false>(tile, const_cast<float*>(p.dout), ch0, p.channels, n_frames, fc, !PK && vec, tid);
        __syncthreads();
        for (int jr = 0; jr < FPW && fc + jr <= fmax; jr += FPR) {
            c32 v[8];
            if (PK) {
                const float* gr = tile + jr;
                const float* gim = tile + NB * TS + jr;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int k = t + 256 * r, km = M - k;              // km = M (k = 0) is the Nyquist bin
                    const c32 sk = k == 0 ? mk(gr[0], 0.f) : mk(0.5f * gr[k * TS], -0.5f * gim[k * TS]);
                    const c32 cm = km == M ? mk(gr[M * TS], 0.f) : mk(0.5f * gr[km * TS], 0.5f * gim[km * TS]);   // conj S_{M-k}
                    const c32 a = sk + cm, b = cmul(sk - cm, wk[r]);
                    v[r] = mk(a.x - b.y, a.y + b.x);
                }
            } else {
                const float* gr = tile + jr + 2 * gi;
                const float* gim = gr + NB * TS;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int k = t + r * TPF;
                    if (r < 4) {
                        const float ra = gr[k * TS], rb = gr[k * TS + 1], ia = gim[k * TS], ib = gim[k * TS + 1];
                        v[r] = k == 0 ? mk(ra, rb) : mk(0.5f * (ra + ib), 0.5f * (rb - ia));
                    } else {
                        const int m = N - k;
                        const float ra = gr[m * TS], rb = gr[m * TS + 1], ia = gim[m * TS], ib = gim[m * TS + 1];
                        v[r] = k == N / 2 ? mk(ra, rb) : mk(0.5f * (ra - ib), 0.5f * (ia + rb));
                    }
                }
            }
            F::run(v, z, t, tw);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = v[r] * wo[r];
            F::store_natural(v, z, t);
            __syncthreads();                                            // every group's windowed frames are in LDS
            for (int jj = 0; jj < FPR; ++jj) {
                const int f = fc + jr + jj;
                if (f >= n_frames) break;
                const int start = f * hop - off;
                // frame jj: component jj & 1 of transform jj / 2 (sample n at zpad(n)); 4096: sample n is component n & 1 of
                // point n / 2
                const float* zs = zf + (PK ? 0 : 2 * (jj >> 1) * F::ZP + (jj & 1));
                auto at = [&](int n) { return PK ? zs[2 * zpad(n >> 1) + (n & 1)] : zs[2 * zpad(n)]; };
#pragma unroll
                for (int i = 0; i < SPT; ++i) {
                    const int n = pt + 256 * i - start;
                    if ((unsigned)n < (unsigned)N) acc[i] += at(n);
                }
                if (left) {
#pragma unroll
                    for (int i = 0; i < SPT; ++i) {
                        const int pi = pt + 256 * i, n = -pi - start;
                        if (pi >= 1 && (unsigned)n < (unsigned)N) acc[i] += at(n);
                    }
                }
                if (right) {
#pragma unroll
                    for (int i = 0; i < SPT; ++i) {
                        const int pi = pt + 256 * i, n = 2 * (T - 1) - pi - start;
                        if (pi <= T - 2 && (unsigned)n < (unsigned)N) acc[i] += at(n);
                    }
                }
            }
            __syncthreads();                                            // z is free for the next round, the tile for the next load
        }
    }
    float* __restrict__ dxr = p.dx + (long)row * T;
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int pi = pt + 256 * i;
        if (pi < s1) dxr[pi] = acc[i] * p.scale;
    }
}

bool spec_shape_ok(int n_fft, int hop, int t_len, long rows, int center) {
    return fft_size_ok(n_fft, 4096) && hop >= 1 && hop <= n_fft && (center ? t_len > n_fft / 2 : t_len >= n_fft) &&
           t_len <= (1 << 30) && rows > 0 && rows < 65536;
    // t_len <= 2^30: the backward's mirror index 2 (T - 1) and the forward's look-ahead (two tiles of frames past the last one,
    // under 2^15 samples at any built size) stay inside an int
}

int frames_of(int n_fft, int hop, int t_len, int center) { return center ? t_len / hop + 1 : (t_len - n_fft) / hop + 1; }

template <int N>
int launch_fwd(const SpecP& p, int rows, hipStream_t stream) {
    const int wx = (p.n_frames + SpecGeom<N>::FPW - 1) / SpecGeom<N>::FPW;
    if constexpr (N == 4096) hipLaunchKernelGGL(spec_fwd4096_kernel, dim3(wx, rows), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(spec_fwd_kernel<N>, dim3(wx, rows), dim3(256), 0, stream, p);
    return rh_check_launch("spectrogram_fwd");
}

template <int N>
int launch_bwd(const SpecP& p, int rows, hipStream_t stream) {
    const int wx = (p.t_len + SpecGeom<N>::SPAN - 1) / SpecGeom<N>::SPAN;
    hipLaunchKernelGGL(spec_bwd_kernel<N>, dim3(wx, rows), dim3(256), 0, stream, p);
    return rh_check_launch("spectrogram_bwd");
}

int check_common(const char* what, const void* a, const void* window, const void* twiddle, const void* b, int64_t rows,
                 int32_t channels, int32_t t_len, int32_t n_fft, int32_t hop, int32_t center, float scale) {
    RH_REQUIRE(a && window && twiddle && b, RH_ERR_INVALID, "%s: null pointer", what);
    RH_REQUIRE(spec_shape_ok(n_fft, hop, t_len, rows, center), RH_ERR_UNSUPPORTED,
               "%s: unsupported geometry (n_fft %d, hop %d, t %d, rows %lld, center %d)", what, n_fft, hop, t_len, (long long)rows,
               center);
    RH_REQUIRE(channels >= 1 && rows % channels == 0, RH_ERR_INVALID, "%s: %lld rows are no multiple of %d channels", what,
               (long long)rows, channels);
    if (const int rc = check_twiddle(what, twiddle)) return rc;
    if (const int rc = check_scale(what, scale)) return rc;
    RH_REQUIRE(rows * (int64_t)(n_fft + 2) * frames_of(n_fft, hop, t_len, center) < (int64_t)1 << 40, RH_ERR_UNSUPPORTED,
               "%s: output too large", what);
    return RH_OK;
}

}  // namespace

extern "C" int rh_spectrogram_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows, int32_t center) {
    return spec_shape_ok(n_fft, hop, t_len, rows, center ? 1 : 0) ? 1 : 0;
}

extern "C" int rh_spectrogram_fwd_f32(const float* x, const float* window, const float* twiddle, int64_t rows, int32_t channels,
                                      int32_t t_len, int32_t n_fft, int32_t hop, int32_t center, float scale, float* out,
                                      rh_stream_t stream) {
    const int rc = check_common("spectrogram_fwd", x, window, twiddle, out, rows, channels, t_len, n_fft, hop, center, scale);
    if (rc != RH_OK) return rc;
    SpecP p = {};
    p.x = x; p.win = window; p.tw = reinterpret_cast<const c32*>(twiddle); p.out = out;
    p.t_len = t_len; p.hop = hop; p.center = center ? 1 : 0; p.channels = channels; p.scale = scale;
    p.n_frames = frames_of(n_fft, hop, t_len, p.center);
    return fft_dispatch<4096>(n_fft, [&](auto n) { return launch_fwd<decltype(n)::value>(p, (int)rows, (hipStream_t)stream); });
}

extern "C" int rh_spectrogram_bwd_f32(const float* dout, const float* window, const float* twiddle, int64_t rows, int32_t channels,
                                      int32_t t_len, int32_t n_fft, int32_t hop, int32_t center, float scale, float* dx,
                                      rh_stream_t stream) {
    const int rc = check_common("spectrogram_bwd", dout, window, twiddle, dx, rows, channels, t_len, n_fft, hop, center, scale);
    if (rc != RH_OK) return rc;
    SpecP p = {};
    p.dout = dout; p.win = window; p.tw = reinterpret_cast<const c32*>(twiddle); p.dx = dx;
    p.t_len = t_len; p.hop = hop; p.center = center ? 1 : 0; p.channels = channels; p.scale = scale;
    p.n_frames = frames_of(n_fft, hop, t_len, p.center);
    return fft_dispatch<4096>(n_fft, [&](auto n) { return launch_bwd<decltype(n)::value>(p, (int)rows, (hipStream_t)stream); });
}
