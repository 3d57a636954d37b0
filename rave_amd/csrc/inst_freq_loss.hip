// WeightedInstantaneousSpectralDistance for one STFT scale with the transform IN the kernel (rave/core.py:347-412 over
// MultiScaleSTFT(magnitude=False), rave/core.py:269-319), forward and backward.  The torch composition runs, per scale and signal,
// a complex STFT, angle, two diffs, a remainder, a cumsum over the frames and another diff through HBM, and autograd keeps every
// one of them; here a frame lives in LDS from the windowed load to the partial sums (forward) or to the overlap-added gradient
// (backward), as in stft_loss.hip, whose transform (fft_lds.inc), pair scheme and overlap-add this unit shares or restates.
//
//   * the transform runs in FLOAT64 (Fft<N, c64>, an f64 twiddle table, exact window products).  A phase is as wrong as the
//     transform's rounding error divided by |bin|, and its gradient carries 1 / |bin|^2: with the f32 pair transform
//     (error ~ 2e-7 of the spectrum's rms in every bin) the near-empty bins of ordinary signals put single IF elements and
//     the unweighted gradient of y several times further from f64 than torch's separate f32 transforms happen to be
//     (profiles/inst_freq_distance.txt, "f32 transform").  In f64 the spectrum is exact to f32 rounding, what remains is one
//     rounding of each bin, atan2f and the f32 arithmetic after it.  No equaliser is needed: two frames of very different
//     level share an f64 transform without seeing each other's noise.
//   * amplitude part: a = |X|, b = |Y|: sum (a-b)^2, sum a^2, sum |log1p a - log1p b| (no epsilon).
//   * phase part: the reference's derivative(unwrap(phi)) is derivative(cumsum(wrap(diff phi))) = wrap(diff phi)[1:] -- the
//     cumulative sum cancels -- so IF[j] = wrap(phi[j+2] - phi[j+1]), j < frames - 2, wrap(d) = ((d + pi) mod 2 pi) - pi in f32
//     with torch.remainder's sign rule.  The element belongs to frame f = j + 2 and needs the phases of frame f - 1: a
//     workgroup owns a span of frames and transforms ONE more frame to its left (if_scan keeps the phases of the last
//     G + 1 frames in an LDS ring).  phase term = sum (m IFx - m IFy)^2 with m = clip(log1p a[f], 0, 1) (weighted) or 1.
//   * exact by construction: bins 0 and n/2 leave the pair split with an imaginary part of +0 (u - u), so their phases are 0 or pi
//     and their IF is exactly 0 or -pi (wrap maps +pi and -pi to -pi, as the reference's f32 arithmetic does); a bin that is
//     exactly zero has phase 0 whatever the signs of its zeros (torch.angle(0) = 0 for the +0 a silent row gives the
//     reference; an in-LDS transform of zeros may produce -0), so a silent row has IF = 0 and a zero gradient.
//   * backward: one launch.  Pass A walks the frames flo - 1 ... fhi + 1 of the span in order and leaves
//     Q[f] = m[f]^2 (IFx[f] - IFy[f]) per bin in an LDS table; pass B is stft_loss_bwd_kernel's: the spectra again, the
//     cotangent of both spectra in place -- amplitude terms, the phase term c (Q[f] - Q[f+1]) (-im, re) / |z|^2 (+ for X, - for
//     Y; wrap has derivative 1, angle has gradient 0 at 0), the mask's gradient to the target c Q^2 / m^3 / (1 + a) where
//     log1p a <= 1 -- the unnormalised inverse, window, overlap-add into the LDS image of the span in four phases by
//     (frame mod 4), the reflected margins folded by the first / last workgroup, one coalesced write (or add) of dx / dy.
//     No atomics anywhere: the bits are reproducible.
//   * sums[0..3] = sum (a-b)^2, sum a^2, sum |log1p a - log1p b|, sum (m (IFx - IFy))^2: per-workgroup partials in
//     (row, workgroup) order, then ONE ordered finalize for all scales -> spectral_distance, phase_distance.
//   * `weighted` is a template parameter: the unweighted instances carry neither the mask's log1p in pass A nor its
//     gradient term in pass B.
#include "common.hpp"
#include <stdlib.h>

namespace {

#include "fft_lds.inc"

struct IfP {
    const float* x;
    const float* y;
    const float* win;
    const c64* tw;           // e^{-2 pi i k / n} in f64
    int rows, t_len, n_frames;
    // forward
    int fpw;                 // frames a workgroup owns
    float* part;             // [workgroups][4]
    float* if_out;           // diagnostics: (rows, 2, n/2 + 1, n_frames - 2) unweighted IFx / IFy, or NULL
    // backward
    int cb, n_blocks;        // hop blocks per workgroup (the last one takes the remainder), blocks of the padded row
    const float* sums;
    const float* gout;       // 2 device scalars: d / d spectral_distance, d / d phase_distance
    float inv_n, inv_np;     // 1 / (rows bins frames), 1 / (rows bins (frames - 2))
    float* dx;
    float* dy;
    int accumulate;
};

constexpr float kPi = 3.14159274101257324f;        // float(pi), float(2 pi): what the reference's f32 tensors see
constexpr float k2Pi = 6.28318548202514648f;

// ((d + pi) mod 2 pi) - pi.  |d| <= 2 pi, so the remainder of s = d + pi is s, s - 2 pi (exact) or, for s < 0, s + 2 pi (rounded
// once): the bits of fmod followed by torch.remainder's sign fix.
__device__ __forceinline__ float wrap_pi(float d) {
    float s = d + kPi;
    if (s >= k2Pi) s -= k2Pi;
    else if (s < 0.f) s += k2Pi;
    return s - kPi;
}

__device__ __forceinline__ float phase_of(c32 z) { return (z.x == 0.f && z.y == 0.f) ? 0.f : atan2f(z.y, z.x); }

// the 8 samples n = t + r n/8 of frame f of both signals (no window yet)
template <int N>
__device__ __forceinline__ void load_frames(c32 (&v)[8], int t_len, const float* __restrict__ xr, const float* __restrict__ yr,
                                            int f, int t, bool valid) {
    constexpr int TPF = N / 8, H = N / 4;
    const int p0 = f * H - N / 2;
    if (valid && p0 >= 0 && p0 + N <= t_len) {
        const float* xa = xr + p0 + t;
        const float* ya = yr + p0 + t;
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(xa[r * TPF], ya[r * TPF]);
        return;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float a = 0.f, b = 0.f;
        if (valid) {
            const int q = reflect_at(p0 + t + r * TPF, t_len);
            a = xr[q];
            b = yr[q];
        }
        v[r] = mk(a, b);
    }
}

__device__ __forceinline__ float wg_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// fn(k, Z_k, Z_{n-k}) for the bins of one transform this thread owns: k = t + m n/8, m < 4, and k = n/2 for t = 0
template <int N, class Fn>
__device__ __forceinline__ void each_bin(const c64* z, int t, Fn&& fn) {
    constexpr int TPF = N / 8;
    const c64* zk = z + zpad(t);
    const c64* zm = z + (t ? zpad(TPF - t) : 0);
#pragma unroll
    for (int m = 0; m < 4; ++m) fn(t + m * TPF, zk[m * TPF / 8 * 9], t ? zm[(7 - m) * TPF / 8 * 9] : (m ? z[zpad(N - m * TPF)] : z[0]));
    if (t == 0) fn(N / 2, z[zpad(N / 2)], z[zpad(N / 2)]);
}

// The pair split of fft_lds.inc's pair_split in f64, rounded to f32 once: X = (Z_k + conj Z_{n-k}) / 2, Y = (Z_k - conj Z_{n-k}) / 2i.
// For k = 0 and n/2 (z1 = z2) both imaginary parts are u - u = +0.
__device__ __forceinline__ void split64(c64 z1, c64 z2, c32& X, c32& Y) {
    X = mk((float)(0.5 * (z1.x + z2.x)), (float)(0.5 * (z1.y - z2.y)));
    Y = mk((float)(0.5 * (z1.y + z2.y)), (float)(0.5 * (z2.x - z1.x)));
}

// The frames [fs, fe) of one row pair in order, G side by side per round: transform, phases of both spectra into the ring
// (slot = (frame - fs) mod (G + 1): the G frames of a round and the one before them), then per owned bin
// sink(f, k, a, b, IFx, IFy, has_if) with has_if = the element f - 2 exists and frame f - 1 was walked.  Every thread of
// the workgroup must call it; it returns after a barrier (z, ring free).
template <int N, class Sink>
__device__ __forceinline__ void if_scan(const IfP& p, const float* __restrict__ xr, const float* __restrict__ yr, int fs, int fe,
                                        c64* zb, c32* ring, Sink&& sink) {
    typedef Fft<N, c64> F;
    constexpr int TPF = F::TPF, G = F::G, NB = N / 2 + 1;
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    c64* z = zb + gi * F::ZP;
    typename F::Tw tw;
    tw.init(t, p.tw);
    float wn[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
    c32 vn[8];
    load_frames<N>(vn, p.t_len, xr, yr, fs + gi, t, fs + gi < fe);
    for (int fb = fs; fb < fe; fb += G) {
        const int f = fb + gi;
        const bool valid = f < fe;
        c64 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk((double)vn[r].x * (double)wn[r], (double)vn[r].y * (double)wn[r]);      // exact products
        load_frames<N>(vn, p.t_len, xr, yr, f + G, t, f + G < fe);
        F::run(v, z, t, tw);
        F::store_natural(v, z, t);
        const int slot = (f - fs) % (G + 1);
        c32* rw = ring + slot * NB;
        const c32* rp = ring + (slot ? slot - 1 : G) * NB;
        if (valid) {
            each_bin<N>(z, t, [&](int k, c64 z1, c64 z2) {
                c32 X, Y;
                split64(z1, z2, X, Y);
                rw[k] = mk(phase_of(X), phase_of(Y));
            });
        }
        __syncthreads();
        if (valid) {
            const bool has = f >= 2 && f > fs;
            each_bin<N>(z, t, [&](int k, c64 z1, c64 z2) {
                c32 X, Y;
                split64(z1, z2, X, Y);
                const float a = __builtin_amdgcn_sqrtf(X.x * X.x + X.y * X.y), b = __builtin_amdgcn_sqrtf(Y.x * Y.x + Y.y * Y.y);
                float ifx = 0.f, ify = 0.f;
                if (has) {
                    const c32 ph = rw[k], pp = rp[k];
                    ifx = wrap_pi(ph.x - pp.x);
                    ify = wrap_pi(ph.y - pp.y);
                }
                sink(f, k, a, b, ifx, ify, has);
            });
        }
        __syncthreads();
    }
}

template <bool W>
__device__ __forceinline__ float mask_of(float a) {
    return W ? fminf(log1pf(a), 1.f) : 1.f;          // clip(log1p a, 0, 1): a >= 0
}

template <int N, bool W>
__global__ __launch_bounds__(256) void inst_freq_fwd_kernel(const IfP p) {
    typedef Fft<N, c64> F;
    constexpr int G = F::G, NB = N / 2 + 1;
    __shared__ c64 zb[G * F::ZP];
    __shared__ c32 ring[(G + 1) * NB];
    __shared__ float red[4];
    const int row = blockIdx.y;
    const int f0 = blockIdx.x * p.fpw;
    const int f1 = min(f0 + p.fpw, p.n_frames);
    const int fs = f0 > 0 ? f0 - 1 : 0;
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    const float* __restrict__ yr = p.y + (long)row * p.t_len;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const long nif = p.n_frames - 2;
    float* __restrict__ dbg = p.if_out ? p.if_out + (long)row * 2 * NB * nif : nullptr;
    if_scan<N>(p, xr, yr, fs, f1, zb, ring, [&](int f, int k, float a, float b, float ifx, float ify, bool has) {
        if (f < f0) return;
        const float d = a - b;
        s0 += d * d;
        s1 += a * a;
        s2 += fabsf(log1pf(a) - log1pf(b));
        if (has) {
            const float m = mask_of<W>(a);
            const float e = m * ifx - m * ify;
            s3 += e * e;
            if (dbg) {
                dbg[(long)k * nif + f - 2] = ifx;
                dbg[((long)NB + k) * nif + f - 2] = ify;
            }
        }
    });
    const float t0 = wg_sum(s0, red), t1 = wg_sum(s1, red), t2 = wg_sum(s2, red), t3 = wg_sum(s3, red);
    if (threadIdx.x == 0) {
        float* o = p.part + 4l * (blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
    }
}

// The ordered finalize of ALL scales + the two sums over the scales in one launch (as stft_loss_finalize_all_kernel)
constexpr int kIfMaxScales = 8;
struct IfFinTable {
    const float* part[kIfMaxScales];
    int nblocks[kIfMaxScales];
    int count;
};
__global__ __launch_bounds__(256) void inst_freq_finalize_all_kernel(const IfFinTable tb, const float* __restrict__ inv_n,
                                                                     float* __restrict__ sums, float* __restrict__ out) {
    __shared__ float red[4];
    float d = 0.f, ph = 0.f;
    for (int sc = 0; sc < tb.count; ++sc) {
        const float* __restrict__ part = tb.part[sc];
        const int nblocks = tb.nblocks[sc];
        float t[4];
        for (int k = 0; k < 4; ++k) {
            float s = 0.f;
            for (int i = threadIdx.x; i < nblocks; i += 256) s += part[i * 4 + k];
            t[k] = wg_sum(s, red);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            for (int k = 0; k < 4; ++k) sums[4 * sc + k] = t[k];
            d += t[0] / t[1] + t[2] * inv_n[2 * sc];
            ph += t[3] * inv_n[2 * sc + 1];
        }
    }
    if (threadIdx.x == 0) {
        out[0] = d;
        out[1] = ph;
    }
}

template <int N, bool W>
__global__ __launch_bounds__(256) void inst_freq_bwd_kernel(const IfP p) {
    typedef Fft<N, c64> F;
    constexpr int TPF = F::TPF, G = F::G, H = N / 4, NB = N / 2 + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    c64* const zb = reinterpret_cast<c64*>(smem);
    c32* const ring = reinterpret_cast<c32*>(zb + G * F::ZP);
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int b0 = blockIdx.x * p.cb;
    const int b1 = blockIdx.x == gridDim.x - 1 ? p.n_blocks : b0 + p.cb;
    const int span = (b1 - b0) * H, q0 = b0 * H;
    const int flo = max(0, b0 - 3), fhi = min(p.n_frames - 1, b1 - 1);
    const int thi = min(p.n_frames - 1, fhi + 1);            // the table holds frames flo ... thi
    float* const tab = reinterpret_cast<float*>(ring + (G + 1) * NB);
    float* const accx = tab + (thi - flo + 1) * NB;
    float* const accy = accx + span;
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    const float* __restrict__ yr = p.y + (long)row * p.t_len;
    c64* z = zb + gi * F::ZP;
    for (int i = tid; i < 2 * span; i += 256) accx[i] = 0.f;
    // pass A: Q[f][k] = m^2 (IFx - IFy) (0 where the element does not exist)
    if_scan<N>(p, xr, yr, max(0, flo - 1), thi + 1, zb, ring, [&](int f, int k, float a, float b, float ifx, float ify, bool has) {
        if (f < flo) return;
        const float m = mask_of<W>(a);
        tab[(f - flo) * NB + k] = has ? m * (m * ifx - m * ify) : 0.f;
    });
    typename F::Tw tw;
    tw.init(t, p.tw);
    float wn[8], wo[8];                                      // window at the samples this thread loads / at those it ends up with
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
#pragma unroll
    for (int u = 0; u < 8 / F::RF; ++u)
#pragma unroll
        for (int r = 0; r < F::RF; ++r) wo[u * F::RF + r] = p.win[F::out_index(t, u, r)];
    const float gs = p.gout[0], A = p.sums[0], B = p.sums[1];
    const float invB = 1.f / B;
    const float c1 = gs * 2.f * invB, c2 = gs * 2.f * A * invB * invB, invN = gs * p.inv_n;
    const float cp = p.gout[1] * 2.f * p.inv_np;
    // gradient w.r.t. the complex bins of X and Y for the pair (Z_k, Z_{n-k}); gh = 0.5 for interior bins (their Hermitian
    // mirror carries the other half), 1 for k = 0 and n/2 (whose imaginary cotangent the real signal cannot see: only .x is
    // used).  qf = Q[f][k], qn = Q[f+1][k].
    auto grads = [&](c64 z1, c64 z2, float gh, float qf, float qn, c64& gx, c64& gy) {
        c32 X, Y;
        split64(z1, z2, X, Y);
        const float a2 = X.x * X.x + X.y * X.y, b2 = Y.x * Y.x + Y.y * Y.y;
        const float a = __builtin_amdgcn_sqrtf(a2), b = __builtin_amdgcn_sqrtf(b2);
        const float d = a - b;
        const float sg = d > 0.f ? invN : (d < 0.f ? -invN : 0.f);
        float da = c1 * d - c2 * a + sg / (1.f + a);
        const float db = -c1 * d - sg / (1.f + b);
        if (W) {
            const float l = log1pf(a);
            if (l <= 1.f && l > 0.f) da += cp * (qf * qf) / (l * l * l) / (1.f + a);      // m = l here: Q^2 / m^3 = m (IFx - IFy)^2
        }
        const float cph = cp * (qf - qn);
        const float ra = a > 0.f ? gh * da / a : 0.f, rb = b > 0.f ? gh * db / b : 0.f;
        const float pa = a > 0.f ? gh * cph / a2 : 0.f, pb = b > 0.f ? -gh * cph / b2 : 0.f;
        gx = mk((double)(X.x * ra - X.y * pa), (double)(X.y * ra + X.x * pa));
        gy = mk((double)(Y.x * rb - Y.y * pb), (double)(Y.y * rb + Y.x * pb));
    };
    __syncthreads();
    for (int ph = 0; ph < 4; ++ph) {
        const int fs = flo + ((ph - flo) & 3);
        c32 vn[8];
        load_frames<N>(vn, p.t_len, xr, yr, fs + 4 * gi, t, fs + 4 * gi <= fhi);
        for (int fb = fs; fb <= fhi; fb += 4 * G) {
            const int f = fb + 4 * gi;
            const bool valid = f <= fhi;
            c64 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = mk((double)vn[r].x * (double)wn[r], (double)vn[r].y * (double)wn[r]);
            load_frames<N>(vn, p.t_len, xr, yr, f + 4 * G, t, f + 4 * G <= fhi);
            F::run(v, z, t, tw);
            F::store_natural(v, z, t);
            // W = Wx + i Wy (Hermitian extensions of the half-weighted gradients), stored SWAPPED (im, re): the inverse
            // transform is swap(FFT(swap(W)))
            {
                const float* tq = tab + (valid ? f - flo : 0) * NB;
                const bool nx = valid && f + 1 <= thi;
                auto q = [&](int k, float& qf, float& qn) {
                    qf = valid ? tq[k] : 0.f;
                    qn = nx ? tq[NB + k] : 0.f;
                };
                c64* zk = z + zpad(t);
                c64* zm = z + (t ? zpad(TPF - t) : 0);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    c64* pk = zk + m * TPF / 8 * 9;                                        // bin k = t + m n/8
                    c64* pm = t ? zm + (7 - m) * TPF / 8 * 9 : z + zpad(N - m * TPF);      // bin n - k (unused for k = 0)
                    c64 gx, gy;
                    float qf, qn;
                    q(t + m * TPF, qf, qn);
                    if (m == 0 && t == 0) {
                        grads(z[0], z[0], 1.f, qf, qn, gx, gy);
                        z[0] = mk(gy.x, gx.x);
                    } else {
                        grads(*pk, *pm, 0.5f, qf, qn, gx, gy);
                        *pk = mk(gx.y + gy.x, gx.x - gy.y);          // swap of (gx + i gy)
                        *pm = mk(gy.x - gx.y, gx.x + gy.y);          // swap of (conj gx + i conj gy)
                    }
                }
                if (t == 0) {
                    c64 gx, gy;
                    float qf, qn;
                    q(N / 2, qf, qn);
                    grads(z[zpad(N / 2)], z[zpad(N / 2)], 1.f, qf, qn, gx, gy);
                    z[zpad(N / 2)] = mk(gy.x, gx.x);
                }
            }
            F::sync();
            {
                const c64* zt = z + zpad(t);
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = zt[r * TPF / 8 * 9];
            }
            F::sync();
            F::run(v, z, t, tw);
            if (valid) {
#pragma unroll
                for (int u = 0; u < 8 / F::RF; ++u)
#pragma unroll
                    for (int r = 0; r < F::RF; ++r) {
                        const int loc = f * H + F::out_index(t, u, r) - q0;
                        if (loc >= 0 && loc < span) {
                            const c64 o = v[u * F::RF + r] * (double)wo[u * F::RF + r];   // swapped: (d frame_y, d frame_x)
                            accx[loc] += (float)o.y;
                            accy[loc] += (float)o.x;
                        }
                    }
            }
        }
        __syncthreads();
    }
    const int T = p.t_len;
    if (b0 == 0) {                                                                // left margin: padded q < n/2 folds onto n/2 + (n/2 - q)
        for (int i = tid + 1; i <= N / 2; i += 256) {
            accx[N / 2 + i] += accx[N / 2 - i];
            accy[N / 2 + i] += accy[N / 2 - i];
        }
        __syncthreads();
    }
    if (b1 == p.n_blocks) {                                                       // right margin: q = T + n/2 + i folds onto T + n/2 - 2 - i
        for (int i = tid; i < N / 2; i += 256) {
            const int qs = T + N / 2 + i - q0, qt = T + N / 2 - 2 - i - q0;
            if (qs < span && qt >= 0) {
                accx[qt] += accx[qs];
                accy[qt] += accy[qs];
            }
        }
        __syncthreads();
    }
    float* __restrict__ dxr = p.dx ? p.dx + (long)row * T : nullptr;
    float* __restrict__ dyr = p.dy ? p.dy + (long)row * T : nullptr;
    for (int i = tid; i < span; i += 256) {
        const int pq = q0 + i - N / 2;
        if (pq < 0 || pq >= T) continue;
        if (dxr) dxr[pq] = p.accumulate ? dxr[pq] + accx[i] : accx[i];
        if (dyr) dyr[pq] = p.accumulate ? dyr[pq] + accy[i] : accy[i];
    }
}

constexpr int kTailMin = 6;       // a remainder shorter than this joins the previous workgroup (the first / last one must own a
                                  // whole reflected margin and the samples it folds onto: n + 1 samples = 4 blocks + 1)
constexpr size_t kLdsMax = 160 * 1024;

bool shape_ok(int n_fft, int hop, int t_len, long rows) {
    return fft_size_ok(n_fft, 2048) && hop * 4 == n_fft &&
           t_len > n_fft / 2 && (long)t_len + 2l * n_fft < 0x7fffffffl && rows > 0 && rows < 65536;
}

int chunks_of(int n_blocks, int cb) {
    int c = n_blocks / cb;
    const int rem = n_blocks - c * cb;
    if (c == 0 || rem >= kTailMin) ++c;
    return c;
}

// dynamic LDS of a backward workgroup whose largest span is `big` hop blocks: G transforms in f64, the phase ring,
// the table (big + 3 frames reach into the span, + 1 to the right) and the two gradient images
size_t bwd_lds(int n_fft, int big) {
    const int G = 256 / (n_fft / 8), NB = n_fft / 2 + 1;
    return (size_t)G * (n_fft + n_fft / 8) * 16 + (size_t)(G + 1) * NB * 8 + (size_t)(big + 4) * NB * 4 +
           2ul * big * (n_fft / 4) * 4;
}

// Hop blocks per backward workgroup: enough workgroups to fill the chip twice where the rows allow it, spans as long as that
// allows (a workgroup transforms 5 frames it does not own in pass A and 3 in pass B), within the LDS (the last workgroup takes up
// to kTailMin - 1 more blocks).
int choose_cb(int n_fft, int n_blocks, long rows) {
    int fit = kTailMin;
    while (fit < 64 && bwd_lds(n_fft, fit + 1 + kTailMin - 1) <= kLdsMax) ++fit;
    const long want = (512 + rows - 1) / rows;
    long cb = (n_blocks + want - 1) / want;
    cb = cb < kTailMin ? kTailMin : (cb > fit ? fit : cb);
    return cb >= n_blocks ? n_blocks : (int)cb;
}

int big_of(int n_blocks, int cb) {
    const int nch = chunks_of(n_blocks, cb);
    const int last = n_blocks - (nch - 1) * cb;
    return last > cb ? last : cb;
}

// frames a forward workgroup owns: it walks one more (to its left), so whole rounds of G are G r - 1 frames (r for G = 1)
int fpw_of(int n_fft, int n_frames, long rows) {
    const int G = 256 / (n_fft / 8);
    auto own = [&](int r) { return G > 1 ? G * r - 1 : r; };
    int r = G > 1 ? (n_frames + G) / G : n_frames;           // one workgroup per row
    while (r > 1 && rows * ((n_frames + own(r) - 1) / own(r)) < 512) r = (r + 1) / 2;
    return own(r);
}

template <int N, bool W>
int launch_fwd(IfP p, int wgs_x, hipStream_t stream) {
    hipLaunchKernelGGL((inst_freq_fwd_kernel<N, W>), dim3(wgs_x, p.rows), dim3(256), 0, stream, p);
    return rh_check_launch("inst_freq_loss_fwd");
}

template <int N, bool W>
int launch_bwd(IfP p, hipStream_t stream) {
    const size_t lds = bwd_lds(N, big_of(p.n_blocks, p.cb));
    auto kern = inst_freq_bwd_kernel<N, W>;
    static bool once = false;
    if (!once) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        once = true;
    }
    if (lds > 160 * 1024) {
        rh_set_error("inst_freq_loss_bwd: span does not fit in LDS");
        return RH_ERR_INVALID;
    }
    hipLaunchKernelGGL(kern, dim3(chunks_of(p.n_blocks, p.cb), p.rows), dim3(256), lds, stream, p);
    return rh_check_launch("inst_freq_loss_bwd");
}

}  // namespace

extern "C" int rh_inst_freq_loss_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows) {
    return shape_ok(n_fft, hop, t_len, rows) ? 1 : 0;
}

extern "C" int64_t rh_inst_freq_loss_workspace_bytes(int32_t n_fft, int32_t t_len, int64_t rows) {
    if (!shape_ok(n_fft, n_fft / 4, t_len, rows)) return 0;
    const int nf = t_len / (n_fft / 4) + 1;
    const int fpw = fpw_of(n_fft, nf, rows);
    return (int64_t)rows * ((nf + fpw - 1) / fpw) * 4 * (int64_t)sizeof(float);
}

extern "C" int rh_inst_freq_loss_fwd_f32(const float* x, const float* y, const float* window, const double* twiddle, int64_t rows,
                                         int32_t t_len, int32_t n_fft, int32_t weighted, float* if_out, void* workspace,
                                         int64_t workspace_bytes, rh_stream_t stream) {
    RH_REQUIRE(x && y && window && workspace, RH_ERR_INVALID, "inst_freq_loss_fwd: null pointer");
    RH_REQUIRE(twiddle && (reinterpret_cast<uintptr_t>(twiddle) & 15) == 0, RH_ERR_INVALID, "inst_freq_loss_fwd: the f64 twiddle table must be non-null and 16-byte aligned");
    RH_REQUIRE(shape_ok(n_fft, n_fft / 4, t_len, rows), RH_ERR_UNSUPPORTED, "inst_freq_loss_fwd: unsupported geometry (n_fft %d, t %d)", n_fft, t_len);
    RH_REQUIRE(workspace_bytes >= rh_inst_freq_loss_workspace_bytes(n_fft, t_len, rows), RH_ERR_WORKSPACE, "inst_freq_loss_fwd: workspace too small");
    IfP p = {};
    p.x = x; p.y = y; p.win = window; p.tw = reinterpret_cast<const c64*>(twiddle);
    p.rows = (int)rows; p.t_len = t_len; p.n_frames = t_len / (n_fft / 4) + 1;
    p.fpw = fpw_of(n_fft, p.n_frames, rows);
    p.part = static_cast<float*>(workspace);
    p.if_out = if_out;
    const int wx = (p.n_frames + p.fpw - 1) / p.fpw;
    return fft_dispatch<2048>(n_fft, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return weighted ? launch_fwd<N, true>(p, wx, (hipStream_t)stream) : launch_fwd<N, false>(p, wx, (hipStream_t)stream);
    });
}

extern "C" int rh_inst_freq_loss_finalize_all_f32(const float* const* partials, const int64_t* partial_bytes, int32_t n_scales,
                                                  const float* inv_n, float* sums, float* out2, rh_stream_t stream) {
    RH_REQUIRE(partials && partial_bytes && inv_n && sums && out2 && n_scales > 0 && n_scales <= kIfMaxScales, RH_ERR_INVALID,
               "inst_freq_loss_finalize_all: bad arguments (1 .. %d scales)", kIfMaxScales);
    IfFinTable tb;
    for (int i = 0; i < n_scales; ++i) {
        RH_REQUIRE(partials[i] && partial_bytes[i] > 0 && partial_bytes[i] % 16 == 0 && partial_bytes[i] / 16 < 0x1fffffffl, RH_ERR_INVALID,
                   "inst_freq_loss_finalize_all: bad partials of scale %d", i);
        tb.part[i] = partials[i];
        tb.nblocks[i] = (int)(partial_bytes[i] / 16);
    }
    tb.count = n_scales;
    hipLaunchKernelGGL(inst_freq_finalize_all_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tb, inv_n, sums, out2);
    return rh_check_launch("inst_freq_loss_finalize_all");
}

extern "C" int rh_inst_freq_loss_bwd_f32(const float* x, const float* y, const float* window, const double* twiddle, int64_t rows,
                                         int32_t t_len, int32_t n_fft, int32_t weighted, const float* sums, const float* grad_out2,
                                         float* dx, float* dy, int32_t accumulate, rh_stream_t stream) {
    RH_REQUIRE(x && y && window && sums && grad_out2, RH_ERR_INVALID, "inst_freq_loss_bwd: null pointer");
    RH_REQUIRE(twiddle && (reinterpret_cast<uintptr_t>(twiddle) & 15) == 0, RH_ERR_INVALID, "inst_freq_loss_bwd: the f64 twiddle table must be non-null and 16-byte aligned");
    RH_REQUIRE(shape_ok(n_fft, n_fft / 4, t_len, rows), RH_ERR_UNSUPPORTED, "inst_freq_loss_bwd: unsupported geometry (n_fft %d, t %d)", n_fft, t_len);
    if (!dx && !dy) return RH_OK;
    IfP p = {};
    p.x = x; p.y = y; p.win = window; p.tw = reinterpret_cast<const c64*>(twiddle);
    p.rows = (int)rows; p.t_len = t_len; p.n_frames = t_len / (n_fft / 4) + 1;
    const int H = n_fft / 4;
    p.n_blocks = (t_len + n_fft + H - 1) / H;
    p.cb = choose_cb(n_fft, p.n_blocks, rows);
    p.sums = sums; p.gout = grad_out2;
    const double nb = (double)rows * (n_fft / 2 + 1);
    p.inv_n = (float)(1.0 / (nb * p.n_frames));
    p.inv_np = (float)(1.0 / (nb * (p.n_frames - 2)));
    p.dx = dx; p.dy = dy; p.accumulate = accumulate;
    return fft_dispatch<2048>(n_fft, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return weighted ? launch_bwd<N, true>(p, (hipStream_t)stream) : launch_bwd<N, false>(p, (hipStream_t)stream);
    });
}
