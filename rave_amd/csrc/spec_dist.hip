// The plain SpectralDistance of the Encodec-style loss for one STFT scale with the transform IN the kernel (rave/core.py:446-490
// without `mel`: torchaudio Spectrogram(n_fft, hop = n_fft / 4, power, normalized, center=False) of both signals, then
// rave/core.py:236-252 mean_difference(y, x, norm) summed over the norms), forward and backward.  The composition unfolds the
// 4x-overlapped frames, multiplies them by the window, transforms them on rocFFT, takes |.|^p of a (rows, bins, frames) tensor
// per signal and reduces the difference with four or five ATen launches per norm -- every one of those tensors exists only to
// become two numbers.  Here a frame lives in LDS from the windowed load to the partial sums (forward) or to the overlap-added
// gradient (backward), as in stft_loss.hip, whose structure this unit restates for uncentred frames and this distance:
//
//   * A = |scale rfft(w frame(y))|^p, B = the same of x, p = 1 or 2; frame f is samples [f hop, f hop + n), frames =
//     (t_len - n) / hop + 1, no padding.  One complex n-point transform per frame PAIR (x -> real part, y -> imaginary part),
//     equalised by a power of two (fft_lds.inc has the transform, the pair scheme and the equaliser).
//   * two transforms of the SAME samples give the same bits, the two halves of a pair transform do not (their rounding errors
//     differ): a pair whose two frames are equal sample by sample is detected (frames_equal) and its difference is 0 by
//     definition, so that identical signals have distance exactly 0 and, with sign(0) = 0, a zero gradient -- what the
//     composition gives.
//   * forward: per workgroup (a span of frames of one row, walked in order) a fixed-tree partial of sum |A - B| and
//     sum (A - B)^2 in (row, workgroup) order; one ordered finalize for ALL scales of a distance.  No atomics, no spectrum in HBM.
//   * backward: the same transform again, the cotangent g inv_n (use_l1 sign(A - B) + use_l2 2 (A - B)) taken through the power
//     (scale S / |S|, exactly 0 where |S| = 0; 2 scale^2 S) to the Hermitian-extended operand W = Wx + i Wy in place, the
//     unnormalised inverse as swap(FFT(swap(W))) -> real part = d frame_x, imaginary part = d frame_y, window, overlap-add into
//     an LDS image of the workgroup's span of the row.  A workgroup owns whole hop blocks and recomputes the 3 frames that
//     reach in from the left; frames are taken in four phases by (frame mod 4), so concurrent transforms add to disjoint
//     samples and every sample has one fixed order of additions.  Both sides ride ONE inverse transform, so a NULL side costs
//     none of its own (only its overlap-add and its store are skipped) and the other side's bits do not depend on it.
//     Samples no frame covers stay at the image's initial 0.
#include "common.hpp"

namespace {

#include "fft_lds.inc"

struct SdP {
    const float* x;
    const float* y;
    const float* win;
    const c32* tw;
    int rows, t_len, n_frames;
    int power;               // 1 or 2
    float scale;             // 1 / sqrt(sum(window^2)) or 1
    // forward
    int fpw;                 // frames per workgroup (multiple of G)
    float* part;             // [workgroups][2]
    // backward
    int cb, n_blocks;        // hop blocks per workgroup (the last one takes the remainder), blocks of the row
    const float* gout;
    float inv_n;
    float use_l1, use_l2;    // 0 or 1
    float* dx;
    float* dy;
    int accumulate;
};

// the 8 samples n = t + r n/8 of frame f of both signals (no window yet); zeros for a frame the workgroup does not own
template <int N>
__device__ __forceinline__ void load_frames(c32 (&v)[8], const float* __restrict__ xr, const float* __restrict__ yr, int f, int t,
                                            bool valid) {
    constexpr int TPF = N / 8, H = N / 4;
    if (valid) {                                             // f < n_frames: f H + N <= t_len
        const float* xa = xr + (long)f * H + t;
        const float* ya = yr + (long)f * H + t;
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(xa[r * TPF], ya[r * TPF]);
        return;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = mk(0.f, 0.f);
}

// 1 iff the two frames of a pair hold the same values sample by sample (all N samples: the TPF threads of the transform; across
// waves through `feq`, one slot per wave -- the barriers inside frame_scale and the transform that follow separate this read
// from the next frame's write).  Every thread of the workgroup must call it.
template <int TPF>
__device__ __forceinline__ int frames_equal(const c32 (&vn)[8], int* feq) {
    int ne = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) ne |= (vn[r].x != vn[r].y) ? 1 : 0;
    constexpr int W = TPF < 64 ? TPF : 64;
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) ne |= __shfl_xor(ne, o, 64);
    if (TPF > 64) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) feq[wave] = ne;
        __syncthreads();
        const int w0 = (threadIdx.x / TPF) * (TPF / 64);
        ne = 0;
#pragma unroll
        for (int i = 0; i < TPF / 64; ++i) ne |= feq[w0 + i];
    }
    return ne ? 0 : 1;
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

template <int N>
__global__ __launch_bounds__(256) void spec_dist_fwd_kernel(const SdP p) {
    typedef Fft<N> F;
    constexpr int TPF = F::TPF, G = F::G;
    __shared__ c32 zb[G * F::ZP];
    __shared__ float red[4];
    __shared__ c32 fmx[4];
    __shared__ int feq[4];
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int f0 = blockIdx.x * p.fpw;
    const int f1 = min(f0 + p.fpw, p.n_frames);
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    const float* __restrict__ yr = p.y + (long)row * p.t_len;
    c32* z = zb + gi * F::ZP;
    typename F::Tw tw;
    tw.init(t, p.tw);
    float wn[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
    float s0 = 0.f, s1 = 0.f;
    const float hs = 0.5f * p.scale;
    const bool p1 = p.power == 1;
    float sc = 1.f, isc = 1.f;       // equaliser of the current frame pair and its inverse (frame_scale)
    int same = 0;                    // the pair's two frames are equal: A - B = 0
    auto bin = [&](c32 z1, c32 z2) {
        c32 X, Y;
        pair_split(z1, z2, hs, hs * isc, X, Y);
        float b = X.x * X.x + X.y * X.y, a = Y.x * Y.x + Y.y * Y.y;      // B (of x) and A (of y) at power 2
        if (p1) {
            a = __builtin_amdgcn_sqrtf(a);
            b = __builtin_amdgcn_sqrtf(b);
        }
        const float d = same ? 0.f : a - b;
        s0 += fabsf(d);
        s1 += d * d;
    };
    c32 vn[8];
    load_frames<N>(vn, xr, yr, f0 + gi, t, f0 + gi < f1);
    for (int fb = f0; fb < f1; fb += G) {
        const bool valid = fb + gi < f1;
        c32 v[8];
        same = frames_equal<TPF>(vn, feq);
        frame_scale<TPF>(vn, fmx, sc, isc, 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mk(vn[r].x, vn[r].y * sc) * wn[r];
        load_frames<N>(vn, xr, yr, fb + G + gi, t, fb + G + gi < f1);      // the next frame's samples fly under this one's passes
        F::run(v, z, t, tw);
        F::store_natural(v, z, t);
        if (valid) {
            // bins k = t + m n/8 and their mirrors n - k = (n/8 - t) + (7 - m) n/8 (t > 0; bin 0 pairs with itself)
            const c32* zk = z + zpad(t);
            const c32* zm = z + (t ? zpad(TPF - t) : 0);
#pragma unroll
            for (int m = 0; m < 4; ++m) bin(zk[m * TPF / 8 * 9], t ? zm[(7 - m) * TPF / 8 * 9] : (m ? z[zpad(N - m * TPF)] : z[0]));
            if (t == 0) bin(z[zpad(N / 2)], z[zpad(N / 2)]);
        }
        F::sync();
    }
    const float t0 = wg_sum(s0, red), t1 = wg_sum(s1, red);
    if (tid == 0) {
        float* o = p.part + 2l * ((long)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = t0; o[1] = t1;
    }
}

// The ordered finalize of ALL scales of one distance + the sum over the scales in one launch (as stft_loss_finalize_all_kernel):
// one workgroup walks the scales, every partial is added in a fixed order.
constexpr int kSdMaxScales = 8;
struct SdFinTable {
    const float* part[kSdMaxScales];
    int nblocks[kSdMaxScales];
    int count;
    float use_l1, use_l2;
};
__global__ __launch_bounds__(256) void spec_dist_finalize_all_kernel(const SdFinTable tb, const float* __restrict__ inv_n,
                                                                     float* __restrict__ sums, float* __restrict__ out) {
    __shared__ float red[4];
    float d = 0.f;
    for (int sc = 0; sc < tb.count; ++sc) {
        const float* __restrict__ part = tb.part[sc];
        const int nblocks = tb.nblocks[sc];
        float t[2];
        for (int k = 0; k < 2; ++k) {
            float s = 0.f;
            for (int i = threadIdx.x; i < nblocks; i += 256) s += part[i * 2l + k];
            t[k] = wg_sum(s, red);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            sums[2 * sc] = t[0]; sums[2 * sc + 1] = t[1];
            d += (tb.use_l1 * t[0] + tb.use_l2 * t[1]) * inv_n[sc];
        }
    }
    if (threadIdx.x == 0) out[0] = d;
}

constexpr int kHeadBytes = 64;     // head of the backward kernel's dynamic LDS: 4 (max |x|, max |y|) slots, 4 equality slots

template <int N>
__global__ __launch_bounds__(256, 3) void spec_dist_bwd_kernel(const SdP p) {
    typedef Fft<N> F;
    constexpr int TPF = F::TPF, G = F::G, H = N / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    c32* const fmx = reinterpret_cast<c32*>(smem);           // 32 bytes: one slot per wave (frame_scale)
    int* const feq = reinterpret_cast<int*>(smem + 32);      // 16 bytes: one slot per wave (frames_equal)
    c32* const zb = reinterpret_cast<c32*>(smem + kHeadBytes);
    float* const accx = reinterpret_cast<float*>(zb + G * F::ZP);
    const int tid = threadIdx.x;
    const int gi = tid / TPF, t = tid - gi * TPF;
    const int row = blockIdx.y;
    const int b0 = blockIdx.x * p.cb;
    const int b1 = blockIdx.x == gridDim.x - 1 ? p.n_blocks : b0 + p.cb;
    const int span = (b1 - b0) * H, q0 = b0 * H;
    float* const accy = accx + span;
    const float* __restrict__ xr = p.x + (long)row * p.t_len;
    const float* __restrict__ yr = p.y + (long)row * p.t_len;
    c32* z = zb + gi * F::ZP;
    for (int i = tid; i < 2 * span; i += 256) accx[i] = 0.f;
    const int flo = max(0, b0 - 3), fhi = min(p.n_frames - 1, b1 - 1);       // frame f covers the blocks f .. f + 3
    typename F::Tw tw;
    tw.init(t, p.tw);
    float wn[8], wo[8];                                      // window at the samples this thread loads / at those it ends up with
#pragma unroll
    for (int r = 0; r < 8; ++r) wn[r] = p.win[t + r * TPF];
#pragma unroll
    for (int u = 0; u < 8 / F::RF; ++u)
#pragma unroll
        for (int r = 0; r < F::RF; ++r) wo[u * F::RF + r] = p.win[F::out_index(t, u, r)];
    const float gn = p.gout[0] * p.inv_n;
    const float l1 = gn * p.use_l1, l2 = 2.f * gn * p.use_l2;
    const float scale = p.scale, hs = 0.5f * p.scale;
    const bool p1 = p.power == 1;
    const bool want_x = p.dx != nullptr, want_y = p.dy != nullptr;
    // gradient w.r.t. the complex bins of the x and the y frame for the pair (Z_k, Z_{n-k}); `gh` = 0.5 for interior bins (their
    // Hermitian mirror carries the other half), 1 for k = 0 and n/2.  X and Y are the SCALED spectra (scale S), A = |Y|^p,
    // B = |X|^p: dA / dS = scale Y / |Y| (p = 1), 2 scale Y (p = 2).  The frame pair is equalised (frame_scale): the transform
    // carried s y, so Y = Y' / s.  The inverse transform is equalised as well, for the same reason (its rounding error is
    // ~ 1e-7 of the norm of BOTH operands): |Wx| = |Wy| at power 1 -- both are the cotangent times a unit vector -- and
    // |Wy| ~ |Wx| / s at power 2, where each is the cotangent times its own spectrum; there the operand takes s Wy and the
    // imaginary part of the inverse transform is divided by s where it is added up (powers of two: exact).
    float sc = 1.f, isc = 1.f;
    float by = 1.f, iby = 1.f;       // the inverse transform's equaliser and its inverse
    int same = 0;
    auto grads = [&](c32 z1, c32 z2, float gh, c32& gx, c32& gy) {
        c32 X, Y;
        pair_split(z1, z2, hs, hs * isc, X, Y);
        float b = X.x * X.x + X.y * X.y, a = Y.x * Y.x + Y.y * Y.y;
        if (p1) {
            a = __builtin_amdgcn_sqrtf(a);
            b = __builtin_amdgcn_sqrtf(b);
        }
        const float d = same ? 0.f : a - b;
        const float sg = d > 0.f ? l1 : (d < 0.f ? -l1 : 0.f);
        const float ca = gh * (sg + l2 * d);                 // d loss / d A; d loss / d B = -ca
        float ra, rb;
        if (p1) {
            ra = a > 0.f ? ca * scale * __builtin_amdgcn_rcpf(a) : 0.f;
            rb = b > 0.f ? -ca * scale * __builtin_amdgcn_rcpf(b) : 0.f;
        } else {
            ra = 2.f * scale * ca;
            rb = -ra;
        }
        gx = X * rb;
        gy = Y * (ra * by);
    };
    __syncthreads();
    for (int ph = 0; ph < 4; ++ph) {
        const int fs = flo + ((ph - flo) & 3);
        c32 vn[8];
        load_frames<N>(vn, xr, yr, fs + 4 * gi, t, fs + 4 * gi <= fhi);
        for (int fb = fs; fb <= fhi; fb += 4 * G) {
            const int f = fb + 4 * gi;
            const bool valid = f <= fhi;
            c32 v[8];
            same = frames_equal<TPF>(vn, feq);
            frame_scale<TPF>(vn, fmx, sc, isc, 1);
            if (!p1) { by = sc; iby = isc; }
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = mk(vn[r].x, vn[r].y * sc) * wn[r];
            load_frames<N>(vn, xr, yr, f + 4 * G, t, f + 4 * G <= fhi);
            F::run(v, z, t, tw);
            F::store_natural(v, z, t);
            // W = Wx + i Wy (Hermitian extensions of the half-weighted gradients), stored SWAPPED (im, re): the inverse
            // transform is swap(FFT(swap(W)))
            {
                c32* zk = z + zpad(t);
                c32* zm = z + (t ? zpad(TPF - t) : 0);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    c32* pk = zk + m * TPF / 8 * 9;                                        // bin k = t + m n/8
                    c32* pm = t ? zm + (7 - m) * TPF / 8 * 9 : z + zpad(N - m * TPF);      // bin n - k (unused for k = 0)
                    c32 gx, gy;
                    if (m == 0 && t == 0) {
                        grads(z[0], z[0], 1.f, gx, gy);
                        z[0] = mk(gy.x, gx.x);
                    } else {
                        grads(*pk, *pm, 0.5f, gx, gy);
                        *pk = mk(gx.y + gy.x, gx.x - gy.y);          // swap of (gx + i gy)
                        *pm = mk(gy.x - gx.y, gx.x + gy.y);          // swap of (conj gx + i conj gy)
                    }
                }
            }
            if (t == 0) {
                c32 gx, gy;
                grads(z[zpad(N / 2)], z[zpad(N / 2)], 1.f, gx, gy);
                z[zpad(N / 2)] = mk(gy.x, gx.x);
            }
            F::sync();
            {
                const c32* zt = z + zpad(t);
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
                            const c32 o = v[u * F::RF + r] * wo[u * F::RF + r];   // swapped: (d frame_y, d frame_x)
                            if (want_x) accx[loc] += o.y;
                            if (want_y) accy[loc] += o.x * iby;
                        }
                    }
            }
        }
        __syncthreads();
    }
    const int T = p.t_len;
    float* __restrict__ dxr = want_x ? p.dx + (long)row * T : nullptr;
    float* __restrict__ dyr = want_y ? p.dy + (long)row * T : nullptr;
    for (int i = tid; i < span; i += 256) {
        const int pq = q0 + i;
        if (pq >= T) break;                                   // the last block of a row may be partial
        if (dxr) dxr[pq] = p.accumulate ? dxr[pq] + accx[i] : accx[i];
        if (dyr) dyr[pq] = p.accumulate ? dyr[pq] + accy[i] : accy[i];
    }
}

constexpr int kTailMin = 6;       // a remainder shorter than this joins the previous workgroup
constexpr size_t kLdsCap = 150 * 1024;      // the cap of stft_loss.hip's backward plan: this unit never asks for more

bool shape_ok(int n_fft, int hop, int t_len, long rows, int power) {
    return fft_size_ok(n_fft, 2048) && hop * 4 == n_fft && t_len >= n_fft && t_len <= (1 << 30) && rows > 0 && rows < 65536 &&
           (power == 1 || power == 2);
}

int frames_of(int n_fft, int t_len) { return (t_len - n_fft) / (n_fft / 4) + 1; }

int chunks_of(int n_blocks, int cb) {
    int c = n_blocks / cb;
    const int rem = n_blocks - c * cb;
    if (c == 0 || rem >= kTailMin) ++c;
    return c;
}

// Hop blocks per workgroup of the backward kernel, by stft_loss.hip's estimate: a workgroup of nb blocks transforms nb + 3
// frames (3 reach in from the left) in four phases of ceil(frames of the phase / G) rounds of G transforms side by side; its
// LDS image grows with nb and bounds the workgroups per CU.  Candidates are the sizes whose phases are whole rounds
// (nb + 3 = 4 G m) plus "the whole row"; the estimate is (residency waves of the grid) x (rounds of the longest workgroup).
int rounds_of(int blocks, int first_frame_cut, int G) {
    int r = 0;
    const int frames = blocks + 3 - first_frame_cut;
    for (int ph = 0; ph < 4; ++ph) r += ((frames - ph + 3) / 4 + G - 1) / G;
    return r;
}
size_t lds_of(int n_fft, int blocks) {
    const int G = 256 / (n_fft / 8);
    return kHeadBytes + (size_t)G * (n_fft + n_fft / 8) * 8 + 2ul * blocks * (n_fft / 4) * 4;
}
int choose_cb(int n_fft, int n_blocks, long rows) {
    const int G = 256 / (n_fft / 8);
    int best = 0;
    double best_cost = 1e30;
    for (int m = 1; m <= 64; ++m) {
        int cb = 4 * G * m - 3;
        if (cb < kTailMin) continue;
        if (cb > n_blocks) cb = n_blocks;
        const int nch = chunks_of(n_blocks, cb);
        const int last = n_blocks - (nch - 1) * cb;
        const int big = last > cb ? last : cb;
        const size_t lds = lds_of(n_fft, big);
        if (lds > kLdsCap) break;
        int per_cu = (int)(160 * 1024 / lds);
        per_cu = per_cu > 3 ? 3 : per_cu;                               // __launch_bounds__(256, 3)
        const double wgs = (double)rows * nch, slots = 256.0 * per_cu;
        const int r_first = rounds_of(nch == 1 ? n_blocks : cb, 3, G);   // the first workgroup has no frames to its left
        const int r_mid = nch > 2 ? rounds_of(cb, 0, G) : 0;
        const int r_last = nch > 1 ? rounds_of(last, 0, G) : 0;
        const int r_max = r_first > r_mid ? (r_first > r_last ? r_first : r_last) : (r_mid > r_last ? r_mid : r_last);
        const double waves = wgs <= slots ? 1.0 : wgs / slots + 0.5;
        const double cost = waves * r_max * (1.0 + 0.5 / per_cu) + 0.15 * nch;      // + set-up / write-out per workgroup
        if (cost < best_cost) { best_cost = cost; best = cb; }
        if (cb == n_blocks) break;
    }
    return best ? best : n_blocks;      // (the smallest candidate always fits; launch_bwd checks the size again)
}

int fpw_of(int n_fft, int n_frames, long rows) {
    const int G = 256 / (n_fft / 8);
    int iters = (n_frames + G - 1) / G;
    // enough workgroups to fill the chip twice over, as few as that allows (per-workgroup set-up + partial sums)
    while (iters > 1 && rows * ((n_frames + G * iters - 1) / (G * iters)) < 1024) iters = (iters + 1) / 2;
    return G * iters;
}

template <int N>
int launch_fwd(SdP p, int wgs_x, hipStream_t stream) {
    hipLaunchKernelGGL(spec_dist_fwd_kernel<N>, dim3(wgs_x, p.rows), dim3(256), 0, stream, p);
    return rh_check_launch("spec_dist_fwd");
}

template <int N>
int launch_bwd(SdP p, hipStream_t stream) {
    const int nch = chunks_of(p.n_blocks, p.cb);
    const int last = p.n_blocks - (nch - 1) * p.cb;                    // blocks of the last workgroup
    const size_t lds = lds_of(N, last > p.cb ? last : p.cb);
    auto kern = spec_dist_bwd_kernel<N>;
    static bool once = false;
    if (!once) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        once = true;
    }
    if (lds > kLdsCap) {
        rh_set_error("spec_dist_bwd: span does not fit in LDS");
        return RH_ERR_INVALID;
    }
    hipLaunchKernelGGL(kern, dim3(nch, p.rows), dim3(256), lds, stream, p);
    return rh_check_launch("spec_dist_bwd");
}

// x and y are read through __restrict__ pointers next to the outputs: the two signals must be two buffers
bool ranges_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * sizeof(float);
    return pa < pb + len && pb < pa + len;
}

int check_common(const char* what, const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                 int32_t t_len, int32_t n_fft, int32_t power, float scale) {
    RH_REQUIRE(x && y && window && twiddle, RH_ERR_INVALID, "%s: null pointer", what);
    RH_REQUIRE(shape_ok(n_fft, n_fft / 4, t_len, rows, power), RH_ERR_UNSUPPORTED,
               "%s: unsupported geometry (n_fft %d, t %d, rows %ld, power %d)", what, n_fft, t_len, (long)rows, power);
    if (int rc = check_twiddle(what, twiddle)) return rc;
    if (int rc = check_scale(what, scale)) return rc;
    RH_REQUIRE(!ranges_overlap(x, y, rows * t_len), RH_ERR_INVALID, "%s: x and y overlap", what);
    return RH_OK;
}

}  // namespace

extern "C" int rh_spec_dist_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows, int32_t power) {
    return shape_ok(n_fft, hop, t_len, rows, power) ? 1 : 0;
}

extern "C" int64_t rh_spec_dist_workspace_bytes(int32_t n_fft, int32_t t_len, int64_t rows) {
    if (!shape_ok(n_fft, n_fft / 4, t_len, rows, 1)) return 0;
    const int nf = frames_of(n_fft, t_len);
    const int fpw = fpw_of(n_fft, nf, rows);
    return (int64_t)rows * ((nf + fpw - 1) / fpw) * 2 * (int64_t)sizeof(float);
}

// Diagnostics / tests (no GPU needed): out6 = {frames per forward workgroup, forward workgroups per row, hop blocks per backward
// workgroup, backward workgroups per row, hop blocks of the LAST backward workgroup, dynamic LDS bytes of the backward launch}
extern "C" int rh_spec_dist_plan_info(int32_t n_fft, int32_t t_len, int64_t rows, int64_t* out6) {
    RH_REQUIRE(out6, RH_ERR_INVALID, "spec_dist_plan_info: null output");
    RH_REQUIRE(shape_ok(n_fft, n_fft / 4, t_len, rows, 1), RH_ERR_UNSUPPORTED, "spec_dist_plan_info: unsupported geometry");
    const int H = n_fft / 4, nf = frames_of(n_fft, t_len);
    const int fpw = fpw_of(n_fft, nf, rows);
    const int n_blocks = (t_len + H - 1) / H;
    const int cb = choose_cb(n_fft, n_blocks, rows);
    const int nch = chunks_of(n_blocks, cb);
    const int last = n_blocks - (nch - 1) * cb;
    out6[0] = fpw; out6[1] = (nf + fpw - 1) / fpw; out6[2] = cb; out6[3] = nch; out6[4] = last;
    out6[5] = (int64_t)lds_of(n_fft, last > cb ? last : cb);
    return RH_OK;
}

extern "C" int rh_spec_dist_fwd_f32(const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                                    int32_t t_len, int32_t n_fft, int32_t power, float scale, void* workspace,
                                    int64_t workspace_bytes, rh_stream_t stream) {
    if (int rc = check_common("spec_dist_fwd", x, y, window, twiddle, rows, t_len, n_fft, power, scale)) return rc;
    RH_REQUIRE(workspace, RH_ERR_INVALID, "spec_dist_fwd: null pointer (workspace)");
    RH_REQUIRE(workspace_bytes >= rh_spec_dist_workspace_bytes(n_fft, t_len, rows), RH_ERR_WORKSPACE, "spec_dist_fwd: workspace too small");
    SdP p = {};
    p.x = x; p.y = y; p.win = window; p.tw = reinterpret_cast<const c32*>(twiddle);
    p.rows = (int)rows; p.t_len = t_len; p.n_frames = frames_of(n_fft, t_len); p.power = power; p.scale = scale;
    p.fpw = fpw_of(n_fft, p.n_frames, rows);
    p.part = static_cast<float*>(workspace);
    const int wx = (p.n_frames + p.fpw - 1) / p.fpw;
    return fft_dispatch<2048>(n_fft, [&](auto n) { return launch_fwd<decltype(n)::value>(p, wx, (hipStream_t)stream); });
}

extern "C" int rh_spec_dist_finalize_all_f32(const float* const* partials, const int64_t* partial_bytes, int32_t n_scales,
                                             const float* inv_n, int32_t use_l1, int32_t use_l2, float* sums, float* total,
                                             rh_stream_t stream) {
    RH_REQUIRE(partials && partial_bytes && inv_n && sums && total && n_scales > 0 && n_scales <= kSdMaxScales, RH_ERR_INVALID,
               "spec_dist_finalize_all: bad arguments (1 .. %d scales)", kSdMaxScales);
    RH_REQUIRE(use_l1 || use_l2, RH_ERR_UNSUPPORTED, "spec_dist_finalize_all: at least one norm");
    SdFinTable tb;
    for (int i = 0; i < n_scales; ++i) {
        RH_REQUIRE(partials[i] && partial_bytes[i] > 0 && partial_bytes[i] % 8 == 0 && partial_bytes[i] / 8 < 0x7fffffffl, RH_ERR_INVALID,
                   "spec_dist_finalize_all: bad partials of scale %d", i);
        tb.part[i] = partials[i];
        tb.nblocks[i] = (int)(partial_bytes[i] / 8);
    }
    tb.count = n_scales;
    tb.use_l1 = use_l1 ? 1.f : 0.f;
    tb.use_l2 = use_l2 ? 1.f : 0.f;
    hipLaunchKernelGGL(spec_dist_finalize_all_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tb, inv_n, sums, total);
    return rh_check_launch("spec_dist_finalize_all");
}

extern "C" int rh_spec_dist_bwd_f32(const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                                    int32_t t_len, int32_t n_fft, int32_t power, float scale, int32_t use_l1, int32_t use_l2,
                                    const float* grad_out, float* dx, float* dy, int32_t accumulate, rh_stream_t stream) {
    if (int rc = check_common("spec_dist_bwd", x, y, window, twiddle, rows, t_len, n_fft, power, scale)) return rc;
    RH_REQUIRE(grad_out, RH_ERR_INVALID, "spec_dist_bwd: null pointer (grad_out)");
    RH_REQUIRE(use_l1 || use_l2, RH_ERR_UNSUPPORTED, "spec_dist_bwd: at least one norm");
    if (!dx && !dy) return RH_OK;
    SdP p = {};
    p.x = x; p.y = y; p.win = window; p.tw = reinterpret_cast<const c32*>(twiddle);
    p.rows = (int)rows; p.t_len = t_len; p.n_frames = frames_of(n_fft, t_len); p.power = power; p.scale = scale;
    const int H = n_fft / 4;
    p.n_blocks = (t_len + H - 1) / H;
    p.cb = choose_cb(n_fft, p.n_blocks, rows);
    p.gout = grad_out;
    p.inv_n = (float)(1.0 / ((double)rows * p.n_frames * (n_fft / 2 + 1)));
    p.use_l1 = use_l1 ? 1.f : 0.f;
    p.use_l2 = use_l2 ? 1.f : 0.f;
    p.dx = dx; p.dy = dy; p.accumulate = accumulate;
    return fft_dispatch<2048>(n_fft, [&](auto n) { return launch_bwd<decltype(n)::value>(p, (hipStream_t)stream); });
}
