// General 2-D convolution (zero padding, stride, dilation in both dims, groups == 1) on the
// f32-input matrix cores, for the Conv2d stacks of the spectral discriminators:
//   rave/discriminator.py:23-74 (EncodecConvNet), rave/descript_discriminator.py:30-66,118-184 (MPD, MRD).
//
// Same implicit-GEMM view as the 1-D kernels (M = out channels, N = output positions, K = (tap,
// in channel)) but the column tile is a 2-D block of TR x TQ output positions (x nb batch items when the
// plane is small), and the staged B operand is the 2-D input patch that block needs:
//   PH = (TR-1)*is_h + tap span_h + 1 rows,  PW = (TQ-1)*is_w + tap span_w + 1 columns,
// zero-filled by (h, w) coordinates -- all four paddings come out of the staging, the im2col matrix is
// never materialised and a tap is just a constant LDS offset.  The data gradient is the same kernel run
// per output phase (alpha_h < sh, alpha_w < sw), with dy * act'(y) formed while staging.
// The weight gradient reduces over 2-D chunks (rk x wk positions of dy) per batch item; split-K partials
// + ordered reduction keep it bitwise deterministic.
//
// This unit is "family 0" of Conv2d: its four kernels, their plans and their launches.  Descriptor validation, the tap plan,
// packing, the choice between the families and the ABI are in conv2d.hip.
#include <cstdlib>
#include "conv2d_plan.hpp"
#include "f32_tile.hpp"

namespace {

struct Conv2P {
    const float* in;
    const float* wp;
    float* out;
    const float* bias;
    const float* in_mul;            // staged value *= act'(in_mul[same index])   (data gradient) or null
    int B, C, M, Mp;
    int in_h, in_w, out_h, out_w;
    int rows, qcols;                // per-phase output grid
    int is_h, is_w, os_h, os_w;
    int TQ, TR, tq_shift, tr_shift, nb, tiles_q, tiles_r;
    int PH, PW, PWp, chp;           // staged patch per (batch item, channel): PH x PW, row pitch PWp, plane pitch chp
    int ck, wlds_floats;
    unsigned magic_pw, magic_ph, magic_ck;   // ceil(2^32/d) reciprocals (0 encodes d == 1); operands stay < 2^20
    int ni, stage_floats;                    // LDS-DMA pipeline: 64-float DMA slots per plane, floats per stage
    unsigned in_bytes, w_bytes;
    int mul_act, epi_act;
    float mul_slope, epi_slope;
    int nphase;
    int ph_oph_h[kPh2], ph_oph_w[kPh2], ph_ntaps[kPh2], ph_tap0[kPh2], ph_minh[kPh2], ph_minw[kPh2];
    long ph_wofs[kPh2];
    int offh[kMaxTaps], offw[kMaxTaps];
};

struct Wgrad2P {
    const float* R;                 // dy  [B][M][r_h][r_w]
    const float* Rmul;              // y (same shape) or null: R *= act'(y)
    const float* S;                 // x   [B][C][s_h][s_w]
    float* out;                     // [Z][M][C*T]
    int B, M, C, T;
    int r_h, r_w, s_h, s_w, is_h, is_w;
    int rk, wk, wk_shift;           // dy chunk: rk rows x wk columns (wk = power of two >= 2)
    int chunks_r, chunks_w, total_chunks, chunks_per_z;
    int pr, PH, PW, PWp, chp, nc_max;
    unsigned magic_pw, magic_ph;
    int nr, ns, r_floats, stage_floats;   // LDS-DMA pipeline: 64-float slots per R row / S plane, floats per stage
    unsigned r_bytes, s_bytes;
    int minh, minw;
    int r_act;
    float r_slope;
    int offh[kMaxTaps], offw[kMaxTaps];
};

template <int TM, int TN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void conv2d_igemm_kernel(const Conv2P p) {
    constexpr int BM = TM * WM * 32;
    constexpr int NT = WM * WN * 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* w_lds = smem;
    float* x_lds = smem + p.wlds_floats;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kh = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;

    const int phase = blockIdx.z;
    const int ntaps = p.ph_ntaps[phase];
    const int tap0 = p.ph_tap0[phase];
    const int minh = p.ph_minh[phase], minw = p.ph_minw[phase];
    const float* __restrict__ wp = p.wp + p.ph_wofs[phase];

    int bx = blockIdx.x;
    const int tq = bx % p.tiles_q;
    bx /= p.tiles_q;
    const int tr = bx % p.tiles_r;
    const int bt = bx / p.tiles_r;
    const int b0 = bt * p.nb, r0 = tr * p.TR, q0 = tq * p.TQ;
    const int m0 = blockIdx.y * BM;
    const int h0 = r0 * p.is_h + minh, w0 = q0 * p.is_w + minw;

    int xb[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = (wn * TN + tn) * 32 + j;
        const int ql = col & (p.TQ - 1);
        const int rl = (col >> p.tq_shift) & (p.TR - 1);
        const int bl = col >> (p.tq_shift + p.tr_shift);
        xb[tn] = (bl * p.ck + kh) * p.chp + rl * p.is_h * p.PWp + ql * p.is_w;
    }
    const int arow = wm * TM * 32 + j + kh * BM;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    for (int c0 = 0; c0 < p.C && ntaps > 0; c0 += p.ck) {
        __syncthreads();
        // ---- stage the 2-D input patches (zero fill by coordinates = all four paddings) ----
        // flat element index -> (batch item, channel, patch row, column); U loads are issued before the first
        // LDS store so that one global-memory latency is paid per U elements, not per element
        constexpr int U = 8;
        const int total = p.nb * p.ck * p.PH * p.PW;
        for (int e0 = tid; e0 < total; e0 += NT * U) {
            float v[U];
            int dsto[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * NT;
                v[u] = 0.f;
                dsto[u] = -1;
                if (e < total) {
                    const int row = mdiv(e, p.magic_pw), w = e - row * p.PW;
                    const int bc = mdiv(row, p.magic_ph), phh = row - bc * p.PH;
                    const int bl = mdiv(bc, p.magic_ck), c = bc - bl * p.ck;
                    const int b = b0 + bl, ch = c0 + c, h = h0 + phh, gw = w0 + w;
                    dsto[u] = bc * p.chp + phh * p.PWp + w;
                    if (b < p.B && ch < p.C && h >= 0 && h < p.in_h && gw >= 0 && gw < p.in_w) {
                        const long idx = (((long)b * p.C + ch) * p.in_h + h) * p.in_w + gw;
                        v[u] = p.in[idx];
                        if (p.in_mul) v[u] *= rh_act_grad(p.in_mul[idx], p.mul_act, p.mul_slope, 0.f);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (dsto[u] >= 0) x_lds[dsto[u]] = v[u];
        }
        // ---- stage the weight tile [tap][c][BM] ----
        constexpr int V = BM / 4;
        constexpr int UW = 4;
        const int wtotal = ntaps * p.ck * V;
        for (int e0 = tid; e0 < wtotal; e0 += NT * UW) {
            f32x4 val[UW];
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const int e = e0 + u * NT;
                val[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (e < wtotal) {
                    const int kr = e / V, v4 = e - kr * V;
                    const int t = mdiv(kr, p.magic_ck), c = kr - t * p.ck;
                    const int ch = c0 + c;
                    const int m = m0 + v4 * 4;
                    if (ch < p.C && m < p.Mp)
                        val[u] = *reinterpret_cast<const f32x4*>(wp + ((long)t * p.C + ch) * p.Mp + m);
                }
            }
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const int e = e0 + u * NT;
                if (e < wtotal) *reinterpret_cast<f32x4*>(w_lds + e * 4) = val[u];
            }
        }
        __syncthreads();
        // ---- MFMA over (tap, channel pair) ----
        for (int t = 0; t < ntaps; ++t) {
            const int toff = (p.offh[tap0 + t] - minh) * p.PWp + (p.offw[tap0 + t] - minw);
            const float* wl = w_lds + t * p.ck * BM + arow;
            const float* xl = x_lds + toff;
            for (int c = 0; c < p.ck; c += 2) {
                float a[TM], b[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) a[tm] = wl[c * BM + tm * 32];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) b[tn] = xl[xb[tn] + c * p.chp];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: bias + output activation ----
    const int oph_h = p.ph_oph_h[phase], oph_w = p.ph_oph_w[phase];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = (wn * TN + tn) * 32 + j;
        const int ql = col & (p.TQ - 1);
        const int rl = (col >> p.tq_shift) & (p.TR - 1);
        const int bl = col >> (p.tq_shift + p.tr_shift);
        const int r = r0 + rl, q = q0 + ql, b = b0 + bl;
        if (r >= p.rows || q >= p.qcols || b >= p.B) continue;
        const int orow = r * p.os_h + oph_h, ocol = q * p.os_w + oph_w;
        if (orow >= p.out_h || ocol >= p.out_w) continue;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int m = m0 + (wm * TM + tm) * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * kh;
                if (m < p.M) {
                    const long idx = (((long)b * p.M + m) * p.out_h + orow) * p.out_w + ocol;
                    float v = acc[tm][tn][rr];
                    if (p.bias) v += p.bias[m];
                    p.out[idx] = rh_act_apply(v, p.epi_act, p.epi_slope, 0.f);
                }
            }
        }
    }
}

constexpr int kNI = 20;                  // max 64-float DMA slots per staged plane (PH*PW <= 1280)

// Same GEMM as conv2d_igemm_kernel, software-pipelined with asynchronous global->LDS DMA
// (buffer_load ... lds): two LDS stages, one barrier per K chunk, no staging registers.  A staged plane is
// the compact PH x PW patch; lane l of DMA slot i always fetches patch element 64 i + l, so its in-plane
// source offset (or the out-of-range marker that makes the DMA write 0.0: all four zero paddings) is
// computed ONCE per workgroup -- per K chunk only a scalar plane base changes.
template <int TM, int TN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void conv2d_dma_kernel(const Conv2P p) {
    constexpr int BM = TM * WM * 32;
    constexpr int NW = WM * WN;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kh = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;

    const int phase = blockIdx.z;
    const int ntaps = p.ph_ntaps[phase];
    const int tap0 = p.ph_tap0[phase];
    const int minh = p.ph_minh[phase], minw = p.ph_minw[phase];
    const unsigned wofs = (unsigned)p.ph_wofs[phase];

    int bx = blockIdx.x;
    const int tq = bx % p.tiles_q;
    bx /= p.tiles_q;
    const int tr = bx % p.tiles_r;
    const int bt = bx / p.tiles_r;
    const int b0 = bt * p.nb, r0 = tr * p.TR, q0 = tq * p.TQ;
    const int m0 = blockIdx.y * BM;
    const int h0 = r0 * p.is_h + minh, w0 = q0 * p.is_w + minw;

    const auto in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
    const auto w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wp), 0, p.w_bytes, 0x00020000);

    int xb[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = (wn * TN + tn) * 32 + j;
        const int ql = col & (p.TQ - 1);
        const int rl = (col >> p.tq_shift) & (p.TR - 1);
        const int bl = col >> (p.tq_shift + p.tr_shift);
        xb[tn] = (bl * p.ck + kh) * p.chp + rl * p.is_h * p.PW + ql * p.is_w;
    }
    const int arow = wm * TM * 32 + j + kh * BM;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    unsigned xo[kNI];
#pragma unroll
    for (int i = 0; i < kNI; ++i) {
        const int e = lane + 64 * i;
        const int row = mdiv(e, p.magic_pw), w = e - row * p.PW;
        const int h = h0 + row, gw = w0 + w;
        const bool ok = i < p.ni && row < p.PH && h >= 0 && h < p.in_h && gw >= 0 && gw < p.in_w;
        xo[i] = ok ? (unsigned)(h * p.in_w + gw) * 4u : kOOB;
    }
    const int planes = p.nb * p.ck;
    const unsigned plane_bytes = (unsigned)p.in_h * (unsigned)p.in_w * 4u;
    const int wrows = ntaps * p.ck;
    const int w_instrs = (wrows * BM + 255) >> 8;   // 256 floats (64 lanes x 16 B) per DMA instruction

    auto issue = [&](int c0, float* stage) {
        for (int q = wave; q < w_instrs; q += NW) {   // weights: LDS image [tap][c][BM], flat
            const int f = q * 256 + lane * 4;
            const int kr = f / BM, col = f - kr * BM;
            const int t = mdiv(kr, p.magic_ck), c = kr - t * p.ck;
            const int ch = c0 + c, m = m0 + col;
            unsigned off = kOOB;
            if (kr < wrows && ch < p.C && m < p.Mp) off = (wofs + (unsigned)(t * p.C + ch) * p.Mp + m) * 4u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_void*)(stage + q * 256), 16, off, 0, 0, 0);
        }
        float* xs = stage + p.wlds_floats;
        for (int pl = wave; pl < planes; pl += NW) {
            const int bl = mdiv(pl, p.magic_ck), c = pl - bl * p.ck;
            const int b = b0 + bl, ch = c0 + c;
            const bool dead = b >= p.B || ch >= p.C;
            const unsigned base = (unsigned)(b * p.C + ch) * plane_bytes;
            float* dst = xs + pl * p.chp;
#pragma unroll
            for (int i = 0; i < kNI; ++i) {
                if (i < p.ni) {
                    const unsigned off = (dead || xo[i] == kOOB) ? kOOB : base + xo[i];
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rsrc, (lds_void*)(dst + i * 64), 4, off, 0, 0, 0);
                }
            }
        }
    };

    const int nchunks = ntaps > 0 ? (p.C + p.ck - 1) / p.ck : 0;
    if (nchunks > 0) issue(0, smem);
    for (int i = 0; i < nchunks; ++i) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // chunk i landed for every wave; everyone is done with the other stage
        if (i + 1 < nchunks) issue((i + 1) * p.ck, smem + ((i + 1) & 1) * p.stage_floats);
        const float* w_lds = smem + (i & 1) * p.stage_floats;
        const float* x_lds = w_lds + p.wlds_floats;
        for (int t = 0; t < ntaps; ++t) {
            const int toff = (p.offh[tap0 + t] - minh) * p.PW + (p.offw[tap0 + t] - minw);
            const float* wl = w_lds + t * p.ck * BM + arow;
            const float* xl = x_lds + toff;
            int c = 0;
            for (; c + 8 <= p.ck; c += 8) {     // 4 k-steps per trip, all LDS reads in flight before the MFMAs
                float a[4][TM], b[4][TN];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) a[u][tm] = wl[(c + 2 * u) * BM + tm * 32];
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) b[u][tn] = xl[xb[tn] + (c + 2 * u) * p.chp];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][tm], b[u][tn], acc[tm][tn], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (; c < p.ck; c += 2) {
                float a[TM], b[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) a[tm] = wl[c * BM + tm * 32];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) b[tn] = xl[xb[tn] + c * p.chp];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: bias + output activation ----
    const int oph_h = p.ph_oph_h[phase], oph_w = p.ph_oph_w[phase];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = (wn * TN + tn) * 32 + j;
        const int ql = col & (p.TQ - 1);
        const int rl = (col >> p.tq_shift) & (p.TR - 1);
        const int bl = col >> (p.tq_shift + p.tr_shift);
        const int r = r0 + rl, q = q0 + ql, b = b0 + bl;
        if (r >= p.rows || q >= p.qcols || b >= p.B) continue;
        const int orow = r * p.os_h + oph_h, ocol = q * p.os_w + oph_w;
        if (orow >= p.out_h || ocol >= p.out_w) continue;
        const long cbase = ((long)b * p.M * p.out_h + orow) * p.out_w + ocol;
        const int plane = p.out_h * p.out_w;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int m = m0 + (wm * TM + tm) * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * kh;
                if (m < p.M) {
                    float v = acc[tm][tn][rr];
                    if (p.bias) v += p.bias[m];
                    p.out[cbase + (long)m * plane] = rh_act_apply(v, p.epi_act, p.epi_slope, 0.f);
                }
            }
        }
    }
}

template <int TM, int TN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void wgrad2d_kernel(const Wgrad2P p) {
    constexpr int BM = TM * WM * 32, BN = TN * WN * 32;
    constexpr int NW = WM * WN;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* r_lds = smem;                 // [BM][pr]
    float* s_lds = smem + BM * p.pr;     // [nc_max][chp]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kh = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;
    const int m0 = blockIdx.y * BM, col0 = blockIdx.x * BN, z = blockIdx.z;
    const int ncols = p.C * p.T;
    const int c_lo = col0 / p.T;

    int sb[TN], ar[TM];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        int col = col0 + (wn * TN + tn) * 32 + j;
        col = min(col, ncols - 1);
        const int c = col / p.T, t = col - c * p.T;
        sb[tn] = (c - c_lo) * p.chp + (p.offh[t] - p.minh) * p.PWp + (p.offw[t] - p.minw) + kh * p.is_w;
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) ar[tm] = ((wm * TM + tm) * 32 + j) * p.pr + kh;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int kelems = p.rk * p.wk;
    const int ch0 = z * p.chunks_per_z;
    const int ch1 = min(ch0 + p.chunks_per_z, p.total_chunks);
    for (int ch = ch0; ch < ch1; ++ch) {
        const int cw = ch % p.chunks_w;
        const int t2 = ch / p.chunks_w;
        const int cr = t2 % p.chunks_r;
        const int b = t2 / p.chunks_r;
        const int hr0 = cr * p.rk, wc0 = cw * p.wk;
        __syncthreads();
        constexpr int U = 8;
        constexpr int NT = NW * 64;
        {   // R tile: [BM][rk*wk] (kelems is a power of two)
            const int ksh = __builtin_ctz(kelems);
            const int total = BM << ksh;
            for (int e0 = tid; e0 < total; e0 += NT * U) {
                float v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = e0 + u * NT;
                    v[u] = 0.f;
                    if (e < total) {
                        const int r = e >> ksh, k = e & (kelems - 1);
                        const int rr = k >> p.wk_shift, ww = k & (p.wk - 1);
                        const int m = m0 + r, h = hr0 + rr, w = wc0 + ww;
                        if (m < p.M && h < p.r_h && w < p.r_w) {
                            const long idx = (((long)b * p.M + m) * p.r_h + h) * p.r_w + w;
                            v[u] = p.R[idx];
                            if (p.Rmul) v[u] *= rh_act_grad(p.Rmul[idx], p.r_act, p.r_slope, 0.f);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = e0 + u * NT;
                    if (e < total) r_lds[(e >> ksh) * p.pr + (e & (kelems - 1))] = v[u];
                }
            }
        }
        {   // S patches: [nc_max][PH][PW]
            const int h0 = hr0 * p.is_h + p.minh, w0 = wc0 * p.is_w + p.minw;
            const int total = p.nc_max * p.PH * p.PW;
            for (int e0 = tid; e0 < total; e0 += NT * U) {
                float v[U];
                int dsto[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = e0 + u * NT;
                    v[u] = 0.f;
                    dsto[u] = -1;
                    if (e < total) {
                        const int row = mdiv(e, p.magic_pw), w = e - row * p.PW;
                        const int cc = mdiv(row, p.magic_ph), phh = row - cc * p.PH;
                        const int c = c_lo + cc, h = h0 + phh, gw = w0 + w;
                        dsto[u] = cc * p.chp + phh * p.PWp + w;
                        if (c < p.C && h >= 0 && h < p.s_h && gw >= 0 && gw < p.s_w)
                            v[u] = p.S[(((long)b * p.C + c) * p.s_h + h) * p.s_w + gw];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (dsto[u] >= 0) s_lds[dsto[u]] = v[u];
            }
        }
        __syncthreads();
        for (int rr = 0; rr < p.rk; ++rr) {
            const float* rl = r_lds + rr * p.wk;
            const float* sl = s_lds + rr * p.is_h * p.PWp;
            for (int ww = 0; ww < p.wk; ww += 2) {
                float a[TM], bb[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) a[tm] = rl[ar[tm] + ww];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bb[tn] = sl[sb[tn] + ww * p.is_w];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], bb[tn], acc[tm][tn], 0, 0, 0);
            }
        }
    }
    float* out = p.out + (long)z * p.M * ncols;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = col0 + (wn * TN + tn) * 32 + j;
        if (col >= ncols) continue;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (m < p.M) out[(long)m * ncols + col] = acc[tm][tn][r];
            }
    }
}


constexpr int kNR = 4;    // 64-float DMA slots per R row   (rk*wk <= 256)
constexpr int kNS = 16;   // 64-float DMA slots per S plane (PH*PW <= 1024)

// Weight gradient for M <= 32 (the spectral discriminators' 32-channel stacks), LDS-DMA double-buffered:
// a workgroup owns 32 x (TN*128) of dW (a range of (c, tap) columns) for its K slice; per chunk of rk x wk
// positions of dy it stages the 32 dy rows and the input patches of its channels with asynchronous DMA
// (per-lane offsets inside a row / plane precomputed once; only validity bits and scalar bases per chunk).
template <int TN>
__global__ __launch_bounds__(256) void wgrad2d_dma_kernel(const Wgrad2P p) {
    constexpr int BN = TN * 128;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.y * 32, col0 = blockIdx.x * BN, z = blockIdx.z;
    const int ncols = p.C * p.T;
    const int c_lo = col0 / p.T;
    const int nc = min(p.nc_max, p.C - c_lo);

    const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.R), 0, p.r_bytes, 0x00020000);
    const auto s_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.S), 0, p.s_bytes, 0x00020000);

    int sb[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        int col = col0 + (wave * TN + tn) * 32 + j;
        col = min(col, ncols - 1);
        const int c = col / p.T, t = col - c * p.T;
        sb[tn] = (c - c_lo) * p.chp + (p.offh[t] - p.minh) * p.PW + (p.offw[t] - p.minw) + kh * p.is_w;
    }
    const int ar = j * p.pr + kh;

    f32x16 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tn][r] = 0.f;

    // per-lane slot geometry: (row, col) inside the dy chunk / the input patch, packed, and the element offset
    unsigned rp[kNR], ro[kNR], sp[kNS], so[kNS];
#pragma unroll
    for (int i = 0; i < kNR; ++i) {
        const int k = lane + 64 * i;
        const int rr = k >> p.wk_shift, ww = k & (p.wk - 1);
        rp[i] = ((unsigned)rr << 16) | (unsigned)ww;
        ro[i] = (unsigned)(rr * p.r_w + ww) * 4u;
    }
#pragma unroll
    for (int i = 0; i < kNS; ++i) {
        const int e = lane + 64 * i;
        const int row = mdiv(e, p.magic_pw), w = e - row * p.PW;
        sp[i] = (i < p.ns && row < p.PH) ? (((unsigned)row << 16) | (unsigned)w) : 0xffffffffu;
        so[i] = (unsigned)(row * p.s_w + w) * 4u;
    }

    auto issue = [&](int ch, float* stage) {
        const int cw = ch % p.chunks_w;
        const int t2 = ch / p.chunks_w;
        const int cr = t2 % p.chunks_r;
        const int b = t2 / p.chunks_r;
        const int hr0 = cr * p.rk, wc0 = cw * p.wk;
        unsigned rmask = 0;
#pragma unroll
        for (int i = 0; i < kNR; ++i) {
            const int rr = rp[i] >> 16, ww = rp[i] & 0xffff;
            if (i < p.nr && hr0 + rr < p.r_h && wc0 + ww < p.r_w) rmask |= 1u << i;
        }
        for (int r = wave; r < 32; r += 4) {
            const int m = m0 + r;
            const bool dead = m >= p.M;
            const unsigned base = (unsigned)(((b * p.M + m) * p.r_h + hr0) * p.r_w + wc0) * 4u;
            float* dst = stage + r * p.pr;
#pragma unroll
            for (int i = 0; i < kNR; ++i) {
                if (i < p.nr) {
                    const unsigned off = (dead || !((rmask >> i) & 1u)) ? kOOB : base + ro[i];
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(r_rsrc, (lds_void*)(dst + i * 64), 4, off, 0, 0, 0);
                }
            }
        }
        const int h0 = hr0 * p.is_h + p.minh, w0 = wc0 * p.is_w + p.minw;
        unsigned smask = 0;
#pragma unroll
        for (int i = 0; i < kNS; ++i) {
            const int h = h0 + (int)(sp[i] >> 16), gw = w0 + (int)(sp[i] & 0xffff);
            if (sp[i] != 0xffffffffu && h >= 0 && h < p.s_h && gw >= 0 && gw < p.s_w) smask |= 1u << i;
        }
        float* xs = stage + p.r_floats;
        const unsigned sbase0 = (unsigned)((h0 * p.s_w + w0) * 4);      // may wrap; only used where the sum is valid
        const unsigned plane_bytes = (unsigned)p.s_h * (unsigned)p.s_w * 4u;
        for (int cc = wave; cc < p.nc_max; cc += 4) {
            const bool dead = cc >= nc;
            const unsigned base = (unsigned)(b * p.C + c_lo + cc) * plane_bytes + sbase0;
            float* dst = xs + cc * p.chp;
#pragma unroll
            for (int i = 0; i < kNS; ++i) {
                if (i < p.ns) {
                    const unsigned off = (dead || !((smask >> i) & 1u)) ? kOOB : base + so[i];
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(s_rsrc, (lds_void*)(dst + i * 64), 4, off, 0, 0, 0);
                }
            }
        }
    };

    const int ch0 = z * p.chunks_per_z;
    const int ch1 = min(ch0 + p.chunks_per_z, p.total_chunks);
    if (ch0 < ch1) issue(ch0, smem);
    for (int ch = ch0; ch < ch1; ++ch) {
        const int i = ch - ch0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (ch + 1 < ch1) issue(ch + 1, smem + ((i + 1) & 1) * p.stage_floats);
        const float* r_lds = smem + (i & 1) * p.stage_floats + ar;
        const float* s_lds = smem + (i & 1) * p.stage_floats + p.r_floats;
        for (int rr = 0; rr < p.rk; ++rr) {
            const float* rl = r_lds + rr * p.wk;
            const float* sl = s_lds + rr * p.is_h * p.PW;
            int ww = 0;
            for (; ww + 8 <= p.wk; ww += 8) {
                float a[4], bb[4][TN];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u] = rl[ww + 2 * u];
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) bb[u][tn] = sl[sb[tn] + (ww + 2 * u) * p.is_w];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bb[u][tn], acc[tn], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (; ww < p.wk; ww += 2) {
                const float a = rl[ww];
                float bb[TN];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bb[tn] = sl[sb[tn] + ww * p.is_w];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb[tn], acc[tn], 0, 0, 0);
            }
        }
    }
    float* out = p.out + (long)z * p.M * ncols;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = col0 + (wave * TN + tn) * 32 + j;
        if (col >= ncols) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (m < p.M) out[(long)m * ncols + col] = acc[tn][r];
        }
    }
}

void fill_common(const Plan2& t, Conv2P* p, int C, int M) {
    p->C = C;
    p->M = M;
    p->Mp = round32(M);
    p->nphase = t.nphase;
    long wofs = 0;
    for (int ph = 0; ph < t.nphase; ++ph) {
        p->ph_oph_h[ph] = t.oph_h[ph];
        p->ph_oph_w[ph] = t.oph_w[ph];
        p->ph_ntaps[ph] = t.ntaps[ph];
        p->ph_tap0[ph] = t.tap0[ph];
        p->ph_minh[ph] = t.minh[ph];
        p->ph_minw[ph] = t.minw[ph];
        p->ph_wofs[ph] = wofs;
        wofs += (long)t.ntaps[ph] * C * p->Mp;
    }
    for (int i = 0; i < t.nslots; ++i) {
        p->offh[i] = t.offh[i];
        p->offw[i] = t.offw[i];
    }
}

// The four workgroup tiles of the f32-input family, by output rows: TM x TN MFMA tiles per wave, WM x WN waves.
struct Tile2 {
    int tm, tn, wm, wn;
    int bm() const { return tm * wm * 32; }
    int bn() const { return tn * wn * 32; }
};

inline Tile2 tile2_of(int M) {
    if (M <= 32) return {1, 2, 1, 4};
    if (M <= 64) return {2, 1, 1, 4};
    if (M % 96 == 0) return {3, 1, 1, 4};
    return {2, 2, 2, 2};
}

// A planned launch of conv2d_dma_kernel (dma) or conv2d_igemm_kernel on one of the four tiles; the tile plan itself is in Conv2P.
struct Launch2 {
    bool dma;
    Tile2 tile;
    size_t lds;
    dim3 grid;
};

// Register-staged kernel: the plan of last resort (an error when even that does not fit).
int plan2(Conv2P& p, const Plan2& t, const Tile2& tl, const char* what, Launch2* l) {
    const int BM = tl.bm(), BN = tl.bn();
    p.TQ = pow2ceil(p.qcols) < BN ? pow2ceil(p.qcols) : BN;
    const int tr_cap = BN / p.TQ;
    p.TR = pow2ceil(p.rows) < tr_cap ? pow2ceil(p.rows) : tr_cap;
    p.nb = BN / (p.TQ * p.TR);
    p.tq_shift = __builtin_ctz(p.TQ);
    p.tr_shift = __builtin_ctz(p.TR);
    p.tiles_q = rh_cdiv(p.qcols, p.TQ);
    p.tiles_r = rh_cdiv(p.rows, p.TR);
    const PatchGeom g = patch_geom(t);
    const int maxtaps = g.maxtaps;
    p.PH = (p.TR - 1) * p.is_h + g.span_h + 1;
    p.PW = (p.TQ - 1) * p.is_w + g.span_w + 1;
    p.PWp = p.PW | 1;
    p.chp = (p.PH * p.PWp) | 1;
    static const int budget = [] {
        const char* e = getenv("RH_CONV2D_STAGE_FLOATS");
        return e ? atoi(e) : 15 * 1024;
    }();
    const int ck = p.ck = ck_for(budget, maxtaps * BM + p.nb * p.chp, p.C, false);
    p.magic_pw = magic32(p.PW);
    p.magic_ph = magic32(p.PH);
    p.magic_ck = magic32(ck);
    p.wlds_floats = maxtaps * ck * BM;
    const size_t lds = sizeof(float) * ((size_t)p.wlds_floats + (size_t)p.nb * ck * p.chp);
    RH_REQUIRE((long)p.nb * ck * p.PH * p.PW < (1l << 20) && (long)maxtaps * ck * BM < (1l << 20), RH_ERR_UNSUPPORTED,
               "%s: tile too large", what);
    RH_REQUIRE(lds <= 160 * 1024, RH_ERR_UNSUPPORTED, "%s: tile needs %zu B of LDS", what, lds);
    const long gx = (long)rh_cdiv(p.B, p.nb) * p.tiles_r * p.tiles_q;
    RH_REQUIRE(gx < (1l << 31), RH_ERR_UNSUPPORTED, "%s: grid too large", what);
    l->dma = false;
    l->tile = tl;
    l->lds = lds;
    l->grid = dim3((unsigned)gx, rh_cdiv(p.M, BM), p.nphase);
    return RH_OK;
}

// LDS-DMA variant: kDma, or why the geometry does not fit its staging scheme (the caller then plans the register-staged kernel):
// a fused derivative, a tensor of 2 GB, a patch of more than 64 * kNI floats even at TR = 1 and TQ = 16, the LDS, the grid.
enum { kDma = 0, kNoDmaFused, kNoDmaBytes, kNoDmaPatch, kNoDmaLds, kNoDmaGrid, kNoDmaOff };
int plan2_dma(Conv2P& p, const Plan2& t, const Tile2& tl, Launch2* l) {
    const int BM = tl.bm(), BN = tl.bn();
    if (p.in_mul) return kNoDmaFused;
    const long in_b = (long)p.B * p.C * p.in_h * p.in_w * 4;
    if (in_b >= (1l << 31)) return kNoDmaBytes;
    const PatchGeom g = patch_geom(t);
    const int span_h = g.span_h, span_w = g.span_w, maxtaps = g.maxtaps;
    const long wfloats = (long)t.nslots * p.C * p.Mp;
    if (wfloats * 4 >= (1l << 31)) return kNoDmaBytes;
    int TQ = pow2ceil(p.qcols) < BN ? pow2ceil(p.qcols) : BN;
    int TR = pow2ceil(p.rows) < BN / TQ ? pow2ceil(p.rows) : BN / TQ;
    auto patch = [&](int tq_, int tr_) { return (long)((tr_ - 1) * p.is_h + span_h + 1) * ((tq_ - 1) * p.is_w + span_w + 1); };
    while (patch(TQ, TR) > 64 * kNI) {
        if (TR > 1) TR >>= 1;
        else if (TQ > 16) TQ >>= 1;
        else return kNoDmaPatch;
    }
    p.TQ = TQ; p.TR = TR;
    p.nb = BN / (TQ * TR);
    p.tq_shift = __builtin_ctz(TQ);
    p.tr_shift = __builtin_ctz(TR);
    p.tiles_q = rh_cdiv(p.qcols, TQ);
    p.tiles_r = rh_cdiv(p.rows, TR);
    p.PH = (TR - 1) * p.is_h + span_h + 1;
    p.PW = (TQ - 1) * p.is_w + span_w + 1;
    p.PWp = p.PW;
    p.ni = (p.PH * p.PW + 63) / 64;
    p.chp = p.ni * 64 + 32;                       // % 64 == 32: the two k-halves of a wave hit disjoint banks
    static const int budget = [] {
        const char* e = getenv("RH_CONV2D_DMA_STAGE_FLOATS");
        return e ? atoi(e) : 8 * 1024;
    }();
    const int ck = p.ck = ck_for(budget, maxtaps * BM + p.nb * p.chp, p.C, true);
    p.magic_pw = magic32(p.PW);
    p.magic_ph = magic32(p.PH);
    p.magic_ck = magic32(ck);
    p.wlds_floats = (maxtaps * ck * BM + 255) & ~255;
    p.stage_floats = p.wlds_floats + p.nb * ck * p.chp;
    const size_t lds = sizeof(float) * 2 * (size_t)p.stage_floats;
    if (lds > 160 * 1024) return kNoDmaLds;
    p.in_bytes = (unsigned)in_b;
    p.w_bytes = (unsigned)(wfloats * 4);
    const long gx = (long)rh_cdiv(p.B, p.nb) * p.tiles_r * p.tiles_q;
    if (gx >= (1l << 31)) return kNoDmaGrid;
    l->dma = true;
    l->tile = tl;
    l->lds = lds;
    l->grid = dim3((unsigned)gx, rh_cdiv(p.M, BM), p.nphase);
    return kDma;
}

// The family-0 launch of a forward / data gradient: the tile by output rows, the LDS-DMA kernel where its staging fits, else the
// register-staged one.  The launch and rh_conv2d_instance_info both take their answer from here.
int plan_conv2(Conv2P& p, const Plan2& t, const char* what, Launch2* l, int* no_dma_why) {
    const Tile2 tl = tile2_of(p.M);
    static const bool no_dma = getenv("RH_CONV2D_NODMA") != nullptr;
    *no_dma_why = kNoDmaOff;
    if (!no_dma) {
        Conv2P q = p;
        *no_dma_why = plan2_dma(q, t, tl, l);
        if (*no_dma_why == kDma) {
            p = q;
            return RH_OK;
        }
    }
    return plan2(p, t, tl, what, l);
}

template <int TM, int TN, int WM, int WN>
void go2(const Conv2P& p, const Launch2& l, hipStream_t stream) {
    if (l.dma) rh_launch_big_lds<conv2d_dma_kernel<TM, TN, WM, WN>>(l.grid, dim3(WM * WN * 64), l.lds, stream, p);
    else rh_launch_big_lds<conv2d_igemm_kernel<TM, TN, WM, WN>>(l.grid, dim3(WM * WN * 64), l.lds, stream, p);
}

int run_conv2(const Conv2P& p, const Launch2& l, hipStream_t stream, const char* what) {
    switch (l.tile.tm * 10 + l.tile.tn) {
        case 12: go2<1, 2, 1, 4>(p, l, stream); break;
        case 21: go2<2, 1, 1, 4>(p, l, stream); break;
        case 31: go2<3, 1, 1, 4>(p, l, stream); break;
        default: go2<2, 2, 2, 2>(p, l, stream); break;
    }
    return rh_check_launch(what);
}

// A planned weight-gradient launch: wgrad2d_dma_kernel<tn> (dma) or wgrad2d_kernel on the bm-row tile of tile2_of
struct W2Plan {
    int bm, bn, Z;
    size_t lds;
    bool dma;
    int tn;
};

// The tap spans of a weight gradient (its taps are one phase); leaves the smallest offsets in p.minh, p.minw
PatchGeom patch_geom(Wgrad2P& p) {
    int maxh = p.offh[0], maxw = p.offw[0];
    p.minh = maxh;
    p.minw = maxw;
    for (int t = 1; t < p.T; ++t) {
        p.minh = p.minh < p.offh[t] ? p.minh : p.offh[t];
        p.minw = p.minw < p.offw[t] ? p.minw : p.offw[t];
        maxh = maxh > p.offh[t] ? maxh : p.offh[t];
        maxw = maxw > p.offw[t] ? maxw : p.offw[t];
    }
    return PatchGeom{maxh - p.minh, maxw - p.minw, p.T};
}

W2Plan plan_w2(Wgrad2P& p) {
    W2Plan w{};
    const Tile2 tl = tile2_of(p.M);
    w.bm = tl.bm();
    w.bn = tl.bn();
    const int ncols = p.C * p.T;
    p.nc_max = (w.bn - 1) / p.T + 2;
    if (p.nc_max > p.C) p.nc_max = p.C;
    p.wk = pow2ceil(p.r_w) < 64 ? pow2ceil(p.r_w) : 64;
    if (p.wk < 2) p.wk = 2;
    p.wk_shift = __builtin_ctz(p.wk);
    const PatchGeom g = patch_geom(p);
    const int span_h = g.span_h, span_w = g.span_w;
    p.PW = (p.wk - 1) * p.is_w + span_w + 1;
    p.PWp = p.PW | 1;
    int rk = 256 / p.wk > 4 ? 256 / p.wk : 4;       // aim at ~256 reduction elements per chunk
    if (rk > pow2ceil(p.r_h)) rk = pow2ceil(p.r_h);
    for (;; rk >>= 1) {
        p.rk = rk;
        p.PH = (rk - 1) * p.is_h + span_h + 1;
        p.chp = (p.PH * p.PWp) | 1;
        p.pr = rk * p.wk + 2;
        w.lds = sizeof(float) * ((size_t)w.bm * p.pr + (size_t)p.nc_max * p.chp);
        static const size_t cap = [] {
            const char* e = getenv("RH_WGRAD2D_LDS_BYTES");
            return e ? (size_t)atol(e) : (size_t)80 * 1024;
        }();
        if (w.lds <= cap || rk == 1) break;
    }
    p.magic_pw = magic32(p.PW);
    p.magic_ph = magic32(p.PH);
    p.chunks_r = rh_cdiv(p.r_h, p.rk);
    p.chunks_w = rh_cdiv(p.r_w, p.wk);
    p.total_chunks = p.B * p.chunks_r * p.chunks_w;
    const int bxy = rh_cdiv(ncols, w.bn) * rh_cdiv(p.M, w.bm);
    int Z = 1024 / (bxy > 0 ? bxy : 1);
    if (Z > p.total_chunks / 4) Z = p.total_chunks / 4;     // at least 4 chunks per slice
    if (Z < 1) Z = 1;
    p.chunks_per_z = rh_cdiv(p.total_chunks, Z);
    w.Z = rh_cdiv(p.total_chunks, p.chunks_per_z);
    return w;
}

template <int TM, int TN, int WM, int WN>
int launch_w2(const Wgrad2P& p, const W2Plan& w, hipStream_t stream) {
    constexpr int BM = TM * WM * 32, BN = TN * WN * 32;
    RH_REQUIRE(w.lds <= 160 * 1024, RH_ERR_UNSUPPORTED, "conv2d_bwd_weight: tile needs %zu B of LDS", w.lds);
    dim3 grid(rh_cdiv(p.C * p.T, BN), rh_cdiv(p.M, BM), w.Z);
    rh_launch_big_lds<wgrad2d_kernel<TM, TN, WM, WN>>(grid, dim3(WM * WN * 64), w.lds, stream, p);
    return rh_check_launch("conv2d_bwd_weight");
}

// LDS-DMA weight-gradient plan (M <= 32, no fused activation derivative); false = use the generic kernel
bool plan_w2_dma(Wgrad2P& p, W2Plan* w, int* tn_out) {
    static const bool off = getenv("RH_WGRAD2D_NODMA") != nullptr;
    if (off || p.M > 32 || p.Rmul) return false;
    const long rb = (long)p.B * p.M * p.r_h * p.r_w * 4, sbytes = (long)p.B * p.C * p.s_h * p.s_w * 4;
    if (rb >= (1l << 31) || sbytes >= (1l << 31)) return false;
    const int ncols = p.C * p.T;
    const int TN = ncols <= 128 ? 1 : (ncols <= 256 ? 2 : 4);
    const int BN = TN * 128;
    p.nc_max = (BN - 1) / p.T + 2;
    if (p.nc_max > p.C) p.nc_max = p.C;
    const PatchGeom g = patch_geom(p);
    const int span_h = g.span_h, span_w = g.span_w;
    static const int stage_cap = [] {
        const char* e = getenv("RH_WGRAD2D_DMA_STAGE_FLOATS");
        return e ? atoi(e) : 10 * 1024;
    }();
    int wk = pow2ceil(p.r_w) < 64 ? pow2ceil(p.r_w) : 64;
    if (wk < 2) wk = 2;
    int rk = 128 / wk > 1 ? 128 / wk : 1;                       // ~128 positions of dy per chunk
    for (;;) {
        if (rk * wk < 64) rk = 64 / wk;                          // a DMA slot is 64 floats
        p.wk = wk; p.rk = rk;
        p.wk_shift = __builtin_ctz(wk);
        p.PH = (rk - 1) * p.is_h + span_h + 1;
        p.PW = (wk - 1) * p.is_w + span_w + 1;
        p.PWp = p.PW;
        p.nr = rk * wk / 64;
        p.ns = (p.PH * p.PW + 63) / 64;
        p.pr = rk * wk + 2;
        p.chp = p.ns * 64 + 1;
        p.r_floats = 32 * p.pr;
        p.stage_floats = p.r_floats + p.nc_max * p.chp;
        const bool fits = p.nr <= kNR && p.ns <= kNS && p.stage_floats <= stage_cap;
        if (fits) break;
        if (rk * wk > 64 && rk > 1) rk >>= 1;                    // shrink the chunk, rows first
        else if (wk > 8) { wk >>= 1; rk = 64 / wk > 1 ? 64 / wk : 1; }
        else if (p.nr <= kNR && p.ns <= kNS && 2 * p.stage_floats * 4 <= 160 * 1024) break;   // over the soft cap only
        else return false;
    }
    p.magic_pw = magic32(p.PW);
    p.magic_ph = magic32(p.PH);
    p.chunks_r = rh_cdiv(p.r_h, p.rk);
    p.chunks_w = rh_cdiv(p.r_w, p.wk);
    p.total_chunks = p.B * p.chunks_r * p.chunks_w;
    p.r_bytes = (unsigned)rb;
    p.s_bytes = (unsigned)sbytes;
    const int bxy = rh_cdiv(ncols, BN);
    int Z = 1024 / bxy;
    if (Z > p.total_chunks / 8) Z = p.total_chunks / 8;          // at least 8 chunks per slice
    if (Z < 1) Z = 1;
    p.chunks_per_z = rh_cdiv(p.total_chunks, Z);
    w->Z = rh_cdiv(p.total_chunks, p.chunks_per_z);
    w->bm = 32;
    w->bn = BN;
    w->lds = sizeof(float) * 2 * (size_t)p.stage_floats;
    *tn_out = TN;
    return true;
}

template <int TN>
int launch_w2_dma(const Wgrad2P& p, const W2Plan& w, hipStream_t stream) {
    dim3 grid(rh_cdiv(p.C * p.T, TN * 128), 1, w.Z);
    rh_launch_big_lds<wgrad2d_dma_kernel<TN>>(grid, dim3(256), w.lds, stream, p);
    return rh_check_launch("conv2d_bwd_weight");
}

// The family-0 weight-gradient launch: the LDS-DMA kernel where its plan fits, else the generic kernel.  The launch and
// rh_conv2d_instance_info both take their answer from here.
W2Plan plan_w2_any(Wgrad2P& p) {
    W2Plan w{};
    int tn = 0;
    if (plan_w2_dma(p, &w, &tn)) {
        w.dma = true;
        w.tn = tn;
        return w;
    }
    return plan_w2(p);
}

int run_w2(const Wgrad2P& p, const W2Plan& w, hipStream_t stream) {
    if (w.dma) return w.tn == 1 ? launch_w2_dma<1>(p, w, stream) : (w.tn == 2 ? launch_w2_dma<2>(p, w, stream) : launch_w2_dma<4>(p, w, stream));
    if (w.bm == 32) return launch_w2<1, 2, 1, 4>(p, w, stream);
    if (w.bm == 64) return launch_w2<2, 1, 1, 4>(p, w, stream);
    if (w.bm == 96) return launch_w2<3, 1, 1, 4>(p, w, stream);
    return launch_w2<2, 2, 2, 2>(p, w, stream);
}

void fill_w2(const rh_conv2d_desc* d, Wgrad2P* p) {
    *p = Wgrad2P{};
    p->B = d->batch; p->M = d->c_out; p->C = d->c_in; p->T = d->kh * d->kw;
    p->r_h = d->h_out; p->r_w = d->w_out; p->s_h = d->h_in; p->s_w = d->w_in;
    p->is_h = d->sh; p->is_w = d->sw;
    p->r_act = d->act; p->r_slope = d->act_slope;
    for (int th = 0; th < d->kh; ++th)
        for (int tw = 0; tw < d->kw; ++tw) {
            p->offh[th * d->kw + tw] = th * d->dh - d->ph;
            p->offw[th * d->kw + tw] = tw * d->dw - d->pw;
        }
}

// Parameter block of a forward (which = 0) / data-gradient (1) call, before its tile plan
void fill_conv2(const rh_conv2d_desc* d, int which, const Plan2& t, const float* in, const float* y, const float* wp,
                const float* bias, float* out, Conv2P* pp) {
    Conv2P& p = *pp;
    p = Conv2P{};
    fill_common(t, &p, which == 0 ? d->c_in : d->c_out, which == 0 ? d->c_out : d->c_in);
    p.in = in; p.wp = wp; p.out = out;
    p.B = d->batch;
    if (which == 0) {
        p.bias = bias;
        p.in_mul = nullptr;
        p.in_h = d->h_in; p.in_w = d->w_in; p.out_h = d->h_out; p.out_w = d->w_out;
        p.rows = d->h_out; p.qcols = d->w_out;
        p.is_h = d->sh; p.is_w = d->sw; p.os_h = 1; p.os_w = 1;
        p.mul_act = RH_ACT_NONE; p.mul_slope = 0.f;
        p.epi_act = d->act; p.epi_slope = d->act_slope;
    } else {
        p.bias = nullptr;
        p.in_mul = d->act == RH_ACT_NONE ? nullptr : y;
        p.in_h = d->h_out; p.in_w = d->w_out; p.out_h = d->h_in; p.out_w = d->w_in;
        p.rows = rh_cdiv(d->h_in, d->sh); p.qcols = rh_cdiv(d->w_in, d->sw);
        p.is_h = 1; p.is_w = 1; p.os_h = d->sh; p.os_w = d->sw;
        p.mul_act = d->act; p.mul_slope = d->act_slope;
        p.epi_act = RH_ACT_NONE; p.epi_slope = 0.f;
    }
}

int64_t w2_scratch(const Wgrad2P& p, const W2Plan& w) {
    return w.Z > 1 ? (int64_t)w.Z * p.M * p.C * p.T * (int64_t)sizeof(float) : 0;
}

}  // namespace

int rh_conv2d_f32_conv(const rh_conv2d_desc* d, int which, const Plan2& t, const float* in, const float* y, const float* wp,
                       const float* bias, float* out, hipStream_t stream, const char* what, int64_t* info) {
    Conv2P p;
    fill_conv2(d, which, t, in, y, wp, bias, out, &p);
    Launch2 l{};
    int no_dma_why = 0;
    if (int e = plan_conv2(p, t, what, &l, &no_dma_why)) return e;
    if (!info) return run_conv2(p, l, stream, what);
    info[0] = l.dma ? K2_DMA : K2_IGEMM; info[1] = l.tile.tm; info[2] = l.tile.tn; info[3] = l.tile.wm; info[4] = l.tile.wn;
    info[5] = p.TR; info[6] = p.TQ; info[7] = p.nb; info[8] = p.PH; info[9] = p.PW; info[10] = p.ck; info[11] = t.nphase;
    info[12] = l.grid.x; info[13] = l.grid.y; info[14] = l.grid.z; info[15] = (int64_t)l.lds; info[16] = p.tiles_r; info[17] = p.tiles_q;
    info[18] = 0;
    info[19] = no_dma_why;
    return RH_OK;
}

int rh_conv2d_f32_wgrad(const rh_conv2d_desc* d, const float* dy, const float* ymul, const float* x, float* dw, void* workspace,
                        int64_t workspace_bytes, hipStream_t stream, int64_t* info) {
    Wgrad2P p;
    fill_w2(d, &p);
    p.R = dy; p.Rmul = ymul; p.S = x;
    const W2Plan w = plan_w2_any(p);
    const int64_t need = w2_scratch(p, w);
    if (info) {
        const Tile2 tl = tile2_of(p.M);
        info[0] = w.dma ? K2_WDMA : K2_WGRAD;
        if (w.dma) info[1] = w.tn;
        else { info[1] = tl.tm; info[2] = tl.tn; info[3] = tl.wm; info[4] = tl.wn; }
        info[5] = p.rk; info[6] = p.wk; info[7] = w.Z; info[8] = p.chunks_per_z;
        info[9] = rh_cdiv(p.C * p.T, w.bn) * rh_cdiv(p.M, w.bm);
        info[10] = p.nc_max; info[11] = (int64_t)w.lds; info[12] = need; info[14] = p.total_chunks; info[15] = p.PH; info[16] = p.PW;
        info[18] = 0;
        info[19] = (need == 0 || (workspace && workspace_bytes >= need)) ? 0 : 1;
        return RH_OK;
    }
    RH_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), RH_ERR_WORKSPACE,
               "conv2d_bwd_weight: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    p.out = w.Z > 1 ? (float*)workspace : dw;
    if (int e = run_w2(p, w, stream)) return e;
    if (w.Z > 1) return rh_reduce_partials_launch((const float*)workspace, dw, (long)p.M * p.C * p.T, w.Z, stream, "conv2d_bwd_weight_reduce");
    return RH_OK;
}

int64_t rh_conv2d_f32_wgrad_workspace(const rh_conv2d_desc* d) {
    Wgrad2P p;
    fill_w2(d, &p);
    // the fused activation derivative (act != NONE) takes the generic kernel; size for the larger of the two
    Wgrad2P q = p;
    W2Plan w{};
    int tn = 0;
    const int64_t need_dma = plan_w2_dma(q, &w, &tn) ? w2_scratch(q, w) : 0;
    const int64_t need_gen = w2_scratch(p, plan_w2(p));
    return need_dma > need_gen ? need_dma : need_gen;
}

