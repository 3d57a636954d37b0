// PQMF analysis / synthesis and their input gradients for M = 2, 4, 8 and 32 bands (rave/pqmf.py CachedPQMF with the
// N_BAND macro of configs/v1.gin rebound).  The 16-band bank of the shipped configs stays in pqmf.hip / pqmf_fold*.hip.
//
// The same two direct-form kernels as pqmf.hip, with the band count a template argument:
//
//   W2B (waveform -> bands):  out[b,k,n]  = sgn(k,n) * sum_{a,r} F[a][r][k] * in[b, M(n+a) + r - shift]
//        analysis forward   and   synthesis backward
//   B2W (bands -> waveform):  out[b,Mn+i] =            sum_{a,c} F[a][c][i] * sgn(c,m) in[b,c,m],  m = n+a-sh
//        synthesis forward  and   analysis backward
//
// sgn(k,n) = -1 iff k odd and n even (reverse_half): index arithmetic, bit-exact.  F is gathered from the module's own
// weight tensor (forward_conv.weight (M,1,K) / inverse_conv.weight (M,M,K2)) while it is staged into LDS, so edited taps
// are honoured.  Every output is one fmaf chain in f32 over (a, then r / c) ascending: no atomics, the same bits every run.
//
// Instruction choice: the vector ALU, for every M.  v_mfma_f32_16x16x4_f32 needs 16 output rows; at M <= 8 half or more
// of each tile would be zeros, and those launches are HBM-bound anyway (8 B/sample against at most 33 M MAC/sample).  The
// f32 MFMA peak equals the f32 vector peak on this chip, so M = 32 runs on the same code instead of a second kernel
// family; it is compute-bound there (1056 MAC/sample).  To keep the FMAs and not the LDS the limit, a thread owns a
// register tile of BPT bands (or output phases) x FPT frames: per tap it reads FPT signal values (conflict-free: odd
// pitch M+1 for the waveform tile, consecutive lanes for the band rows) and BPT filter values (one wave-uniform address,
// a broadcast) for BPT*FPT FMAs.
//
// Workgroup = 256 threads = (256 / G) frame lanes x G band groups, G = M / BPT; it produces F = 256 / G * FPT frames:
//
//     M   BPT  FPT  G    F     taps per filter chunk   LDS per workgroup at A = 33 (W2B / B2W)
//     2    2    8   1  2048    all                     25 500 B / 17 176 B
//     4    4    4   1  1024    all                     23 252 B / 19 024 B
//     8    8    2   1   512    all                     28 068 B / 25 888 B
//    32    8    4   4   256    4                       54 532 B / 53 376 B
//
// LDS budget at M = 32: the whole filter operand is 33*32*32 floats = 132 KiB, which with the signal tile (38 KiB) does
// not fit a CU's 160 KiB next to anything else.  The filter is therefore staged in chunks of 4 polyphase taps (16 KiB)
// behind the signal tile, which is staged once; 54 KiB per workgroup stays below the 64 KiB that needs no raised limit
// and lets two workgroups share a CU, so one stages while the other computes.
#include "pqmf_bands.hpp"

namespace {

constexpr int kMaxA = 40;      // polyphase taps the launcher stages (the designed banks have 33)
constexpr int kThreads = 256;

enum FilterMode { F_ANALYSIS_FWD = 0, F_SYNTH_BWD = 1, F_SYNTH_FWD = 2, F_ANALYSIS_BWD = 3 };

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct BandsP {
    const float* in;
    const float* w;
    float* out;
    int rows;      // B * channels
    int in_len;    // W2B: samples per row ; B2W: frames per band row
    int out_len;   // W2B: frames per band row ; B2W: samples per row
    int n_tiles;   // frame tiles per row
    int A;         // polyphase taps
    int shift;     // W2B: sample shift ; B2W: frame shift `sh`
    int K;         // kernel length of w's last dim
    int pad_left;
    int mode;
};

template <int M> struct Tile;
template <> struct Tile<2>  { static constexpr int BPT = 2, FPT = 8, CA = kMaxA; };
template <> struct Tile<4>  { static constexpr int BPT = 4, FPT = 4, CA = kMaxA; };
template <> struct Tile<8>  { static constexpr int BPT = 8, FPT = 2, CA = kMaxA; };
template <> struct Tile<32> { static constexpr int BPT = 8, FPT = 4, CA = 4; };
template <int M> constexpr int groups() { return M / Tile<M>::BPT; }
template <int M> constexpr int lanes() { return kThreads / groups<M>(); }          // frame lanes per band group
template <int M> constexpr int frames() { return lanes<M>() * Tile<M>::FPT; }      // F

// Filter element F[a][x][i], as pqmf.hip's with 16 -> M.
template <int M>
__device__ __forceinline__ float filter_elem(const BandsP& p, int a, int x, int i) {
    switch (p.mode) {
        case F_ANALYSIS_FWD: {  // F[a][r][k] = Wf[k, M a + r]
            const int t = M * a + x;
            return t < p.K ? p.w[(long)i * p.K + t] : 0.f;
        }
        case F_SYNTH_BWD: {  // F[a][r][c] = M * Wi[M-1 - r, c, K2 - 1 - a]
            const int t = p.K - 1 - a;
            return t >= 0 ? (float)M * p.w[((long)(M - 1 - x) * M + i) * p.K + t] : 0.f;
        }
        case F_SYNTH_FWD: {  // F[a][c][i] = M * Wi[M-1 - i, c, a]
            return a < p.K ? (float)M * p.w[((long)(M - 1 - i) * M + x) * p.K + a] : 0.f;
        }
        default: {  // F_ANALYSIS_BWD: F[a][k][r] = Wf[k, r + pad_left + M (sh - a)]
            const int t = i + p.pad_left + M * (p.shift - a);
            return (t >= 0 && t < p.K) ? p.w[(long)x * p.K + t] : 0.f;
        }
    }
}

template <int M, bool W2B>
__global__ __launch_bounds__(kThreads) void pqmf_bands_kernel(BandsP p) {
    constexpr int BPT = Tile<M>::BPT, FPT = Tile<M>::FPT, CA = Tile<M>::CA;
    constexpr int TPF = lanes<M>(), F = frames<M>();
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int na_max = p.A < CA ? p.A : CA;
    float* a_lds = smem;                          // [taps of the chunk][M][M]
    float* s_lds = smem + na_max * M * M;         // W2B: [(F + A) frames][M + 1] ; B2W: [M][F + A]
    const int tid = threadIdx.x;
    const int row = blockIdx.x / p.n_tiles;
    const int n0 = (blockIdx.x % p.n_tiles) * F;
    const int width = F + p.A;

    if (W2B) {
        const int n_samp = M * width;
        const long base = (long)M * n0 - p.shift;
        const float* in = p.in + (long)row * p.in_len;
        for (int e = tid; e < n_samp; e += kThreads) {
            const long s = base + e;
            s_lds[(e / M) * (M + 1) + (e % M)] = (s >= 0 && s < p.in_len) ? in[s] : 0.f;
        }
    } else {
        const float* in = p.in + (long)row * M * p.in_len;
        for (int c = tid >> 6; c < M; c += kThreads / 64) {
            for (int e = tid & 63; e < width; e += 64) {
                const int m = n0 + e - p.shift;
                float v = 0.f;
                if (m >= 0 && m < p.in_len) {
                    v = in[(long)c * p.in_len + m];
                    if ((c & 1) && !(m & 1)) v = -v;
                }
                s_lds[c * width + e] = v;
            }
        }
    }

    const int f = tid % TPF, g = tid / TPF;       // g is uniform in a wave: TPF is a multiple of 64
    float acc[FPT][BPT];
#pragma unroll
    for (int q = 0; q < FPT; ++q)
#pragma unroll
        for (int j = 0; j < BPT; ++j) acc[q][j] = 0.f;

    for (int a0 = 0; a0 < p.A; a0 += CA) {
        const int na = p.A - a0 < CA ? p.A - a0 : CA;
        if (a0) __syncthreads();                  // everyone is done with the previous chunk
        for (int e = tid; e < na * M * M; e += kThreads) {
            const int i = e % M, kidx = e / M;
            a_lds[e] = filter_elem<M>(p, a0 + kidx / M, kidx % M, i);
        }
        __syncthreads();
        for (int al = 0; al < na; ++al) {
            const int a = a0 + al;
            const float* sp = W2B ? s_lds + (f + a) * (M + 1) : s_lds + f + a;
#pragma unroll(M < 8 ? M : 8)
            for (int x = 0; x < M; ++x) {
                const float* fp = a_lds + (al * M + x) * M + g * BPT;
                float b[FPT];
#pragma unroll
                for (int q = 0; q < FPT; ++q) b[q] = W2B ? sp[q * TPF * (M + 1) + x] : sp[x * width + q * TPF];
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const float w = fp[j];
#pragma unroll
                    for (int q = 0; q < FPT; ++q) acc[q][j] = fmaf(w, b[q], acc[q][j]);
                }
            }
        }
    }

    if (W2B) {
        float* out = p.out + (long)row * M * p.out_len;
#pragma unroll
        for (int q = 0; q < FPT; ++q) {
            const int n = n0 + f + q * TPF;
            if (n < p.out_len) {
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int band = g * BPT + j;
                    float v = acc[q][j];
                    if ((band & 1) && !(n & 1)) v = -v;
                    out[(long)band * p.out_len + n] = v;
                }
            }
        }
    } else {
        constexpr int V = BPT >= 4 ? 4 : 2;
        float* out = p.out + (long)row * p.out_len;
        // rows start at multiples of V floats when out_len is one; the base pointer may be only 4-byte aligned
        const bool vec = (p.out_len % V) == 0 && (reinterpret_cast<uintptr_t>(p.out) % (V * sizeof(float))) == 0;
#pragma unroll
        for (int q = 0; q < FPT; ++q) {
            const long o = (long)M * (n0 + f + q * TPF) + g * BPT;
            if (vec && o + BPT <= p.out_len) {
#pragma unroll
                for (int j = 0; j < BPT; j += V) {
                    if (V == 4) *reinterpret_cast<f32x4*>(out + o + j) = f32x4{acc[q][j], acc[q][j + 1], acc[q][j + 2], acc[q][j + 3]};
                    else *reinterpret_cast<f32x2*>(out + o + j) = f32x2{acc[q][j], acc[q][j + 1]};
                }
            } else {
#pragma unroll
                for (int j = 0; j < BPT; ++j)
                    if (o + j < p.out_len) out[o + j] = acc[q][j];
            }
        }
    }
}

template <int M>
int launch_m(const BandsP& p, bool w2b, hipStream_t stream) {
    const int grid = p.rows * p.n_tiles;
    if (grid <= 0) return RH_OK;
    const int na = p.A < Tile<M>::CA ? p.A : Tile<M>::CA;
    const int width = frames<M>() + p.A;
    const size_t lds = sizeof(float) * (size_t)(na * M * M + (w2b ? width * (M + 1) : M * width));   // <= 55.5 KiB at A = 40
    if (w2b) hipLaunchKernelGGL((pqmf_bands_kernel<M, true>), dim3(grid), dim3(kThreads), lds, stream, p);
    else hipLaunchKernelGGL((pqmf_bands_kernel<M, false>), dim3(grid), dim3(kThreads), lds, stream, p);
    return rh_check_launch(w2b ? "pqmf_bands_w2b" : "pqmf_bands_b2w");
}

int launch(BandsP& p, int n_band, int frames_out, bool w2b, hipStream_t stream) {
    p.n_tiles = rh_cdiv(frames_out, rh_pqmf_bands_tile_frames(n_band));
    switch (n_band) {
        case 2: return launch_m<2>(p, w2b, stream);
        case 4: return launch_m<4>(p, w2b, stream);
        case 8: return launch_m<8>(p, w2b, stream);
        default: return launch_m<32>(p, w2b, stream);
    }
}

}  // namespace

bool rh_pqmf_bands_has(int n_band) { return n_band == 2 || n_band == 4 || n_band == 8 || n_band == 32; }

int rh_pqmf_bands_tile_frames(int n_band) {
    switch (n_band) {
        case 2: return frames<2>();
        case 4: return frames<4>();
        case 8: return frames<8>();
        case 32: return frames<32>();
        default: return 0;
    }
}

int rh_pqmf_bands_analysis_fwd(const float* x, const float* w, int rows, int t_len, int n_band, int kernel, int pad_left,
                               int n_frames, float* y, hipStream_t stream) {
    BandsP p{};
    p.in = x; p.w = w; p.out = y; p.rows = rows; p.in_len = t_len; p.out_len = n_frames;
    RH_REQUIRE(kernel > 0 && rh_cdiv(kernel, n_band) <= kMaxA, RH_ERR_UNSUPPORTED, "pqmf analysis: kernel %d too long", kernel);
    p.A = rh_cdiv(kernel, n_band); p.shift = pad_left; p.K = kernel; p.pad_left = pad_left;
    p.mode = F_ANALYSIS_FWD;
    return launch(p, n_band, n_frames, true, stream);
}

int rh_pqmf_bands_analysis_bwd(const float* dy, const float* w, int rows, int t_len, int n_band, int kernel, int pad_left,
                               int n_frames, float* dx, hipStream_t stream) {
    BandsP p{};
    p.in = dy; p.w = w; p.out = dx; p.rows = rows; p.in_len = n_frames; p.out_len = t_len;
    RH_REQUIRE(kernel > 0 && pad_left >= 0 && rh_cdiv(kernel, n_band) <= kMaxA && pad_left / n_band <= kMaxA, RH_ERR_UNSUPPORTED,
               "pqmf analysis bwd: unsupported geometry");
    int sh = kernel - 1 - pad_left;
    sh = sh > 0 ? rh_cdiv(sh, n_band) : 0;
    p.shift = sh; p.K = kernel; p.pad_left = pad_left;
    p.A = (n_band - 1 + pad_left + n_band * sh) / n_band + 1;
    p.mode = F_ANALYSIS_BWD;
    RH_REQUIRE(p.A <= kMaxA, RH_ERR_UNSUPPORTED, "pqmf analysis bwd: unsupported geometry");
    return launch(p, n_band, rh_cdiv(t_len, n_band), false, stream);
}

int rh_pqmf_bands_synthesis_fwd(const float* y, const float* w, int rows, int n_frames, int n_band, int kernel, int pad_left,
                                int n_out, float* x, hipStream_t stream) {
    BandsP p{};
    p.in = y; p.w = w; p.out = x; p.rows = rows; p.in_len = n_frames; p.out_len = n_out * n_band;
    RH_REQUIRE(kernel > 0 && kernel <= kMaxA, RH_ERR_UNSUPPORTED, "pqmf synthesis: kernel %d too long", kernel);
    p.A = kernel; p.shift = pad_left; p.K = kernel; p.pad_left = pad_left;
    p.mode = F_SYNTH_FWD;
    return launch(p, n_band, n_out, false, stream);
}

int rh_pqmf_bands_synthesis_bwd(const float* dx, const float* w, int rows, int n_frames, int n_band, int kernel, int pad_left,
                                int n_out, float* dy, hipStream_t stream) {
    BandsP p{};
    p.in = dx; p.w = w; p.out = dy; p.rows = rows; p.in_len = n_out * n_band; p.out_len = n_frames;
    RH_REQUIRE(kernel > 0 && kernel <= kMaxA, RH_ERR_UNSUPPORTED, "pqmf synthesis bwd: kernel %d too long", kernel);
    p.A = kernel; p.shift = n_band * (kernel - 1 - pad_left); p.K = kernel; p.pad_left = pad_left;
    p.mode = F_SYNTH_BWD;
    return launch(p, n_band, n_frames, true, stream);
}
