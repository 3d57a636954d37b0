// The recurrent latent layer: torch.nn.GRU(H, H, num_layers = L, batch_first = True) with h0 = 0, as rave.blocks.GRU wraps
// it (rave/blocks.py:295-319), forward and full backpropagation through time, on the model's own (B, H, T) tensors -- the two
// permute(0, 2, 1) of the reference are addressing here, no transposed copy of x, y, dy or dx exists.  Gates in torch's
// order (r, z, n):
//
//   r = s(W_ir x + b_ir + W_hr h + b_hr)     z = s(W_iz x + b_iz + W_hz h + b_hz)
//   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))     h' = (1 - z) * n + z * h
//
// Per layer, forward:  (1) the input projections of ALL steps, gi = X W_ih^T + b_ih, one small f32 product (gemm_kernel);
// (2) the recurrence (gru_fwd_kernel<H>): one workgroup of 3H threads per batch row, thread j keeps row j of W_hh in H
// registers for the whole walk, h lives in LDS and is read as broadcast 16-byte words, two barriers per step (after the 3H
// dot products, after the H state updates).  Backward, layers in reverse: (1) the reverse walk (gru_bwd_kernel<H>): thread
// (g, k) keeps COLUMN k of gate block g of W_hh, the three partial sums of W_hh^T dgh are added in a fixed order; it leaves
// the gate gradients dgi / dgh of every step; (2) d input = dgi W_ih (gemm_kernel; layer 0 writes dx in (B, H, T));
// (3) dW_ih = dgi^T X, dW_hh = dgh^T H_prev (one gemm_kernel launch, two products) and the bias gradients (colsum_kernel).
// Every sum has one order: nothing here uses an atomic, results are bit-identical from run to run.  f32 throughout; every
// global access is a 4-byte one (pointers need 4-byte alignment only).
//
// Workspace (floats; M = B T):  [ per layer: hs (B, T + 1, H): row 0 of a batch row = h0 = 0, row t + 1 = h_t | training:
// gates (B, T, 4, H): r, z, n, W_hn h + b_hn ]  then scratch: forward gi (M, 3H); backward dgi (M, 3H), dgh (M, 3H),
// d input (M, H).  Without training one hs block is shared by all layers and nothing else is kept.
#include <cmath>
#include "common.hpp"

namespace {

constexpr int kGruMaxH = 128, kGruMaxL = 4;

// finite for every finite argument: expf(-x) overflows to +Inf for x < -88.7 (1 / Inf = 0) and underflows to 0 above 103
__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- the recurrence ---------------------------------------------------------------------------------------------------
// gi (B, T, 3H); hs (B, T + 1, H); gates (B, T, 4, H) or null; y (B, H, T) or null (the last layer's output)
template <int H>
__global__ __launch_bounds__(3 * H) void gru_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ whh,
                                                         const float* __restrict__ bhh, float* __restrict__ hs,
                                                         float* __restrict__ gates, float* __restrict__ y, int T) {
    __shared__ __attribute__((aligned(16))) float h_s[H];
    __shared__ float gh_s[3 * H];
    __shared__ float stage[3 * H * 17];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    float w[H];
    // row tid of W_hh through LDS, 16 columns at a time (coalesced 64-byte runs in, conflict-free stride 17 out)
#pragma unroll
    for (int k0 = 0; k0 < H; k0 += 16) {
        for (int e = tid; e < 3 * H * 16; e += 3 * H) stage[(e >> 4) * 17 + (e & 15)] = whh[(long long)(e >> 4) * H + k0 + (e & 15)];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 16; ++c) w[k0 + c] = stage[tid * 17 + c];
        __syncthreads();
    }
    const float bias = bhh[tid];
    gi += b * T * 3 * H;
    hs += b * (T + 1) * H;
    if (gates) gates += b * T * 4 * H;
    if (y) y += b * H * T;
    float gr = 0.f, gz = 0.f, gn = 0.f, hp = 0.f;
    if (tid < H) {
        h_s[tid] = 0.f;
        hs[tid] = 0.f;
        gr = gi[tid]; gz = gi[H + tid]; gn = gi[2 * H + tid];
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        float a0 = bias, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(&h_s[k]);
            a0 = fmaf(w[k], hv[0], a0);
            a1 = fmaf(w[k + 1], hv[1], a1);
            a2 = fmaf(w[k + 2], hv[2], a2);
            a3 = fmaf(w[k + 3], hv[3], a3);
        }
        gh_s[tid] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (tid < H) {
            const float r = gru_sigmoid(gr + gh_s[tid]);
            const float z = gru_sigmoid(gz + gh_s[H + tid]);
            const float hn = gh_s[2 * H + tid];
            const float n = tanhf(fmaf(r, hn, gn));
            hp = (1.f - z) * n + z * hp;
            h_s[tid] = hp;
            hs[(long long)(t + 1) * H + tid] = hp;
            if (gates) {
                float* g = gates + (long long)t * 4 * H + tid;
                g[0] = r; g[H] = z; g[2 * H] = n; g[3 * H] = hn;
            }
            if (y) y[(long long)tid * T + t] = hp;
            if (t + 1 < T) {
                const float* nx = gi + (long long)(t + 1) * 3 * H + tid;
                gr = nx[0]; gz = nx[H]; gn = nx[2 * H];
            }
        }
        __syncthreads();
    }
}

// dy(b, t, k) = dy[b * dy_sb + t * dy_st + k * dy_sk]: the caller's (B, H, T) cotangent for the last layer, the (B, T, H)
// input gradient of the layer above otherwise.  dgi, dgh (B, T, 3H).
template <int H>
__global__ __launch_bounds__(3 * H) void gru_bwd_kernel(const float* __restrict__ dy, long long dy_sb, long long dy_st,
                                                         long long dy_sk, const float* __restrict__ gates,
                                                         const float* __restrict__ hs, const float* __restrict__ whh,
                                                         float* __restrict__ dgi, float* __restrict__ dgh, int T) {
    __shared__ __attribute__((aligned(16))) float dg_s[3 * H];
    __shared__ float part_s[3 * H];
    const int tid = threadIdx.x;
    const int g = tid / H, k = tid - g * H;
    const long long b = blockIdx.x;
    float w[H];                                         // column k of gate block g (coalesced: consecutive k)
#pragma unroll
    for (int j = 0; j < H; ++j) w[j] = whh[(long long)(g * H + j) * H + k];
    dy += b * dy_sb + k * dy_sk;
    gates += b * T * 4 * H;
    hs += b * (T + 1) * H;
    dgi += b * T * 3 * H;
    dgh += b * T * 3 * H;
    float carry = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        float dhz = 0.f;
        if (tid < H) {
            const float* gt = gates + (long long)t * 4 * H + tid;
            const float r = gt[0], z = gt[H], n = gt[2 * H], hn = gt[3 * H];
            const float hprev = hs[(long long)t * H + tid];
            const float dh = dy[t * dy_st] + carry;
            const float dnp = dh * (1.f - z) * (1.f - n * n);
            const float dzp = dh * (hprev - n) * z * (1.f - z);
            const float drp = dnp * hn * r * (1.f - r);
            const float dnh = dnp * r;
            float* o = dgi + (long long)t * 3 * H + tid;
            o[0] = drp; o[H] = dzp; o[2 * H] = dnp;
            o = dgh + (long long)t * 3 * H + tid;
            o[0] = drp; o[H] = dzp; o[2 * H] = dnh;
            dg_s[tid] = drp; dg_s[H + tid] = dzp; dg_s[2 * H + tid] = dnh;
            dhz = dh * z;
        }
        if (t == 0) break;                              // h0 is a constant: nothing flows further back
        __syncthreads();
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int j = 0; j < H; j += 4) {
            const f32x4 dv = *reinterpret_cast<const f32x4*>(&dg_s[g * H + j]);
            a0 = fmaf(w[j], dv[0], a0);
            a1 = fmaf(w[j + 1], dv[1], a1);
            a2 = fmaf(w[j + 2], dv[2], a2);
            a3 = fmaf(w[j + 3], dv[3], a3);
        }
        part_s[tid] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (tid < H) carry = dhz + ((part_s[tid] + part_s[H + tid]) + part_s[2 * H + tid]);
    }
}

// ---- the products around it ---------------------------------------------------------------------------------------------
// One index of an operand: offset(i) = (i / R) * so + (i % R) * si, or i * si with R == 0.  The split form addresses a
// (batch row, step) pair inside (B, H, T) and (B, T + 1, H) tensors.
struct GruDim {
    int R;
    long long so, si;
};
__device__ __forceinline__ long long gru_off(const GruDim& d, int i) {
    if (d.R == 0) return i * d.si;
    const int q = i / d.R;
    return q * d.so + (i - q * d.R) * d.si;
}
// C(m, n) = sum_k A(m, k) B(k, n) + bias[n]
struct GruGemm {
    const float* A; GruDim ar, ac;
    const float* B; GruDim br, bc;
    float* C; GruDim cr, cc;
    const float* bias;
    int M, N, K;
    int a_mfast, b_nfast;        // which index of the operand runs along consecutive addresses (picks the coalesced tile load)
};
struct GruGemmTable { GruGemm g[2]; };

constexpr int kGT = 32;          // tile edge in m, n and k

__global__ __launch_bounds__(256) void gru_gemm_kernel(const GruGemmTable tb) {
    const GruGemm& p = tb.g[blockIdx.z];
    __shared__ float As[kGT][kGT + 1];                                   // [k][m]
    __shared__ __attribute__((aligned(16))) float Bs[kGT][kGT + 4];      // [k][n]
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * kGT, n0 = blockIdx.y * kGT;
    if (m0 >= p.M || n0 >= p.N) return;                                  // (the two products of a launch may differ in size)
    const int lo = tid & 31, hi = tid >> 5;                              // hi: 0..7
    const int ty = tid >> 3, tx = (tid & 7) * 4;
    // the tile-load coordinates that do not move with k
    long long a_fix[4], b_fix[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + (p.a_mfast ? lo : hi + 8 * i);
        a_fix[i] = m < p.M ? gru_off(p.ar, m) : -1;
        const int n = n0 + (p.b_nfast ? lo : hi + 8 * i);
        b_fix[i] = n < p.N ? gru_off(p.bc, n) : -1;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += kGT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ka = p.a_mfast ? hi + 8 * i : lo, ma = p.a_mfast ? lo : hi + 8 * i;
            As[ka][ma] = (a_fix[i] >= 0 && k0 + ka < p.K) ? p.A[a_fix[i] + gru_off(p.ac, k0 + ka)] : 0.f;
            const int kb = p.b_nfast ? hi + 8 * i : lo, nb = p.b_nfast ? lo : hi + 8 * i;
            Bs[kb][nb] = (b_fix[i] >= 0 && k0 + kb < p.K) ? p.B[b_fix[i] + gru_off(p.br, k0 + kb)] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kGT; ++k) {
            const float a = As[k][ty];
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[k][tx]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(a, bv[j], acc[j]);
        }
        __syncthreads();
    }
    const int m = m0 + ty;
    if (m >= p.M) return;
    const long long co = gru_off(p.cr, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + tx + j;
        if (n < p.N) p.C[co + gru_off(p.cc, n)] = acc[j] + (p.bias ? p.bias[n] : 0.f);
    }
}

// out[j] = sum_i a[i * ld + j]: four interleaved row classes, each summed in row order, then added in class order
struct GruColsum { const float* a[2]; float* out[2]; };
__global__ __launch_bounds__(256) void gru_colsum_kernel(const GruColsum tb, int rows, int ld) {
    __shared__ float red[4][64];
    const float* a = tb.a[blockIdx.y];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    float s = 0.f;
    if (j < ld)
        for (int i = g; i < rows; i += 4) s += a[(long long)i * ld + j];
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && j < ld) tb.out[blockIdx.y][j] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

template <int H>
void launch_fwd(int B, hipStream_t st, const float* gi, const float* whh, const float* bhh, float* hs, float* gates, float* y, int T) {
    hipLaunchKernelGGL(gru_fwd_kernel<H>, dim3(B), dim3(3 * H), 0, st, gi, whh, bhh, hs, gates, y, T);
}
template <int H>
void launch_bwd(int B, hipStream_t st, const float* dy, long long sb, long long stt, long long sk, const float* gates,
                const float* hs, const float* whh, float* dgi, float* dgh, int T) {
    hipLaunchKernelGGL(gru_bwd_kernel<H>, dim3(B), dim3(3 * H), 0, st, dy, sb, stt, sk, gates, hs, whh, dgi, dgh, T);
}
#define GRU_DISPATCH(H, fn, ...)                    \
    switch (H) {                                    \
        case 16: fn<16>(__VA_ARGS__); break;        \
        case 32: fn<32>(__VA_ARGS__); break;        \
        case 48: fn<48>(__VA_ARGS__); break;        \
        case 64: fn<64>(__VA_ARGS__); break;        \
        case 80: fn<80>(__VA_ARGS__); break;        \
        case 96: fn<96>(__VA_ARGS__); break;        \
        case 112: fn<112>(__VA_ARGS__); break;      \
        default: fn<128>(__VA_ARGS__); break;       \
    }

GruDim plain(long long stride) { return GruDim{0, 0, stride}; }

void launch_gemm(hipStream_t st, const GruGemmTable& tb, int count) {
    int M = 0, N = 0;
    for (int i = 0; i < count; ++i) { M = tb.g[i].M > M ? tb.g[i].M : M; N = tb.g[i].N > N ? tb.g[i].N : N; }
    hipLaunchKernelGGL(gru_gemm_kernel, dim3(rh_cdiv(M, kGT), rh_cdiv(N, kGT), count), dim3(256), 0, st, tb);
}

// sizes (floats) of the workspace sections
struct GruLayout {
    int64_t hs, gates, per_layer, saved, total;
};
GruLayout gru_layout(int64_t B, int64_t H, int64_t T, int64_t L, int training) {
    GruLayout o;
    o.hs = B * (T + 1) * H;
    o.gates = training ? B * T * 4 * H : 0;
    o.per_layer = o.hs + o.gates;
    o.saved = training ? L * o.per_layer : o.hs;
    o.total = o.saved + B * T * H * (training ? 7 : 3);
    return o;
}

int gru_check_sizes(const char* who, int32_t B, int32_t H, int32_t T, int32_t L) {
    RH_REQUIRE(rh_gru_supported(H, L) == 1, RH_ERR_UNSUPPORTED,
               "%s: hidden size %d x %d layers is not built (hidden: a multiple of 16 in [16, %d]; layers: 1..%d)", who, (int)H,
               (int)L, kGruMaxH, kGruMaxL);
    RH_REQUIRE(B >= 1 && T >= 1, RH_ERR_UNSUPPORTED, "%s: batch %d x %d steps (both must be >= 1)", who, (int)B, (int)T);
    RH_REQUIRE((int64_t)B * ((int64_t)T + 1) < (int64_t)0x7fffffff / (4 * kGruMaxH), RH_ERR_UNSUPPORTED,
               "%s: batch %d x %d steps exceeds 32-bit row indexing", who, (int)B, (int)T);
    return RH_OK;
}

int gru_check_items(const char* who, const rh_gru_item* items, int32_t L, bool bwd) {
    RH_REQUIRE(items, RH_ERR_INVALID, "%s: null layer table", who);
    for (int l = 0; l < L; ++l) {
        const rh_gru_item& it = items[l];
        RH_REQUIRE(it.w_ih && it.w_hh && it.b_ih && it.b_hh, RH_ERR_INVALID, "%s: layer %d: null parameter pointer", who, l);
        RH_REQUIRE(!bwd || (it.dw_ih && it.dw_hh && it.db_ih && it.db_hh), RH_ERR_INVALID, "%s: layer %d: null gradient pointer", who, l);
    }
    return RH_OK;
}

}  // namespace

extern "C" int rh_gru_supported(int32_t hidden, int32_t layers) {
    return hidden >= 16 && hidden <= kGruMaxH && hidden % 16 == 0 && layers >= 1 && layers <= kGruMaxL ? 1 : 0;
}

extern "C" int rh_gru_workspace_bytes(int32_t batch, int32_t hidden, int32_t t_len, int32_t layers, int32_t training, int64_t* bytes) {
    if (int e = gru_check_sizes("gru_workspace_bytes", batch, hidden, t_len, layers)) return e;
    RH_REQUIRE(bytes, RH_ERR_INVALID, "gru_workspace_bytes: null result pointer");
    *bytes = 4 * gru_layout(batch, hidden, t_len, layers, training != 0).total;
    return RH_OK;
}

extern "C" int rh_gru_fwd_f32(const float* x, const rh_gru_item* layers, int32_t n_layers, int32_t batch, int32_t hidden,
                              int32_t t_len, int32_t training, float* y, void* workspace, int64_t workspace_bytes,
                              rh_stream_t stream) {
    const int B = batch, H = hidden, T = t_len, L = n_layers;
    if (int e = gru_check_sizes("gru_fwd", B, H, T, L)) return e;
    if (int e = gru_check_items("gru_fwd", layers, L, false)) return e;
    RH_REQUIRE(x && y && workspace, RH_ERR_INVALID, "gru_fwd: null pointer");
    const GruLayout lay = gru_layout(B, H, T, L, training != 0);
    RH_REQUIRE(workspace_bytes >= 4 * lay.total, RH_ERR_WORKSPACE, "gru_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes,
               (long long)(4 * lay.total));
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* gi = ws + lay.saved;
    const int M = B * T;
    const float* hs_prev = nullptr;
    for (int l = 0; l < L; ++l) {
        float* hs = ws + (training ? l * lay.per_layer : 0);
        float* gates = training ? hs + lay.hs : nullptr;
        GruGemmTable tb{};
        GruGemm& p = tb.g[0];
        if (l == 0) {                                   // x (B, H, T)
            p.A = x; p.ar = GruDim{T, (long long)H * T, 1}; p.ac = plain(T); p.a_mfast = 1;
        } else {                                        // rows 1.. of the layer below (B, T + 1, H)
            p.A = hs_prev + H; p.ar = GruDim{T, (long long)(T + 1) * H, H}; p.ac = plain(1); p.a_mfast = 0;
        }
        p.B = layers[l].w_ih; p.br = plain(1); p.bc = plain(H); p.b_nfast = 0;
        p.C = gi; p.cr = plain(3 * H); p.cc = plain(1);
        p.bias = layers[l].b_ih;
        p.M = M; p.N = 3 * H; p.K = H;
        launch_gemm(st, tb, 1);
        if (int e = rh_check_launch("gru_fwd input projection")) return e;
        // (without training every layer shares one hs block: its projection above has been enqueued before the walk rewrites it)
        GRU_DISPATCH(H, launch_fwd, B, st, gi, layers[l].w_hh, layers[l].b_hh, hs, gates, l == L - 1 ? y : nullptr, T)
        if (int e = rh_check_launch("gru_fwd recurrence")) return e;
        hs_prev = hs;
    }
    return RH_OK;
}

extern "C" int rh_gru_bwd_f32(const float* dy, const float* x, const rh_gru_item* layers, int32_t n_layers, int32_t batch,
                              int32_t hidden, int32_t t_len, float* dx, void* workspace, int64_t workspace_bytes,
                              rh_stream_t stream) {
    const int B = batch, H = hidden, T = t_len, L = n_layers;
    if (int e = gru_check_sizes("gru_bwd", B, H, T, L)) return e;
    if (int e = gru_check_items("gru_bwd", layers, L, true)) return e;
    RH_REQUIRE(dy && x && dx && workspace, RH_ERR_INVALID, "gru_bwd: null pointer");
    const GruLayout lay = gru_layout(B, H, T, L, 1);
    RH_REQUIRE(workspace_bytes >= 4 * lay.total, RH_ERR_WORKSPACE, "gru_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes,
               (long long)(4 * lay.total));
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int M = B * T;
    float* dgi = ws + lay.saved;
    float* dgh = dgi + (int64_t)M * 3 * H;
    float* dinp = dgh + (int64_t)M * 3 * H;             // (B, T, H)
    for (int l = L - 1; l >= 0; --l) {
        const float* hs = ws + l * lay.per_layer;
        const float* gates = hs + lay.hs;
        const rh_gru_item& it = layers[l];
        if (l == L - 1) {
            GRU_DISPATCH(H, launch_bwd, B, st, dy, (long long)H * T, 1ll, (long long)T, gates, hs, it.w_hh, dgi, dgh, T)
        } else {
            GRU_DISPATCH(H, launch_bwd, B, st, dinp, (long long)T * H, (long long)H, 1ll, gates, hs, it.w_hh, dgi, dgh, T)
        }
        if (int e = rh_check_launch("gru_bwd recurrence")) return e;
        // the layer's input as an (M, H) operand
        const float* inp; GruDim ir, ic; int i_rowfast;
        if (l == 0) { inp = x; ir = GruDim{T, (long long)H * T, 1}; ic = plain(T); i_rowfast = 1; }
        else { inp = ws + (l - 1) * lay.per_layer + H; ir = GruDim{T, (long long)(T + 1) * H, H}; ic = plain(1); i_rowfast = 0; }
        {   // d input = dgi W_ih: the layer below's dy, or dx in (B, H, T)
            GruGemmTable tb{};
            GruGemm& p = tb.g[0];
            p.A = dgi; p.ar = plain(3 * H); p.ac = plain(1); p.a_mfast = 0;
            p.B = it.w_ih; p.br = plain(H); p.bc = plain(1); p.b_nfast = 1;
            if (l == 0) { p.C = dx; p.cr = ir; p.cc = ic; }
            else { p.C = dinp; p.cr = plain(H); p.cc = plain(1); }
            p.M = M; p.N = H; p.K = 3 * H;
            launch_gemm(st, tb, 1);
            if (int e = rh_check_launch("gru_bwd input gradient")) return e;
        }
        {   // dW_ih = dgi^T inp, dW_hh = dgh^T h_prev (rows 0..T-1 of hs: h_{t-1}, zero at t = 0)
            GruGemmTable tb{};
            for (int q = 0; q < 2; ++q) {
                GruGemm& p = tb.g[q];
                p.A = q ? dgh : dgi; p.ar = plain(1); p.ac = plain(3 * H); p.a_mfast = 1;
                if (q) { p.B = hs; p.br = GruDim{T, (long long)(T + 1) * H, H}; p.bc = plain(1); p.b_nfast = 1; }
                else { p.B = inp; p.br = ir; p.bc = ic; p.b_nfast = !i_rowfast; }
                p.C = q ? it.dw_hh : it.dw_ih; p.cr = plain(H); p.cc = plain(1);
                p.M = 3 * H; p.N = H; p.K = M;
            }
            launch_gemm(st, tb, 2);
            if (int e = rh_check_launch("gru_bwd weight gradient")) return e;
        }
        GruColsum cs{{dgi, dgh}, {it.db_ih, it.db_hh}};
        hipLaunchKernelGGL(gru_colsum_kernel, dim3(rh_cdiv(3 * H, 64), 2), dim3(256), 0, st, cs, M, 3 * H);
        if (int e = rh_check_launch("gru_bwd bias gradient")) return e;
    }
    return RH_OK;
}
