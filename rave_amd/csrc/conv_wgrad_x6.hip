// Weight gradient of the 1-D convolutions, f32 results from the 16-bit matrix cores ("x6", see conv_x6_kernel.inc for the
// numerics).  Product build (RH_X6_F16 = 1): both operands are scaled by a power of two taken from their range slots
// (common.hpp) and split into two f16 pieces, three v_mfma_f32_32x32x16_f16 per product block, smallest terms first.
// Comparison build (RH_X6_F16 = 0, rave_amd/_var): the 3-way exact bf16 split of rounds 2-5, six bf16 MFMAs per block.
//   out[z][m][c*T + t] = sum_{(b,n) in K slice z} actR(R[b][m][n]) * actS(S[b][c][n*is + off[t]])
// (conv_params.hpp: WgradP; R = dy, S = x for Conv1d, the roles swap for ConvTranspose1d).
//
// GEMM view: rows m, columns (c, t), reduction over POSITIONS -- the contiguous axis of both operands.  A 16-deep MFMA
// k block is 16 consecutive positions of one batch item, and lane (j, g)'s fragment is 8 consecutive samples of one
// row: no transposition anywhere, every thread converts whole fragments.  Per step (32 positions = two k blocks):
//   * every thread owns (row, octet) tasks of the R tile and (column, octet) -- plane mode: (channel, octet) -- tasks of the
//     S tile: it loads the 8 samples straight from HBM/L2 one step ahead (buffer loads: padding and ragged tails read 0.0;
//     consecutive lanes take consecutive octets of one row, i.e. whole 128-byte lines), applies LeakyReLU, scales and splits,
//     and writes kX6P 16-byte fragments [k block][g][piece][row] to LDS;
//   * fragments by ds_read_b128, kKS * RH_X6_NPROD MFMAs per 32 x 32 output tile and step.
// Both operands need the conversion (the forward kernel gets its weights pre-split), so VALU work per MFMA decides.
// K is split over (batch, position) ranges; the partial sums are combined in slice order by reduce_partials_kernel (or left to
// the caller's batched reduction: rh_defer_reduce).
//
// Layout of this file: emit (conversion of 8 samples), the STAGING LAYER (scales, step geometry, R tasks, S tasks, the MFMA k
// block, the tile store -- each written once), then the kernels, each no more than its LDS layout, its barriers and its main loop
// over that layer; then the host side: Wx6Env (the switches), plan_wx6 = wx6_eligible -> wx6_choose_tile -> wx6_slice_k,
// wx6_instance / launch_wx6, and the entry points: plan once (rh_wgrad_x6_plan), then launch or describe that plan.  A further tile shape is a further loop, not a further copy.
//
// Two tile shapes (wx6_choose_tile chooses by the layer):
//   * wgrad_x6_kernel: four waves, workgroup tile 32 TM WM rows x 64 WN columns, wave tile 32 TM x 64, one LDS stage, two
//     barriers per step, two or three workgroups per CU whose phases interleave -- every eligible layer that does not take the
//     wide tile: 32 ... 64 gradient rows (on rows of at most 1024 positions), more than 96 rows, or more than 288 columns;
//     40 instances (tests/wgrad_matrix.py runs each of them, and each of the 8 wide ones, against f64);
//   * wgrad_x6_wide_kernel: ONE workgroup tile over all rows (65 ... 96) and all columns (<= 288), one wave per 32 columns
//     (3, 4, 6 or 9 waves, wave tile 96 x 32) -- the C = 96 layers and the stem of the v2 model.  RH_WGRAD_X6_WIDE=0 sends
//     them to the 4-wave kernel.
//
// Measured (C = 192 k = 3 layer, 83 us; ablation builds): MFMA + barriers alone 36 us of loop, loads + conversion alone
// 33 us, together 58 us -- the phases do not overlap, and no schedule made them: wave priorities (s_setprio by wave slot
// / block parity) changed nothing; a barrier ping-pong of two 4-wave teams in one workgroup (one multiplies while the
// other converts) was 1.2 ... 2x slower; converting the next step INSIDE the MFMA sequence of the same wave (two LDS
// stages, 16-position steps, sched_group_barrier interleave: 1 MFMA + 6 VALU) gained 3 % on long rows and lost up to
// 40 % on short ones.  The probe tools/probe/mfma_valu_overlap.hip shows why: on this SIMD the time of a VALU
// instruction ADDS to the MFMA time whichever wave issues it (MFMA alone 34-40 cycles, + 6 VALU = 46, two such waves
// 90 per pair).  What pays is fewer VALU instructions per sample.
#include <cstdlib>
#include <mutex>
#include <new>
#include <type_traits>
#include "conv_params.hpp"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kOOB = 0x80000000u;

struct Wx6P {
    const float* R;
    const float* S;
    float* out;                 // [Z][M][N] partials (or dw itself when Z == 1)
    float* rsum;                // [Z][M] row sums of R over the K slice = partial bias gradients (R = dy), or null
    int B, M, C, T, N;          // N = C * T
    int r_row, s_row, s_valid, is;
    float r_slope, s_slope;     // LeakyReLU slope of the operand's activation; 1 = none
    int steps_per_b;            // ceil(r_row / (16 * kKS))
    int total_steps, steps_per_z;
    unsigned r_bytes, s_bytes;
    int minoff, maxoff;
    int p8, cpb, chmax;         // plane mode (PL): octets of a channel image, channel pitch in bytes, channel images reserved
    int av;                     // wide tile: rows of R are 16-byte aligned (the AV template flag of the 4-wave kernel, as a uniform branch)
    unsigned b_stage;           // wide tile: bytes of one stage of the S fragments / planes
    const unsigned* r_range;    // range slots of R and S (f16 build: common.hpp)
    const unsigned* s_range;
    int off[kMaxTaps];
};

typedef u32x4 u32x4_u __attribute__((aligned(2)));      // 16 bytes at any 2-byte alignment: ds_read_b128 serves it at 1.4x the aligned cost

// LeakyReLU (slope in [0, 1]; 1 = none) + split of 8 samples -> kX6P 16-byte fragments.  f16 build: the samples are scaled
// by `sc` (power of two, from the operand's range slot) and split hi / lo with packed converts, ~5 VALU per sample; bf16 build:
// exact 3-way truncation split, ~7.5.  VALU work is NOT free next to the matrix cores on this chip
// (tools/probe/mfma_valu_overlap.hip) -- every instruction saved here is matrix time.
__device__ __forceinline__ void emit(const float (&v)[8], float slope, float sc, u32x4* dst, int piece_stride) {
#if RH_X6_F16
    u32x4 hi, lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float a = v[2 * k] * sc, b = v[2 * k + 1] * sc;
        a = rh_max1(a, a * slope);
        b = rh_max1(b, b * slope);
        const rh_h2 h = rh_h2_split(a, b);
        hi[k] = h.hi; lo[k] = h.lo;
    }
    dst[0] = hi;
    dst[piece_stride] = lo;
#else
    unsigned h[3][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = rh_max1(v[i], v[i] * slope);
        rh_bf3_split(x, h[0][i], h[1][i], h[2][i]);
    }
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
        u32x4 pk;
#pragma unroll
        for (int k = 0; k < 4; ++k) pk[k] = __builtin_amdgcn_perm(h[s3][2 * k + 1], h[s3][2 * k], 0x07060302u);   // high halves
        dst[s3 * piece_stride] = pk;
    }
#endif
}

// ---- The staging layer: what both kernels below (and the next tile shape) share.  A kernel keeps its own LDS layout constants,
// stage count, barriers and main loop, and builds them from these pieces:
//   wx6_scales        the power-of-two scales of R, S and the result, from the two range slots
//   wx6_step          where step st lies: batch item, first position, and whether it touches an edge of R / S
//   Wx6RTasks         this thread's (row, octet) tasks of the R tile: table, loads (ragged tail), row sums, conversion
//   Wx6STasks         its (column, octet) -- planes: (channel, octet) -- tasks of the S tile: table, loads (edges), conversion
//   wx6_mma           one k block of one wave: fragments of TM row tiles x TN column tiles, RH_X6_NPROD products each
//   wx6_store_tile    one 32 x 32 accumulator tile, un-scaled, rows < M
// Everything is __forceinline__ and the tables live in registers: the structs are taken apart by the compiler.
constexpr int kKS = 2;              // MFMA k blocks (16 positions each) per step
constexpr int kOct = 2 * kKS;       // 8-sample octets per row and step
constexpr int kSpan = 16 * kKS;     // positions per step

// Fragments of ONE k block of an operand tile: [g][piece][rows], with 4 fragments of padding per g block.  The kOct = 4 lanes
// that convert the four octets of one row write to (k block, g) = (0,0), (0,1), (1,0), (1,1): without the padding those blocks
// are 3 * rows fragments = a multiple of 256 bytes apart and every ds_write_b128 was a 4-way bank conflict (PMC:
// SQ_LDS_BANK_CONFLICT 60 % of SQ_LDS_IDX_ACTIVE); with it the four lanes land 64 bytes apart.
constexpr int wx6_gs(int rows) { return kX6P * rows + 4; }                                       // g stride (fragments)
constexpr int wx6_stage(int rows) { return kKS * 2 * wx6_gs(rows); }                             // fragments of one stage: [kKS][g][piece][rows]
constexpr int wx6_slot(int o, int row, int rows) { return (o >> 1) * 2 * wx6_gs(rows) + (o & 1) * wx6_gs(rows) + row; }      // of (octet, row)

struct Wx6Scale { float r, s, out; };
__device__ __forceinline__ Wx6Scale wx6_scales(const Wx6P& p) {
#if RH_X6_F16
    int inv_r, inv_s;
    Wx6Scale sc;
    sc.r = __uint_as_float(rh_x6_scale_bits(rh_range_max(p.r_range), &inv_r));
    sc.s = __uint_as_float(rh_x6_scale_bits(rh_range_max(p.s_range), &inv_s));
    sc.out = __uint_as_float(rh_x6_unscale_bits(inv_r, inv_s));
    return sc;
#else
    return Wx6Scale{1.f, 1.f, 1.f};
#endif
}

struct Wx6Step {
    int n;                      // first position (of R) inside the batch item
    unsigned rs, ss;            // byte offset of (batch item, position) in R / S
    bool r_tail, s_edge;        // (uniform) the step reaches past the end of R's rows / touches an edge of S: loads test every sample
};
template <bool PL>
__device__ __forceinline__ Wx6Step wx6_step(const Wx6P& p, int st) {
    Wx6Step sp;
    const int b = st / p.steps_per_b;
    sp.n = (st - b * p.steps_per_b) * kSpan;
    sp.rs = (unsigned)((b * p.M * p.r_row + sp.n) * 4);
    sp.ss = (unsigned)((b * p.C * p.s_row + sp.n * p.is) * 4);
    sp.r_tail = sp.n + kSpan > p.r_row;
    sp.s_edge = PL ? (sp.n + p.minoff < 0 || sp.n + p.minoff + 8 * p.p8 > p.s_valid || sp.r_tail)
                   : (sp.n * p.is + p.minoff < 0 || (sp.n + kSpan - 1) * p.is + p.maxoff >= p.s_valid || sp.r_tail);
    return sp;
}

// R tasks of one thread of an NT-thread workgroup whose tile starts at row m0 and holds BM rows.  A task = 8 consecutive samples
// of one row; consecutive lanes take consecutive octets of the SAME row (kOct lanes x 32 bytes = one 128-byte line per row), so
// that a load instruction touches 64 / kOct rows instead of 64.
template <int NT, int BM>
struct Wx6RTasks {
    static constexpr int NA = (kOct * BM + NT - 1) / NT;        // tasks per thread and step
    unsigned off[NA];           // byte offset of sample 0 in R at step 0 (kOOB: no such row)
    int dst[NA], pos[NA];       // fragment slot in the A stage (-1: none), position of sample 0 inside the step
    float v[NA][8];             // the samples of the step loaded last
    float sum[NA];              // their running sum: the bias gradient when R = dy

    __device__ __forceinline__ void init(const Wx6P& p, int tid, int m0) {
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int u = tid + NT * q;
            const int o = u % kOct, m = u / kOct;
            const bool ok = m < BM && m0 + m < p.M;
            dst[q] = m < BM ? wx6_slot(o, m, BM) : -1;
            pos[q] = 8 * o;
            off[q] = ok ? (unsigned)(((m0 + m) * p.r_row + 8 * o) * 4) : kOOB;
            sum[q] = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[q][i] = 0.f;          // (a wave that skips its loads adds zeros to the row sums)
        }
    }
    // av: rows of R are 16-byte aligned -> two 16-byte loads instead of eight 4-byte ones.  The whole element offset goes into
    // the per-lane operand (the bounds check must see it), nothing into the scalar offset.
    template <class RSRC>
    __device__ __forceinline__ void load(const Wx6P& p, RSRC rsrc, const Wx6Step& sp, bool av) {
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const unsigned base = off[q] == kOOB ? kOOB : off[q] + sp.rs;
            if (av) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    unsigned o = base == kOOB ? kOOB : base + 16u * h;
                    if (sp.r_tail) o = sp.n + pos[q] + 4 * h < p.r_row ? o : kOOB;      // r_row % 4 == 0: all or nothing
                    const u32x4 x = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0));
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[q][4 * h + i] = __uint_as_float(x[i]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    unsigned o = base == kOOB ? kOOB : base + 4u * i;
                    if (sp.r_tail) o = sp.n + pos[q] + i < p.r_row ? o : kOOB;
                    v[q][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o, 0, 0));
                }
            }
        }
    }
    // Bias gradient = row sums of dy, from the samples converted anyway (one pass over dy for weight AND bias gradient).  The
    // order is part of the result: pairwise over the 8 samples, per task and step, then the butterfly over the row's kOct lanes.
    __device__ __forceinline__ void add_rows() {
#pragma unroll
        for (int q = 0; q < NA; ++q)
            sum[q] += ((v[q][0] + v[q][1]) + (v[q][2] + v[q][3])) + ((v[q][4] + v[q][5]) + (v[q][6] + v[q][7]));
    }
    __device__ __forceinline__ void store_sums(const Wx6P& p, int tid, int m0, int z) const {
#pragma unroll
        for (int q = 0; q < NA; ++q) {          // the kOct lanes of a row are neighbours: fixed-order butterfly, lane of octet 0 writes
            float s = sum[q];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            const int u = tid + NT * q;
            const int m = u / kOct;
            if ((u % kOct) == 0 && m < BM && m0 + m < p.M) p.rsum[(long)z * p.M + m0 + m] = s;
        }
    }
    __device__ __forceinline__ void convert(const Wx6P& p, float sc, u32x4* a_stage) const {
#pragma unroll
        for (int q = 0; q < NA; ++q)
            if (dst[q] >= 0) emit(v[q], p.r_slope, sc, a_stage + dst[q], BM);
    }
};

// S tasks of one thread of an NT-thread workgroup whose tile starts at column n0 and holds BN columns; `first` is the thread's
// first task (tid: dealt from thread 0 up; NT - 1 - tid: from the last thread down), the others follow NT apart.
//   !PL: (column, octet) tasks, kOct * BN of them, into fragments [kKS][g][piece][BN] like the R tile;
//   PL ("planes"): (channel, octet) tasks -- the 32 + reach positions (p.p8 octets) of every channel the tile touches, converted
//   ONCE PER POSITION into 16-bit ELEMENT planes [piece][channel][position]; the fragment of column (c, t) is the 16-byte LDS read
//   at channel c's image + the tap's element offset (any 2-byte alignment: tools/probe/lds_unaligned.hip).
// Offsets inside the stage are in bytes in both modes.
template <int NT, int NB, int BN, bool PL>
struct Wx6STasks {
    static_assert(PL || NT * NB == kOct * BN, "the (column, octet) tasks fill NB whole rounds");
    unsigned off[NB];           // byte offset of sample 0 in S at step 0 (kOOB: no such column / channel)
    int dst[NB], p0[NB];        // byte offset in the S stage (-1: none), position of sample 0 relative to n * is
    float v[NB][8];
    int c_lo;                   // PL: first channel of the tile
    unsigned piece;             // bytes between the pieces of a fragment

    // part: columns past the end of the weight tensor convert nothing (their LDS slots keep whatever they hold: a column of the
    // S operand only reaches its own output column, which is never stored)
    __device__ __forceinline__ void init(const Wx6P& p, int first, int n0, bool part) {
        c_lo = PL ? n0 / p.T : 0;
        const int n_ch = PL ? min(p.N - 1, n0 + BN - 1) / p.T - c_lo + 1 : 0;                // channel images the tile needs
        piece = PL ? (unsigned)(p.chmax * p.cpb) : 16u * BN;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int u = first + NT * q;
            if constexpr (PL) {
                const int ch = u / p.p8, o = u - ch * p.p8;
                const bool ok = ch < n_ch;
                dst[q] = ok ? ch * p.cpb + o * 16 : -1;
                p0[q] = p.minoff + 8 * o;
                off[q] = ok ? (unsigned)(((c_lo + ch) * p.s_row + p0[q]) * 4) : kOOB;
            } else {
                const int o = u % kOct, col = u / kOct;
                const int cc = (n0 + col) / p.T, t = (n0 + col) - cc * p.T;
                const bool ok = n0 + col < p.N;
                dst[q] = (ok || !part) ? wx6_slot(o, col, BN) * 16 : -1;
                p0[q] = 8 * o * p.is + (ok ? p.off[t] : 0);
                off[q] = ok ? (unsigned)((cc * p.s_row + p0[q]) * 4) : kOOB;
            }
        }
    }
    // byte offset of the fragments of column n, tile tn of the wave, from the wave's k-block base (kblock)
    __device__ __forceinline__ unsigned column(const Wx6P& p, int n, int tn) const {
        if constexpr (PL) {
            if (n >= p.N) return 0u;
            const int cc = n / p.T, t = n - cc * p.T;
            return (unsigned)((cc - c_lo) * p.cpb + (p.off[t] - p.minoff) * 2);      // channel image + element offset of the tap
        } else {
            return 16u * 32u * tn;
        }
    }
    // byte offset of k block kb for lane half g of the wave whose first column (inside the tile) is col0 + lane j
    __device__ __forceinline__ static int kblock(int kb, int g, int colj) {
        return PL ? (kb * 16 + g * 8) * 2 : (kb * 2 * wx6_gs(BN) + g * wx6_gs(BN) + colj) * 16;
    }
    // the strided loads of rounds 0 .. nq - 1; a sample is out of range (reads 0.0) outside [0, s_valid)
    template <class RSRC>
    __device__ __forceinline__ void load(const Wx6P& p, RSRC rsrc, const Wx6Step& sp, int nq) {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            if (q >= nq) continue;                                                  // uniform: a whole round without tasks
            const unsigned base = off[q] == kOOB ? kOOB : off[q] + sp.ss;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                unsigned o = base == kOOB ? kOOB : base + 4u * (unsigned)(i * p.is);
                if (sp.s_edge) {
                    const int pos = sp.n * p.is + p0[q] + i * p.is;
                    o = (pos >= 0 && pos < p.s_valid) ? o : kOOB;
                }
                v[q][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o, 0, 0));
            }
        }
    }
    __device__ __forceinline__ void convert(const Wx6P& p, float sc, unsigned char* b_stage, int nq) const {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            if (q >= nq || dst[q] < 0) continue;
            emit(v[q], p.s_slope, sc, reinterpret_cast<u32x4*>(b_stage + dst[q]), (int)(piece >> 4));
        }
    }
};

// One k block of one wave: the A fragments of TM 32-row tiles (al: the lane's row of tile 0 in the k block's [g][piece][BM]) times
// the B fragments of TN 32-column tiles (bl + bcol[tn] + piece s3; PL: a 16-byte read at 2-byte alignment, a plain C++ load through
// a 2-byte-aligned vector type that the compiler emits as ds_read_b128, counts and schedules like the aligned reads).  Products
// smallest terms first; order inside a step: product, row tile, column tile.  live2 (uniform): the second column tile holds
// columns of the weight tensor at all -- a dead tile's slots hold stale data: read, never multiplied.
template <int TM, int TN, int BM, bool PL>
__device__ __forceinline__ void wx6_mma(f32x16 (&acc)[TM][TN], const u32x4* al, const unsigned char* bl, const unsigned (&bcol)[TN],
                                        unsigned piece, bool live2) {
    constexpr int SA[RH_X6_NPROD] = RH_X6_SA, SB[RH_X6_NPROD] = RH_X6_SB;
    rh_x6_frag afr[TM][kX6P], bfr[TN][kX6P];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int s3 = 0; s3 < kX6P; ++s3) afr[tm][s3] = __builtin_bit_cast(rh_x6_frag, al[s3 * BM + tm * 32]);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int s3 = 0; s3 < kX6P; ++s3) {
            const unsigned char* f = bl + bcol[tn] + (unsigned)s3 * piece;
            if constexpr (PL) bfr[tn][s3] = __builtin_bit_cast(rh_x6_frag, *reinterpret_cast<const u32x4_u*>(f));
            else bfr[tn][s3] = __builtin_bit_cast(rh_x6_frag, *reinterpret_cast<const u32x4*>(f));
        }
#pragma unroll
    for (int q = 0; q < RH_X6_NPROD; ++q)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            acc[tm][0] = RH_X6_MFMA(afr[tm][SA[q]], bfr[0][SB[q]], acc[tm][0]);
            if constexpr (TN == 2) {
                if (live2) acc[tm][1] = RH_X6_MFMA(afr[tm][SA[q]], bfr[1][SB[q]], acc[tm][1]);
            }
        }
}

// One wave's 32 x 32 accumulator tile -> rows mb + ... (mb: first row of the tile + 4 g) of column col < N of this K slice's partials
__device__ __forceinline__ void wx6_store_tile(const Wx6P& p, float* __restrict__ outz, const f32x16& acc, int mb, int col, float osc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        if (m < p.M) outz[(long)m * p.N + col] = RH_X6_F16 ? acc[r] * osc : acc[r];
    }
}

// ---- The 4-wave tile.
// AV: rows of R are 16-byte aligned (Wx6RTasks::load)
// PART: the last column tile holds whole 32-column MFMA tiles past the end of the weight tensor -- their columns are
// neither converted nor multiplied (a separate instantiation: the two uniform branches cost 14 VGPRs, which would take the
// 64-row variants from three workgroups per CU to two)
// PL ("planes", round 5; Wx6STasks): the S operand of a stride-1 layer with several taps is staged ONCE PER POSITION.  A tap is an
// address offset; nothing is converted per tap: C = 96, k = 3 converts
// (96 + 91) x 32 samples per step instead of (96 + 256) x 32, dilation 9 (96 + 134) x 32; C >= 192 (192 + 46) instead of
// (192 + 128).  Same products in the same order: bit-identical weight gradients (tests/test_gpu_dispatch.py; at the tile edges and
// tails: tests/test_gpu_wgrad_matrix.py).
// MEASURED SLOWER from C = 192 on and therefore opt-in there (profiles/round5_negative_wgrad_planes.txt, round 6: plan_wx6): the
// 64-row variants need 158-169 registers, two workgroups per CU instead of three where they pass 168 (forced under it they spill).
template <int TM, int WM, int WN, bool AV, bool PART, bool PL>
__global__ __launch_bounds__(256, 2) void wgrad_x6_kernel(const Wx6P p) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int NT = 256, BM = 32 * TM * WM, BN = 64 * WN;
    // PL: (channel, octet) tasks -- at most BN / 2 + 2 channel images of <= 7 octets
    constexpr int NB = PL ? ((BN / 2 + 2) * 7 + NT - 1) / NT : kOct * BN / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* const a_st = reinterpret_cast<u32x4*>(smem_raw);              // [kKS][g][piece][BM]
    unsigned char* const b_st = smem_raw + wx6_stage(BM) * 16;           // [kKS][g][piece][BN]   (PL: [piece][channel][position])

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, g = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN, z = blockIdx.z;

    const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.R), 0, p.r_bytes, 0x00020000);
    const auto s_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.S), 0, p.s_bytes, 0x00020000);
    const Wx6Scale sc = wx6_scales(p);

    Wx6RTasks<NT, BM> rt;
    Wx6STasks<NT, NB, BN, PL> stk;
    rt.init(p, tid, m0);
    stk.init(p, tid, n0, PART);
    unsigned bcol[2];                                                     // this lane's two columns
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) bcol[tn] = stk.column(p, n0 + wn * 64 + tn * 32 + j, tn);

    f32x16 acc[TM][2];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // the first column tile of every row tile adds up the row sums
    const bool want_rsum = p.rsum != nullptr && blockIdx.x == 0;      // uniform
    auto load = [&](int st) {
        const Wx6Step sp = wx6_step<PL>(p, st);
        rt.load(p, r_rsrc, sp, AV);
        stk.load(p, s_rsrc, sp, NB);
    };
    auto convert = [&]() {
        if (want_rsum) rt.add_rows();
        rt.convert(p, sc.r, a_st);
        stk.convert(p, sc.s, b_st, NB);
    };

    const int st0 = z * p.steps_per_z;
    const int nst = min(p.steps_per_z, p.total_steps - st0);
    if (nst > 0) {
        load(st0);
        convert();
    }
    __syncthreads();
    const u32x4* const al = a_st + g * wx6_gs(BM) + wm * TM * 32 + j;
    // How many of this wave's two 32-column tiles hold columns of the weight tensor at all (wave-uniform).  The 96-row layers
    // run 96 x 256 workgroup tiles over N = 288 (k = 3) or 96 (k = 1) columns: the second tile of the former holds 32 live
    // columns, the only tile of the latter 96 -- multiplying (and converting) the dead ones cost those layers 30-40 %.
    const int live_tn = !PART ? 2 : (n0 + wn * 64 >= p.N ? 0 : (n0 + wn * 64 + 32 >= p.N ? 1 : 2));
    const bool live1 = live_tn >= 1, live2 = live_tn == 2;            // scalar (wn, n0, N are): uniform branches below
    // one LDS stage: the next step's samples wait in registers while the matrix cores work on this step's fragments
    // (the other workgroup of the CU runs its MFMAs while this one converts)
    for (int s = 0; s < nst; ++s) {
        const bool more = s + 1 < nst;
        if (more) load(st0 + s + 1);
        if (live1) {
#pragma unroll
            for (int kb = 0; kb < kKS; ++kb)
                wx6_mma<TM, 2, BM, PL>(acc, al + kb * 2 * wx6_gs(BM), b_st + stk.kblock(kb, g, wn * 64 + j), bcol, stk.piece, live2);
        }
        __syncthreads();                 // every wave is done reading this step's fragments
        if (more) convert();
        __syncthreads();
    }

    if (want_rsum) rt.store_sums(p, tid, m0, z);
    // ---- partial sums of this K slice
    float* __restrict__ outz = p.out + (long)z * p.M * p.N;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int col = n0 + wn * 64 + tn * 32 + j;
        if (col >= p.N) continue;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) wx6_store_tile(p, outz, acc[tm][tn], m0 + (wm * TM + tm) * 32 + 4 * g, col, sc.out);
    }
}

// ---- The column-complete tile for layers with at most 96 gradient rows and at most 288 columns (v2: C = 96 k = 3 / k = 1, the stem).
// The 4-wave kernel above runs those as 96 x 256 workgroup tiles: N = 288 needs two, the second with 32 live columns, and every
// workgroup of it loads and converts all 96 dy rows to feed a ninth of the MFMAs; N = 96 / 112 leave three of the four waves'
// column ranges partly or wholly dead.  Here ONE workgroup tile covers all rows and all columns: NW waves, wave w owns the three
// 32-row MFMA tiles of columns 32 w .. 32 w + 31 (TM = 3, TN = 1: 48 accumulator registers), so the 27 tiles of N = 288 divide over
// nine waves exactly.  Per step dy is loaded and converted once per workgroup, and x once per position (PL) or once per column
// (pointwise / strided layers).  The thread -> task tables follow the wave count; the S tasks are dealt from the last thread down,
// so that the waves without R tasks (nine waves: 384 R tasks over 576 threads) take the second round of S tasks.  NW is rounded
// up to 3, 4, 6 or 9: a wave whose 32 columns lie past the weight tensor takes its share of the conversion of live samples, but
// reads no fragments and multiplies nothing.
// Two fragment stages, ONE barrier per step: the next step is converted into the other stage while slower waves still multiply
// (one stage with two barriers, as above, measured 1 ... 4 % slower on every layer: profiles/wgrad_wide_tile_sweep.txt).  Same K
// slicing => the same sums in the same order as the 4-wave kernel: bit-identical gradients (tests/test_gpu_wgrad_wide.py).
// p.av is the 4-wave kernel's AV as a uniform branch.
template <int NW, bool PL>
__global__ __launch_bounds__(64 * NW) void wgrad_x6_wide_kernel(const Wx6P p) {
    constexpr int TM = 3, BM = 32 * TM, BN = 32 * NW, NT = 64 * NW;
    // S tasks: kOct * BN = 2 NT (column, octet) tasks; PL: at most BN / 2 channel images of <= 7 octets = 1.75 NT
    constexpr int NB = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* const a_st = reinterpret_cast<u32x4*>(smem_raw);                               // [2][kKS][g][piece][BM]
    unsigned char* const b_st = smem_raw + 2 * wx6_stage(BM) * 16;                        // [2] x p.b_stage bytes

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, g = lane >> 5;
    const int z = blockIdx.x;

    const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.R), 0, p.r_bytes, 0x00020000);
    const auto s_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.S), 0, p.s_bytes, 0x00020000);
    const Wx6Scale sc = wx6_scales(p);

    Wx6RTasks<NT, BM> rt;
    Wx6STasks<NT, NB, BN, PL> stk;
    rt.init(p, tid, 0);
    stk.init(p, NT - 1 - tid, 0, true);              // dead columns convert nothing
    const int nq = PL ? (p.C * p.p8 + NT - 1) / NT : NB;             // (uniform) task rounds that hold a task at all
    // nine waves: waves 6 ... 8 have no R task (scalar branch; with a partly filled second round -- four waves -- the same
    // test costs 11 registers and a wave per SIMD, so those lanes load out of range instead)
    const bool r_wave = !(NT > kOct * BM && 64 * wave >= kOct * BM);
    const int col = 32 * wave + j;                                       // this lane's column
    const bool live = 32 * wave < p.N;                                   // scalar: does this wave own columns of the weight tensor at all
    const unsigned bcol[1] = {stk.column(p, col, 0)};

    f32x16 acc[TM][1];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tm][0][r] = 0.f;

    const bool want_rsum = p.rsum != nullptr;
    auto load = [&](int st) {
        const Wx6Step sp = wx6_step<PL>(p, st);
        if (r_wave) rt.load(p, r_rsrc, sp, p.av != 0);
        stk.load(p, s_rsrc, sp, nq);
    };
    auto convert = [&](int stage) {
        if (want_rsum) rt.add_rows();
        rt.convert(p, sc.r, a_st + stage * wx6_stage(BM));
        stk.convert(p, sc.s, b_st + stage * p.b_stage, nq);
    };
    auto multiply = [&](int stage) {
        const u32x4* const al = a_st + stage * wx6_stage(BM) + g * wx6_gs(BM) + j;
        const unsigned char* const bs = b_st + stage * p.b_stage;
#pragma unroll
        for (int kb = 0; kb < kKS; ++kb)
            wx6_mma<TM, 1, BM, PL>(acc, al + kb * 2 * wx6_gs(BM), bs + stk.kblock(kb, g, col), bcol, stk.piece, false);
    };

    const int st0 = z * p.steps_per_z;
    const int nst = min(p.steps_per_z, p.total_steps - st0);
    if (nst > 0) {
        load(st0);
        convert(0);
    }
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const bool more = s + 1 < nst;
        if (more) load(st0 + s + 1);
        // the stage written here was last read in step s - 1, and every wave has passed that step's barrier
        if (live) multiply(s & 1);
        if (more) convert((s + 1) & 1);
        __syncthreads();
    }

    if (want_rsum) rt.store_sums(p, tid, 0, z);
    // ---- partial sums of this K slice
    if (col < p.N) {
        float* __restrict__ outz = p.out + (long)z * p.M * p.N;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) wx6_store_tile(p, outz, acc[tm][0], tm * 32 + 4 * g, col, sc.out);
    }
}

struct Wx6Plan {
    int tm, wm, rt, ct, Z, steps_per_z;
    int planes;              // the S operand staged once per position as 16-bit element planes (PL)
    int nw;                  // > 0: the column-complete tile (wgrad_x6_wide_kernel) with nw waves
    int own_z;               // the wide tile with its own K slicing (0: the 4-wave plan's, RH_WGRAD_X6_WIDE=2)
    size_t lds;
};

// The switches, read here and nowhere else.  The first four are read on every call (the tests flip them at run time), the last
// two once per process.
struct Wx6Env {
    bool off;                // RH_WGRAD_X6=0: this path takes nothing
    int planes;              // RH_WGRAD_X6_PLANES: 1 / 0 = plane staging everywhere / nowhere it can go, -1 (unset) = by the layer
    int wide;                // RH_WGRAD_X6_WIDE: 0 = 4-wave tiles only, 2 = the wide tile with the 4-wave plan's K slicing; default 1
    int blocks;              // RH_WGRAD_X6_BLOCKS: workgroups the K slicing aims at (-1: the resident ones); 0 = default
    int all;                 // RH_WGRAD_X6_ALL: also the <= 64-row layers on long sequences
    int tm;                  // RH_WGRAD_X6_TM: 1 ... 3 forces the row tiles per wave
    bool forced_tm() const { return tm >= 1 && tm <= 3; }
};

Wx6Env read_wx6_env() {
    const auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    static const int all = num("RH_WGRAD_X6_ALL", 0), tm = num("RH_WGRAD_X6_TM", 0);
    const char* pe = getenv("RH_WGRAD_X6_PLANES");
    return Wx6Env{num("RH_WGRAD_X6", 1) == 0, pe ? (pe[0] == '1' ? 1 : 0) : -1, num("RH_WGRAD_X6_WIDE", 1), num("RH_WGRAD_X6_BLOCKS", 0), all, tm};
}

// Step 1: does the layer take this path at all.
bool wx6_eligible(const WgradP& w, const Wx6Env& env, const unsigned* r_range, const unsigned* s_range) {
    if (env.off) return false;
    if (RH_X6_F16 && (!r_range || !s_range)) return false;      // no range slots (rh_x6_set_ranges): f32-input MFMA kernels
    if (w.inner != 1 || w.T > kMaxTaps || w.B <= 0 || w.r_row <= 0) return false;
    if ((w.r_act != RH_ACT_NONE && w.r_act != RH_ACT_LEAKY) || (w.s_act != RH_ACT_NONE && w.s_act != RH_ACT_LEAKY)) return false;
    // the conversion applies LeakyReLU as max(x, slope x)
    if ((w.r_act == RH_ACT_LEAKY && !(w.r_slope >= 0.f && w.r_slope <= 1.f)) || (w.s_act == RH_ACT_LEAKY && !(w.s_slope >= 0.f && w.s_slope <= 1.f))) return false;
    if (w.M < 32 || (long)w.C * w.T < 64) return false;            // tiny GEMMs (first discriminator layers): f32 kernels
    // Measured per layer (profiles/round2_layer_table_b32.txt): 1.2x ... 1.6x over the f32-MFMA kernel (wgrad_dma_kernel)
    // wherever the weight tensor offers a few output tiles -- everything but the <= 96-row layers on long sequences
    // (C = 96 at 4096 positions: one to three tiles, so K is cut into hundreds of slices whose partial tiles cost more
    // than the matrix work; the f32 kernel's 96-column tiles and LDS-DMA row segments win there).
    // (round 3: with conflict-free fragment writes and the cheaper conversion the 96-row layers moved over too -- C = 96 k = 3
    // 115 -> 100 us, k = 1 59 -> 56; the 32-row output layer stays: 94 us on the f32 kernel against 120 here)
    if (!env.all && w.M <= 64 && w.r_row > 1024) return false;
    // byte offsets are 32-bit
    return 4ull * w.B * w.M * (unsigned long long)w.r_row < 0x7fffffffull && 4ull * w.B * w.C * (unsigned long long)w.s_row < 0x7fffffffull;
}

// Plane staging (PL) of a tile that touches at most chmax channels: stride-1 layers with several taps whose reach fits the image
// (<= 7 octets per channel: the k = 3 units up to dilation 9 -- reach 18 --, the k = 7 stem).  Fills p8 / cpb / chmax; returns
// whether the layer can be staged that way, *bytes = one stage of the image.
bool wx6_plane_geometry(const WgradP& w, int chmax, Wx6P* p, size_t* bytes) {
    const int reach = w.maxoff - w.minoff;
    p->p8 = (32 + reach + 7) / 8;
    p->cpb = 16 * ((p->p8 & 1) ? p->p8 : p->p8 + 1);            // odd number of 16-byte slots: channel images start on different banks
    p->chmax = chmax;
    *bytes = (size_t)kX6P * chmax * p->cpb + 32;
    return w.is == 1 && w.T >= 2 && reach >= 0 && p->p8 <= 7 && 4l * (w.s_row + 64) * w.C * w.B < 0x7fffffffl;
}

// Step 2: the tile.  Returns the number of output tiles the 4-wave plan has (what its K slicing divides by).
int wx6_choose_tile(const WgradP& w, const Wx6Env& env, Wx6P* p, Wx6Plan* pl) {
    const int Mp = (w.M + 31) & ~31;
    // 4-wave tiles.  96-row wave tiles (TM = 3: 216 VGPRs, two workgroups per CU) convert the least per MFMA, but 64-row ones
    // (TM = 2: 158 VGPRs, 50 KB of LDS) fit THREE workgroups per CU, and a third set of phases to interleave is worth more wherever
    // 128-row workgroup tiles divide the rows (measured per layer: C = 384 k = 3 76 -> 68 us, 384 -> 768 k = 8 111 -> 96,
    // C = 768 91 -> 85; M = 192 loses a quarter of the tile and stays on TM = 3)
    // -- and the reduction is long enough: pointwise layers (C = 384 / 768, k = 1) lose 5 ... 19 % with it
    pl->tm = (Mp % 128 == 0 && Mp >= 256 && w.T > 1) ? 2 : (Mp % 96 == 0 ? 3 : (Mp % 64 == 0 ? 2 : 1));
    if (env.forced_tm()) pl->tm = env.tm;
    pl->wm = Mp >= 64 * pl->tm ? 2 : 1;
    const int BM = 32 * pl->tm * pl->wm, BN = 64 * (4 / pl->wm);
    pl->rt = rh_cdiv(w.M, BM);
    pl->ct = rh_cdiv(p->N, BN);
    const int four_wave_tiles = pl->rt * pl->ct;
    // The column-complete tile (wgrad_x6_wide_kernel): 65 ... 96 gradient rows and at most 288 columns -- one workgroup tile over
    // the whole weight tensor, one wave per 32 columns.  RH_WGRAD_X6_WIDE: 0 = the 4-wave tiles above; 2 = the wide tile with the
    // K slicing the 4-wave plan would take (same sums in the same order: the bit-identity tests and A/B runs).
    // A forced RH_WGRAD_X6_PLANES or RH_WGRAD_X6_TM asks for a 4-wave instance by name and gets it.
    pl->nw = 0; pl->own_z = 0;
    size_t plane_bytes;
    if (env.wide != 0 && env.planes < 0 && !env.forced_tm() && w.M > 64 && w.M <= 96 && p->N <= 288) {
        const int tiles = rh_cdiv(p->N, 32);
        pl->nw = tiles <= 3 ? 3 : (tiles <= 4 ? 4 : (tiles <= 6 ? 6 : 9));
        pl->own_z = env.wide != 2;
        pl->tm = 3; pl->wm = 1; pl->rt = 1; pl->ct = 1;
        pl->planes = wx6_plane_geometry(w, w.C, p, &plane_bytes);       // the tile touches every channel, and only those
        p->av = w.r_row % 4 == 0 && ((uintptr_t)w.R & 15) == 0;
        p->b_stage = (unsigned)(pl->planes ? (plane_bytes + 15) / 16 * 16 : (size_t)wx6_stage(32 * pl->nw) * 16);
        pl->lds = 2 * ((size_t)wx6_stage(96) * 16 + p->b_stage);          // two stages
    } else {
        // Plane staging on the 4-wave tile (no instance for 32-row wave tiles: that one needed scratch).  Round 6
        // (compiler-visible unaligned reads, two f16 pieces): faster where the rows are few and the conversion dominates
        // -- M <= 96: C = 96 k = 3 104 -> 89 us, stem / output layer +3 % -- slower from C = 192 on (C = 384 k = 3 59 -> 79 us):
        // on by default for M <= 96, RH_WGRAD_X6_PLANES = 1 / 0 forces it everywhere / nowhere.
        const bool on = env.planes >= 0 ? env.planes == 1 : Mp <= 96;
        pl->planes = wx6_plane_geometry(w, BN / w.T + 2, p, &plane_bytes) && on && pl->tm >= 2;
        pl->lds = (size_t)wx6_stage(BM) * 16 + (pl->planes ? plane_bytes : (size_t)wx6_stage(BN) * 16);
    }
    return four_wave_tiles;
}

// Step 3: K slices over (batch, position) ranges of at least 4 steps (128 positions).
void wx6_slice_k(const Wx6Env& env, int four_wave_tiles, Wx6P* p, Wx6Plan* pl) {
    // One round of workgroups (512) -- every extra slice is another copy of the whole weight tensor written and
    // re-read.  (Rounds 2-4 ran two rounds, 1024, when the weight tensor has >= 32 tiles: measured per layer then, slower
    // in the step now.)
    // round 5, A/B on two boxes (tools/debug/exp_r5_*.sh): 512 everywhere 10.02-10.04 ms per step against 10.08-10.09 with two
    // rounds (1024) for the many-tile layers, 10.11 with "resident slots" (768 for TM = 2: RH_WGRAD_X6_BLOCKS=-1 -- 64-row wave
    // tiles fit three per CU, the others two), 10.10 at 384, 10.35 at 640
    // wide tile, measured per layer at batch 32 (profiles/wgrad_wide_tile.md): nine-wave workgroups are resident one per CU (122
    // registers: two would need <= 96 and spill 20), and ONE round of them, 256 slices, is fastest (C = 96 k = 3: 58 us against
    // 67 at 512, 95 at 128); the 3- / 4- / 6-wave ones keep 512
    const int dflt = pl->nw == 9 && pl->own_z ? 256 : 512;
    const int target = env.blocks > 0 ? env.blocks : (env.blocks < 0 ? (pl->tm == 2 ? 768 : 512) : dflt);
    int Z = rh_cdiv(target, pl->own_z ? 1 : four_wave_tiles);
    const int zmax = p->total_steps / 4 > 0 ? p->total_steps / 4 : 1;
    if (Z > zmax) Z = zmax;
    if (Z < 1) Z = 1;
    pl->steps_per_z = rh_cdiv(p->total_steps, Z);
    pl->Z = rh_cdiv(p->total_steps, pl->steps_per_z);
    p->steps_per_z = pl->steps_per_z;
}

bool plan_wx6(const WgradP& w, Wx6P* p, Wx6Plan* pl, const unsigned* r_range, const unsigned* s_range) {
    const Wx6Env env = read_wx6_env();
    if (!wx6_eligible(w, env, r_range, s_range)) return false;
    *p = Wx6P{};
    p->R = w.R; p->S = w.S;
    p->B = w.B; p->M = w.M; p->C = w.C; p->T = w.T; p->N = w.C * w.T;
    p->r_row = w.r_row; p->s_row = w.s_row; p->s_valid = w.s_valid; p->is = w.is;
    p->r_slope = w.r_act == RH_ACT_LEAKY ? w.r_slope : 1.f;
    p->s_slope = w.s_act == RH_ACT_LEAKY ? w.s_slope : 1.f;
    p->steps_per_b = rh_cdiv(w.r_row, kSpan);
    p->total_steps = w.B * p->steps_per_b;
    p->r_bytes = (unsigned)(4ull * w.B * w.M * w.r_row); p->s_bytes = (unsigned)(4ull * w.B * w.C * w.s_row);
    p->minoff = w.minoff; p->maxoff = w.maxoff;
    p->r_range = r_range; p->s_range = s_range;
    for (int t = 0; t < w.T; ++t) p->off[t] = w.off[t];
    wx6_slice_k(env, wx6_choose_tile(w, env, p, pl), p, pl);
    return true;
}

// ---- Launch.  One helper per kernel INSTANCE (the kernel is the template argument, so the once_flag is its own): raises the
// dynamic LDS limit once, then launches.
using Wx6Launch = void (*)(dim3 grid, int threads, size_t lds, hipStream_t stream, const Wx6P& p);

template <void (*KERN)(Wx6P)>
void launch_wx6(dim3 grid, int threads, size_t lds, hipStream_t stream, const Wx6P& p) {
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    rh_launch_main(KERN, grid, dim3(threads), lds, stream, p);
}

// f(std::integral_constant<int, V>) for the V of Vs that equals v (null if none does): run-time value -> template argument
template <int... Vs, class F>
Wx6Launch wx6_pick(int v, F f) {
    Wx6Launch r = nullptr;
    ((v == Vs ? (void)(r = f(std::integral_constant<int, Vs>{})) : (void)0), ...);
    return r;
}

// The instance of a plan, by name: what wx6_instance turns into a kernel and rh_wgrad_x6_instance_info reports.
struct Wx6Inst {
    int nw;                  // > 0: wgrad_x6_wide_kernel<nw, pl>; 0: wgrad_x6_kernel<tm, wm, 4 / wm, av, part, pl>
    int tm, wm;
    int av;                  // rows of R are 16-byte aligned (wide tile: the uniform p.av, no template argument)
    int part;                // 32-column MFMA tiles do not fill the last workgroup tile (4-wave kernel only)
    int pl;
};

Wx6Inst wx6_inst_of(const Wx6P& p, const Wx6Plan& pl) {
    if (pl.nw > 0) return Wx6Inst{pl.nw, 3, 1, p.av, 0, pl.planes};
    const int av = p.r_row % 4 == 0 && ((uintptr_t)p.R & 15) == 0;
    const int part = rh_cdiv(p.N, 32) % (2 * (4 / pl.wm)) != 0;
    return Wx6Inst{0, pl.tm, pl.wm, av, part, pl.planes && pl.tm >= 2};
}

// The kernel of an instance: wgrad_x6_wide_kernel<NW, PL> (8) or wgrad_x6_kernel<TM, WM, 4 / WM, AV, PART, PL> (40: the plan asks
// for no plane staging with TM = 1, and there is no such instance).
Wx6Launch wx6_instance(const Wx6Inst& in) {
    if (in.nw > 0)
        return wx6_pick<3, 4, 6, 9>(in.nw, [&](auto NW) {
            return wx6_pick<0, 1>(in.pl, [&](auto PL) -> Wx6Launch { return launch_wx6<wgrad_x6_wide_kernel<decltype(NW)::value, decltype(PL)::value != 0>>; });
        });
    return wx6_pick<1, 2, 3>(in.tm, [&](auto TM) {
        return wx6_pick<1, 2>(in.wm, [&](auto WM) {
            return wx6_pick<0, 1>(in.av, [&](auto AV) {
                return wx6_pick<0, 1>(in.part, [&](auto PART) {
                    return wx6_pick<0, 1>(in.pl, [&](auto PL) -> Wx6Launch {
                        constexpr int tm = decltype(TM)::value, wm = decltype(WM)::value;
                        constexpr bool planes = decltype(PL)::value != 0 && tm >= 2;
                        return launch_wx6<wgrad_x6_kernel<tm, wm, 4 / wm, decltype(AV)::value != 0, decltype(PART)::value != 0, planes>>;
                    });
                });
            });
        });
    });
}

// What rh_wgrad_x6_plan leaves in RhWx6Planned::state.
struct Wx6Planned {
    Wx6P p;
    Wx6Plan pl;
};
static_assert(sizeof(Wx6Planned) <= sizeof(RhWx6Planned::state) && alignof(Wx6Planned) <= 16 && std::is_trivially_copyable<Wx6Planned>::value,
              "RhWx6Planned::state holds a Wx6Planned");
const Wx6Planned& wx6_planned(const RhWx6Planned& q) { return *reinterpret_cast<const Wx6Planned*>(q.state); }

}  // namespace

bool rh_wgrad_x6_plan(const WgradP& w, const unsigned* r_range, const unsigned* s_range, RhWx6Planned* out) {
    Wx6Planned* const q = new (out->state) Wx6Planned{};
    if (!plan_wx6(w, &q->p, &q->pl, r_range, s_range)) return false;
    out->Z = q->pl.Z;
    // partial weight tiles (Z > 1) + partial row sums for the fused bias gradient (always reserved)
    out->ws_bytes = (q->pl.Z > 1 ? (int64_t)q->pl.Z * w.M * w.C * w.T : 0) * (int64_t)sizeof(float) + (int64_t)q->pl.Z * w.M * (int64_t)sizeof(float);
    return true;
}

// out4 = {waves per workgroup, workgroups, K slices, plane staging} of the planned launch
void rh_wgrad_x6_plan_info(const RhWx6Planned& planned, int32_t* out4) {
    const Wx6Plan& pl = wx6_planned(planned).pl;
    out4[0] = pl.nw > 0 ? pl.nw : 4;
    out4[1] = pl.rt * pl.ct * pl.Z;
    out4[2] = pl.Z;
    out4[3] = pl.planes;
}

// The instance of the planned launch (the plan's R carries the alignment of R): wx6_inst_of, what the launch itself asks.  out16 =
// {1, wide, NW or tm, wm, AV, PART, PL, Z, steps_per_z, total_steps, tile rows, tile columns, steps_per_b, p8, chmax, row tiles *
// column tiles}
void rh_wgrad_x6_instance_info(const RhWx6Planned& planned, int32_t* out16) {
    const Wx6P& p = wx6_planned(planned).p;
    const Wx6Plan& pl = wx6_planned(planned).pl;
    const Wx6Inst in = wx6_inst_of(p, pl);
    const int32_t v[16] = {1, in.nw > 0, in.nw > 0 ? in.nw : in.tm, in.nw > 0 ? 0 : in.wm, in.av, in.part, in.pl, pl.Z, pl.steps_per_z,
                           p.total_steps, in.nw > 0 ? 96 : 32 * in.tm * in.wm, in.nw > 0 ? 32 * in.nw : 64 * (4 / in.wm), p.steps_per_b,
                           in.pl ? p.p8 : 0, in.pl ? p.chmax : 0, pl.rt * pl.ct};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
}

// ws must hold planned.ws_bytes.  The weight partials of a split K range stay UNREDUCED in ws ([Z][M][C*T]) for the caller's
// reduction tail (conv_wgrad.hip: finish_dw); the row-sum (bias) partials behind them are reduced here.
int rh_wgrad_x6_launch(const RhWx6Planned& planned, float* dw, float* rsum_out, void* ws, hipStream_t stream) {
    Wx6P p = wx6_planned(planned).p;
    const Wx6Plan& pl = wx6_planned(planned).pl;
    p.out = pl.Z > 1 ? (float*)ws : dw;
    float* const rs_part = (float*)ws + (pl.Z > 1 ? (long)pl.Z * p.M * p.C * p.T : 0);
    p.rsum = rsum_out ? (pl.Z > 1 ? rs_part : rsum_out) : nullptr;
    const dim3 grid = pl.nw > 0 ? dim3(pl.Z) : dim3(pl.ct, pl.rt, pl.Z);
    wx6_instance(wx6_inst_of(p, pl))(grid, pl.nw > 0 ? 64 * pl.nw : 256, pl.lds, stream, p);
    if (int e = rh_check_launch("conv1d_bwd_weight_x6")) return e;
    if (pl.Z > 1 && rsum_out) return rh_reduce_partials_launch(rs_part, rsum_out, p.M, pl.Z, stream, "conv1d_bwd_bias_reduce");
    return RH_OK;
}
