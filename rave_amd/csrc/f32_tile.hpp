// What the f32-input matrix-core kernels ("family 0": v_mfma_f32_32x32x2_f32, exact f32, k-ordered sums) of conv_igemm.hip,
// conv_igemm_dma.hip, conv_wgrad.hip and conv2d_f32.hip share: the LDS-DMA constants, the 32-bit reciprocal division and the
// plan arithmetic of their launches.  The kernel bodies share no code on purpose: lane decomposition, accumulator zeroing,
// the MFMA k-steps and the stores were tried as inline functions here, and each of them alone changed the register allocation
// of every instance it touched (profiles/f32_tile_refactor.txt).
#pragma once
#include "common.hpp"

typedef __attribute__((address_space(3))) void lds_void;   // LDS destination of a buffer_load ... lds
constexpr unsigned kOOB = 0x80000000u;                      // >= any descriptor size we accept -> the DMA writes zeros

inline int round32(int m) { return (m + 31) & ~31; }
inline int pow2ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
// ceil(2^32 / d) for mdiv(); 0 encodes d == 1
inline unsigned magic32(int d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + d - 1) / d); }
// n / d for n * d < 2^32 with magic = magic32(d)
__device__ __forceinline__ unsigned mdiv(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }

// Channels per K chunk: what fits `budget_floats` at `per_ch` floats per channel, even (mult8: a multiple of 8 from 8 up, for
// the 4-step k loop), 2 ... 32, and no more than C rounded up to even.
inline int ck_for(int budget_floats, int per_ch, int C, bool mult8) {
    int ck = budget_floats / per_ch;
    ck &= (mult8 && ck >= 8) ? ~7 : ~1;
    if (ck > 32) ck = 32;
    if (ck < 2) ck = 2;
    const int cmax = (C + 1) & ~1;
    return ck > cmax ? cmax : ck;
}
