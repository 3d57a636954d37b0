// Tap plan of a 2-D convolution call and the entry points of its f32-input kernel family (conv2d_f32.hip); the router
// (conv2d.hip) builds the plan once and hands it to whichever family takes the call.
#pragma once
#include "conv_params.hpp"

constexpr int kPh2 = 8;   // max sh*sw

struct Plan2 {
    int nphase = 0;
    int oph_h[kPh2], oph_w[kPh2], ntaps[kPh2], tap0[kPh2], minh[kPh2], minw[kPh2], maxh[kPh2], maxw[kPh2];
    int nslots = 0;
    int kk[kMaxTaps], offh[kMaxTaps], offw[kMaxTaps];
};

// What a staged input patch has to cover beyond the output block itself: the largest tap span of any phase in both dimensions,
// and the most taps of a phase (at least 1).
struct PatchGeom {
    int span_h, span_w, maxtaps;
};
inline PatchGeom patch_geom(const Plan2& t) {
    PatchGeom g{0, 0, 1};
    for (int i = 0; i < t.nphase; ++i) {
        g.span_h = g.span_h > t.maxh[i] - t.minh[i] ? g.span_h : t.maxh[i] - t.minh[i];
        g.span_w = g.span_w > t.maxw[i] - t.minw[i] ? g.span_w : t.maxw[i] - t.minw[i];
        g.maxtaps = g.maxtaps > t.ntaps[i] ? g.maxtaps : t.ntaps[i];
    }
    return g;
}

// Kernels of rh_conv2d_instance_info (include/rave_hip.h)
enum { K2_X6 = 0, K2_DMA, K2_IGEMM, K2_SMALLM, K2_SMALLC, K2_WX6, K2_WDMA, K2_WGRAD };

// conv2d_f32.hip: the f32-input MFMA kernels ("family 0"), which take every call the other families leave.  info == null: plan
// and launch; else plan, fill info[0 .. 19] as include/rave_hip.h documents (kernel, template arguments, tile plan, and in
// info[19] why the LDS-DMA kernel was not taken / whether the scratch offered is too small) and launch nothing.
// which: 0 = forward, 1 = data gradient (y: the activated output whose act'(y) is folded into dy while staging, or null).
int rh_conv2d_f32_conv(const rh_conv2d_desc* d, int which, const Plan2& t, const float* in, const float* y, const float* wp,
                       const float* bias, float* out, hipStream_t stream, const char* what, int64_t* info);
// workspace: behind the bias scratch; ymul: y of a fused activation derivative or null
int rh_conv2d_f32_wgrad(const rh_conv2d_desc* d, const float* dy, const float* ymul, const float* x, float* dw, void* workspace,
                        int64_t workspace_bytes, hipStream_t stream, int64_t* info);
// split-K scratch of the weight gradient, for the larger of the two plans a call may take
int64_t rh_conv2d_f32_wgrad_workspace(const rh_conv2d_desc* d);
