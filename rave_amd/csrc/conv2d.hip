// General 2-D convolution (zero padding, stride, dilation in both dims, groups == 1) for the Conv2d stacks of the spectral
// discriminators: rave/discriminator.py:23-74 (EncodecConvNet), rave/descript_discriminator.py:30-66,118-184 (MPD, MRD).
//
// This unit is the ABI: descriptor validation, the tap plan (forward: one phase; data gradient: one phase per output phase
// alpha_h < sh, alpha_w < sw), weight packing, and the choice of the kernel family that runs a call.  The kernels are in
// conv2d_f32.hip (f32-input matrix cores, "family 0"), conv2d_x6.hip, wgrad2d_x6.hip, conv2d_smallm.hip and conv2d_smallc.hip.
#include "conv2d_plan.hpp"
#include "conv2d_x6.hpp"
#include "f32_tile.hpp"

// wgrad2d_x6.hip: weight gradient on the bf16 matrix cores (<= 32 output channels, stride 1 along W)
int64_t rh_wgrad2d_x6_workspace(const rh_conv2d_desc* d);
int rh_wgrad2d_x6_launch(const rh_conv2d_desc* d, const float* dy, const float* x, float* dw, void* ws, int64_t ws_bytes,
                         hipStream_t stream, bool* used, const unsigned* dy_range, const unsigned* x_range);
bool rh_wgrad2d_x6_plan_as_called(const rh_conv2d_desc* d, const float* dy, const float* x, const void* ws, int64_t ws_bytes,
                                  const unsigned* dy_range, const unsigned* x_range, long* out12);
// conv2d_smallm.hip: vector-ALU kernels for convolutions with <= 4 output rows (first-layer data gradient, scoring conv)
bool rh_conv2d_smallm_eligible(const rh_conv2d_desc* d, int which);
int rh_conv2d_smallm_launch(const rh_conv2d_desc* d, int which, const float* in, const float* wp, const float* bias, float* out,
                            hipStream_t stream);
void rh_conv2d_smallm_plan_info(const rh_conv2d_desc* d, int which, long* out12);

// conv2d_smallc.hip: vector-ALU forward for <= 4 input channels (the first conv of the spectral discriminators' stacks)
bool rh_conv2d_smallc_fwd_eligible(const rh_conv2d_desc* d);
int rh_conv2d_smallc_fwd_launch(const rh_conv2d_desc* d, const float* x, const float* wp_fwd, const float* bias, float* y,
                                hipStream_t stream);
void rh_conv2d_smallc_fwd_plan_info(const rh_conv2d_desc* d, long* out9);

namespace {

int validate2(const rh_conv2d_desc* d) {
    RH_REQUIRE(d, RH_ERR_INVALID, "conv2d: null descriptor");
    RH_REQUIRE(d->batch >= 0 && d->c_in > 0 && d->c_out > 0 && d->h_in > 0 && d->w_in > 0 && d->h_out > 0 &&
                   d->w_out > 0,
               RH_ERR_INVALID, "conv2d: bad sizes");
    RH_REQUIRE(d->kh >= 1 && d->kw >= 1 && d->sh >= 1 && d->sw >= 1 && d->dh >= 1 && d->dw >= 1 && d->ph >= 0 &&
                   d->pw >= 0,
               RH_ERR_INVALID, "conv2d: kernel/stride/dilation must be >= 1, padding >= 0");
    RH_REQUIRE(d->kh * d->kw <= kMaxTaps, RH_ERR_UNSUPPORTED, "conv2d: %d x %d taps > %d", d->kh, d->kw, kMaxTaps);
    RH_REQUIRE(d->sh * d->sw <= kPh2, RH_ERR_UNSUPPORTED, "conv2d: stride %d x %d > %d phases", d->sh, d->sw, kPh2);
    RH_REQUIRE(d->act == RH_ACT_NONE || d->act == RH_ACT_LEAKY, RH_ERR_UNSUPPORTED,
               "conv2d: output activation must be none or leaky");
    const int ho = (d->h_in + 2 * d->ph - d->dh * (d->kh - 1) - 1) / d->sh + 1;
    const int wo = (d->w_in + 2 * d->pw - d->dw * (d->kw - 1) - 1) / d->sw + 1;
    RH_REQUIRE(d->h_in + 2 * d->ph - d->dh * (d->kh - 1) - 1 >= 0 && d->w_in + 2 * d->pw - d->dw * (d->kw - 1) - 1 >= 0,
               RH_ERR_INVALID, "conv2d: kernel larger than the padded input");
    RH_REQUIRE(ho == d->h_out && wo == d->w_out, RH_ERR_INVALID, "conv2d: (h_out, w_out) = (%d, %d), geometry gives (%d, %d)",
               d->h_out, d->w_out, ho, wo);
    RH_REQUIRE((int64_t)d->h_in * d->w_in < (1ll << 30) && (int64_t)d->h_out * d->w_out < (1ll << 30), RH_ERR_UNSUPPORTED,
               "conv2d: plane too large");
    return RH_OK;
}

// which: 0 = forward operand, 1 = data-gradient operand
void build_plan2(const rh_conv2d_desc* d, int which, Plan2* pl) {
    Plan2& t = *pl;
    if (which == 0) {
        t.nphase = 1;
        t.oph_h[0] = t.oph_w[0] = 0;
        t.tap0[0] = 0;
        for (int th = 0; th < d->kh; ++th)
            for (int tw = 0; tw < d->kw; ++tw) {
                t.kk[t.nslots] = th * d->kw + tw;
                t.offh[t.nslots] = th * d->dh - d->ph;
                t.offw[t.nslots] = tw * d->dw - d->pw;
                ++t.nslots;
            }
        t.ntaps[0] = t.nslots;
    } else {
        for (int ah = 0; ah < d->sh; ++ah)
            for (int aw = 0; aw < d->sw; ++aw) {
                const int ph = t.nphase++;
                t.oph_h[ph] = ah;
                t.oph_w[ph] = aw;
                t.tap0[ph] = t.nslots;
                int n = 0;
                for (int th = 0; th < d->kh; ++th) {
                    const int nh = ah + d->ph - th * d->dh;
                    if (nh % d->sh != 0) continue;
                    for (int tw = 0; tw < d->kw; ++tw) {
                        const int nw = aw + d->pw - tw * d->dw;
                        if (nw % d->sw != 0) continue;
                        t.kk[t.nslots] = th * d->kw + tw;
                        t.offh[t.nslots] = nh / d->sh;
                        t.offw[t.nslots] = nw / d->sw;
                        ++t.nslots;
                        ++n;
                    }
                }
                t.ntaps[ph] = n;
            }
    }
    for (int ph = 0; ph < t.nphase; ++ph) {
        t.minh[ph] = t.maxh[ph] = t.minw[ph] = t.maxw[ph] = 0;
        for (int i = 0; i < t.ntaps[ph]; ++i) {
            const int oh = t.offh[t.tap0[ph] + i], ow = t.offw[t.tap0[ph] + i];
            if (i == 0 || oh < t.minh[ph]) t.minh[ph] = oh;
            if (i == 0 || oh > t.maxh[ph]) t.maxh[ph] = oh;
            if (i == 0 || ow < t.minw[ph]) t.minw[ph] = ow;
            if (i == 0 || ow > t.maxw[ph]) t.maxw[ph] = ow;
        }
    }
}

int fill_pack2(const rh_conv2d_desc* d, int which, const float* w, float* wp, PackP* p) {
    *p = PackP{};
    if (!wp) return RH_OK;
    Plan2 t;
    build_plan2(d, which, &t);
    p->w = w; p->scale = nullptr; p->wp = wp;
    p->C = which == 0 ? d->c_in : d->c_out;
    p->M = which == 0 ? d->c_out : d->c_in;
    p->Mp = round32(p->M);
    p->k = d->kh * d->kw;
    p->m_major = which == 0 ? 1 : 0;      // w[co][ci][kk]: forward m = co (m-major), data gradient m = ci (c-major)
    p->total = (long)t.nslots * p->C * p->Mp;
    p->nslots = t.nslots;
    for (int i = 0; i < t.nslots; ++i) p->kk[i] = t.kk[i];
    // bf16x6 section behind the f32 one (conv2d_x6.hip): fragments [phase][chunk][tap][g][piece][Mp] -- the mode-1 layout
    // of the 1-D packer with (kh, kw) taps as its taps
    long ph_ofs[kPh2];
    const long units = rh_conv2d_x6_units(p->C, p->M, t.nphase, t.ntaps, ph_ofs);
    if (units > 0 && units * 4 < 0x7fffffffl) {
        p->wq = reinterpret_cast<unsigned*>(wp + p->total);
        p->x6_mode = 1;
        p->range = p->wq + units * 4;          // {max |w|, max row sum |w|, 0, 0} behind the fragments (conv_host.hip)
        for (int ph = 0; ph < t.nphase; ++ph)
            for (int tl = 0; tl < t.ntaps[ph]; ++tl) {
                p->q2a[t.tap0[ph] + tl] = (int)(ph_ofs[ph] + (long)tl * 2 * kX6P * p->Mp);
                p->q2n[t.tap0[ph] + tl] = t.ntaps[ph] * 2 * kX6P * p->Mp;
            }
    }
    return RH_OK;
}

// Parameters of the bf16x6 launch (conv2d_x6.hip) from the tap plan; the tile plan is made there.
void fill_c2x(const Plan2& t, int C, int M, const float* wp, C2X* q) {
    *q = C2X{};
    q->C = C; q->M = M; q->Mp = round32(M);
    q->nphase = t.nphase;
    const long total = (long)t.nslots * C * q->Mp;
    const long units = rh_conv2d_x6_units(C, M, t.nphase, t.ntaps, q->ph_q2ofs);
    q->wq = (units > 0 && units * 4 < 0x7fffffffl) ? reinterpret_cast<const unsigned*>(wp + total) : nullptr;
    q->wq_bytes = (unsigned)(units * 16);
    for (int ph = 0; ph < t.nphase; ++ph) {
        q->ph_oph_h[ph] = t.oph_h[ph]; q->ph_oph_w[ph] = t.oph_w[ph];
        q->ph_ntaps[ph] = t.ntaps[ph]; q->ph_tap0[ph] = t.tap0[ph];
        q->ph_minh[ph] = t.minh[ph]; q->ph_minw[ph] = t.minw[ph];
        q->ph_maxh[ph] = t.maxh[ph]; q->ph_maxw[ph] = t.maxw[ph];
    }
    for (int i = 0; i < t.nslots; ++i) { q->offh[i] = t.offh[i]; q->offw[i] = t.offw[i]; }
}

}  // namespace

extern "C" int64_t rh_conv2d_packed_floats(const rh_conv2d_desc* d, int which) {
    if (validate2(d)) return -1;
    const int64_t M = which == 0 ? d->c_out : d->c_in;
    const int64_t C = which == 0 ? d->c_in : d->c_out;
    const int64_t base = (int64_t)d->kh * d->kw * C * round32((int)M);
    // + the bf16x6 fragments of the same weights (6 bytes per weight: conv2d_x6.hip), for channel counts in blocks of 16
    const int T = d->kh * d->kw;
    const long units = rh_conv2d_x6_units((int)C, (int)M, 1, &T, nullptr);
    return base + ((units > 0 && units * 4 < 0x7fffffffl) ? units * 4 + 4 : 0);      // (+ the range record)
}

// Diagnostics (tests): which kernel family a forward (which = 0) / data-gradient (1) launch of this geometry takes and, for
// the bf16x6 kernels, its tile plan.  out[16] = {family (0 = f32-input MFMA, 1 = bf16x6, 2 = vector ALU: conv2d_smallm.hip), tm, tn, tasks per thread, TR, TQ,
// nb, LDS bytes, workgroups, PH, PW, P, largest tap offset inside the patch, phases, row tiles, column tiles}.
extern "C" int rh_conv2d_plan_info(const rh_conv2d_desc* d, int32_t which, int64_t* out) {
    if (int e = validate2(d)) return e;
    RH_REQUIRE(out && (which == 0 || which == 1), RH_ERR_INVALID, "conv2d_plan_info: bad arguments");
    for (int i = 0; i < 16; ++i) out[i] = 0;
    rh_conv2d_desc dd = *d;
    if (which == 1) dd.act = RH_ACT_NONE;              // (the data gradient sees dy with act'(y) folded in)
    if (rh_conv2d_smallm_eligible(&dd, which) || (which == 0 && rh_conv2d_smallc_fwd_eligible(d))) { out[0] = 2; return RH_OK; }
    Plan2 t;
    build_plan2(d, which, &t);
    C2X q;
    static float dummy_w[4] __attribute__((aligned(16)));
    const int C = which == 0 ? d->c_in : d->c_out, M = which == 0 ? d->c_out : d->c_in;
    fill_c2x(t, C, M, dummy_w, &q);
    if (!q.wq) return RH_OK;
    q.wq = reinterpret_cast<const unsigned*>(dummy_w);      // (alignment test only: nothing is launched)
    q.in = dummy_w; q.out = dummy_w;
    q.B = d->batch;
    if (which == 0) {
        q.in_h = d->h_in; q.in_w = d->w_in; q.out_h = d->h_out; q.out_w = d->w_out; q.rows = d->h_out; q.qcols = d->w_out;
        q.is_h = d->sh; q.is_w = d->sw; q.os_h = 1; q.os_w = 1;
    } else {
        q.in_h = d->h_out; q.in_w = d->w_out; q.out_h = d->h_in; q.out_w = d->w_in;
        q.rows = rh_cdiv(d->h_in, d->sh); q.qcols = rh_cdiv(d->w_in, d->sw);
        q.is_h = 1; q.is_w = 1; q.os_h = d->sh; q.os_w = d->sw;
    }
    long v[8];
    if (!rh_conv2d_x6_plan_query(q, v)) return RH_OK;
    out[0] = 1;
    for (int i = 0; i < 8; ++i) out[1 + i] = v[i];
    // (the query works on a copy: redo the geometry-only part for the patch figures)
    const int span_h = patch_geom(t).span_h, span_w = patch_geom(t).span_w;     // (a phase without taps has span 0)
    const long TR = v[3], TQ = v[4], nb = v[5];
    const long PH = (TR - 1) * q.is_h + span_h + 1, PW = (TQ - 1) * q.is_w + span_w + 1;
    out[9] = PH; out[10] = PW; out[11] = nb * PH * PW;
    out[12] = (long)span_h * PW + span_w;
    out[13] = t.nphase;
    out[14] = rh_cdiv(q.rows, (int)TR); out[15] = rh_cdiv(q.qcols, (int)TQ);
    return RH_OK;
}

extern "C" int rh_conv2d_pack_f32(const rh_conv2d_desc* d, const float* w, float* wp_fwd, float* wp_bwd,
                                  rh_stream_t stream) {
    if (int e = validate2(d)) return e;
    RH_REQUIRE(w, RH_ERR_INVALID, "conv2d_pack: null weight");
    PackP a, b;
    if (int e = fill_pack2(d, 0, w, wp_fwd, &a)) return e;
    if (int e = fill_pack2(d, 1, w, wp_bwd, &b)) return e;
    // (rows = output channels = dim 0 of w, columns = c_in * kh * kw: the range records of both copies, then the pack)
    return rh_pack_launch(a, b, (hipStream_t)stream, "conv2d_pack", w, d->c_out, (long)d->c_in * d->kh * d->kw);
}

namespace {

constexpr int kInfo2 = 24;

// Parameter block of a forward (which = 0) / data-gradient (1) call for conv2d_x6_kernel (family 0 fills its own: conv2d_f32.hip)
void fill_conv2(const rh_conv2d_desc* d, int which, const Plan2& t, const float* in, const float* wp, const float* bias, float* out,
                const unsigned* in_range, unsigned* out_range, C2X* qq) {
    C2X& q = *qq;
    fill_c2x(t, which == 0 ? d->c_in : d->c_out, which == 0 ? d->c_out : d->c_in, wp, &q);
    q.in = in; q.out = out;
    q.B = d->batch;
    if (which == 0) {
        q.bias = bias;
        q.in_h = d->h_in; q.in_w = d->w_in; q.out_h = d->h_out; q.out_w = d->w_out;
        q.rows = d->h_out; q.qcols = d->w_out;
        q.is_h = d->sh; q.is_w = d->sw; q.os_h = 1; q.os_w = 1;
        q.out_act = d->act; q.out_slope = d->act_slope;
    } else {
        q.bias = nullptr;
        q.in_h = d->h_out; q.in_w = d->w_out; q.out_h = d->h_in; q.out_w = d->w_in;
        q.rows = rh_cdiv(d->h_in, d->sh); q.qcols = rh_cdiv(d->w_in, d->sw);
        q.is_h = 1; q.is_w = 1; q.os_h = d->sh; q.os_w = d->sw;
        q.out_act = RH_ACT_NONE; q.out_slope = 0.f;
    }
    q.in_range = in_range; q.out_range = out_range;
}

// The one place that decides which kernel a forward (which = 0) / data-gradient (1) call runs, in the order it tries them: the
// vector-ALU kernels, conv2d_x6_kernel, then family 0.  info == null: launch it (*x6 = conv2d_x6_kernel ran, which publishes the
// output's range itself); else fill info[kInfo2] as include/rave_hip.h documents and launch nothing.
int route_conv2(const rh_conv2d_desc* d, int which, const float* in, const float* y, const float* wp, const float* bias, float* out,
                const unsigned* in_range, unsigned* out_range, hipStream_t stream, bool* x6, int64_t* info) {
    *x6 = false;
    const char* what = which == 0 ? "conv2d_fwd" : "conv2d_bwd_data";
    Plan2 t;
    build_plan2(d, which, &t);
    C2X q;
    fill_conv2(d, which, t, in, wp, bias, out, in_range, out_range, &q);
    if (rh_conv2d_smallm_eligible(d, which)) {
        if (!info) return rh_conv2d_smallm_launch(d, which, in, wp, bias, out, stream);
        long v[12];
        rh_conv2d_smallm_plan_info(d, which, v);
        info[0] = K2_SMALLM; info[1] = v[0]; info[2] = v[1]; info[3] = v[2];
        info[5] = v[3]; info[6] = v[4]; info[7] = 1; info[8] = v[5]; info[9] = v[6]; info[10] = v[7]; info[11] = 1;
        info[12] = v[9]; info[13] = 1; info[14] = 1; info[15] = v[8]; info[16] = v[10]; info[17] = v[11]; info[18] = 2;
        return RH_OK;
    }
    if (which == 0 && rh_conv2d_smallc_fwd_eligible(d)) {
        if (!info) return rh_conv2d_smallc_fwd_launch(d, in, wp, bias, out, stream);
        long v[9];
        rh_conv2d_smallc_fwd_plan_info(d, v);
        info[0] = K2_SMALLC; info[1] = v[0];
        info[5] = v[1]; info[6] = v[2]; info[7] = 1; info[8] = v[3]; info[9] = v[4]; info[10] = d->c_in; info[11] = 1;
        info[12] = v[6]; info[13] = 1; info[14] = 1; info[15] = v[5]; info[16] = v[7]; info[17] = v[8]; info[18] = 2;
        return RH_OK;
    }
    // exact f32 on the bf16 matrix cores where the geometry allows (C in blocks of 16): conv2d_x6.hip.  A data gradient takes it
    // when the caller has folded act'(y) into dy (rave_amd.ops._Conv2dFn.backward).
    if ((which == 0 || d->act == RH_ACT_NONE) && q.wq) {
        if (!info) {
            if (int e = rh_conv2d_x6_launch(q, stream, which == 0 ? "conv2d_fwd_x6" : "conv2d_bwd_data_x6", x6)) return e;
            if (*x6) return RH_OK;
        } else {
            long v[15];
            if (rh_conv2d_x6_plan_as_called(q, v)) {
                info[0] = K2_X6; info[1] = v[0]; info[2] = v[1]; info[3] = v[2];
                info[5] = v[3]; info[6] = v[4]; info[7] = v[5]; info[8] = v[8]; info[9] = v[9]; info[10] = 16; info[11] = t.nphase;
                info[12] = v[10]; info[13] = v[11]; info[14] = v[12]; info[15] = v[6]; info[16] = v[13]; info[17] = v[14]; info[18] = 1;
                return RH_OK;
            }
        }
    }
    if (d->batch <= 0) return RH_OK;
    return rh_conv2d_f32_conv(d, which, t, in, y, wp, bias, out, stream, what, info);
}

// The one place that decides which kernel a weight-gradient call runs: wgrad2d_x6_kernel where the geometry, the range slots and the
// scratch offered allow, else family 0.  workspace: behind the bias scratch.  info as in route_conv2.
int route_wgrad2(const rh_conv2d_desc* d, const float* dy, const float* ymul, const float* x, float* dw, void* workspace,
                 int64_t workspace_bytes, const unsigned* dy_range, const unsigned* x_range, hipStream_t stream, int64_t* info) {
    if (d->act == RH_ACT_NONE) {      // (the caller has folded act'(y) into dy) -- bf16x6 kernel where the geometry allows
        if (!info) {
            bool used = false;
            if (int e = rh_wgrad2d_x6_launch(d, dy, x, dw, workspace, workspace_bytes, stream, &used, dy_range, x_range)) return e;
            if (used) return RH_OK;
        } else {
            long v[12];
            if (rh_wgrad2d_x6_plan_as_called(d, dy, x, workspace, workspace_bytes, dy_range, x_range, v)) {
                info[0] = K2_WX6; info[1] = v[0]; info[2] = v[1];
                info[5] = v[2]; info[6] = v[3]; info[7] = v[4]; info[8] = 0; info[9] = v[5];
                info[10] = d->c_in < 32 ? d->c_in : 32; info[11] = v[7]; info[12] = v[8]; info[14] = v[6]; info[15] = v[9]; info[16] = v[10];
                info[18] = 1;
                return RH_OK;
            }
        }
    }
    return rh_conv2d_f32_wgrad(d, dy, ymul, x, dw, workspace, workspace_bytes, stream, info);
}

}  // namespace

extern "C" int rh_conv2d_fwd_f32(const rh_conv2d_desc* d, const float* x, const float* wp_fwd, const float* bias,
                                 float* y, rh_stream_t stream) {
    const RhKernelEventsScope events;
    const unsigned* in_range = nullptr;
    unsigned* out_range = nullptr;
    rh_take_ranges(nullptr, &in_range, &out_range, nullptr);       // consumed by this call whatever happens below
    if (int e = validate2(d)) return e;
    if (d->batch == 0) return RH_OK;
    RH_REQUIRE(x && wp_fwd && y, RH_ERR_INVALID, "conv2d_fwd: null pointer");
    bool x6 = false;
    if (int e = route_conv2(d, 0, x, nullptr, wp_fwd, bias, y, in_range, out_range, (hipStream_t)stream, &x6, nullptr)) return e;
    // kernels other than conv2d_x6_kernel do not publish the output's range: a requested slot is filled by a pass over y
    if (x6 || !out_range) return RH_OK;
    return rh_amax_f32(y, (int64_t)d->batch * d->c_out * d->h_out * d->w_out, out_range, stream);
}

extern "C" int rh_conv2d_bwd_data_f32(const rh_conv2d_desc* d, const float* dy, const float* y, const float* wp_bwd,
                                      float* dx, rh_stream_t stream) {
    const RhKernelEventsScope events;
    const unsigned* in_range = nullptr;
    unsigned* out_range = nullptr;
    rh_take_ranges(nullptr, &in_range, &out_range, nullptr);
    if (int e = validate2(d)) return e;
    if (d->batch == 0) return RH_OK;
    RH_REQUIRE(dy && wp_bwd && dx, RH_ERR_INVALID, "conv2d_bwd_data: null pointer");
    RH_REQUIRE(d->act == RH_ACT_NONE || y, RH_ERR_INVALID, "conv2d_bwd_data: the output activation needs y");
    bool x6 = false;
    if (int e = route_conv2(d, 1, dy, y, wp_bwd, nullptr, dx, in_range, out_range, (hipStream_t)stream, &x6, nullptr)) return e;
    if (x6 || !out_range) return RH_OK;
    return rh_amax_f32(dx, (int64_t)d->batch * d->c_in * d->h_in * d->w_in, out_range, stream);
}

// 1 = the weight gradient of this geometry runs on the bf16 matrix cores (wgrad2d_x6.hip), 0 = f32-input MFMA kernels
extern "C" int rh_conv2d_bwd_weight_kernel_family(const rh_conv2d_desc* d) {
    if (validate2(d) || d->act != RH_ACT_NONE) return 0;
    return rh_wgrad2d_x6_workspace(d) >= 0 ? 1 : 0;
}

extern "C" int64_t rh_conv2d_workspace_bytes(const rh_conv2d_desc* d) {
    if (validate2(d)) return -1;
    if (d->batch == 0) return 0;
    int64_t best = rh_conv2d_f32_wgrad_workspace(d);
    const int64_t need_x6 = rh_wgrad2d_x6_workspace(d);
    if (need_x6 > best) best = need_x6;
    return best + rh_bias_grad_workspace(d->c_out);
}

extern "C" int rh_conv2d_bwd_weight_f32(const rh_conv2d_desc* d, const float* dy, const float* y, const float* x,
                                        float* dw, float* dbias, void* workspace, int64_t workspace_bytes,
                                        rh_stream_t stream_) {
    const RhKernelEventsScope events;
    const unsigned *dy_range = nullptr, *x_range = nullptr;
    rh_take_ranges(&dy_range, &x_range, nullptr, nullptr);
    if (int e = validate2(d)) return e;
    hipStream_t stream = (hipStream_t)stream_;
    RH_REQUIRE(dw && (d->batch == 0 || (dy && x)), RH_ERR_INVALID, "conv2d_bwd_weight: null pointer");
    RH_REQUIRE(d->act == RH_ACT_NONE || d->batch == 0 || y, RH_ERR_INVALID,
               "conv2d_bwd_weight: the output activation needs y");
    const long nw = (long)d->c_out * d->c_in * d->kh * d->kw;
    if (d->batch == 0) {
        if (hipError_t e = hipMemsetAsync(dw, 0, nw * sizeof(float), stream)) return (int)e;
        if (dbias)
            if (hipError_t e = hipMemsetAsync(dbias, 0, d->c_out * sizeof(float), stream)) return (int)e;
        return RH_OK;
    }
    const float* ymul = d->act == RH_ACT_NONE ? nullptr : y;
    const int64_t bias_ws = rh_bias_grad_workspace(d->c_out);
    if (dbias) {
        RH_REQUIRE(workspace && workspace_bytes >= bias_ws, RH_ERR_WORKSPACE,
                   "conv2d_bwd_weight: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)bias_ws);
        // the first c_out*64 floats of the workspace; the split-K partials follow
        if (int e = rh_bias_grad_launch(dy, ymul, (float*)workspace, dbias, d->batch, d->c_out,
                                        (long)d->h_out * d->w_out, d->act, d->act_slope, stream))
            return e;
    }
    workspace = workspace ? (void*)((char*)workspace + bias_ws) : nullptr;
    workspace_bytes = workspace_bytes > bias_ws ? workspace_bytes - bias_ws : 0;
    return route_wgrad2(d, dy, ymul, x, dw, workspace, workspace_bytes, dy_range, x_range, stream, nullptr);
}

extern "C" int rh_conv2d_instance_info(const rh_conv2d_desc* d, int32_t which, int32_t ranges_armed, int32_t data_aligned16,
                                       int32_t packed_aligned16, int64_t workspace_bytes, int64_t* out) {
    RH_REQUIRE(out && which >= 0 && which <= 2, RH_ERR_INVALID, "conv2d_instance_info: bad arguments");
    for (int i = 0; i < kInfo2; ++i) out[i] = 0;
    out[0] = -1;
    if (int e = validate2(d)) return e;
    if (d->batch == 0) return RH_OK;
    // stand-ins with the stated properties: nothing is launched and nothing dereferenced
    static const unsigned slot[kRangeSlotWords] = {};
    static float mem[64] __attribute__((aligned(64)));
    float* data = mem + (data_aligned16 ? 0 : 1);
    float* packed = mem + 16 + (packed_aligned16 ? 0 : 1);
    const unsigned* range = ranges_armed ? slot : nullptr;
    if (which < 2) {
        bool x6 = false;
        return route_conv2(d, which, data, data, packed, nullptr, data, range, nullptr, nullptr, &x6, out);
    }
    const int64_t bias_ws = rh_bias_grad_workspace(d->c_out);
    out[13] = bias_ws;
    void* ws = workspace_bytes > bias_ws ? (void*)mem : nullptr;
    return route_wgrad2(d, data, d->act == RH_ACT_NONE ? nullptr : data, data, data, ws, workspace_bytes > bias_ws ? workspace_bytes - bias_ws : 0,
                        range, range, nullptr, out);
}
