// The host side of the fused fp32 CNN kernels, behind all of them in the translation unit: one launch path per family.
//
//   descriptor net   k_cyl_net_wg | _w24k | _w25t (csrc/convnet_wg.hip, _w24k.hip, _w25t.hip) and their _rerun twins take the same
//                    arguments (CylWgParams): cyl_check states the rules of a stack once, cyl_prepare fills the parameters and picks
//                    the kernel (cyl_kernel_for), cyl_launch launches it -- the plain kernel, or with P.only_if its masked twin.
//   cost net         k_cost_net_w24b and its _rerun twin (csrc/costnet_body.hip) run every layer form: cost_net_prepare fills the
//                    parameters with the filter sets an entry point takes (none, three or five; the rest null), cost_net_launch
//                    launches, cost_net_run is what the six dense and gathered entry points share.
//
// Everything is checked before the first device call, and every message names the entry point it always named.  The split-safe entry
// points (csrc/split_safe.hip) prepare the same way and hand the prepared fp32 re-run to one body per family.
#include "common.h"

// ---- descriptor net ---------------------------------------------------------------------------------------------------------------
// relu_host[l] beside the ReLU bit: bit 1 (WG_F24_FLAG): the layer's filter buffer holds the F(2x4) set behind the F(2x2) set
// (128-output layers, csrc/convnet_w24.hip); bit 2 (BUF_CYL_F24K): likewise for the 64-output layers of Cin % 64 == 0, in the K-split
// form of csrc/convnet_w24k.hip or the pass-split form of csrc/convnet_w24p.hip as `form` says.
#define WG_F24_FLAG BUF_CYL_F24
#define BUF_CYL_FORM_LIBRARY BUF_CYL_FORM_PASS_SPLIT      // what BUF_CYL_FORM_DEFAULT means (profiles/f24p_ab.md)
static inline bool wg_f24_flagged(int relu) { return relu >= 2; }

// A kernel and its masked twin; the LDS grants are per kernel symbol
typedef void (*CylKernelFn)(const float*, CylWgParams, float*);
struct CylKernel { CylKernelFn plain, rerun; LdsGrant grant, grant_rerun; };
static CylKernel cyl_wg = { k_cyl_net_wg, k_cyl_net_wg_rerun }, cyl_w24k = { k_cyl_net_w24k, k_cyl_net_w24k_rerun },
                 cyl_w25t = { k_cyl_net_w25t, k_cyl_net_w25t_rerun };

// The kernel of a stack (rules checked).  An entry point that takes sets of the layers' own (sets: any of the three arrays) runs
// k_cyl_net_w25t, whatever the sets hold; else by the relu words -- none above 1: k_cyl_net_wg; bit 2 somewhere in the K-split form:
// k_cyl_net_w24k; everything else: k_cyl_net_w25t, whose body holds every other layer form.
static CylKernel& cyl_kernel_for(const int* relu, int form, bool sets)
{
    if (sets) return cyl_w25t;
    bool flagged = false, ksplit = false;
    for (int l = 0; l < WG_LAYERS; l++) {
        flagged |= wg_f24_flagged(relu[l]);
        ksplit |= (relu[l] & BUF_CYL_F24K) != 0;
    }
    if (!flagged) return cyl_wg;
    if (form == BUF_CYL_FORM_DEFAULT) form = BUF_CYL_FORM_LIBRARY;
    return ksplit && form == BUF_CYL_FORM_K_SPLIT ? cyl_w24k : cyl_w25t;
}

// The widths k_cyl_net_wg is built for, stated once: what buf_cylindrical_net_wg accepts and buf_cylindrical_net_wg_supports reports.
// follow: the rule that only 32-output layers follow a 32-output layer (stacks with sets of their own state it per layer form instead).
static int wg_check_widths(const int* cin, const int* cout, bool follow = true)
{
    for (int l = 0; l < WG_LAYERS; l++) {
        const int ci = cin[l], co = cout[l];
        BUF_REQUIRE(ci > 0 && ci % 16 == 0 && ci <= WG_MAXC && (co == 32 || co == 64 || co == 128), BUF_EINVAL,
                    "buf_cylindrical_net_wg: layer %d has unsupported widths %d -> %d", l, ci, co);
        BUF_REQUIRE(co != 128 || ci % 32 == 0, BUF_EINVAL,
                    "buf_cylindrical_net_wg: layer %d has unsupported widths %d -> %d (128 output channels need Cin %% 32 == 0)", l, ci, co);
        BUF_REQUIRE(co != 32 || (ci % 32 == 0 && ci <= 64), BUF_EINVAL,
                    "buf_cylindrical_net_wg: layer %d has unsupported widths %d -> %d (32 output channels need Cin = 32 or 64)", l, ci, co);
        BUF_REQUIRE(l == 0 || ci == cout[l - 1], BUF_EINVAL, "buf_cylindrical_net_wg: layer %d width mismatch", l);
        // The 32-output layers hand their K-split partial sums over through the rows of the channels 64..95, zero words included
        // (wg_layer_mksplit); those words are written once at kernel start, so no wider layer may follow.
        BUF_REQUIRE(!follow || l == 0 || cout[l - 1] != 32 || co == 32, BUF_EINVAL,
                    "buf_cylindrical_net_wg: layer %d has unsupported widths %d -> %d (only 32-output layers may follow a 32-output layer)", l, ci, co);
    }
    BUF_REQUIRE(cout[WG_LAYERS - 1] == 32, BUF_EINVAL, "buf_cylindrical_net_wg: the last layer must have 32 channels");
    return BUF_OK;
}

// The flag rules of a stack that carries bit 1 or bit 2 somewhere (widths already checked)
static int w24_check_flags(const int* cin, const int* cout, const int* relu)
{
    for (int l = 0; l < WG_LAYERS; l++) {
        BUF_REQUIRE(relu[l] >= 0 && relu[l] <= (BUF_CYL_F24K | WG_F24_FLAG | 1), BUF_EINVAL,
                    "buf_cylindrical_net_wg: layer %d has the relu word %d (bit 0: ReLU, bits 1 and 2: the F(2x4) flags, nothing above)", l, relu[l]);
        BUF_REQUIRE(!(relu[l] & BUF_CYL_F24K) || (cout[l] == 64 && cin[l] % 64 == 0), BUF_EINVAL,
                    "buf_cylindrical_net_wg: the K-split F(2x4) flag (bit 2) goes only on layers with 64 output channels and Cin %% 64 == 0 "
                    "(layer %d: %d -> %d, flags %d)", l, cin[l], cout[l], relu[l]);
        BUF_REQUIRE(((relu[l] & WG_F24_FLAG) != 0) == (cout[l] == 128), BUF_EINVAL,
                    "buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer %d: %d -> %d, flags %d)",
                    l, cin[l], cout[l], relu[l]);
    }
    return BUF_OK;
}

// The rules of a stack, stated once (host only).  wt24_host, wt25_host: the layers' own F(2x4) / F(2x5) sets (nullable per layer; only
// whether an entry is null is looked at), or null as a whole for an entry point that takes none.  `who` is named where a rule is about
// the sets; the width and flag rules name buf_cylindrical_net_wg, whoever asks.
//   without sets   the rules of buf_cylindrical_net_wg: its widths, and the flag rules once a word above 1 is there;
//   with sets      wt24_host[l] (buf_winograd_f24_tile_weights, a buffer of its own) goes on a layer that carries neither F(2x4) flag
//                  and has 64 or 32 output channels; wt25_host[l] (buf_winograd_f25_tile_weights) on a layer with 64 or 32 output
//                  channels and Cin % 16 == 0, whatever F(2x4) flag or set it carries (the F(2x5) set wins; the layer's other buffers
//                  are not read).  A 32-output layer with either set leaves the zero words alone: wider layers may follow it.
//                  taps_host[l] (buf_cyl_row6_tile_taps; entry points that take the array only) goes on a layer with 128 output channels.
static int cyl_check(const int* cin, const int* cout, const int* relu, const float* const* wt24_host, const float* const* wt25_host, const char* who,
                     const float* const* taps_host = nullptr)
{
    for (int l = 0; taps_host && l < WG_LAYERS; l++)
        BUF_REQUIRE(!taps_host[l] || cout[l] == 128, BUF_EINVAL, "%s: layer %d (%d -> %d) takes no row-6 tap set (128 output channels)", who, l,
                    cin[l], cout[l]);
    if (!wt24_host && !wt25_host) {
        if (int rc = wg_check_widths(cin, cout)) return rc;
        for (int l = 0; l < WG_LAYERS; l++)
            if (wg_f24_flagged(relu[l])) return w24_check_flags(cin, cout, relu);
        return BUF_OK;
    }
    for (int l = 0; wt25_host && l < WG_LAYERS; l++)
        BUF_REQUIRE(!wt25_host[l] || ((cout[l] == 64 || cout[l] == 32) && cin[l] > 0 && cin[l] % 16 == 0), BUF_EINVAL,
                    "%s: layer %d (%d -> %d) takes no F(2x5) set (64 or 32 output channels, Cin %% 16 == 0)", who, l, cin[l], cout[l]);
    if (int rc = wg_check_widths(cin, cout, false)) return rc;
    if (int rc = w24_check_flags(cin, cout, relu)) return rc;
    bool f22_ran = false;
    int f22_layer = -1;
    for (int l = 0; l < WG_LAYERS; l++) {
        const bool own24 = wt24_host && wt24_host[l], own25 = wt25_host && wt25_host[l];
        BUF_REQUIRE(!own24 || (!(relu[l] & (WG_F24_FLAG | W24K_FLAG)) && (cout[l] == 64 || cout[l] == 32)), BUF_EINVAL,
                    "%s: layer %d (%d -> %d, flags %d) takes no F(2x4) set of its own (64 or 32 output channels, no F(2x4) flag)",
                    who, l, cin[l], cout[l], relu[l]);
        // wg_layer_mksplit hands its partial sums over through the zero words of the channels 64..95, which are written once per kernel
        // (see wg_check_widths): once a 32-output layer WITHOUT a set has run, only 32-output layers may follow, to the end of the stack
        BUF_REQUIRE(!f22_ran || cout[l] == 32, BUF_EINVAL,
                    "%s: layer %d has unsupported widths %d -> %d (once a 32-output layer in the F(2x2) form has run, layer %d here, "
                    "only 32-output layers may follow)", who, l, cin[l], cout[l], f22_layer);
        if (cout[l] == 32 && !own24 && !own25 && !f22_ran) { f22_ran = true; f22_layer = l; }
    }
    return BUF_OK;
}

// 0 when the Winograd fp32 kernel is built for this stack of widths (what buf_cylindrical_net_wg would accept), else BUF_EINVAL with the reason
extern "C" int buf_cylindrical_net_wg_supports(const int* cin_host, const int* cout_host)
{
    BUF_REQUIRE(cin_host && cout_host, BUF_EINVAL, "buf_cylindrical_net_wg_supports: null argument");
    return wg_check_widths(cin_host, cout_host);
}

// 0 when buf_cylindrical_net_wg / _wg_all / _w25 would accept these widths with these relu words and sets (host only, no device call),
// else BUF_EINVAL with the reason
extern "C" int buf_cylindrical_net_wg_flags(const int* cin_host, const int* cout_host, const int* relu_host)
{
    BUF_REQUIRE(cin_host && cout_host && relu_host, BUF_EINVAL, "buf_cylindrical_net_wg_flags: null argument");
    return cyl_check(cin_host, cout_host, relu_host, nullptr, nullptr, "buf_cylindrical_net_wg");
}

extern "C" int buf_cylindrical_net_wg_all_flags(const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host)
{
    BUF_REQUIRE(cin_host && cout_host && relu_host && wt24_host, BUF_EINVAL, "buf_cylindrical_net_wg_all_flags: null argument");
    return cyl_check(cin_host, cout_host, relu_host, wt24_host, nullptr, "buf_cylindrical_net_wg_all");
}

extern "C" int buf_cylindrical_net_w25_flags(const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host,
                                             const float* const* wt25_host)
{
    BUF_REQUIRE(cin_host && cout_host && relu_host && wt24_host && wt25_host, BUF_EINVAL, "buf_cylindrical_net_w25_flags: null argument");
    return cyl_check(cin_host, cout_host, relu_host, wt24_host, wt25_host, "buf_cylindrical_net_w25");
}

// Everything an entry point checks about its stack, the kernel's parameters and the kernel, without a device call.  The set arrays as
// for cyl_check: an entry point that takes one has checked that it is there.  taps_host, order: of buf_cylindrical_net_w25t and its twin.
static int cyl_prepare(const float* const* wt_host, const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                       const float* const* wt24_host, const float* const* wt25_host, int form, const char* who, CylWgParams& P, CylKernel*& K,
                       const float* const* taps_host = nullptr, int order = 0)
{
    BUF_REQUIRE(wt_host && bias_host && cin_host && cout_host && relu_host, BUF_EINVAL, "%s: null argument", who);
    for (int l = 0; l < WG_LAYERS; l++) {
        P.wt[l] = wt_host[l]; P.bias[l] = bias_host[l];
        P.cin[l] = cin_host[l]; P.cout[l] = cout_host[l]; P.relu[l] = relu_host[l];
        P.taps[l] = nullptr;
        BUF_REQUIRE(P.wt[l] && P.bias[l], BUF_EINVAL, "%s: null weights for layer %d", who, l);
    }
    if (int rc = cyl_check(P.cin, P.cout, P.relu, wt24_host, wt25_host, who, taps_host)) return rc;
    P.only_if = nullptr;
    K = &cyl_kernel_for(P.relu, form, wt24_host || wt25_host || taps_host);
    if (K == &cyl_wg) return BUF_OK;                      // takes the buffers and the words as they are
    for (int l = 0; l < WG_LAYERS; l++) {
        if (wt25_host && wt25_host[l]) { P.wt[l] = wt25_host[l]; P.relu[l] = (P.relu[l] & 1) | W25_FLAG; }
        else if (P.relu[l] & WG_F24_FLAG) P.wt[l] += W24_SET_F22(P.cin[l]);
        else if (P.relu[l] & W24K_FLAG) P.wt[l] += WG_BLOCKS * P.cout[l] * P.cin[l];       // behind the layer's F(2x2) set
        else if (wt24_host && wt24_host[l]) { P.wt[l] = wt24_host[l]; P.relu[l] |= W24K_FLAG; }
        P.relu[l] &= ~WG_F24_FLAG;
        if (taps_host && P.cout[l] == 128) {              // (the row-6 words: csrc/convnet_w25t.hip)
            if (taps_host[l]) { P.taps[l] = taps_host[l]; P.relu[l] |= W25T_TAPS; }
            if (order & BUF_CYL_ROW6_FIRST) P.relu[l] |= W25T_FIRST;
        }
    }
    return BUF_OK;
}

#ifdef WG_STAMP
// per-layer wave cycles of k_cyl_net_wg (to the wave's arrival at the closing barrier | wait there), second half of the workgroups
static int wg_stamp_report(const CylWgParams& P, int npatch, void* stream)
{
    BUF_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    long long* h = (long long*)malloc((size_t)npatch * (4 * 20 + 4) * sizeof(long long));
    BUF_CHECK_HIP(hipMemcpy(h, P.stamps, (size_t)npatch * (4 * 20 + 4) * sizeof(long long), hipMemcpyDeviceToHost));
    double comp[WG_LAYERS][4] = {}, wait[WG_LAYERS][4] = {}, tot = 0, pre = 0; long n = 0;
    for (int b = npatch / 2; b < npatch; b++, n++)
        for (int w = 0; w < 4; w++) {
            const long long* q = h + ((size_t)b * 4 + w) * 20;
            for (int l = 0; l < WG_LAYERS; l++) { comp[l][w] += (double)(q[2 * l + 1] - q[2 * l]); wait[l][w] += (double)(q[2 * l + 2] - q[2 * l + 1]); }
            if (w == 0) { tot += (double)(q[2 * WG_LAYERS] - q[0]); pre += (double)(q[0] - q[17]); }
        }
    if (n && npatch >= 1024) {
        double dc = 0, dr = 0;
        for (int b = npatch / 2; b < npatch; b++) { const long long* q = h + (size_t)npatch * 80 + (size_t)b * 4; dc += (double)(q[2] - q[0]); dr += (double)(q[3] - q[1]); }
        fprintf(stderr, "  WG_STAMP in-kernel clock: %.0f shader cycles per workgroup over %.0f ticks of the 100 MHz counter -> %.3f GHz\n", dc / n, dr / n, dc / dr * 0.1);
        fprintf(stderr, "WG_STAMP: %ld workgroups, layers total %.0f cycles per patch, input phase %.0f\n", n, tot / n, pre / n);
        for (int l = 0; l < WG_LAYERS; l++) {
            const double mf = 38.0 * (P.cin[l] / 4) * (P.cout[l] / 16) / 4;     // MFMAs per wave
            fprintf(stderr, "  layer %d %3d->%3d: MFMAs/wave %5.0f | to barrier %7.0f %7.0f %7.0f %7.0f | wait %6.0f %6.0f %6.0f %6.0f | cycles per MFMA slot %.1f\n",
                    l, P.cin[l], P.cout[l], mf, comp[l][0] / n, comp[l][1] / n, comp[l][2] / n, comp[l][3] / n, wait[l][0] / n, wait[l][1] / n,
                    wait[l][2] / n, wait[l][3] / n, (comp[l][0] + wait[l][0]) / n / (2 * mf));
        }
    }
    free(h); (void)hipFree(P.stamps);
    return BUF_OK;
}
#endif

// x f32[np,Cin0,140] -> y f32[np,32,140] through kernel K with the prepared P; P.only_if (DEVICE int32[np]): the masked twin instead,
// whose workgroups return at once where the word is 0.
static int cyl_launch(CylKernel& K, const float* x, int npatch, CylWgParams P, float* y, void* stream)
{
    const size_t lds = sizeof(float) * WG_BUF;
    if (int rc = P.only_if ? grant_dynamic_lds((const void*)K.rerun, lds, K.grant_rerun) : grant_dynamic_lds((const void*)K.plain, lds, K.grant)) return rc;
    double macs = 0;
    for (int l = 0; l < WG_LAYERS; l++) macs += 9.0 * P.cin[l] * P.cout[l];
    TimedSpan span;
    bool timed = !P.only_if && timing_begin((hipStream_t)stream, &span, 2.0 * 140 * macs * npatch, BUF_TIMED_CYL_NET);   // (a masked re-run is not a full launch)
#ifdef WG_STAMP
    if (&K == &cyl_wg) BUF_CHECK_HIP(hipMalloc(&P.stamps, (size_t)npatch * (4 * 20 + 4) * sizeof(long long)));
#endif
    const CylKernelFn kernel = P.only_if ? K.rerun : K.plain;
    kernel<<<npatch, WG_THREADS, lds, (hipStream_t)stream>>>(x, P, y);
    if (timed) timing_end((hipStream_t)stream, &span);
    BUF_LAUNCH_CHECK();
#ifdef WG_STAMP
    if (&K == &cyl_wg) return wg_stamp_report(P, npatch, stream);
#endif
    return BUF_OK;
}

// x f32[np,48,140] -> y f32[np,32,140]; weights in the Winograd-domain tiling (see CylWgParams), the layers whose relu word carries
// bit 1 or 2 with their F(2x4) set behind it.  form: BUF_CYL_FORM_* of the layers that carry bit 2.
extern "C" int buf_cylindrical_net_wg_form(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                                           const int* cin_host, const int* cout_host, const int* relu_host, int form, float* y, void* stream)
{
    BUF_REQUIRE(npatch >= 0, BUF_EINVAL, "buf_cylindrical_net_wg: npatch=%d", npatch);
    BUF_REQUIRE(form >= BUF_CYL_FORM_DEFAULT && form <= BUF_CYL_FORM_PASS_SPLIT, BUF_EINVAL,
                "buf_cylindrical_net_wg: form=%d (-1: the library's default, 0: K split, 1: pass split)", form);
    if (npatch == 0) return BUF_OK;
    BUF_REQUIRE(x && y, BUF_EINVAL, "buf_cylindrical_net_wg: null argument");
    CylWgParams P;
    CylKernel* K;
    if (int rc = cyl_prepare(wt_host, bias_host, cin_host, cout_host, relu_host, nullptr, nullptr, form, "buf_cylindrical_net_wg", P, K)) return rc;
    return cyl_launch(*K, x, npatch, P, y, stream);
}

extern "C" int buf_cylindrical_net_wg(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                                      const int* cin_host, const int* cout_host, const int* relu_host, float* y, void* stream)
{
    return buf_cylindrical_net_wg_form(x, npatch, wt_host, bias_host, cin_host, cout_host, relu_host, BUF_CYL_FORM_DEFAULT, y, stream);
}

// The same with sets of the layers' own: wt24_host (per layer an optional F(2x4) set), w25: wt25_host (per layer an optional F(2x5)
// set), w25t: taps_host (per layer an optional row-6 tap set) and order.  All of them run k_cyl_net_w25t.
static int cyl_net_own_sets(const char* who, const float* x, int npatch, const float* const* wt_host, const float* const* bias_host, const int* cin_host,
                            const int* cout_host, const int* relu_host, const float* const* wt24_host, const float* const* wt25_host, bool w25, float* y,
                            void* stream, bool w25t = false, const float* const* taps_host = nullptr, int order = 0)
{
    BUF_REQUIRE(npatch >= 0, BUF_EINVAL, "%s: npatch=%d", who, npatch);
    BUF_REQUIRE(!w25t || (order & ~BUF_CYL_ROW6_FIRST) == 0, BUF_EINVAL, "%s: order=%d (0, or BUF_CYL_ROW6_FIRST = 1)", who, order);
    if (npatch == 0) return BUF_OK;
    BUF_REQUIRE(x && y && wt24_host && (wt25_host || !w25) && (taps_host || !w25t), BUF_EINVAL, "%s: null argument", who);
    CylWgParams P;
    CylKernel* K;
    if (int rc = cyl_prepare(wt_host, bias_host, cin_host, cout_host, relu_host, wt24_host, wt25_host, BUF_CYL_FORM_DEFAULT, who, P, K, taps_host, order)) return rc;
    return cyl_launch(*K, x, npatch, P, y, stream);
}

// x f32[np,Cin0,140] -> y f32[np,32,140]: buf_cylindrical_net_wg with, per layer, an optional F(2x4) set of its own
extern "C" int buf_cylindrical_net_wg_all(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host, const int* cin_host,
                                          const int* cout_host, const int* relu_host, const float* const* wt24_host, float* y, void* stream)
{
    return cyl_net_own_sets("buf_cylindrical_net_wg_all", x, npatch, wt_host, bias_host, cin_host, cout_host, relu_host, wt24_host, nullptr, false, y, stream);
}

// x f32[np,Cin0,140] -> y f32[np,32,140]: buf_cylindrical_net_wg_all with, per layer, an optional F(2x5) set
extern "C" int buf_cylindrical_net_w25(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host, const int* cin_host,
                                       const int* cout_host, const int* relu_host, const float* const* wt24_host, const float* const* wt25_host, float* y,
                                       void* stream)
{
    return cyl_net_own_sets("buf_cylindrical_net_w25", x, npatch, wt_host, bias_host, cin_host, cout_host, relu_host, wt24_host, wt25_host, true, y, stream);
}

// x f32[np,Cin0,140] -> y f32[np,32,140]: buf_cylindrical_net_w25 with, per 128-output layer, an optional row-6 tap
// set, and the order of the two rounds there
extern "C" int buf_cylindrical_net_w25t(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host, const int* cin_host,
                                        const int* cout_host, const int* relu_host, const float* const* wt24_host, const float* const* wt25_host,
                                        const float* const* taps_host, int order, float* y, void* stream)
{
    return cyl_net_own_sets("buf_cylindrical_net_w25t", x, npatch, wt_host, bias_host, cin_host, cout_host, relu_host, wt24_host, wt25_host, true, y, stream,
                            true, taps_host, order);
}

// ---- cost net ---------------------------------------------------------------------------------------------------------------------
// The kernel and its masked twin; the LDS grants are per kernel symbol
struct CostKernel { void (*plain)(const float*, const float*, CostNetParams, float*); void (*rerun)(const float*, const float*, CostNetParams, float*); LdsGrant grant, grant_rerun; };
static CostKernel cost_kernel = { k_cost_net_w24b, k_cost_net_w24b_rerun };

// The kernel parameters of a launch.  f24_host: the first nsets (0, 3 or 5: what the entry point takes) filter sets of CostNetParams::f24,
// DEVICE pointers with nullable entries; the sets behind them are null, and a layer without a set runs its first form.  only_if: the
// masked twin's flags.
static int cost_net_prepare(CostNetParams& P, const float* const* wt_host, const float* const* bias_host, const float* const* f24_host, int nsets,
                            const long long* s_rows, const long long* t_rows, int ele_n, const int* only_if, const char* who)
{
    for (int l = 0; l < CV_LAYERS; l++) {
        P.wt[l] = wt_host[l]; P.bias[l] = bias_host[l];
        BUF_REQUIRE(P.wt[l] && P.bias[l], BUF_EINVAL, "%s: null weights for layer %d", who, l);
    }
    P.s_rows = s_rows; P.t_rows = t_rows;
    P.chan_floats = s_rows ? ele_n * 20 : 100;
    P.row_floats = 32 * P.chan_floats;
    P.skip_floats = s_rows ? 20 : 0;                         // elevation row 0 of every channel is not part of the cost volume
    P.only_if = only_if;
    for (int i = 0; i < 5; i++) P.f24[i] = i < nsets ? f24_host[i] : nullptr;
    return BUF_OK;
}

// EXECUTED flops per match of the net with every layer in its first form: layer 0 in its separated form (S-term 60 x 480 x 32,
// T-term 54 x 288 x 32 MAC instead of the dense 972 x 864 x 32), then the valid convolutions 18x3x18 -> 16x1x16 -> 14 -> 12 -> 10 -> 8 -> 6 -> 4 -> 2 -> 1:
// 2 * sum(out positions * K * Cout), layers 1..5 with 16 products per 2 x 2 output tile (Winograd) = 0.0519 GFLOP.  The dense algorithmic count of SURVEY 8d is 0.160 GFLOP/match
// (bench.py reports both; the roofline fraction is taken on the executed count).
static const double cost_net_macs_per_match =
    60.0 * 480 * 32 + 54.0 * 288 * 32 + 16.0 * 64 * 96 * 64 +
    16.0 * (49.0 * 64 * 64 + 36.0 * 64 * 128 + 25.0 * 128 * 128 + 16.0 * 128 * 64) +        // layers 2..5: 16 components per 2 x 2 tile
    36.0 * 576 * 64 + 16.0 * 576 * 32 + 4.0 * 288 * 32 + 1.0 * 128 * 20;

#ifdef CV_STAMP
static int cv_stamp_begin(int m, long long** stamps)
{
    BUF_CHECK_HIP(hipMalloc(stamps, (size_t)m * 16 * sizeof(long long)));
    BUF_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(cv_stamp_ptr), stamps, sizeof(*stamps)));
    return BUF_OK;
}
static int cv_stamp_end(int m, long long* stamps, void* stream)
{
    if (m >= 2048) {
        BUF_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        long long* h = (long long*)malloc((size_t)m * 16 * sizeof(long long));
        BUF_CHECK_HIP(hipMemcpy(h, stamps, (size_t)m * 16 * sizeof(long long), hipMemcpyDeviceToHost));
        static const char* name[8] = { "A.1 (layer 0 maps)", "A.2 (layer 1)", "layer 2", "layer 3", "layer 4", "layer 5", "layer 6", "layers 7-9" };
        double d[8] = {};
        for (int b = m / 2; b < m; b++)
            for (int i = 0; i < 8; i++) d[i] += (double)(h[(size_t)b * 16 + i + 1] - h[(size_t)b * 16 + i]);
        for (int i = 0; i < 8; i++) fprintf(stderr, "  CV_STAMP k_cost_net_w24b %-20s %8.0f cycles per match\n", name[i], d[i] / (m - m / 2));
        free(h);
    }
    (void)hipFree(stamps);
    return BUF_OK;
}
#endif

// m matches through the kernel with the prepared P; with only_if in it the masked twin instead
static int cost_net_launch(const float* s_eq, const float* t_eq, int m, const CostNetParams& P, float* ind_out, void* stream)
{
    const bool rerun = P.only_if != nullptr;
    size_t lds = sizeof(float) * CV_BUF;
    if (int rc = rerun ? grant_dynamic_lds((const void*)cost_kernel.rerun, lds, cost_kernel.grant_rerun) : grant_dynamic_lds((const void*)cost_kernel.plain, lds, cost_kernel.grant)) return rc;
    // whatever forms the layers take, the span keeps the first forms' figure (16 products per 2 x 2 tile in layers 1..5, layer 6 direct):
    // bench.py counts the matches of a launch by it (a masked re-run is not a full launch)
    TimedSpan span;
    bool timed = !rerun && timing_begin((hipStream_t)stream, &span, 2.0 * cost_net_macs_per_match * m, BUF_TIMED_COST_NET);
#ifdef CV_STAMP
    long long* stamps = nullptr;
    if (int rc = cv_stamp_begin(m, &stamps)) return rc;
#endif
    const auto kernel = rerun ? cost_kernel.rerun : cost_kernel.plain;
    kernel<<<m, CV_THREADS, lds, (hipStream_t)stream>>>(s_eq, t_eq, P, ind_out);
    if (timed) timing_end((hipStream_t)stream, &span);
    BUF_LAUNCH_CHECK();
#ifdef CV_STAMP
    if (int rc = cv_stamp_end(m, stamps, stream)) return rc;
#endif
    return BUF_OK;
}

// What the dense and the gathered entry points share.  Dense (s_rows, t_rows null): s_eq, t_eq f32[m,32,5,20]; gathered: s_eq = t_eq =
// equi f32[rows,32,ele_n,20] with int64 row ids on the device.  nsets: the filter sets the entry point takes; those that take any need f24_host.
static int cost_net_run(const char* who, int nsets, bool gathered, const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows,
                        const long long* t_rows, int m, const float* const* wt_host, const float* const* bias_host, const float* const* f24_host,
                        float* ind_out, void* stream)
{
    if (gathered) BUF_REQUIRE(m >= 0 && ele_n == 7, BUF_EINVAL, "%s: m=%d ele_n=%d (the kernel is built for ele_n = 7)", who, m, ele_n);
    else BUF_REQUIRE(m >= 0, BUF_EINVAL, "%s: m=%d", who, m);
    if (m == 0) return BUF_OK;
    BUF_REQUIRE(s_eq && t_eq && (!gathered || (s_rows && t_rows)) && wt_host && bias_host && (f24_host || nsets == 0) && ind_out,
                BUF_EINVAL, "%s: null argument", who);
    CostNetParams P;
    if (int rc = cost_net_prepare(P, wt_host, bias_host, f24_host, nsets, s_rows, t_rows, ele_n, nullptr, who)) return rc;
    return cost_net_launch(s_eq, t_eq, m, P, ind_out, stream);
}

// s_eq, t_eq f32[m,32,5,20] (elevation rows 1..5 of the equivariant maps) -> ind f32[m]
extern "C" int buf_cost_volume_net(const float* s_eq, const float* t_eq, int m, const float* const* wt_host,
                                   const float* const* bias_host, float* ind_out, void* stream)
{
    return cost_net_run("buf_cost_volume_net", 0, false, s_eq, t_eq, 7, nullptr, nullptr, m, wt_host, bias_host, nullptr, ind_out, stream);
}

// The same with the gather fused in: equi f32[rows,32,ele_n,20] holds the FULL equivariant maps of all keypoints, match i pairs
// row s_rows[i] with row t_rows[i] (int64, device) and the kernel reads elevation rows 1..5 of each (ele_n = 7) directly.
extern "C" int buf_cost_volume_net_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                          const float* const* wt_host, const float* const* bias_host, float* ind_out, void* stream)
{
    return cost_net_run("buf_cost_volume_net_gather", 0, true, equi, equi, ele_n, s_rows, t_rows, m, wt_host, bias_host, nullptr, ind_out, stream);
}

// buf_cost_volume_net with f24_host[3] (nullable entries, DEVICE pointers): the F(2x4) sets of layers 2 and 4 (buf_winograd_f24_tile_weights
// of the [Cout][Cin][3][3] filters) and the F(2x2) set of layer 6 (buf_winograd_tile_filters, group 1).  A layer without a set runs its
// F(2x2) form (layer 6: the direct form) from wt_host, as in buf_cost_volume_net.
extern "C" int buf_cost_volume_net_w24(const float* s_eq, const float* t_eq, int m, const float* const* wt_host, const float* const* bias_host,
                                       const float* const* f24_host, float* ind_out, void* stream)
{
    return cost_net_run("buf_cost_volume_net_w24", 3, false, s_eq, t_eq, 7, nullptr, nullptr, m, wt_host, bias_host, f24_host, ind_out, stream);
}

extern "C" int buf_cost_volume_net_w24_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                              const float* const* wt_host, const float* const* bias_host, const float* const* f24_host,
                                              float* ind_out, void* stream)
{
    return cost_net_run("buf_cost_volume_net_w24_gather", 3, true, equi, equi, ele_n, s_rows, t_rows, m, wt_host, bias_host, f24_host, ind_out, stream);
}

// buf_cost_volume_net_w24 with f24_host[5] (nullable entries, DEVICE pointers): the three sets of that entry point, then the F(2x4) sets
// (buf_winograd_f24_tile_weights) of layer 1's collapsed filter [64][96 = (dk, c)][dn][dl] and of layer 3's [128][64][3][3].  A layer
// without a set runs its F(2x2) form from wt_host.
extern "C" int buf_cost_volume_net_w24b(const float* s_eq, const float* t_eq, int m, const float* const* wt_host, const float* const* bias_host,
                                        const float* const* f24_host, float* ind_out, void* stream)
{
    return cost_net_run("buf_cost_volume_net_w24b", 5, false, s_eq, t_eq, 7, nullptr, nullptr, m, wt_host, bias_host, f24_host, ind_out, stream);
}

extern "C" int buf_cost_volume_net_w24b_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                               const float* const* wt_host, const float* const* bias_host, const float* const* f24_host,
                                               float* ind_out, void* stream)
{
    return cost_net_run("buf_cost_volume_net_w24b_gather", 5, true, equi, equi, ele_n, s_rows, t_rows, m, wt_host, bias_host, f24_host, ind_out, stream);
}
