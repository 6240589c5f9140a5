// The split-f16 CNN kernels, safe by construction (round 6).
//
// The split form (csrc/convnet_h3.hip, csrc/costnet_h3.hip) carries every fp32 operand as hi + 2^-11 lo' in two f16 numbers: it needs
// every input and every hidden activation below the f16 range (|v| < 65504).  Rounds 4-5 raised an error AFTER the step when the range
// watch tripped.  Here the decision is made on the device, per patch / per match, in the same stream, without a host round trip:
//   1. the flags (int32 per patch) are cleared, the split kernel runs and sets flags[p] = 1 for every patch whose input or hidden
//      activation left the range (a NaN counts: the watch compares bit patterns / uses !(a < limit));
//   2. the fp32 kernel (csrc/convnet_wg.hip, csrc/costnet_body.hip) is launched over the same grid with only_if = flags: a workgroup whose
//      flag is clear returns at once, a flagged one recomputes its patch with the fp32 kernel's arithmetic and overwrites the result.
// The outputs are therefore those of the split kernel where it is valid and, bit for bit, those of the fp32 kernel elsewhere; nothing
// is ever returned from behind an overflow.  Cost when nothing trips (the normal case): one memset and np workgroups that exit on
// their first instruction (measured: tools/split_safe_probe.py).  status_dev (nullable) keeps its meaning (bit 0: some launch tripped).
#include "common.h"


// The descriptor net's body: K and P are the fp32 re-run as cyl_prepare (csrc/cnn_launch.hip) left it, so every rule of the stack has
// been checked before the first device call here.  x f32[np,Cin0,140] -> without head: y_or_equi = y f32[np,32,140]; with head_params
// (DEVICE f32[545], buf_descriptor_head): desc f32[np,32] and y_or_equi = equi f32[np,32,140].  wt_split_host: the filters in the split
// kernel's tiling (buf_split_tile_filters), bias_host shared.  flags_ws: DEVICE int32[np] (scratch; after the call flags_ws[p] != 0
// marks the patches that took the fp32 kernel).
static int cyl_split_safe(const float* x, int npatch, const void* const* wt_split_host, const float* const* bias_host, const int* cin_host,
                          const int* cout_host, const int* relu_host, CylKernel& K, CylWgParams P, const float* head_params, float* y_or_equi,
                          float* desc, int* status_dev, int* flags_ws, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_CHECK_HIP(hipMemsetAsync(flags_ws, 0, sizeof(int) * (size_t)npatch, s));
    // the split kernel knows 0 / 1 only: without the fp32 kernel's F(2x4) flags.  (A stack with sets of its own has passed
    // w24_check_flags: its words are 0..7, and this is relu_host[l] & 1 for them.)
    int relu_split[WG_LAYERS];
    for (int l = 0; l < WG_LAYERS; l++) relu_split[l] = wg_f24_flagged(relu_host[l]) ? (relu_host[l] & 1) : relu_host[l];
    int rc = h3_launch(x, npatch, wt_split_host, bias_host, cin_host, cout_host, relu_split, head_params ? nullptr : y_or_equi, head_params,
                       desc, head_params ? y_or_equi : nullptr, status_dev, stream, flags_ws);
    if (rc) return rc;
    P.only_if = flags_ws;
    rc = cyl_launch(K, x, npatch, P, y_or_equi, stream);
    if (rc) return rc;
    if (head_params) {
        k_desc_head_masked<<<npatch, DH_THREADS, 0, s>>>(y_or_equi, head_params, desc, y_or_equi, flags_ws);
        BUF_LAUNCH_CHECK();
    }
    return BUF_OK;
}

// wt_wg_host: the filters in the fp32 kernel's tiling (buf_winograd_tile_weights; relu_host may carry the fp32 kernel's F(2x4) flags).
// form: BUF_CYL_FORM_* of the fp32 re-run, as for buf_cylindrical_net_wg_form.
extern "C" int buf_cylindrical_net_split_safe_form(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                                   const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                                   int form, const float* head_params, float* y_or_equi, float* desc, int* status_dev,
                                                   int* flags_ws, void* stream)
{
    BUF_REQUIRE(npatch >= 0, BUF_EINVAL, "buf_cylindrical_net_split_safe: npatch=%d", npatch);
    if (npatch == 0) return BUF_OK;
    BUF_REQUIRE(x && y_or_equi && flags_ws && wt_split_host && wt_wg_host && bias_host && cin_host && cout_host && relu_host, BUF_EINVAL,
                "buf_cylindrical_net_split_safe: null argument");
    BUF_REQUIRE(!head_params || desc, BUF_EINVAL, "buf_cylindrical_net_split_safe: head without desc");
    BUF_REQUIRE(form >= BUF_CYL_FORM_DEFAULT && form <= BUF_CYL_FORM_PASS_SPLIT, BUF_EINVAL,
                "buf_cylindrical_net_split_safe: form=%d (-1: the library's default, 0: K split, 1: pass split)", form);
    if (int rc = buf_cylindrical_net_wg_flags(cin_host, cout_host, relu_host)) return rc;       // the re-run must exist for these widths and take these relu words: stated before its weights are looked at
    CylWgParams P;
    CylKernel* K;
    if (int rc = cyl_prepare(wt_wg_host, bias_host, cin_host, cout_host, relu_host, nullptr, nullptr, form, "buf_cylindrical_net_wg", P, K)) return rc;
    return cyl_split_safe(x, npatch, wt_split_host, bias_host, cin_host, cout_host, relu_host, *K, P, head_params, y_or_equi, desc, status_dev, flags_ws, stream);
}

extern "C" int buf_cylindrical_net_split_safe(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                              const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                              const float* head_params, float* y_or_equi, float* desc, int* status_dev, int* flags_ws,
                                              void* stream)
{
    return buf_cylindrical_net_split_safe_form(x, npatch, wt_split_host, wt_wg_host, bias_host, cin_host, cout_host, relu_host, BUF_CYL_FORM_DEFAULT,
                                               head_params, y_or_equi, desc, status_dev, flags_ws, stream);
}

// The two entry points whose re-run takes sets of the layers' own: `who` they are, `who_f32` the fp32 entry point whose rules these are
static int cyl_split_safe_own_sets(const char* who, const char* who_f32, const float* x, int npatch, const void* const* wt_split_host,
                                   const float* const* wt_wg_host, const float* const* bias_host, const int* cin_host, const int* cout_host,
                                   const int* relu_host, const float* const* wt24_host, const float* const* wt25_host, bool w25, const float* head_params,
                                   float* y_or_equi, float* desc, int* status_dev, int* flags_ws, void* stream, bool w25t = false,
                                   const float* const* taps_host = nullptr, int order = 0)
{
    BUF_REQUIRE(npatch >= 0, BUF_EINVAL, "%s: npatch=%d", who, npatch);
    BUF_REQUIRE(!w25t || (order & ~BUF_CYL_ROW6_FIRST) == 0, BUF_EINVAL, "%s: order=%d (0, or BUF_CYL_ROW6_FIRST = 1)", who, order);
    if (npatch == 0) return BUF_OK;
    BUF_REQUIRE(x && y_or_equi && flags_ws && wt_split_host, BUF_EINVAL, "%s: null argument", who);
    BUF_REQUIRE(!head_params || desc, BUF_EINVAL, "%s: head without desc", who);
    BUF_REQUIRE(wt24_host && (wt25_host || !w25) && (taps_host || !w25t), BUF_EINVAL, "%s: null argument", who_f32);
    CylWgParams P;
    CylKernel* K;
    if (int rc = cyl_prepare(wt_wg_host, bias_host, cin_host, cout_host, relu_host, wt24_host, wt25_host, BUF_CYL_FORM_DEFAULT, who_f32, P, K, taps_host, order))
        return rc;
    return cyl_split_safe(x, npatch, wt_split_host, bias_host, cin_host, cout_host, relu_host, *K, P, head_params, y_or_equi, desc, status_dev, flags_ws, stream);
}

// The same with wt24_host as for buf_cylindrical_net_wg_all; the re-run of every entry point with sets is k_cyl_net_w25t_rerun
extern "C" int buf_cylindrical_net_split_safe_all(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                                  const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                                  const float* const* wt24_host, const float* head_params, float* y_or_equi, float* desc,
                                                  int* status_dev, int* flags_ws, void* stream)
{
    return cyl_split_safe_own_sets("buf_cylindrical_net_split_safe_all", "buf_cylindrical_net_wg_all", x, npatch, wt_split_host, wt_wg_host, bias_host,
                                   cin_host, cout_host, relu_host, wt24_host, nullptr, false, head_params, y_or_equi, desc, status_dev, flags_ws, stream);
}

// The same with wt24_host and wt25_host as for buf_cylindrical_net_w25
extern "C" int buf_cylindrical_net_split_safe_w25(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                                  const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                                  const float* const* wt24_host, const float* const* wt25_host, const float* head_params,
                                                  float* y_or_equi, float* desc, int* status_dev, int* flags_ws, void* stream)
{
    return cyl_split_safe_own_sets("buf_cylindrical_net_split_safe_w25", "buf_cylindrical_net_w25", x, npatch, wt_split_host, wt_wg_host, bias_host,
                                   cin_host, cout_host, relu_host, wt24_host, wt25_host, true, head_params, y_or_equi, desc, status_dev, flags_ws, stream);
}

// The same with taps_host and order as for buf_cylindrical_net_w25t
extern "C" int buf_cylindrical_net_split_safe_w25t(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                                   const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                                   const float* const* wt24_host, const float* const* wt25_host, const float* const* taps_host,
                                                   int order, const float* head_params, float* y_or_equi, float* desc, int* status_dev,
                                                   int* flags_ws, void* stream)
{
    return cyl_split_safe_own_sets("buf_cylindrical_net_split_safe_w25t", "buf_cylindrical_net_w25t", x, npatch, wt_split_host, wt_wg_host, bias_host,
                                   cin_host, cout_host, relu_host, wt24_host, wt25_host, true, head_params, y_or_equi, desc, status_dev, flags_ws, stream,
                                   true, taps_host, order);
}

// The cost net likewise: dense inputs (s_rows == null: s_eq, t_eq f32[m,32,5,20]) or the gathered form (s_eq = t_eq = equi
// f32[rows,32,ele_n,20] with ele_n = 7 and int64 row ids).  wt_split_host: 11 planes (buf_split_tile_gemm), wt_f32_host: the 10 matrices of
// buf_cost_volume_net; the two bias sets as for those entry points.  flags_ws: DEVICE int32[m].  The re-run is the fp32 kernel's masked twin with
// the nsets sets of f24_host as the fp32 entry point of the same suffix takes them, so the flagged matches carry, bit for bit, what that
// call returns.
static int cost_split_safe(const char* who, int nsets, const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows,
                           const long long* t_rows, int m, const void* const* wt_split_host, const float* const* bias_split_host,
                           const float* const* wt_f32_host, const float* const* bias_f32_host, const float* const* f24_host, float* ind_out,
                           int* status_dev, int* flags_ws, void* stream)
{
    BUF_REQUIRE(m >= 0, BUF_EINVAL, "%s: m=%d", who, m);
    if (m == 0) return BUF_OK;
    BUF_REQUIRE(s_eq && t_eq && wt_split_host && bias_split_host && wt_f32_host && bias_f32_host && (f24_host || nsets == 0) &&
                ind_out && flags_ws, BUF_EINVAL, "%s: null argument", who);
    BUF_REQUIRE((s_rows == nullptr) == (t_rows == nullptr), BUF_EINVAL, "%s: one row list without the other", who);
    BUF_REQUIRE(!s_rows || ele_n == 7, BUF_EINVAL, "%s: ele_n=%d (the kernels are built for ele_n = 7)", who, ele_n);
    CostNetParams P;
    if (int rc = cost_net_prepare(P, wt_f32_host, bias_f32_host, f24_host, nsets, s_rows, t_rows, ele_n, flags_ws, who)) return rc;
    BUF_CHECK_HIP(hipMemsetAsync(flags_ws, 0, sizeof(int) * (size_t)m, (hipStream_t)stream));
    if (int rc = cost_net_h3_launch(s_eq, t_eq, m, wt_split_host, bias_split_host, s_rows, t_rows, ele_n, ind_out, status_dev, stream, who, flags_ws)) return rc;
    return cost_net_launch(s_eq, t_eq, m, P, ind_out, stream);
}

extern "C" int buf_cost_volume_net_split_safe(const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows, const long long* t_rows,
                                              int m, const void* const* wt_split_host, const float* const* bias_split_host,
                                              const float* const* wt_f32_host, const float* const* bias_f32_host, float* ind_out,
                                              int* status_dev, int* flags_ws, void* stream)
{
    return cost_split_safe("buf_cost_volume_net_split_safe", 0, s_eq, t_eq, ele_n, s_rows, t_rows, m, wt_split_host, bias_split_host, wt_f32_host,
                           bias_f32_host, nullptr, ind_out, status_dev, flags_ws, stream);
}

// f24_host[3] as for buf_cost_volume_net_w24
extern "C" int buf_cost_volume_net_split_safe_w24(const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows, const long long* t_rows,
                                                  int m, const void* const* wt_split_host, const float* const* bias_split_host,
                                                  const float* const* wt_f32_host, const float* const* bias_f32_host, const float* const* f24_host,
                                                  float* ind_out, int* status_dev, int* flags_ws, void* stream)
{
    return cost_split_safe("buf_cost_volume_net_split_safe_w24", 3, s_eq, t_eq, ele_n, s_rows, t_rows, m, wt_split_host, bias_split_host, wt_f32_host,
                           bias_f32_host, f24_host, ind_out, status_dev, flags_ws, stream);
}

// f24_host[5] as for buf_cost_volume_net_w24b
extern "C" int buf_cost_volume_net_split_safe_w24b(const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows, const long long* t_rows,
                                                   int m, const void* const* wt_split_host, const float* const* bias_split_host,
                                                   const float* const* wt_f32_host, const float* const* bias_f32_host, const float* const* f24_host,
                                                   float* ind_out, int* status_dev, int* flags_ws, void* stream)
{
    return cost_split_safe("buf_cost_volume_net_split_safe_w24b", 5, s_eq, t_eq, ele_n, s_rows, t_rows, m, wt_split_host, bias_split_host, wt_f32_host,
                           bias_f32_host, f24_host, ind_out, status_dev, flags_ws, stream);
}
