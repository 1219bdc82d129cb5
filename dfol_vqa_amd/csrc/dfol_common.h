// Shared device helpers and ABI plumbing for the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/dfol_vqa.h"

#define DFOL_EPS 1e-20f          // util.py:25
#define DFOL_WAVE 64

void dfol_set_error(const char* fmt, ...);
uint32_t* dfol_range_status_ptr();      // the calling thread's status word for the fp16-range kernels (dfol_set_range_status), or NULL

#define DFOL_REQUIRE(cond, ...)                 \
    do {                                        \
        if (!(cond)) {                          \
            dfol_set_error(__VA_ARGS__);        \
            return 1;                           \
        }                                       \
    } while (0)

#define DFOL_LAUNCH_CHECK(name)                                                          \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) {                                                          \
            dfol_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));        \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

// ---- transcendental helpers -----------------------------------------------------------------------
// The logic kernels evaluate exp and log once or twice per byte they stream, so they use the hardware
// v_exp_f32 / v_log_f32 directly (1 ulp each; arguments are log-probabilities <= 0 and probabilities in
// [1e-20, 2], so neither overflow nor denormal-input handling is needed).  -DDFOL_PRECISE_MATH swaps in
// the libm versions for A/B parity runs.
__device__ __forceinline__ float dfol_exp(float x) {
#ifdef DFOL_PRECISE_MATH
    return expf(x);
#else
    return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f);
#endif
}

__device__ __forceinline__ float dfol_log(float x) {
#ifdef DFOL_PRECISE_MATH
    return logf(x);
#else
    return __builtin_amdgcn_logf(x) * 0.69314718055994530942f;
#endif
}

// util.py:22-25
__device__ __forceinline__ float dfol_slog(float x) { return dfol_log(fmaxf(x, DFOL_EPS)); }
// util.py:35-36
__device__ __forceinline__ float dfol_lnot(float x) { return dfol_slog(1.0f - dfol_exp(x)); }
// util.py:46-47 with beta = 1:  log(max(alpha + (1 - 2 alpha) e^x, eps)); c = 1 - 2 alpha
__device__ __forceinline__ float dfol_pnot(float x, float alpha, float c) { return dfol_slog(alpha + c * dfol_exp(x)); }
// d/dx log(max(alpha + c e^x, eps)),  c = 1 - 2 alpha  (the clamp has zero gradient below the floor)
__device__ __forceinline__ float dfol_dpnot(float x, float alpha, float c) {
    const float e = dfol_exp(x);
    const float d = alpha + c * e;
    return d > DFOL_EPS ? c * e / d : 0.f;
}

// A stored likelihood as every logic cell reads it:  v = min(ll, 0)  (batch_base_ops.py:194), then the predicate's negation  l' = pnot(v)
// (:212-213) in a launch that has any negated predicate (alpha_n = 1 for a negated one, cn = 1 - 2 alpha_n).  One spelling for the ungated
// and gated forward and backward kernels.
__device__ __forceinline__ float dfol_prep(float ll, int any_neg, float alpha_n, float cn) {
    float v = fminf(ll, 0.f);
    if (any_neg) v = dfol_pnot(v, alpha_n, cn);
    return v;
}
// d l' / d ll
__device__ __forceinline__ float dfol_dprep(float ll, int any_neg, float alpha_n, float cn) {
    const float v = fminf(ll, 0.f);
    float d = ll < 0.f ? 1.f : 0.f;                        // -relu(-x): subgradient 0 at and above 0 (torch relu)
    if (any_neg) d *= dfol_dpnot(v, alpha_n, cn);
    return d;
}

// ---- activations ------------------------------------------------------------------------------------------------------------------
// Sigmoid on the hardware exp2 / rcp (1 ulp each, absolute error < 2e-7), the form of the streaming kernels and the producers of the
// matrix-pipe kernels: it ignores -DDFOL_PRECISE_MATH.
__device__ __forceinline__ float dfol_sigmoid_hw(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * x)); }
// its derivative h (1 - h), h = dfol_sigmoid_hw(x)
__device__ __forceinline__ float dfol_dsigmoid_hw(float x) {
    const float h = dfol_sigmoid_hw(x);
    return h * (1.0f - h);
}

// The epilogue activations of the matrix-pipe linear kernels: branch-free forms on dfol_exp / dfol_log and the hardware rcp (1 ulp each;
// absolute error < 2e-7 on these ranges).  They follow -DDFOL_PRECISE_MATH through dfol_exp / dfol_log.
template <int ACT>
__device__ __forceinline__ float dfol_act(float x) {
    if (ACT == DFOL_ACT_SIGMOID) return __builtin_amdgcn_rcpf(1.0f + dfol_exp(-x));
    if (ACT == DFOL_ACT_ELU) return fmaxf(x, dfol_exp(fminf(x, 0.f)) - 1.0f);
    if (ACT == DFOL_ACT_LOGSIGMOID) return fminf(x, 0.f) - dfol_log(1.0f + dfol_exp(-fabsf(x)));
    return x;
}

// ---- box positions ----------------------------------------------------------------------------------------------------------------
// batch_gqa_boxfeatures_pipeline.py:208-211: position column k of {x, y, w, h} / max({W, H, W, H}, 1) from t = (W, H, x, y, w, h); one fp32
// division per column, shared by box_positions_kernel and the feature store's cached-row kernel so the two agree bit for bit
__device__ __forceinline__ float dfol_box_position(const float* t, int k) { return t[2 + k] / fmaxf(t[k & 1], 1.f); }

// ---- object pairs -----------------------------------------------------------------------------------------------------------------
// batch_gqa_boxfeatures_pipeline.py:263-279: {distance, angle, sign dx, sign dy} of subject box ps and object box po ({x, y, w, h})
__device__ __forceinline__ float4 dfol_pair_geometry(const float* ps, const float* po) {
    const float x1 = ps[0], y1 = ps[1], w1 = ps[2], h1 = ps[3], x2 = po[0], y2 = po[1], w2 = po[2], h2 = po[3];
    const float dx = x1 + w1 / 2.0f - x2 - w2 / 2.0f, dy = y1 + h1 / 2.0f - y2 - h2 / 2.0f;
    const float dist = sqrtf(dx * dx + dy * dy);
    return make_float4(dist, asinf(dy / fmaxf(dist, 1e-10f)), (x2 - x1 > 0.f) ? 1.f : ((x2 - x1 < 0.f) ? -1.f : 0.f),
                       (y2 - y1 > 0.f) ? 1.f : ((y2 - y1 < 0.f) ? -1.f : 0.f));
}

// Ordered pair e of an image of n >= 2 objects, the diagonal left out (util.py:87-103): subject s = e / (n - 1), object o != s
__device__ __forceinline__ void dfol_offdiag_slot(int e, int n, int& s, int& o) {
    s = e / (n - 1);
    const int oo = e - s * (n - 1);
    o = oo + (oo >= s);
}
// The same without the integer-division sequence: (e + 0.5) / (n - 1) is at least 0.5 / (n - 1) away from an integer.
// How far that carries.  m = n - 1, e < m (m + 1), x = e + 0.5.  The exact quotient is x / m = s + (oo + 0.5) / m with 0 <= oo <= m - 1, so
// truncation yields s as long as the computed quotient p is off by LESS than 0.5 / m.  What is rounded on the way:
//   (float)e, (float)m  exact (integers below 2^24);   (float)e + 0.5f  exact while e < 2^23 (2 e + 1 fits 24 bits);
//   r = v_rcp_f32(m)    within 1 ulp of 1 / m (the instruction's documented accuracy), and an ulp of v is at most 2^-23 |v|: r = (1 + d1) / m,
//                       |d1| <= 2^-23;
//   p = fl(x r)         one rounding to nearest: p = x r (1 + d2), |d2| <= 2^-24  (p >= 0.5 / m is far from the denormals).
// |p - x / m| <= (x / m) ((1 + 2^-23)(1 + 2^-24) - 1) < (x / m) 1.5000001 2^-23, which is below 0.5 / m iff x < 2^23 / 3.0000002 = 2 796 202.5.
// The largest x is m (m + 1) - 0.5:  m = 1671 gives 2 793 911.5 (in; also below 2^23, so the sum above is exact), m = 1672 gives 2 797 255.5
// (out).  The decode therefore equals dfol_offdiag_slot for every pair of an image of n <= 1672 objects; the launchers that use it refuse
// max_n above DFOL_OFFDIAG_RCP_MAX_N, a round figure well inside that (at 1024 the error term uses 0.375 of the 0.5 / m it has).  The bound
// rests on this derivation: on the device the decode has run at up to 300 objects (tests/test_pair_infer_shapes_gpu.py against float64, and
// the 100-object launches of the other pair tests), never at the bound itself; tests/test_pair_infer_shapes_gpu.py restates the arithmetic on
// the host with the reciprocal off by an ulp either way.
#define DFOL_OFFDIAG_RCP_MAX_N 1024
__device__ __forceinline__ void dfol_offdiag_slot_rcp(int e, int n, int& s, int& o) {
    s = (int)(((float)e + 0.5f) * __builtin_amdgcn_rcpf((float)(n - 1)));
    const int oo = e - s * (n - 1);
    o = oo + (oo >= s);
}

// ---- EXISTS aggregation without cancellation ----------------------------------------------------------
// The reference aggregates an EXISTS variable as  log_not(sum_i log_not(u_i)) = log(1 - prod_i (1 - y_i)),  y_i = e^{u_i}
// (util.py:35-36, batch_base_ops.py:102-133, batch_base_types.py:115-123).  Evaluated as written in fp32, every factor 1 - y_i is
// rounded at 2^-25 ABSOLUTE, and the final 1 - e^S amplifies that by 1 / (1 - e^S): the reference's own fp32 run carries 1e-5 .. 1e-4 of
// noise on a log-probability of -4.  The kernels keep the COMPLEMENT  q = 1 - prod (1 - y_i)  instead, by the recurrence of the
// probabilistic OR:   q <- q + y - q y   (= 1 - (1 - q)(1 - y)).
// q is a sum of non-negative terms, so every step is accurate RELATIVE to q (2^-24 per step, no cancellation anywhere), and the
// aggregate is simply log(max(q, eps)): the float64 value of the reference's formula to ~1e-6 in the log domain, whatever the size of q.
// The reference's per-term clamp max(1 - y, eps) only matters when y = 1, where both forms give q = 1 (log 1 = 0); its outer clamp
// max(1 - e^S, eps) is the max(q, eps) here.  y > 1 (a prior above log 1) is not handled by this form: callers detect it and fall back
// to the general, clamping code.
__device__ __forceinline__ float dfol_or(float q, float y) { return fmaf(-q, y, q + y); }

// Sum over all 64 lanes; every lane gets the total.
__device__ __forceinline__ float dfol_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- DPP reductions ---------------------------------------------------------------------------------
// x + (x of the lane selected by the DPP control word); lanes whose source is masked off add 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dfol_dpp_add(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}

// Sum over aligned groups of G consecutive lanes (G = 1..64, power of two) without touching LDS: quad permutes and row
// mirrors inside each 16-lane row, then row_bcast15 / row_bcast31 across rows.  The total is valid in the LAST lane of
// each group (for G <= 16 in every lane of the group).
template <int G>
__device__ __forceinline__ float dfol_group_sum(float x) {
    if (G >= 2) x = dfol_dpp_add<0xB1, 0xF>(x);       // quad_perm [1,0,3,2]
    if (G >= 4) x = dfol_dpp_add<0x4E, 0xF>(x);       // quad_perm [2,3,0,1]
    if (G >= 8) x = dfol_dpp_add<0x141, 0xF>(x);      // row_half_mirror
    if (G >= 16) x = dfol_dpp_add<0x140, 0xF>(x);     // row_mirror
    if (G >= 32) x = dfol_dpp_add<0x142, 0xA>(x);     // row_bcast15 into rows 1 and 3
    if (G >= 64) x = dfol_dpp_add<0x143, 0xC>(x);     // row_bcast31 into rows 2 and 3
    return x;
}

// The lane selected by the DPP control word hands over its value; lanes whose source is masked off get 0 (the neutral element of OR).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dfol_dpp_or(float q) {
    const float o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(q), CTRL, ROW_MASK, 0xF, false));
    return fmaf(o, 1.0f - q, q);                         // q + o (1 - q): the DPP move folds into the multiply-add
}

// Probabilistic OR over aligned groups of G consecutive lanes, same lane schedule as dfol_group_sum (valid in the LAST lane of each
// group; for G <= 16 in every lane).  1 - q is rounded once per step, but it enters as a FACTOR of the incoming term, so the step
// stays accurate relative to q.
template <int G>
__device__ __forceinline__ float dfol_group_or(float q) {
    if (G >= 2) q = dfol_dpp_or<0xB1, 0xF>(q);
    if (G >= 4) q = dfol_dpp_or<0x4E, 0xF>(q);
    if (G >= 8) q = dfol_dpp_or<0x141, 0xF>(q);
    if (G >= 16) q = dfol_dpp_or<0x140, 0xF>(q);
    if (G >= 32) q = dfol_dpp_or<0x142, 0xA>(q);
    if (G >= 64) q = dfol_dpp_or<0x143, 0xC>(q);
    return q;
}

// Eight bf16 bit patterns (one 16-byte load of a bf16 relation tile) widened to fp32: exact, a bf16 is the upper half of an fp32.
__device__ __forceinline__ void bf16x8_to_f32(const uint4 w, float (&l)[8]) {
    const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        l[2 * i] = __uint_as_float(v[i] << 16);
        l[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}

static inline int dfol_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- host: lanes per row of the wavefront-per-predicate kernels -------------------------------------------------------------------
// A row of `groups` 16-byte column groups is covered by LPR lanes, LPR the smallest power of two >= groups (at most MAX_LPR, 32 or 64: the
// bf16 kernels own eight columns per lane and stop at 32).  launch(std::integral_constant<int, LPR>) gets it as a compile-time value.
template <int MAX_LPR = 64, class Launch>
static inline void dfol_dispatch_lpr(int groups, Launch&& launch) {
    static_assert(MAX_LPR == 32 || MAX_LPR == 64, "dfol_dispatch_lpr: the ladders end at 32 or 64");
    if (groups <= 1) launch(std::integral_constant<int, 1>{});
    else if (groups <= 2) launch(std::integral_constant<int, 2>{});
    else if (groups <= 4) launch(std::integral_constant<int, 4>{});
    else if (groups <= 8) launch(std::integral_constant<int, 8>{});
    else if (groups <= 16) launch(std::integral_constant<int, 16>{});
    else if (MAX_LPR == 32 || groups <= 32) launch(std::integral_constant<int, 32>{});
    else if constexpr (MAX_LPR == 64) launch(std::integral_constant<int, 64>{});
}
