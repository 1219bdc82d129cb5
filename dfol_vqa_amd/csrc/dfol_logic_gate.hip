// The logic cell with the trainable gate (`trainable_gate: True`): gated forms of the Filter and Relate kernels, forward and backward, and of the
// one-posterior Relate (forward on prev-row tiles for inference; forward and backward on subject-row tiles for the train step).
//
// Reference: NeuralLogicGate, batch_base_ops.py:19-38, used by BatchBayesianLogicCell._forward_core at :99-102 and :135-138: every
// `x + log_p` of the cell becomes G_k(x, log_p), k the axis whose prior is joined.  With W_k [6, 2], c_k [6] (nn.Linear(2, 6)):
//     alpha = sigmoid(W_k [a, b] + c_k)
//     va = alpha0 + alpha3 (1 - 2 alpha0) e^a        vb = alpha1 + alpha4 (1 - 2 alpha1) e^b
//     G  = log(max(alpha2 + alpha5 (1 - 2 alpha2) max(va, eps) max(vb, eps), eps))
// (the reference takes e^(log va + log vb) of two clamped logarithms, util.py:46-47: the product is the same value with one logarithm).
// m = e^G is a probability, so the quantifier transform of an inner term, F(G) = log(max(q + (1 - 2 q) m, eps)), needs no exponential,
// and an EXISTS aggregation 1 - prod (1 - m) is kept in the complement form q <- q + m - q m (dfol_or, dfol_common.h) with no
// logarithm per element.  The complement fast path of the ungated kernel (one e^l' for both directions times e^prior) does not apply:
// the two directions have different inner terms.  What both directions share is l' and e^l'.
//
// The gate's 18 parameters per axis are wave-uniform (scalar registers); a column's prior, its exponential and its share W[:,1] b + c of
// the six pre-activations are computed once per wavefront (forward), a row's once per row.
//
// Backward: the formulas as written, clamps included (zero gradient below a floor), recomputed from the inputs.  The parameter
// gradient is a sum over every element of the launch: per-thread sums -> wavefront (shuffles) -> workgroup (LDS, wavefront order) ->
// one row of a scratch buffer per workgroup -> a second kernel adds the rows in a fixed order.  No atomics: two runs give the same bits.
//
// Layout of the Relate family.  Every forward kernel computes, for one predicate, one or two aggregations of the same shape
//     post[i] = G_out( F( agg_{j < n, j != i} F( G_in(l'[.], pv[j]) ) ), xv[i] ),     F and agg by the quantifier of the summed-out axis j,
// described by a GatePred record (whose prior is summed out, whose is kept, the two gates, quantifier, negation).  The kernels differ only in
// which axis of the tile j runs along and in the tile's number format, and are put together from
//     gate_col_sweep   j along rows, NS <= 256: the aggregates stay in a lane's registers                     (fp32: 4 columns per lane, bf16: 8)
//     gate_row_put / gate_row_finish   j along columns, NS <= 256: group reduction per row into the wavefront's LDS row, outer gate per row
//     gate_big_cols / gate_big_rows   the same two directions for NS > 256, a workgroup per predicate
// The two-posterior kernel relate_gate_fwd_kernel keeps its own fused loop (one tile load and one e^l' serve both directions) around the
// element step and the two tails.  relate_keep_gate_fwd_kernel is written out on its own: built from the shared sweeps it computed the same
// bits 2 - 3 % slower (profiles/r23_gate_refactor.txt).  The backward kernels share the record and the parameter-sum epilogue; their sweeps
// are their own.
#include "dfol_common.h"

namespace {

struct GateW {
    float w0[6], w1[6], c[6];
};

__device__ __forceinline__ GateW gate_load(const float* __restrict__ g) {      // float[18]: W row-major [6][2], then c [6]
    GateW G;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        G.w0[i] = g[2 * i];
        G.w1[i] = g[2 * i + 1];
        G.c[i] = g[12 + i];
    }
    return G;
}

// sigmoid(z) and 1 - sigmoid(z), each accurate relative to itself (e <= 1: no overflow, no cancellation on either side)
__device__ __forceinline__ void gate_sig(float z, float& al, float& om) {
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896340736f * fabsf(z));
    const float r = __builtin_amdgcn_rcpf(1.0f + e), er = e * r;
    const bool pos = z >= 0.f;
    al = pos ? r : er;
    om = pos ? er : r;
}

__device__ __forceinline__ void gate_zb(const GateW& G, float b, float* zb) {
#pragma unroll
    for (int i = 0; i < 6; ++i) zb[i] = fmaf(G.w1[i], b, G.c[i]);
}

// m = e^G(a, b) from a, ea = e^a, zb = W[:,1] b + c, eb = e^b
__device__ __forceinline__ float gate_m(const GateW& G, float a, float ea, const float* zb, float eb) {
    float al[6], om[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) gate_sig(fmaf(G.w0[i], a, zb[i]), al[i], om[i]);
    const float va = fmaxf(fmaf(al[3] * (om[0] - al[0]), ea, al[0]), DFOL_EPS);
    const float vb = fmaxf(fmaf(al[4] * (om[1] - al[1]), eb, al[1]), DFOL_EPS);
    return fmaxf(fmaf(al[5] * (om[2] - al[2]), va * vb, al[2]), DFOL_EPS);
}

__device__ __forceinline__ float gate_log(const GateW& G, float a, float b) {
    float zb[6];
    gate_zb(G, b, zb);
    return dfol_log(gate_m(G, a, dfol_exp(a), zb, dfol_exp(b)));
}

// Backward of one gate.  g is the gradient of G = log m (from_log) or of m itself; da, db are returned, the parameter gradients are
// added into acc[18] (the layout of the parameters).
__device__ __forceinline__ void gate_bwd(const GateW& G, float a, float b, float g, bool from_log, float& da, float& db, float* acc) {
    float al[6], om[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) gate_sig(fmaf(G.w0[i], a, fmaf(G.w1[i], b, G.c[i])), al[i], om[i]);
    const float ea = dfol_exp(a), eb = dfol_exp(b);
    const float k0 = om[0] - al[0], k1 = om[1] - al[1], k2 = om[2] - al[2];
    const float va_raw = fmaf(al[3] * k0, ea, al[0]), vb_raw = fmaf(al[4] * k1, eb, al[1]);
    const float va = fmaxf(va_raw, DFOL_EPS), vb = fmaxf(vb_raw, DFOL_EPS), pv = va * vb;
    const float m_raw = fmaf(al[5] * k2, pv, al[2]);
    float dm = 0.f;
    if (m_raw > DFOL_EPS) dm = from_log ? g / m_raw : g;
    float dal[6];
    dal[2] = dm * (1.f - 2.f * al[5] * pv);
    dal[5] = dm * k2 * pv;
    const float dpv = dm * al[5] * k2;
    const float dva = va_raw > DFOL_EPS ? dpv * vb : 0.f, dvb = vb_raw > DFOL_EPS ? dpv * va : 0.f;
    dal[0] = dva * (1.f - 2.f * al[3] * ea);
    dal[3] = dva * k0 * ea;
    dal[1] = dvb * (1.f - 2.f * al[4] * eb);
    dal[4] = dvb * k1 * eb;
    float xa = dva * al[3] * k0 * ea, xb = dvb * al[4] * k1 * eb;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float dz = dal[i] * al[i] * om[i];
        xa = fmaf(dz, G.w0[i], xa);
        xb = fmaf(dz, G.w1[i], xb);
        acc[2 * i] = fmaf(dz, a, acc[2 * i]);
        acc[2 * i + 1] = fmaf(dz, b, acc[2 * i + 1]);
        acc[12 + i] += dz;
    }
    da = xa;
    db = xb;
}

// A predicate's negation: alpha_n = 1 for a negated predicate of a launch that has any, cn = 1 - 2 alpha_n
struct GateNeg {
    int any_neg;
    float alpha_n, cn;
};

__device__ __forceinline__ GateNeg gate_neg_load(const uint8_t* __restrict__ neg, int any_neg, int p) {
    GateNeg N;
    N.any_neg = any_neg;
    N.alpha_n = (any_neg && neg[p]) ? 1.f : 0.f;
    N.cn = 1.f - 2.f * N.alpha_n;
    return N;
}

// l' = negation(min(ll, 0)) (batch_base_ops.py:194, :212-213) and its derivative: dfol_prep / dfol_dprep (dfol_common.h) on a GateNeg
__device__ __forceinline__ float gate_prep(float ll, const GateNeg& N) { return dfol_prep(ll, N.any_neg, N.alpha_n, N.cn); }
__device__ __forceinline__ float gate_dpnot(float x, float alpha, float c) { return dfol_dpnot(x, alpha, c); }
__device__ __forceinline__ float gate_dprep(float ll, const GateNeg& N) { return dfol_dprep(ll, N.any_neg, N.alpha_n, N.cn); }

// The quantifier of a summed-out axis: kf = 1 - 2 qf, ex = EXISTS, ident = a lone predicate's literal FOR_ALL branch (:104-108)
struct GateQuant {
    float qf, kf;
    bool ex, ident;
};

__device__ __forceinline__ GateQuant gate_quant_load(const float* __restrict__ quant, int p, int identity_forall) {
    GateQuant Q;
    Q.qf = quant[p];
    Q.kf = 1.f - 2.f * Q.qf;
    Q.ex = Q.qf == 1.f;
    Q.ident = identity_forall && Q.qf == 0.f;
    return Q;
}

// One inner term of an aggregation from m = e^G: EXISTS keeps the probability (complement form), otherwise F(G) = log(max(q + k m, eps))
// (FOR_ALL: log m = G itself, also in the lone predicate's literal branch, :104-108)
__device__ __forceinline__ float gate_term(float m, const GateQuant& Q) { return Q.ex ? m : dfol_slog(fmaf(Q.kf, m, Q.qf)); }
__device__ __forceinline__ float gate_join(float acc, float t, bool ex) { return ex ? dfol_or(acc, t) : acc + t; }
// the aggregate after the outer transform (:129-133): a log-probability
__device__ __forceinline__ float gate_outer(float agg, const GateQuant& Q) {
    return Q.ex ? dfol_slog(agg) : (Q.ident ? agg : dfol_pnot(agg, Q.qf, Q.kf));
}

// ---------------------------------------------------------------------------------------------------
// filter (arity 1): post[o] = G_0(l'[o], prior[o])
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void filter_gate_fwd_kernel(const float* __restrict__ att_in, const float* __restrict__ ll,
                                                              const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj,
                                                              const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active,
                                                              int64_t total4, int NS4, const float* __restrict__ gate, float* __restrict__ att_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const GateW G = gate_load(gate);
    const int p = (int)(idx / NS4), c0 = (int)(idx - (int64_t)p * NS4) * 4;
    const int q = pred_q[p], n = n_obj[q];
    const float4 a4 = *reinterpret_cast<const float4*>(att_in + ((int64_t)q * NS4 * 4 + c0));
    const float4 l4 = *reinterpret_cast<const float4*>(ll + idx * 4);
    const float av[4] = {a4.x, a4.y, a4.z, a4.w}, l[4] = {l4.x, l4.y, l4.z, l4.w};
    float o[4];
    const bool act = active == nullptr || active[p];
    const GateNeg N = gate_neg_load(neg, any_neg, p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = av[j];                                                         // no-op token: the prior row (:385)
        if (act) o[j] = gate_log(G, gate_prep(l[j], N), av[j]);               // :135-136
        if (c0 + j >= n) o[j] = 0.f;
    }
    *reinterpret_cast<float4*>(att_out + idx * 4) = make_float4(o[0], o[1], o[2], o[3]);
}

constexpr int FG_THREADS = 256;

// one thread per element; the workgroup's parameter partial goes to scratch[blockIdx.x][18]
__global__ __launch_bounds__(FG_THREADS) void filter_gate_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ att_in,
                                                                     const float* __restrict__ ll, const int32_t* __restrict__ pred_q,
                                                                     const int32_t* __restrict__ n_obj, const uint8_t* __restrict__ neg, int any_neg,
                                                                     const uint8_t* __restrict__ active, int64_t total, int NS,
                                                                     const float* __restrict__ gate, float* __restrict__ scratch,
                                                                     float* __restrict__ g_prior, float* __restrict__ g_ll) {
    __shared__ float wpart[FG_THREADS / 64][18];
    const int64_t i = (int64_t)blockIdx.x * FG_THREADS + threadIdx.x;
    const GateW G = gate_load(gate);
    float acc[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) acc[k] = 0.f;
    if (i < total) {
        const int p = (int)(i / NS), c = (int)(i - (int64_t)p * NS);
        const int q = pred_q[p], n = n_obj[q];
        float dp = 0.f, dl = 0.f;
        if (c < n) {
            const float g = g_out[i];
            if (active == nullptr || active[p]) {
                const GateNeg N = gate_neg_load(neg, any_neg, p);
                const float raw = ll[i];
                float da;
                gate_bwd(G, gate_prep(raw, N), att_in[(int64_t)q * NS + c], g, true, da, dp, acc);
                dl = da * gate_dprep(raw, N);
            } else {
                dp = g;                                                       // posterior = prior
            }
        }
        if (g_prior) g_prior[i] = dp;
        if (g_ll) g_ll[i] = dl;
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const float s = dfol_wave_sum(acc[k]);
        if (lane == 0) wpart[w][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 18) {
        float s = wpart[0][threadIdx.x];
        for (int j = 1; j < FG_THREADS / 64; ++j) s += wpart[j][threadIdx.x];
        scratch[(int64_t)blockIdx.x * 18 + threadIdx.x] = s;
    }
}

// out[k] = sum over the rows of scratch [rows, width], k < width: one wavefront per k, lane l adds rows l, l + 64, ... in order, then the
// fixed shuffle tree.  out_a gets columns [0, 18), out_b (may be NULL) columns [18, 36).
__global__ __launch_bounds__(64) void gate_param_reduce_kernel(const float* __restrict__ scratch, int64_t rows, int width, float* __restrict__ out_a,
                                                               float* __restrict__ out_b) {
    const int k = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int64_t r = lane; r < rows; r += 64) s += scratch[r * width + k];
    s = dfol_wave_sum(s);
    if (lane == 0) {
        if (k < 18) {
            if (out_a) out_a[k] = s;
        } else if (out_b) {
            out_b[k - 18] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// relate (arity 2): the predicate record
// ---------------------------------------------------------------------------------------------------
// One aggregation of one predicate: post[i] = G_out( F( agg_{j < n, j != i} F( G_in(l'[.], pv[j]) ) ), xv[i] ), F and agg by Q.
template <class TileT = float>
struct GatePred {
    int q, n, NS;
    const float* pv;          // the summed-out variable's attention (rows of question q)
    const float* xv;          // the kept variable's attention
    const TileT* tp;          // the predicate's NS x NS tile
    float* out;
    bool xs;                  // single posterior: the kept variable is the subject (axis 0)
    GateNeg N;
    GateQuant Q;
    GateW GI, GO;             // inner gate: the summed-out axis', outer gate: the kept axis'
};

// The single-posterior kernels' record.  x = the freshly selected variable (kept), prev = the incoming one (summed out).  The two axes hold
// different gates, so the launch says which axis x is on: x_is_subject[p] -> x on axis 0 (outer gate = gate_s, inner gate = gate_o), else x
// on axis 1 (outer = gate_o, inner = gate_s).  False for a no-op predicate (a question without this operator): its gates and quantifier are
// not read.  `post` may be NULL (backward).
template <class TileT>
__device__ __forceinline__ bool gate_pred_load(GatePred<TileT>& g, int p, const float* __restrict__ x_att, const float* __restrict__ prev_att,
                                               const TileT* __restrict__ tile, const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj,
                                               const float* __restrict__ quant_prev, const uint8_t* __restrict__ x_is_subject,
                                               const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int NS,
                                               int identity_forall, const float* __restrict__ gate_s, const float* __restrict__ gate_o,
                                               float* __restrict__ post) {
    g.q = pred_q[p];
    g.n = min(n_obj[g.q], NS);
    g.NS = NS;
    g.pv = prev_att + (int64_t)g.q * NS;
    g.xv = x_att + (int64_t)p * NS;
    g.tp = tile + (int64_t)p * NS * NS;
    g.out = post ? post + (int64_t)p * NS : nullptr;
    if (active && !active[p]) return false;
    g.xs = x_is_subject[p] != 0;
    g.GI = gate_load(g.xs ? gate_o : gate_s);
    g.GO = gate_load(g.xs ? gate_s : gate_o);
    g.N = gate_neg_load(neg, any_neg, p);
    g.Q = gate_quant_load(quant_prev, p, identity_forall);
    return true;
}

// the no-op predicate of a single-posterior kernel: attention passes through (as relate_one_fwd_kernel); stride = the threads on the predicate
template <class TileT>
__device__ __forceinline__ void gate_passthrough(const GatePred<TileT>& g, int tid, int stride) {
    for (int c = tid; c < g.NS; c += stride) g.out[c] = c < g.n ? g.pv[c] : 0.f;
}

// The two-posterior kernels' records.  Rows = variable R, columns = variable C:
//   vR:  post_R[r] = G_R( F_C( agg_{c != r} F_C( G_C(l'[r,c], prior_C[c]) ) ), prior_R[r] )        summed out along columns
//   vC:  post_C[c] = G_C( F_R( agg_{r != c} F_R( G_R(l'[r,c], prior_R[r]) ) ), prior_C[c] )        summed out along rows
// Writes what needs no arithmetic - a no-op predicate's posterior = prior (batch_base_ops.py:563-564), zeros for a posterior nobody wants -
// and returns false when nothing is left to compute.
__device__ __forceinline__ bool gate_pred_load2(GatePred<>& vR, GatePred<>& vC, bool& wantR, bool& wantC, int p, const float* __restrict__ prior_R,
                                                const float* __restrict__ prior_C, const float* __restrict__ tile,
                                                const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj,
                                                const float* __restrict__ quant_R, const float* __restrict__ quant_C, const uint8_t* __restrict__ neg,
                                                int any_neg, const uint8_t* __restrict__ active, const uint8_t* __restrict__ want, int want_R_bit,
                                                int want_C_bit, int NS, int flags, const float* __restrict__ gate_R, const float* __restrict__ gate_C,
                                                float* __restrict__ post_R, float* __restrict__ post_C, int tid, int stride) {
    const int q = pred_q[p];
    const int n = min(n_obj[q], NS);
    const int wbits = want ? want[p] : 3;
    wantR = (wbits & want_R_bit) && post_R;
    wantC = (wbits & want_C_bit) && post_C;
    const float* pR = prior_R + (int64_t)q * NS;
    const float* pC = prior_C + (int64_t)q * NS;
    float* oR = post_R ? post_R + (int64_t)p * NS : nullptr;
    float* oC = post_C ? post_C + (int64_t)p * NS : nullptr;
    if (active && !active[p]) {
        for (int c = tid; c < NS; c += stride) {
            if (oR) oR[c] = (wantR && c < n) ? pR[c] : 0.f;
            if (oC) oC[c] = (wantC && c < n) ? pC[c] : 0.f;
        }
        return false;
    }
    if (!wantR && oR)
        for (int c = tid; c < NS; c += stride) oR[c] = 0.f;
    if (!wantC && oC)
        for (int c = tid; c < NS; c += stride) oC[c] = 0.f;
    if (!wantR && !wantC) return false;
    const GateW GR = gate_load(gate_R), GC = gate_load(gate_C);
    const int identity_forall = flags & DFOL_RELATE_LONE_FORALL_IDENTITY;
    const GateNeg N = gate_neg_load(neg, any_neg, p);
    const float* tp = tile + (int64_t)p * NS * NS;
    vR = {q, n, NS, pC, pR, tp, oR, false, N, gate_quant_load(quant_C, p, identity_forall), GC, GR};
    vC = {q, n, NS, pR, pC, tp, oC, false, N, gate_quant_load(quant_R, p, identity_forall), GR, GC};
    return true;
}

// ---------------------------------------------------------------------------------------------------
// relate forward, NS <= 256: one wavefront per predicate.  A lane owns CPL consecutive columns (one 16-byte load: four floats, or eight bf16
// widened exactly), LPR lanes cover a row, 64 / LPR rows per iteration; lanes beyond the width read valid columns (cl) and rows beyond n read
// row n - 1, and both are masked.  Padding and self-relations contribute nothing (:112).  An element costs six sigmoids and one e^l'.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_cols(const float* __restrict__ a, float (&l)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(a);
    l[0] = t.x, l[1] = t.y, l[2] = t.z, l[3] = t.w;
}
__device__ __forceinline__ void load_cols(const uint16_t* __restrict__ a, float (&l)[8]) { bf16x8_to_f32(*reinterpret_cast<const uint4*>(a), l); }

// the inner term F(G_in(v, b)) of one element (:99-100, :108) from v = l', ea = e^v and the summed-out object's zb = W[:,1] b + c, eb = e^b
template <class TileT>
__device__ __forceinline__ float gate_elem(const GatePred<TileT>& g, float v, float ea, const float* zb, float eb) {
    return gate_term(gate_m(g.GI, v, ea, zb, eb), g.Q);
}

// Tail of a column aggregation: the row slots are joined by shuffles, the outer gate (:133, :135-136) runs once per column in the lanes of
// row slot 0, CPL / 4 16-byte stores.
template <int LPR, int CPL, class TileT>
__device__ __forceinline__ void gate_col_finish(const GatePred<TileT>& g, float (&cacc)[CPL], int rs, int c0) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
#pragma unroll
        for (int m = 32; m >= LPR; m >>= 1) cacc[j] = gate_join(cacc[j], __shfl_xor(cacc[j], m, 64), g.Q.ex);
    }
    if (rs == 0 && c0 < g.NS) {
#pragma unroll
        for (int h = 0; h < CPL / 4; ++h) {
            float xj[4], o[4];
            load_cols(g.xv + c0 + 4 * h, xj);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (c0 + 4 * h + j < g.n) ? gate_log(g.GO, gate_outer(cacc[4 * h + j], g.Q), xj[j]) : 0.f;
            *reinterpret_cast<float4*>(g.out + c0 + 4 * h) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// The column sweep: the summed-out variable along rows, the aggregates of a lane's columns in its registers; a row's prior, its exponential
// and its share of the six pre-activations are computed once per row.
template <int LPR, int CPL, class TileT>
__device__ __forceinline__ void gate_col_sweep(const GatePred<TileT>& g, int lane) {
    constexpr int RPI = 64 / LPR;
    const int cg = lane % LPR, rs = lane / LPR, c0 = cg * CPL, cl = min(c0, g.NS - CPL);
    float cacc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) cacc[j] = 0.f;
    for (int r0 = 0; r0 < g.n; r0 += RPI) {
        const int r = r0 + rs, rc = min(r, g.n - 1);
        float l[CPL];
        load_cols(g.tp + (int64_t)rc * g.NS + cl, l);
        const float pr = g.pv[rc];
        float zb[6];
        gate_zb(g.GI, pr, zb);
        const float eb = dfol_exp(pr);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = c0 + j;
            const bool keep = r < g.n && c < g.n && c != r;
            const float v = gate_prep(l[j], g.N);
            const float t = gate_elem(g, v, dfol_exp(v), zb, eb);
            cacc[j] = gate_join(cacc[j], keep ? t : 0.f, g.Q.ex);
        }
    }
    gate_col_finish<LPR, CPL>(g, cacc, rs, c0);
}

// A lane's four columns as summed-out objects: their share of the pre-activations and e^prior (once per wavefront)
__device__ __forceinline__ void gate_cols_prior(const GateW& G, const float* __restrict__ prior4, float (&zb)[4][6], float (&eb)[4]) {
    float pc[4];
    load_cols(prior4, pc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gate_zb(G, pc[j], zb[j]);
        eb[j] = dfol_exp(pc[j]);
    }
}

// a row's aggregate over the LPR lanes that share it (valid in the last lane of the group) into the wavefront's LDS row
template <int LPR>
__device__ __forceinline__ void gate_row_put(float* row_agg, float racc, bool ex, int cg, int r, int n) {
    racc = ex ? dfol_group_or<LPR>(racc) : dfol_group_sum<LPR>(racc);
    if (cg == LPR - 1 && r < n) row_agg[r] = racc;
}

// tail of a row aggregation: the outer gate (:133, :135-136) in the lane that owns the row
__device__ __forceinline__ void gate_row_finish(const GatePred<>& g, const float* row_agg, int lane) {
    __builtin_amdgcn_wave_barrier();                     // LDS is in order within a wavefront; this only pins the schedule
    for (int c = lane; c < g.NS; c += 64) {
        float o = 0.f;
        if (c < g.n) o = gate_log(g.GO, gate_outer(row_agg[c], g.Q), g.xv[c]);
        g.out[c] = o;
    }
}

// ---------------------------------------------------------------------------------------------------
// relate forward, NS > 256: one workgroup of 256 threads per predicate
// ---------------------------------------------------------------------------------------------------
// summed out along rows: a thread per column, rows in order
__device__ __forceinline__ void gate_big_cols(const GatePred<>& g, int tid) {
    for (int c = tid; c < g.NS; c += 256) {
        float o = 0.f;
        if (c < g.n) {
            float acc = 0.f;
            for (int r = 0; r < g.n; ++r) {
                if (r == c) continue;
                const float v = gate_prep(g.tp[(int64_t)r * g.NS + c], g.N);
                float zb[6];
                gate_zb(g.GI, g.pv[r], zb);
                acc = gate_join(acc, gate_elem(g, v, dfol_exp(v), zb, dfol_exp(g.pv[r])), g.Q.ex);
            }
            o = gate_log(g.GO, gate_outer(acc, g.Q), g.xv[c]);
        }
        g.out[c] = o;
    }
}

__device__ __forceinline__ float gate_wave_join(float x, bool ex) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = gate_join(x, __shfl_xor(x, m, 64), ex);
    return x;
}

// summed out along columns: a workgroup reduction per row - thread partials, the wavefront's shuffle tree, the four wavefronts' partials joined in
// wavefront order.  The loop runs over all NS rows and holds barriers: call it only under a condition that is the same for the whole
// workgroup, so that every thread reaches every barrier.
__device__ __forceinline__ void gate_big_rows(const GatePred<>& g, float* part, int tid) {
    const int w = tid >> 6, lane = tid & 63;
    for (int r = 0; r < g.NS; ++r) {
        float s = 0.f;
        if (r < g.n)
            for (int c = tid; c < g.n; c += 256) {
                if (c == r) continue;
                const float v = gate_prep(g.tp[(int64_t)r * g.NS + c], g.N);
                float zb[6];
                gate_zb(g.GI, g.pv[c], zb);
                s = gate_join(s, gate_elem(g, v, dfol_exp(v), zb, dfol_exp(g.pv[c])), g.Q.ex);
            }
        s = gate_wave_join(s, g.Q.ex);
        if (lane == 0) part[w] = s;
        __syncthreads();
        if (tid == 0) {
            const float tot = gate_join(gate_join(gate_join(part[0], part[1], g.Q.ex), part[2], g.Q.ex), part[3], g.Q.ex);
            g.out[r] = r < g.n ? gate_log(g.GO, gate_outer(tot, g.Q), g.xv[r]) : 0.f;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// relate, both posteriors
// ---------------------------------------------------------------------------------------------------
// NS <= 256, the geometry of relate_fwd_kernel.  One loop serves both directions - a tile load and an e^l' per element are shared - so it is
// neither sweep but their element steps side by side, with the sweeps' tails.
template <int LPR>
__global__ __launch_bounds__(256) void relate_gate_fwd_kernel(
    const float* __restrict__ prior_R, const float* __restrict__ prior_C, const float* __restrict__ tile,
    const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj, const float* __restrict__ quant_R,
    const float* __restrict__ quant_C, const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active,
    const uint8_t* __restrict__ want, int want_R_bit, int want_C_bit, int P, int NS, int flags,
    const float* __restrict__ gate_R, const float* __restrict__ gate_C, float* __restrict__ post_R, float* __restrict__ post_C) {
    constexpr int RPI = 64 / LPR;
    __shared__ float row_agg[4][256];
    // (the predicate is the same for the whole wavefront: said so, everything derived from it - the gates' 36 parameters among it - is scalar)
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    GatePred<> vR, vC;
    bool wantR, wantC;
    if (!gate_pred_load2(vR, vC, wantR, wantC, p, prior_R, prior_C, tile, pred_q, n_obj, quant_R, quant_C, neg, any_neg, active, want, want_R_bit,
                         want_C_bit, NS, flags, gate_R, gate_C, post_R, post_C, lane, 64))
        return;
    const int n = vC.n;
    const int cg = lane % LPR, rs = lane / LPR, c0 = cg * 4, cl = min(c0, NS - 4);
    float zbC[4][6], ebC[4];
    gate_cols_prior(vR.GI, vR.pv + cl, zbC, ebC);
    float cacc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < n; r0 += RPI) {
        const int r = r0 + rs, rc = min(r, n - 1);
        float l[4];
        load_cols(vC.tp + (int64_t)rc * NS + cl, l);
        const float pr = vC.pv[rc];
        float zbR[6];
        gate_zb(vC.GI, pr, zbR);
        const float ebR = dfol_exp(pr);
        float racc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            const bool keep = r < n && c < n && c != r;
            const float v = gate_prep(l[j], vC.N);
            const float ea = dfol_exp(v);
            if (wantR) {
                const float t = gate_elem(vR, v, ea, zbC[j], ebC[j]);
                racc = gate_join(racc, keep ? t : 0.f, vR.Q.ex);
            }
            if (wantC) {
                const float t = gate_elem(vC, v, ea, zbR, ebR);
                cacc[j] = gate_join(cacc[j], keep ? t : 0.f, vC.Q.ex);
            }
        }
        if (wantR) gate_row_put<LPR>(row_agg[wave_in_block], racc, vR.Q.ex, cg, r, n);
    }
    if (wantR) gate_row_finish(vR, row_agg[wave_in_block], lane);
    if (wantC) gate_col_finish<LPR, 4>(vC, cacc, rs, c0);
}

// NS > 256, as relate_big_fwd_kernel
__global__ __launch_bounds__(256) void relate_gate_big_fwd_kernel(
    const float* __restrict__ prior_R, const float* __restrict__ prior_C, const float* __restrict__ tile,
    const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj, const float* __restrict__ quant_R,
    const float* __restrict__ quant_C, const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active,
    const uint8_t* __restrict__ want, int want_R_bit, int want_C_bit, int NS, int flags, const float* __restrict__ gate_R,
    const float* __restrict__ gate_C, float* __restrict__ post_R, float* __restrict__ post_C) {
    __shared__ float part[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    GatePred<> vR, vC;
    bool wantR, wantC;
    if (!gate_pred_load2(vR, vC, wantR, wantC, p, prior_R, prior_C, tile, pred_q, n_obj, quant_R, quant_C, neg, any_neg, active, want, want_R_bit,
                         want_C_bit, NS, flags, gate_R, gate_C, post_R, post_C, tid, 256))
        return;
    if (wantC) gate_big_cols(vC, tid);
    if (wantR) gate_big_rows(vR, part, tid);             // (wantR is the workgroup's: every thread reaches the barriers)
}

// ---------------------------------------------------------------------------------------------------
// relate backward, both posteriors: one workgroup per predicate, its wavefronts on rows r = w, w + waves, ..., lane = column (the scheme of
// relate_bwd_kernel): sweep 1 recomputes the aggregates as written (S[r] = sum_c F_C(G_C), T[c] = sum_r F_R(G_R)), the outer gates are
// differentiated by the thread that owns the row / column, sweep 2 takes the element gradients.  Every thread keeps the 2 x 18 parameter
// sums of its elements; the workgroup's total goes to scratch[p][36] (R's 18, then C's).
// ---------------------------------------------------------------------------------------------------
// The parameter sums of a workgroup: wavefront totals into wsum [waves][36] (`first`'s 18, then `second`'s), a barrier - which also publishes
// whatever else the caller left in LDS - and the wavefronts added in order into sc[36].
__device__ __forceinline__ void gate_param_sums(const float (&first)[18], const float (&second)[18], float* wsum, float* __restrict__ sc) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, tid = threadIdx.x, nw = (int)blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const float a = dfol_wave_sum(first[k]), b = dfol_wave_sum(second[k]);
        if (lane == 0) {
            wsum[w * 36 + k] = a;
            wsum[w * 36 + 18 + k] = b;
        }
    }
    __syncthreads();
    if (tid < 36) {
        float s = wsum[tid];
        for (int j = 1; j < nw; ++j) s += wsum[j * 36 + tid];
        sc[tid] = s;
    }
}

constexpr int GB_WAVES = 8;
__global__ __launch_bounds__(64 * GB_WAVES) void relate_gate_bwd_kernel(
    const float* __restrict__ prior_R, const float* __restrict__ prior_C, const float* __restrict__ tile,
    const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj, const float* __restrict__ quant_R,
    const float* __restrict__ quant_C, const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active,
    const float* __restrict__ g_post_R, const float* __restrict__ g_post_C, int NS, int identity_forall,
    const float* __restrict__ gate_R, const float* __restrict__ gate_C, float* __restrict__ scratch,
    float* __restrict__ g_prior_R, float* __restrict__ g_prior_C, float* __restrict__ g_tile) {
    extern __shared__ float gate_bwd_lds[];              // (5 + waves) NS floats + waves x 36
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, tid = threadIdx.x, nw = (int)blockDim.x >> 6, nt = (int)blockDim.x;
    float* sS = gate_bwd_lds;                             // row aggregates, later the rows' prior gradients
    float* sGR = sS + NS;                                 // d loss / d S[r]
    float* sGC = sGR + NS;                                // d loss / d T[c]
    float* sDR = sGC + NS;                                // the outer gates' gradients of prior_R / prior_C
    float* sDC = sDR + NS;
    float* part_base = sDC + NS;
    float* wsum = part_base + (size_t)nw * NS;            // [nw][36]
    auto part = [&](int wave, int c) -> float& { return part_base[wave * NS + c]; };
    const int p = blockIdx.x;
    const int q = pred_q[p];
    const int n = min(n_obj[q], NS);
    const float* pR = prior_R + (int64_t)q * NS;
    const float* pC = prior_C + (int64_t)q * NS;
    const float* tp = tile + (int64_t)p * NS * NS;
    float* gt = g_tile ? g_tile + (int64_t)p * NS * NS : nullptr;
    const float* gR = g_post_R ? g_post_R + (int64_t)p * NS : nullptr;
    const float* gC = g_post_C ? g_post_C + (int64_t)p * NS : nullptr;
    float* sc = scratch + (int64_t)p * 36;

    if (active && !active[p]) {                            // posterior = prior: the gradient passes straight through, the gates see nothing
        for (int c = tid; c < NS; c += nt) {
            if (g_prior_R) g_prior_R[(int64_t)p * NS + c] = (gR && c < n) ? gR[c] : 0.f;
            if (g_prior_C) g_prior_C[(int64_t)p * NS + c] = (gC && c < n) ? gC[c] : 0.f;
        }
        if (gt)
            for (int e = tid; e < NS * NS; e += nt) gt[e] = 0.f;
        if (tid < 36) sc[tid] = 0.f;
        return;
    }
    const GateW GR = gate_load(gate_R), GC = gate_load(gate_C);
    const GateNeg N = gate_neg_load(neg, any_neg, p);
    const GateQuant QR = gate_quant_load(quant_R, p, identity_forall), QC = gate_quant_load(quant_C, p, identity_forall);
    float accR[18], accC[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) accR[k] = accC[k] = 0.f;

    // sweep 1
    for (int c0 = 0; c0 < NS; c0 += 64) {
        const int c = c0 + lane;
        float t_acc = 0.f;
        const float pc = c < n ? pC[c] : 0.f;
        float zbc[6];
        gate_zb(GC, pc, zbc);
        const float ebc = dfol_exp(pc);
        for (int r = w; r < n; r += nw) {
            float s_part = 0.f;
            if (c < n && c != r) {
                const float v = gate_prep(tp[(int64_t)r * NS + c], N), ea = dfol_exp(v);
                if (gR) s_part = dfol_slog(fmaf(QC.kf, gate_m(GC, v, ea, zbc, ebc), QC.qf));
                if (gC) {
                    float zbr[6];
                    gate_zb(GR, pR[r], zbr);
                    t_acc += dfol_slog(fmaf(QR.kf, gate_m(GR, v, ea, zbr, dfol_exp(pR[r])), QR.qf));
                }
            }
            s_part = dfol_wave_sum(s_part);
            if (lane == 0) sS[r] = (c0 == 0 ? 0.f : sS[r]) + s_part;
        }
        if (c < NS) part(w, c) = t_acc;
    }
    __syncthreads();
    // the outer gates: G_R(F_C(S[i]), prior_R[i]) and G_C(F_R(T[i]), prior_C[i])
    for (int i = tid; i < n; i += nt) {
        float T = part(0, i);
        for (int j = 1; j < nw; ++j) T += part(j, i);
        float dS = 0.f, dT = 0.f, dbr = 0.f, dbc = 0.f;
        if (gR) {
            const float S = sS[i], a = QC.ident ? S : dfol_pnot(S, QC.qf, QC.kf);
            float da;
            gate_bwd(GR, a, pR[i], gR[i], true, da, dbr, accR);
            dS = da * (QC.ident ? 1.f : gate_dpnot(S, QC.qf, QC.kf));
        }
        if (gC) {
            const float a = QR.ident ? T : dfol_pnot(T, QR.qf, QR.kf);
            float da;
            gate_bwd(GC, a, pC[i], gC[i], true, da, dbc, accC);
            dT = da * (QR.ident ? 1.f : gate_dpnot(T, QR.qf, QR.kf));
        }
        sGR[i] = dS;
        sGC[i] = dT;
        sDR[i] = dbr;
        sDC[i] = dbc;
    }
    __syncthreads();
    // sweep 2
    for (int c0 = 0; c0 < NS; c0 += 64) {
        const int c = c0 + lane;
        float dpc = 0.f;
        const float pc = c < n ? pC[c] : 0.f;
        const float gcc = c < n ? sGC[c] : 0.f;
        for (int r = w; r < NS; r += nw) {
            float dl = 0.f, dpr_part = 0.f;
            if (r < n && c < n && c != r) {
                const float raw = tp[(int64_t)r * NS + c];
                const float v = gate_prep(raw, N), ea = dfol_exp(v);
                float dv = 0.f;
                if (gR) {                                      // t = log(max(qC + kC m, eps)), m = e^G_C(v, pc)
                    float zb[6];
                    gate_zb(GC, pc, zb);
                    const float u = fmaf(QC.kf, gate_m(GC, v, ea, zb, dfol_exp(pc)), QC.qf);
                    const float dm = u > DFOL_EPS ? sGR[r] * QC.kf / u : 0.f;
                    float da, db;
                    gate_bwd(GC, v, pc, dm, false, da, db, accC);
                    dv += da;
                    dpc += db;
                }
                if (gC) {
                    const float pr = pR[r];
                    float zb[6];
                    gate_zb(GR, pr, zb);
                    const float u = fmaf(QR.kf, gate_m(GR, v, ea, zb, dfol_exp(pr)), QR.qf);
                    const float dm = u > DFOL_EPS ? gcc * QR.kf / u : 0.f;
                    float da, db;
                    gate_bwd(GR, v, pr, dm, false, da, db, accR);
                    dv += da;
                    dpr_part = db;
                }
                dl = dv * gate_dprep(raw, N);
            }
            if (gt && c < NS) gt[(int64_t)r * NS + c] = dl;
            if (g_prior_R) {                                   // row totals over the column chunks collect in LDS (sS is free by now)
                dpr_part = dfol_wave_sum(dpr_part);
                if (lane == 0 && r < n) sS[r] = (c0 == 0 ? sDR[r] : sS[r]) + dpr_part;
            }
        }
        if (c < NS) part(w, c) = dpc;
    }
    gate_param_sums(accR, accC, wsum, sc);                 // (its barrier also publishes sweep 2's sS and part)
    for (int c = tid; c < NS; c += nt) {
        if (g_prior_C) {
            float t = part(0, c);
            for (int j = 1; j < nw; ++j) t += part(j, c);
            g_prior_C[(int64_t)p * NS + c] = c < n ? t + sDC[c] : 0.f;
        }
        if (g_prior_R) g_prior_R[(int64_t)p * NS + c] = c < n ? sS[c] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------
// relate, single posterior (the gated form of relate_one_fwd_kernel, dfol_logic.hip): the three gates of GQARelateBatch and the arity-2
// cell in one launch, only the kept posterior written.  The tile comes with prev's objects along rows: the column sweep.
// ---------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void relate_one_gate_fwd_kernel(
    const float* __restrict__ x_att, const float* __restrict__ prev_att, const float* __restrict__ tile, const int32_t* __restrict__ pred_q,
    const int32_t* __restrict__ n_obj, const float* __restrict__ quant_prev, const uint8_t* __restrict__ x_is_subject,
    const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int P, int NS, int identity_forall,
    const float* __restrict__ gate_s, const float* __restrict__ gate_o, float* __restrict__ post) {
    // (the predicate is the same for the whole wavefront: said so, everything derived from it - the gates' 36 parameters among it - is scalar)
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    GatePred<> g;
    if (!gate_pred_load(g, p, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, any_neg, active, NS, identity_forall, gate_s,
                        gate_o, post)) {
        gate_passthrough(g, lane, 64);
        return;
    }
    gate_col_sweep<LPR, 4>(g, lane);
}

// NS > 256, as relate_one_big_kernel
__global__ __launch_bounds__(256) void relate_one_gate_big_kernel(
    const float* __restrict__ x_att, const float* __restrict__ prev_att, const float* __restrict__ tile, const int32_t* __restrict__ pred_q,
    const int32_t* __restrict__ n_obj, const float* __restrict__ quant_prev, const uint8_t* __restrict__ x_is_subject,
    const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int NS, int identity_forall,
    const float* __restrict__ gate_s, const float* __restrict__ gate_o, float* __restrict__ post) {
    const int p = blockIdx.x, tid = threadIdx.x;
    GatePred<> g;
    if (!gate_pred_load(g, p, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, any_neg, active, NS, identity_forall, gate_s,
                        gate_o, post)) {
        gate_passthrough(g, tid, 256);
        return;
    }
    gate_big_cols(g, tid);
}

// The same one posterior on bf16 tiles (relation_tile_dtype: bf16 with trainable_gate: True, DFOL_GATE_BF16=1; NS a multiple of 8, <= 256): the
// geometry of relate_one_bf16_kernel (dfol_logic.hip) - a lane owns EIGHT consecutive columns, LPR = NS / 8 lanes cover a row - around the
// same column sweep, term for term.  Only the stored likelihoods are rounded; which rows share a lane differs from the fp32 kernel, so the two
// agree to rounding, not to the bit.
template <int LPR>
__global__ __launch_bounds__(256) void relate_one_gate_bf16_kernel(
    const float* __restrict__ x_att, const float* __restrict__ prev_att, const uint16_t* __restrict__ tile, const int32_t* __restrict__ pred_q,
    const int32_t* __restrict__ n_obj, const float* __restrict__ quant_prev, const uint8_t* __restrict__ x_is_subject,
    const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int P, int NS, int identity_forall,
    const float* __restrict__ gate_s, const float* __restrict__ gate_o, float* __restrict__ post) {
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));      // (wave-uniform: the gates' 36 parameters stay scalar)
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    GatePred<uint16_t> g;
    if (!gate_pred_load(g, p, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, any_neg, active, NS, identity_forall, gate_s,
                        gate_o, post)) {
        gate_passthrough(g, lane, 64);
        return;
    }
    gate_col_sweep<LPR, 8>(g, lane);
}

// ---------------------------------------------------------------------------------------------------
// relate, single posterior, on the SUBJECT-ROW tile of the train step (oracle.block_likelihood stores subjects along rows for every
// predicate; the inference prefetch that turns prev's objects onto the rows does not run under autograd).  The predicate's flag picks,
// wave-uniformly, which axis is summed out:
//     x_is_subject[p]:  prev along columns: row aggregates      (inner gate_o, outer gate_s)
//     otherwise:        prev along rows: column aggregates      (inner gate_s, outer gate_o)
// The column branch is gate_col_sweep's loop; the row branch is the row half of relate_gate_fwd_kernel (a column's prev, e^prev and share of
// the pre-activations once per wavefront, the row aggregate by the group reduction, the outer gate in the lane that owns the row).  Both are
// written out here and not taken from the shared helpers: that form measured 2 - 3 % slower at the same bits (see the top of the file).
// ---------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void relate_keep_gate_fwd_kernel(
    const float* __restrict__ x_att, const float* __restrict__ prev_att, const float* __restrict__ tile, const int32_t* __restrict__ pred_q,
    const int32_t* __restrict__ n_obj, const float* __restrict__ quant_prev, const uint8_t* __restrict__ x_is_subject,
    const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int P, int NS, int identity_forall,
    const float* __restrict__ gate_s, const float* __restrict__ gate_o, float* __restrict__ post) {
    constexpr int RPI = 64 / LPR;
    __shared__ float row_agg[4][256];
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    const int q = pred_q[p];
    const int n = min(n_obj[q], NS);
    const float* pv = prev_att + (int64_t)q * NS;
    const float* xv = x_att + (int64_t)p * NS;
    float* out = post + (int64_t)p * NS;
    if (active && !active[p]) {                         // question without this operator: attention passes through
        for (int c = lane; c < NS; c += 64) out[c] = c < n ? pv[c] : 0.f;
        return;
    }
    const bool xs = x_is_subject[p] != 0;
    const GateW GI = gate_load(xs ? gate_o : gate_s), GO = gate_load(xs ? gate_s : gate_o);      // inner: prev's axis, outer: x's
    const int cg = lane % LPR, rs = lane / LPR, c0 = cg * 4, cl = min(c0, NS - 4);               // (lanes beyond the width read a valid column)
    const GateNeg N = gate_neg_load(neg, any_neg, p);
    const GateQuant Q = gate_quant_load(quant_prev, p, identity_forall);
    const bool ex = Q.ex;
    const float* tp = tile + (int64_t)p * NS * NS;
    if (xs) {                                           // prev along columns: row aggregates
        const float4 pc4 = *reinterpret_cast<const float4*>(pv + cl);
        const float pc[4] = {pc4.x, pc4.y, pc4.z, pc4.w};
        float zbC[4][6], ebC[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gate_zb(GI, pc[j], zbC[j]);
            ebC[j] = dfol_exp(pc[j]);
        }
        for (int r0 = 0; r0 < n; r0 += RPI) {
            const int r = r0 + rs, rc = min(r, n - 1);
            const float4 t4 = *reinterpret_cast<const float4*>(tp + (int64_t)rc * NS + cl);
            const float l[4] = {t4.x, t4.y, t4.z, t4.w};
            float racc = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j;
                const bool keep = r < n && c < n && c != r;
                const float v = gate_prep(l[j], N);
                const float t = gate_term(gate_m(GI, v, dfol_exp(v), zbC[j], ebC[j]), Q);
                racc = gate_join(racc, keep ? t : 0.f, ex);
            }
            racc = ex ? dfol_group_or<LPR>(racc) : dfol_group_sum<LPR>(racc);
            if (cg == LPR - 1 && r < n) row_agg[wave_in_block][r] = racc;
        }
        __builtin_amdgcn_wave_barrier();                 // LDS is in order within a wavefront; this only pins the schedule
        for (int c = lane; c < NS; c += 64) {
            float o = 0.f;
            if (c < n) o = gate_log(GO, gate_outer(row_agg[wave_in_block][c], Q), xv[c]);
            out[c] = o;
        }
        return;
    }
    float cacc[4] = {0.f, 0.f, 0.f, 0.f};               // prev along rows: column aggregates, in registers
    for (int r0 = 0; r0 < n; r0 += RPI) {
        const int r = r0 + rs, rc = min(r, n - 1);
        const float4 t4 = *reinterpret_cast<const float4*>(tp + (int64_t)rc * NS + cl);
        const float l[4] = {t4.x, t4.y, t4.z, t4.w};
        const float pr = pv[rc];
        float zb[6];
        gate_zb(GI, pr, zb);
        const float eb = dfol_exp(pr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            const bool keep = r < n && c < n && c != r;
            const float v = gate_prep(l[j], N);
            const float t = gate_term(gate_m(GI, v, dfol_exp(v), zb, eb), Q);
            cacc[j] = gate_join(cacc[j], keep ? t : 0.f, ex);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int m = 32; m >= LPR; m >>= 1) cacc[j] = gate_join(cacc[j], __shfl_xor(cacc[j], m, 64), ex);
    }
    if (rs == 0 && c0 < NS) {
        const float4 x4 = *reinterpret_cast<const float4*>(xv + c0);
        const float xj[4] = {x4.x, x4.y, x4.z, x4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (c0 + j < n) ? gate_log(GO, gate_outer(cacc[j], Q), xj[j]) : 0.f;
        *reinterpret_cast<float4*>(out + c0) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// NS > 256, as relate_gate_big_fwd_kernel
__global__ __launch_bounds__(256) void relate_keep_gate_big_kernel(
    const float* __restrict__ x_att, const float* __restrict__ prev_att, const float* __restrict__ tile, const int32_t* __restrict__ pred_q,
    const int32_t* __restrict__ n_obj, const float* __restrict__ quant_prev, const uint8_t* __restrict__ x_is_subject,
    const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int NS, int identity_forall,
    const float* __restrict__ gate_s, const float* __restrict__ gate_o, float* __restrict__ post) {
    __shared__ float part[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    GatePred<> g;
    if (!gate_pred_load(g, p, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, any_neg, active, NS, identity_forall, gate_s,
                        gate_o, post)) {
        gate_passthrough(g, tid, 256);
        return;
    }
    if (g.xs) gate_big_rows(g, part, tid);               // (xs is the workgroup's: every thread reaches the barriers)
    else gate_big_cols(g, tid);
}

// ---------------------------------------------------------------------------------------------------
// backward of the single posterior on the subject-row tile: relate_gate_bwd_kernel's scheme (a workgroup per predicate, its wavefronts on rows
// r = w, w + waves, ..., lane = column) restricted to the kept direction.  Sweep 1 recomputes the one aggregate as written (sum of logs, EXISTS
// too), the outer gate is differentiated by the thread that owns the element, sweep 2 takes the element gates.  Every thread keeps the 2 x 18
// parameter sums of its elements (inner and outer gate); the workgroup's total goes to scratch[p][36] as [axis 0's 18 | axis 1's 18], the halves
// picked by the predicate's flag, and gate_param_reduce_kernel adds the rows.
// ---------------------------------------------------------------------------------------------------
constexpr int KB_WAVES = 8;
__global__ __launch_bounds__(64 * KB_WAVES) void relate_keep_gate_bwd_kernel(
    const float* __restrict__ g_post, const float* __restrict__ x_att, const float* __restrict__ prev_att, const float* __restrict__ tile,
    const int32_t* __restrict__ pred_q, const int32_t* __restrict__ n_obj, const float* __restrict__ quant_prev,
    const uint8_t* __restrict__ x_is_subject, const uint8_t* __restrict__ neg, int any_neg, const uint8_t* __restrict__ active, int NS,
    int identity_forall, const float* __restrict__ gate_s, const float* __restrict__ gate_o, float* __restrict__ scratch,
    float* __restrict__ g_x, float* __restrict__ g_prev, float* __restrict__ g_tile) {
    extern __shared__ float keep_bwd_lds[];              // (2 + waves) NS floats + waves x 36
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, tid = threadIdx.x, nw = (int)blockDim.x >> 6, nt = (int)blockDim.x;
    float* sA = keep_bwd_lds;                             // x on rows: the row aggregates; x on columns: the rows' prev gradients (sweep 2)
    float* sG = sA + NS;                                  // d loss / d aggregate
    float* part_base = sG + NS;                           // x on columns: the column aggregates' partials; x on rows: the columns' prev gradients
    float* wsum = part_base + (size_t)nw * NS;            // [nw][36]
    auto part = [&](int wave, int c) -> float& { return part_base[wave * NS + c]; };
    const int p = blockIdx.x;
    const float* gp = g_post + (int64_t)p * NS;
    float* gt = g_tile + (int64_t)p * NS * NS;
    float* gx = g_x + (int64_t)p * NS;
    float* gpv = g_prev + (int64_t)p * NS;
    float* sc = scratch + (int64_t)p * 36;
    GatePred<> g;
    if (!gate_pred_load(g, p, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, any_neg, active, NS, identity_forall, gate_s,
                        gate_o, (float*)nullptr)) {        // posterior = prev: the gradient passes straight through, the gates see nothing
        for (int c = tid; c < NS; c += nt) {
            gpv[c] = c < g.n ? gp[c] : 0.f;
            gx[c] = 0.f;
        }
        for (int e = tid; e < NS * NS; e += nt) gt[e] = 0.f;
        if (tid < 36) sc[tid] = 0.f;
        return;
    }
    const int n = g.n;
    const float *pv = g.pv, *xv = g.xv, *tp = g.tp;
    const bool xs = g.xs;                                  // (the workgroup's: every branch on it is uniform)
    const GateW &GI = g.GI, &GO = g.GO;
    const float qf = g.Q.qf, kf = g.Q.kf;
    const bool ident = g.Q.ident;
    float accI[18], accO[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) accI[k] = accO[k] = 0.f;

    // sweep 1: the aggregate over prev's axis
    for (int c0 = 0; c0 < NS; c0 += 64) {
        const int c = c0 + lane;
        if (xs) {                                          // S[r] = sum_c F(G_in(l'[r][c], prev[c]))
            const float pc = c < n ? pv[c] : 0.f;
            float zbc[6];
            gate_zb(GI, pc, zbc);
            const float ebc = dfol_exp(pc);
            for (int r = w; r < n; r += nw) {
                float s_part = 0.f;
                if (c < n && c != r) {
                    const float v = gate_prep(tp[(int64_t)r * NS + c], g.N);
                    s_part = dfol_slog(fmaf(kf, gate_m(GI, v, dfol_exp(v), zbc, ebc), qf));
                }
                s_part = dfol_wave_sum(s_part);
                if (lane == 0) sA[r] = (c0 == 0 ? 0.f : sA[r]) + s_part;
            }
        } else {                                           // T[c] = sum_r F(G_in(l'[r][c], prev[r]))
            float t_acc = 0.f;
            for (int r = w; r < n; r += nw) {
                if (c < n && c != r) {
                    const float v = gate_prep(tp[(int64_t)r * NS + c], g.N);
                    const float pr = pv[r];
                    float zbr[6];
                    gate_zb(GI, pr, zbr);
                    t_acc += dfol_slog(fmaf(kf, gate_m(GI, v, dfol_exp(v), zbr, dfol_exp(pr)), qf));
                }
            }
            if (c < NS) part(w, c) = t_acc;
        }
    }
    __syncthreads();
    // the outer gate G_out(F(A[i]), x[i]), by the thread that owns element i
    for (int i = tid; i < NS; i += nt) {
        float dA = 0.f, dx = 0.f;
        if (i < n) {
            float A;
            if (xs) {
                A = sA[i];
            } else {
                A = part(0, i);
                for (int j = 1; j < nw; ++j) A += part(j, i);
            }
            const float a = ident ? A : dfol_pnot(A, qf, kf);
            float da;
            gate_bwd(GO, a, xv[i], gp[i], true, da, dx, accO);
            dA = da * (ident ? 1.f : gate_dpnot(A, qf, kf));
        }
        sG[i] = dA;
        gx[i] = dx;
    }
    __syncthreads();
    // sweep 2: the element gates
    for (int c0 = 0; c0 < NS; c0 += 64) {
        const int c = c0 + lane;
        if (xs) {
            const float pc = c < n ? pv[c] : 0.f;
            float zbc[6];
            gate_zb(GI, pc, zbc);
            const float ebc = dfol_exp(pc);
            float dpc = 0.f;
            for (int r = w; r < NS; r += nw) {
                float dl = 0.f;
                if (r < n && c < n && c != r) {            // t = log(max(q + k m, eps)), m = e^G_in(v, prev[c])
                    const float raw = tp[(int64_t)r * NS + c];
                    const float v = gate_prep(raw, g.N);
                    const float u = fmaf(kf, gate_m(GI, v, dfol_exp(v), zbc, ebc), qf);
                    const float dm = u > DFOL_EPS ? sG[r] * kf / u : 0.f;
                    float da, db;
                    gate_bwd(GI, v, pc, dm, false, da, db, accI);
                    dpc += db;
                    dl = da * gate_dprep(raw, g.N);
                }
                if (c < NS) gt[(int64_t)r * NS + c] = dl;
            }
            if (c < NS) part(w, c) = dpc;
        } else {
            const float gcc = c < n ? sG[c] : 0.f;
            for (int r = w; r < NS; r += nw) {
                float dl = 0.f, dpr = 0.f;
                if (r < n && c < n && c != r) {
                    const float raw = tp[(int64_t)r * NS + c];
                    const float v = gate_prep(raw, g.N);
                    const float pr = pv[r];
                    float zbr[6];
                    gate_zb(GI, pr, zbr);
                    const float u = fmaf(kf, gate_m(GI, v, dfol_exp(v), zbr, dfol_exp(pr)), qf);
                    const float dm = u > DFOL_EPS ? gcc * kf / u : 0.f;
                    float da;
                    gate_bwd(GI, v, pr, dm, false, da, dpr, accI);
                    dl = da * gate_dprep(raw, g.N);
                }
                if (c < NS) gt[(int64_t)r * NS + c] = dl;
                dpr = dfol_wave_sum(dpr);                  // row totals over the column chunks collect in LDS
                if (lane == 0 && r < n) sA[r] = (c0 == 0 ? 0.f : sA[r]) + dpr;
            }
        }
    }
    float acc0[18], acc1[18];                              // axis 0's gate first
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        acc0[k] = xs ? accO[k] : accI[k];
        acc1[k] = xs ? accI[k] : accO[k];
    }
    gate_param_sums(acc0, acc1, wsum, sc);                 // (its barrier also publishes sweep 2's sA and part)
    for (int c = tid; c < NS; c += nt) {
        float t = 0.f;
        if (c < n) {
            if (xs) {
                t = part(0, c);
                for (int j = 1; j < nw; ++j) t += part(j, c);
            } else {
                t = sA[c];
            }
        }
        gpv[c] = t;
    }
}

}      // namespace

extern "C" int dfol_filter_gate_fwd_f32(const float* att_in, const float* ll, const int32_t* pred_q, const int32_t* n_obj, const uint8_t* neg,
                                        int32_t any_neg, const uint8_t* active, int32_t P, int32_t NS, const float* gate, float* att_out,
                                        void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0, "filter_gate_fwd: bad sizes P=%d NS=%d", P, NS);
    if (P == 0) return 0;
    DFOL_REQUIRE(att_in && ll && pred_q && n_obj && gate && att_out, "filter_gate_fwd: null pointer");
    DFOL_REQUIRE(!any_neg || neg, "filter_gate_fwd: any_neg set but neg is NULL");
    const int64_t total4 = (int64_t)P * (NS / 4);
    hipLaunchKernelGGL(filter_gate_fwd_kernel, dim3(dfol_cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream, att_in, ll, pred_q, n_obj, neg,
                       any_neg, active, total4, NS / 4, gate, att_out);
    DFOL_LAUNCH_CHECK("filter_gate_fwd");
    return 0;
}

extern "C" int64_t dfol_filter_gate_bwd_scratch(int32_t P, int32_t NS) {
    return P <= 0 || NS <= 0 ? 0 : (int64_t)dfol_cdiv((int64_t)P * NS, FG_THREADS) * 18;
}

extern "C" int dfol_filter_gate_bwd_f32(const float* g_out, const float* att_in, const float* ll, const int32_t* pred_q, const int32_t* n_obj,
                                        const uint8_t* neg, int32_t any_neg, const uint8_t* active, int32_t P, int32_t NS, const float* gate,
                                        float* scratch, float* g_prior, float* g_ll, float* g_gate, void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0, "filter_gate_bwd: bad sizes P=%d NS=%d", P, NS);
    DFOL_REQUIRE(g_gate, "filter_gate_bwd: null pointer (g_gate)");
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) {
        hipLaunchKernelGGL(gate_param_reduce_kernel, dim3(18), dim3(64), 0, st, (const float*)nullptr, (int64_t)0, 18, g_gate, (float*)nullptr);
        DFOL_LAUNCH_CHECK("filter_gate_bwd (reduce)");
        return 0;
    }
    DFOL_REQUIRE(g_out && att_in && ll && pred_q && n_obj && gate && scratch, "filter_gate_bwd: null pointer");
    DFOL_REQUIRE(!any_neg || neg, "filter_gate_bwd: any_neg set but neg is NULL");
    const int64_t total = (int64_t)P * NS;
    const int blocks = dfol_cdiv(total, FG_THREADS);
    hipLaunchKernelGGL(filter_gate_bwd_kernel, dim3(blocks), dim3(FG_THREADS), 0, st, g_out, att_in, ll, pred_q, n_obj, neg, any_neg, active, total,
                       NS, gate, scratch, g_prior, g_ll);
    DFOL_LAUNCH_CHECK("filter_gate_bwd");
    hipLaunchKernelGGL(gate_param_reduce_kernel, dim3(18), dim3(64), 0, st, (const float*)scratch, (int64_t)blocks, 18, g_gate, (float*)nullptr);
    DFOL_LAUNCH_CHECK("filter_gate_bwd (reduce)");
    return 0;
}

extern "C" int dfol_relate_gate_fwd_f32(const float* prior_s, const float* prior_o, const float* tile, const int32_t* pred_q,
                                        const int32_t* n_obj, const float* quant_s, const float* quant_o, const uint8_t* neg, int32_t any_neg,
                                        const uint8_t* active, const uint8_t* want, int32_t P, int32_t NS, int32_t orientation, int32_t flags,
                                        const float* gate_s, const float* gate_o, float* post_s, float* post_o, void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0, "relate_gate_fwd: bad sizes P=%d NS=%d (NS: a multiple of 4)", P, NS);
    DFOL_REQUIRE(orientation == 0 || orientation == 1, "relate_gate_fwd: bad orientation %d", orientation);
    if (P == 0) return 0;
    DFOL_REQUIRE(prior_s && prior_o && tile && pred_q && n_obj && quant_s && quant_o && gate_s && gate_o, "relate_gate_fwd: null pointer");
    DFOL_REQUIRE(post_s || post_o, "relate_gate_fwd: no output requested");
    DFOL_REQUIRE(!any_neg || neg, "relate_gate_fwd: any_neg set but neg is NULL");
    const bool sr = orientation == DFOL_TILE_SUBJECT_ROWS;
    const float *pR = sr ? prior_s : prior_o, *pC = sr ? prior_o : prior_s;
    const float *qR = sr ? quant_s : quant_o, *qC = sr ? quant_o : quant_s;
    const float *gR = sr ? gate_s : gate_o, *gC = sr ? gate_o : gate_s;
    float *oR = sr ? post_s : post_o, *oC = sr ? post_o : post_s;
    const int bR = sr ? DFOL_WANT_SUBJECT : DFOL_WANT_OBJECT, bC = sr ? DFOL_WANT_OBJECT : DFOL_WANT_SUBJECT;
    hipStream_t st = (hipStream_t)stream;
    if (NS > 256) {
        hipLaunchKernelGGL(relate_gate_big_fwd_kernel, dim3(P), dim3(256), 0, st, pR, pC, tile, pred_q, n_obj, qR, qC, neg, any_neg, active, want,
                           bR, bC, NS, flags, gR, gC, oR, oC);
        DFOL_LAUNCH_CHECK("relate_gate_fwd (NS > 256)");
        return 0;
    }
    dfol_dispatch_lpr(NS / 4, [&](auto lpr) {
        hipLaunchKernelGGL(relate_gate_fwd_kernel<decltype(lpr)::value>, dim3(dfol_cdiv(P, 4)), dim3(256), 0, st, pR, pC, tile, pred_q, n_obj, qR, qC, neg,
                           any_neg, active, want, bR, bC, P, NS, flags, gR, gC, oR, oC);
    });
    DFOL_LAUNCH_CHECK("relate_gate_fwd");
    return 0;
}

extern "C" int dfol_relate_one_gate_fwd_f32(const float* x_att, const float* prev_att, const float* tile, const int32_t* pred_q,
                                            const int32_t* n_obj, const float* quant_prev, const uint8_t* x_is_subject, const uint8_t* neg,
                                            int32_t any_neg, const uint8_t* active, int32_t P, int32_t NS, int32_t lone_forall_identity,
                                            const float* gate_s, const float* gate_o, float* post, void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0, "relate_one_gate_fwd: bad sizes P=%d NS=%d (NS: a multiple of 4)", P, NS);
    if (P == 0) return 0;
    DFOL_REQUIRE(x_att && prev_att && tile && pred_q && n_obj && quant_prev && x_is_subject && gate_s && gate_o && post,
                 "relate_one_gate_fwd: null pointer");
    DFOL_REQUIRE(!any_neg || neg, "relate_one_gate_fwd: any_neg set but neg is NULL");
    hipStream_t st = (hipStream_t)stream;
    if (NS > 256) {
        hipLaunchKernelGGL(relate_one_gate_big_kernel, dim3(P), dim3(256), 0, st, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg,
                           any_neg, active, NS, lone_forall_identity, gate_s, gate_o, post);
        DFOL_LAUNCH_CHECK("relate_one_gate_fwd (NS > 256)");
        return 0;
    }
    dfol_dispatch_lpr(NS / 4, [&](auto lpr) {
        hipLaunchKernelGGL(relate_one_gate_fwd_kernel<decltype(lpr)::value>, dim3(dfol_cdiv(P, 4)), dim3(256), 0, st, x_att, prev_att, tile, pred_q,
                           n_obj, quant_prev, x_is_subject, neg, any_neg, active, P, NS, lone_forall_identity, gate_s, gate_o, post);
    });
    DFOL_LAUNCH_CHECK("relate_one_gate_fwd");
    return 0;
}

extern "C" int dfol_relate_one_gate_fwd_bf16(const float* x_att, const float* prev_att, const uint16_t* tile, const int32_t* pred_q,
                                             const int32_t* n_obj, const float* quant_prev, const uint8_t* x_is_subject, const uint8_t* neg,
                                             int32_t any_neg, const uint8_t* active, int32_t P, int32_t NS, int32_t lone_forall_identity,
                                             const float* gate_s, const float* gate_o, float* post, void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 8 == 0 && NS <= 256, "relate_one_gate_fwd_bf16: bad sizes P=%d NS=%d (NS: multiple of 8, <= 256)", P, NS);
    if (P == 0) return 0;
    DFOL_REQUIRE(x_att && prev_att && tile && pred_q && n_obj && quant_prev && x_is_subject && gate_s && gate_o && post,
                 "relate_one_gate_fwd_bf16: null pointer");
    DFOL_REQUIRE(!any_neg || neg, "relate_one_gate_fwd_bf16: any_neg set but neg is NULL");
    hipStream_t st = (hipStream_t)stream;
    dfol_dispatch_lpr<32>(NS / 8, [&](auto lpr) {
        hipLaunchKernelGGL(relate_one_gate_bf16_kernel<decltype(lpr)::value>, dim3(dfol_cdiv(P, 4)), dim3(256), 0, st, x_att, prev_att, tile, pred_q,
                           n_obj, quant_prev, x_is_subject, neg, any_neg, active, P, NS, lone_forall_identity, gate_s, gate_o, post);
    });
    DFOL_LAUNCH_CHECK("relate_one_gate_fwd_bf16");
    return 0;
}

extern "C" int dfol_relate_gate_bwd_f32(const float* prior_s, const float* prior_o, const float* tile, const int32_t* pred_q,
                                        const int32_t* n_obj, const float* quant_s, const float* quant_o, const uint8_t* neg, int32_t any_neg,
                                        const uint8_t* active, const float* g_post_s, const float* g_post_o, int32_t P, int32_t NS,
                                        int32_t orientation, int32_t lone_forall_identity, const float* gate_s, const float* gate_o,
                                        float* scratch, float* g_prior_s, float* g_prior_o, float* g_tile, float* g_gate_s, float* g_gate_o,
                                        void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0 && NS <= 1024, "relate_gate_bwd: bad sizes P=%d NS=%d (NS: a multiple of 4, <= 1024)", P, NS);
    DFOL_REQUIRE(orientation == 0 || orientation == 1, "relate_gate_bwd: bad orientation");
    DFOL_REQUIRE(g_gate_s && g_gate_o, "relate_gate_bwd: null pointer (g_gate)");
    const bool sr = orientation == DFOL_TILE_SUBJECT_ROWS;
    hipStream_t st = (hipStream_t)stream;
    if (P > 0) {
        DFOL_REQUIRE(prior_s && prior_o && tile && pred_q && n_obj && quant_s && quant_o && gate_s && gate_o && scratch && (g_post_s || g_post_o),
                     "relate_gate_bwd: null pointer");
        DFOL_REQUIRE(!any_neg || neg, "relate_gate_bwd: any_neg set but neg is NULL");
        // (5 + waves) NS floats of rows / columns and waves x 36 of parameter sums: eight wavefronts while that stays within 48 KB, else four
        // (NS <= 1024: 37.4 KB)
        auto lds_bytes = [NS](int waves) { return ((size_t)(5 + waves) * NS + (size_t)waves * 36) * sizeof(float); };
        const int waves = lds_bytes(GB_WAVES) <= 48 * 1024 ? GB_WAVES : 4;
        const size_t lds = lds_bytes(waves);
        hipLaunchKernelGGL(relate_gate_bwd_kernel, dim3(P), dim3(64 * waves), lds, st, sr ? prior_s : prior_o, sr ? prior_o : prior_s, tile, pred_q,
                           n_obj, sr ? quant_s : quant_o, sr ? quant_o : quant_s, neg, any_neg, active, sr ? g_post_s : g_post_o,
                           sr ? g_post_o : g_post_s, NS, lone_forall_identity, sr ? gate_s : gate_o, sr ? gate_o : gate_s, scratch,
                           sr ? g_prior_s : g_prior_o, sr ? g_prior_o : g_prior_s, g_tile);
        DFOL_LAUNCH_CHECK("relate_gate_bwd");
    }
    hipLaunchKernelGGL(gate_param_reduce_kernel, dim3(36), dim3(64), 0, st, (const float*)scratch, (int64_t)P, 36, sr ? g_gate_s : g_gate_o,
                       sr ? g_gate_o : g_gate_s);
    DFOL_LAUNCH_CHECK("relate_gate_bwd (reduce)");
    return 0;
}

extern "C" int dfol_relate_keep_gate_fwd_f32(const float* x_att, const float* prev_att, const float* tile, const int32_t* pred_q,
                                             const int32_t* n_obj, const float* quant_prev, const uint8_t* x_is_subject, const uint8_t* neg,
                                             int32_t any_neg, const uint8_t* active, int32_t P, int32_t NS, int32_t lone_forall_identity,
                                             const float* gate_s, const float* gate_o, float* post, void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0, "relate_keep_gate_fwd: bad sizes P=%d NS=%d (NS: a multiple of 4)", P, NS);
    if (P == 0) return 0;
    DFOL_REQUIRE(x_att && prev_att && tile && pred_q && n_obj && quant_prev && x_is_subject && gate_s && gate_o && post,
                 "relate_keep_gate_fwd: null pointer");
    DFOL_REQUIRE(!any_neg || neg, "relate_keep_gate_fwd: any_neg set but neg is NULL");
    hipStream_t st = (hipStream_t)stream;
    if (NS > 256) {
        hipLaunchKernelGGL(relate_keep_gate_big_kernel, dim3(P), dim3(256), 0, st, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg,
                           any_neg, active, NS, lone_forall_identity, gate_s, gate_o, post);
        DFOL_LAUNCH_CHECK("relate_keep_gate_fwd (NS > 256)");
        return 0;
    }
    dfol_dispatch_lpr(NS / 4, [&](auto lpr) {
        hipLaunchKernelGGL(relate_keep_gate_fwd_kernel<decltype(lpr)::value>, dim3(dfol_cdiv(P, 4)), dim3(256), 0, st, x_att, prev_att, tile, pred_q,
                           n_obj, quant_prev, x_is_subject, neg, any_neg, active, P, NS, lone_forall_identity, gate_s, gate_o, post);
    });
    DFOL_LAUNCH_CHECK("relate_keep_gate_fwd");
    return 0;
}

extern "C" int dfol_relate_keep_gate_bwd_f32(const float* g_post, const float* x_att, const float* prev_att, const float* tile,
                                             const int32_t* pred_q, const int32_t* n_obj, const float* quant_prev, const uint8_t* x_is_subject,
                                             const uint8_t* neg, int32_t any_neg, const uint8_t* active, int32_t P, int32_t NS,
                                             int32_t lone_forall_identity, const float* gate_s, const float* gate_o, float* scratch, float* g_x,
                                             float* g_prev, float* g_tile, float* g_gate_s, float* g_gate_o, void* stream) {
    DFOL_REQUIRE(P >= 0 && NS > 0 && NS % 4 == 0 && NS <= 1024, "relate_keep_gate_bwd: bad sizes P=%d NS=%d (NS: a multiple of 4, <= 1024)", P, NS);
    DFOL_REQUIRE(g_gate_s && g_gate_o, "relate_keep_gate_bwd: null pointer (g_gate)");
    hipStream_t st = (hipStream_t)stream;
    if (P > 0) {
        DFOL_REQUIRE(g_post && x_att && prev_att && tile && pred_q && n_obj && quant_prev && x_is_subject && gate_s && gate_o && scratch && g_x &&
                         g_prev && g_tile,
                     "relate_keep_gate_bwd: null pointer");
        DFOL_REQUIRE(!any_neg || neg, "relate_keep_gate_bwd: any_neg set but neg is NULL");
        // (2 + waves) NS floats of rows / columns and waves x 36 of parameter sums (NS <= 1024: 41.2 KB)
        const size_t lds = ((size_t)(2 + KB_WAVES) * NS + (size_t)KB_WAVES * 36) * sizeof(float);
        hipLaunchKernelGGL(relate_keep_gate_bwd_kernel, dim3(P), dim3(64 * KB_WAVES), lds, st, g_post, x_att, prev_att, tile, pred_q, n_obj, quant_prev,
                           x_is_subject, neg, any_neg, active, NS, lone_forall_identity, gate_s, gate_o, scratch, g_x, g_prev, g_tile);
        DFOL_LAUNCH_CHECK("relate_keep_gate_bwd");
    }
    hipLaunchKernelGGL(gate_param_reduce_kernel, dim3(36), dim3(64), 0, st, (const float*)scratch, (int64_t)P, 36, g_gate_s, g_gate_o);
    DFOL_LAUNCH_CHECK("relate_keep_gate_bwd (reduce)");
    return 0;
}
