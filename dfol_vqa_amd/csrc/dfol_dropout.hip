// The kernels of the dropout training route: counter-based dropout masks, and the deterministic backward of the pair matrix.
//
// The reference puts nn.Dropout(p) in front of every nn.Linear of its three MLPs and of the featurizer (gqa_interpreter_experiments.py:29, 32,
// 73) and trains in train() mode.  On the full-table dataflow every one of those Dropouts acts on a tensor that exists in memory - the
// [pairs, 2(D + 4) + 4] pair matrix included - so one element-wise kernel gives the reference's semantics at every site.
//
// The mask rule.  A mask is a pure function of (seed, rank, step, site, row, column); nothing of it is ever stored.
//
//   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written out below: a counter of four
//   and a key of two 32-bit words; ten rounds of
//       (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),      M0 = 0xD2511F53, M1 = 0xCD9E8D57
//   with (k0, k1) += (0x9E3779B9, 0xBB67AE85) between rounds (nine bumps).
//
//   stream state  {seed u64, step u64, key u32[2], rank u32, pad u32}: 32 bytes on the device.
//   advance       step += 1;  key = the first two words of Philox(counter = (step_lo, step_hi, rank, 0), key = (seed_lo, seed_hi)).
//                 The step lives on the device, so a replayed graph draws new masks on every replay.
//   mask          the elements (row, 4g .. 4g + 3) of site s use the four words w[0 .. 3] of
//                     Philox(counter = (row_lo, row_hi, g, s), key = state.key);
//                 rows are 64-bit: the pair matrix of 256 images x 100 objects has 2.5M rows x 1036 columns > 2^32 elements.
//                 Element j is KEPT iff (u64)w[j] >= T,  T = floor(p 2^32) with p the fp32 argument widened to double (the product is exact):
//                 P(kept) = 1 - T / 2^32, within 2^-32 of 1 - p.
//   value         kept: y = x * scale, scale = 1.0f / (1.0f - p), one fp32 division on the host;  dropped: y = +0.0f by SELECTION, so an inf
//                 or NaN under a dropped element does not leak (0 * inf would).
//   backward      the same entry point over the incoming gradient with the same (key, site): gx = keep ? g * scale : 0.
//
// dropout_kernel: a wavefront per row (rows of fewer than 64 groups share one: `lpr` lanes each), lanes side by side over the row's groups of
// four columns, a grid-stride loop over rows.  The access width - 16, 8 or 4 bytes - follows the addresses of the row in x and in y, uniform
// over the row's lanes, as in dfol_store.hip: the featurizer's input is a view whose row stride of F + 6 floats leaves every other row only
// 8-byte aligned.  The tail group of a width that is no multiple of four uses the leading words of its group, element by element.  In place
// (x == y) is fine: a lane reads its group before it writes it, and no other lane touches that group.  No LDS, no atomics.
//
// pair_features_bwd_kernel: the backward of dfol_pair_features_f32 (dfol_dense.hip) without atomics.  Pair row of (image q, subject s, object o):
// pair_off[q] + s (n - 1) + (o < s ? o : o - 1).  Object t collects columns [0, D) of its n - 1 CONSECUTIVE rows as subject and columns [D, 2D)
// of its n - 1 STRIDED rows as object, each in ascending partner order, then adds the two sums: one fixed order, so two runs give the same bits.
#include "dfol_common.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct Philox4 {
    uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += PHILOX_W0, k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// One lane of one launch: the state is 32 bytes and the whole update a few hundred instructions.
__global__ void dropout_advance_kernel(uint32_t* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint2 seed = *reinterpret_cast<const uint2*>(state);
    uint2 step = *reinterpret_cast<const uint2*>(state + 2);
    const uint32_t rank = state[6];
    step.x += 1u;
    step.y += step.x == 0u ? 1u : 0u;
    const Philox4 k = philox4x32_10(step.x, step.y, rank, 0u, seed.x, seed.y);
    *reinterpret_cast<uint2*>(state + 2) = step;
    *reinterpret_cast<uint2*>(state + 4) = make_uint2(k.w[0], k.w[1]);
}

constexpr int DR_WAVES = 4;                 // wavefronts of a workgroup
constexpr int DR_TARGET_BLOCKS = 4096;      // workgroups of a launch when the matrix has the rows for it: 16 per CU, the loop takes the rest

__device__ __forceinline__ float dr_value(float x, uint32_t w, uint64_t thr, float scale) { return (uint64_t)w >= thr ? x * scale : 0.0f; }

// the full group g of one row; AW = floats per access
template <int AW>
__device__ __forceinline__ void dr_group(const float* xr, float* yr, int g, const Philox4& r, uint64_t thr, float scale) {
    float v[4];
    if (AW == 4) {
        const float4 a = *reinterpret_cast<const float4*>(xr + 4 * g);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else if (AW == 2) {
        const float2 a = *reinterpret_cast<const float2*>(xr + 4 * g), b = *reinterpret_cast<const float2*>(xr + 4 * g + 2);
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
        v[0] = xr[4 * g], v[1] = xr[4 * g + 1], v[2] = xr[4 * g + 2], v[3] = xr[4 * g + 3];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = dr_value(v[j], r.w[j], thr, scale);
    if (AW == 4) {
        *reinterpret_cast<float4*>(yr + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (AW == 2) {
        *reinterpret_cast<float2*>(yr + 4 * g) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(yr + 4 * g + 2) = make_float2(v[2], v[3]);
    } else {
        yr[4 * g] = v[0], yr[4 * g + 1] = v[1], yr[4 * g + 2] = v[2], yr[4 * g + 3] = v[3];
    }
}

template <int AW>
__device__ __forceinline__ void dr_row(const float* xr, float* yr, int cols, int64_t row, uint32_t site, uint32_t k0, uint32_t k1, uint64_t thr,
                                       float scale, int l, int lpr) {
    const int full = cols >> 2;
    const uint32_t r_lo = (uint32_t)(uint64_t)row, r_hi = (uint32_t)((uint64_t)row >> 32);
    for (int g = l; g < full; g += lpr) dr_group<AW>(xr, yr, g, philox4x32_10(r_lo, r_hi, (uint32_t)g, site, k0, k1), thr, scale);
    const int tail = cols & 3;
    if (tail && (full % lpr) == l) {                                 // the lane whose turn the tail group would be
        const Philox4 r = philox4x32_10(r_lo, r_hi, (uint32_t)full, site, k0, k1);
        for (int j = 0; j < tail; ++j) yr[4 * full + j] = dr_value(xr[4 * full + j], r.w[j], thr, scale);
    }
}

// x and y may be the same matrix (no __restrict__)
__global__ __launch_bounds__(DR_WAVES * 64) void dropout_kernel(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int cols,
                                                                uint64_t thr, float scale, const uint32_t* __restrict__ key, uint32_t site,
                                                                int lpr) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rpw = 64 / lpr, sub = lane / lpr, l = lane & (lpr - 1);
    const uint32_t k0 = key[0], k1 = key[1];
    const int64_t step = (int64_t)gridDim.x * DR_WAVES * rpw;
    for (int64_t row = ((int64_t)blockIdx.x * DR_WAVES + wave) * rpw + sub; row < rows; row += step) {
        const float* xr = x + row * ldx;
        float* yr = y + row * ldy;
        const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(xr) | reinterpret_cast<uintptr_t>(yr)) & 15);
        if (mis == 0)
            dr_row<4>(xr, yr, cols, row, site, k0, k1, thr, scale, l, lpr);
        else if ((mis & 7) == 0)
            dr_row<2>(xr, yr, cols, row, site, k0, k1, thr, scale, l, lpr);
        else
            dr_row<1>(xr, yr, cols, row, site, k0, k1, thr, scale, l, lpr);
    }
}

// One block per (image, object t); threads side by side over the D columns, each summing its column over t's 2 (n - 1) pair rows.
constexpr int PB_THREADS = 256;

__global__ __launch_bounds__(PB_THREADS) void pair_features_bwd_kernel(const float* __restrict__ g, int64_t ld_g, int D,
                                                                       const int32_t* __restrict__ obj_off, const int64_t* __restrict__ pair_off,
                                                                       int max_n, float* __restrict__ g_obj, int64_t ld_obj) {
    const int q = blockIdx.x / max_n, t = blockIdx.x % max_n;
    const int first = obj_off[q], n = obj_off[q + 1] - first;
    if (t >= n) return;
    const int m = n - 1;                                             // partners of t (0 for an image of one object: a zero row)
    const float* base = g + pair_off[q] * ld_g;
    const float* as_subject = base + (int64_t)t * m * ld_g;          // rows t m .. t m + m - 1, partner ascending
    float* out = g_obj + (int64_t)(first + t) * ld_obj;
    for (int c = threadIdx.x; c < D; c += PB_THREADS) {
        float sum_s = 0.f, sum_o = 0.f;
#pragma unroll 4
        for (int k = 0; k < m; ++k) sum_s += as_subject[(int64_t)k * ld_g + c];
#pragma unroll 4
        for (int k = 0; k < m; ++k) {                                // k-th partner s of t as object: s = k < t ? k : k + 1, t's slot in s's rows
            const int s = k < t ? k : k + 1;
            sum_o += base[((int64_t)s * m + (t < s ? t : t - 1)) * ld_g + D + c];
        }
        out[c] = sum_s + sum_o;
    }
}

}  // namespace

extern "C" int dfol_dropout_advance(void* state, void* stream) {
    DFOL_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "dropout_advance: the state must be a 32-byte record, 8-byte aligned");
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<uint32_t*>(state));
    DFOL_LAUNCH_CHECK("dropout_advance");
    return 0;
}

extern "C" int dfol_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int32_t cols, float p, const void* key,
                                uint32_t site, void* stream) {
    DFOL_REQUIRE(rows >= 0 && cols >= 1 && ldx >= cols && ldy >= cols, "dropout: bad sizes rows=%lld cols=%d ldx=%lld ldy=%lld", (long long)rows, cols,
                 (long long)ldx, (long long)ldy);
    DFOL_REQUIRE(p >= 0.f && p < 1.f, "dropout: p=%g is not in [0, 1)", (double)p);
    if (rows == 0) return 0;
    DFOL_REQUIRE(x && y && key, "dropout: null pointer");
    DFOL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 && (reinterpret_cast<uintptr_t>(key) & 3) == 0,
                 "dropout: misaligned pointer");
    const uint64_t thr = (uint64_t)((double)p * 4294967296.0);       // floor(p 2^32): the product is exact in double
    const float scale = 1.0f / (1.0f - p);
    const int groups = dfol_cdiv(cols, 4);
    int lpr = 1;                                                     // lanes per row: a group each up to 64 groups, then the whole wavefront
    while (lpr < 64 && lpr < groups) lpr *= 2;
    const int64_t waves = (rows + 64 / lpr - 1) / (64 / lpr);
    int64_t blocks = (waves + DR_WAVES - 1) / DR_WAVES;
    blocks = blocks < DR_TARGET_BLOCKS ? blocks : DR_TARGET_BLOCKS;
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)blocks), dim3(DR_WAVES * 64), 0, (hipStream_t)stream, x, ldx, y, ldy, rows, cols, thr, scale,
                       static_cast<const uint32_t*>(key), site, lpr);
    DFOL_LAUNCH_CHECK("dropout");
    return 0;
}

extern "C" int dfol_pair_features_bwd_f32(const float* g_pair, int64_t ld_pair, int32_t D, const int32_t* obj_off, const int64_t* pair_off, int32_t Q,
                                          int32_t max_n, float* g_obj, int64_t ld_obj, void* stream) {
    DFOL_REQUIRE(Q >= 0 && D >= 1 && max_n >= 0 && ld_obj >= D && ld_pair >= 2 * (int64_t)D, "pair_features_bwd: bad sizes");
    if (Q == 0 || max_n == 0) return 0;
    DFOL_REQUIRE((int64_t)Q * max_n < (1ll << 31), "pair_features_bwd: Q * max_n = %lld blocks are more than a launch takes", (long long)Q * max_n);
    DFOL_REQUIRE(obj_off && pair_off && g_obj && (g_pair || max_n <= 1), "pair_features_bwd: null pointer");
    hipLaunchKernelGGL(pair_features_bwd_kernel, dim3((unsigned)Q * max_n), dim3(PB_THREADS), 0, (hipStream_t)stream, g_pair, ld_pair, D, obj_off,
                       pair_off, max_n, g_obj, ld_obj);
    DFOL_LAUNCH_CHECK("pair_features_bwd");
    return 0;
}
