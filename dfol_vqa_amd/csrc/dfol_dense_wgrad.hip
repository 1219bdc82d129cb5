// Weight gradient of a dense layer on the matrix cores:  dW[n][k] = sum_m dY[m][n] * X[m][k]      (dW = dY^T X, "TN" product)
//
// Training path (the reference gets it from torch autograd through nn.Linear, gqa_interpreter_experiments.py:26-33, 73-74, under
// trainer.py:436).  The contraction runs over the ROWS of two row-major matrices - millions of rows for the pair MLP (one row per
// ordered object pair) against a tiny [HID2, HID1] result - the shape vendor GEMMs handle worst (7.5 ms plain / 3.4 ms as a batched
// product for [300 x 2.5M] x [2.5M x 256]).
//
// v_mfma_f32_32x32x2_f32 takes ONE float per lane and operand: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31].
// With i = output row n, j = output column k and the MFMA's k = the row m, both operands are what a lane reads with a plain coalesced
// load: 32 consecutive floats of row m (lanes 0..31) and of row m + 1 (lanes 32..63).  No LDS, no transposes, exact fp32 (the
// matrix pipe's fmaf chain).  A wavefront owns TN x TK tiles of 32 x 32 (TN * TK * 16 accumulator registers, one wavefront per
// SIMD), so a step of two rows costs TN + TK loads for TN * TK MFMAs of 64 cycles; the next step's operands are in flight under them.
// The rows are cut into slabs, one workgroup (four wavefronts = four output blocks of the same rows, sharing them through L1 / L2)
// per slab and block group; every slab writes its partial [N, K] block and a second kernel adds the slabs in a FIXED order:
// no atomics, bit-identical from run to run.
#include "dfol_common.h"
#include "dfol_split.h"
#include "dfol_wgrad.h"

#include <stdlib.h>
#include <string.h>

#include <type_traits>

#ifndef W3B_ALIGN
#define W3B_ALIGN 1
#endif
#ifndef W3B_D
#define W3B_D 4                 // steps of rows in flight in the bf16-storage weight gradient (1..4)
#endif

template <int TN, int TK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wgrad_tn_kernel(
    const float* __restrict__ dY, int64_t ld_dy, const float* __restrict__ X, int64_t ld_x, int M, int N, int K, int rows_per_slab,
    int nb_n, int nb_k, float* __restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int blk = blockIdx.y * 4 + wave;
    if (blk >= nb_n * nb_k) return;
    const int bn = blk / nb_k, bk = blk - bn * nb_k;
    const int n0 = bn * 32 * TN, k0 = bk * 32 * TK;
    const int slab = blockIdx.x;
    const int m_begin = slab * rows_per_slab, m_end = min(M, m_begin + rows_per_slab);
    const int col = lane & 31, half = lane >> 5;

    const float* pa[TN];
    const float* pb[TK];
    bool oka[TN], okb[TK];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const int n = n0 + 32 * t + col;
        oka[t] = n < N;
        pa[t] = dY + min(n, N - 1);
    }
#pragma unroll
    for (int u = 0; u < TK; ++u) {
        const int k = k0 + 32 * u + col;
        okb[u] = k < K;
        pb[u] = X + min(k, K - 1);
    }
    f32x16 acc[TN][TK];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int u = 0; u < TK; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

    float a[TN], b[TK], an[TN], bn_[TK];
    auto load = [&](int m, float (&ra)[TN], float (&rb)[TK]) {
        const int row = m + half;
        const bool live = row < m_end;
        const int64_t r = min(row, M - 1);
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const float v = pa[t][r * ld_dy];
            ra[t] = (live && oka[t]) ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < TK; ++u) {
            const float v = pb[u][r * ld_x];
            rb[u] = (live && okb[u]) ? v : 0.f;
        }
    };
    if (m_begin < m_end) load(m_begin, a, b);
    for (int m = m_begin; m < m_end; m += 2) {
        if (m + 2 < m_end) load(m + 2, an, bn_);            // in flight under this step's MFMAs
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int u = 0; u < TK; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[u], acc[t][u], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < TN; ++t) a[t] = an[t];
#pragma unroll
        for (int u = 0; u < TK; ++u) b[u] = bn_[u];
    }
    // C/D layout of the 32x32 tile: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* out = part + (int64_t)slab * wgrad_slab_stride((int64_t)N * K);
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int u = 0; u < TK; ++u) {
            const int k = k0 + 32 * u + col;
            if (k >= K) continue;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int n = n0 + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (n < N) out[(int64_t)n * K + k] = acc[t][u][i];
            }
        }
}

// The same product with 16-byte loads and a four-step prefetch ring (N % 4 == 0 and K % 4 == 0: every layer of the reference's model).
// The order of the MFMA's k index is free (it is summed over) and so is the assignment of output rows / columns to tile rows / columns,
// as long as the epilogue writes with the same map.  So a lane loads FOUR consecutive floats of its row - columns 4c .. 4c+3 for
// c = lane & 31 - and register j of that float4 is the operand of tile j, whose 32 rows are the columns {4i + j}: one
// global_load_dwordx4 feeds four tiles.  A wavefront owns a 128 x 128 block of dW (4 x 4 tiles = all 256 accumulator registers; five
// row tiles do not fit: the allocator then shuffles accumulators through scratch inside the loop); the last row block of N = 300 has 44
// live rows and runs with two row tiles (TN template), so 40 tiles are computed where 37.5 are needed.  The four wavefronts of a
// workgroup take four consecutive row slabs of the SAME block.  One wavefront per SIMD cannot hide HBM latency by switching wavefronts,
// so four steps (eight rows) of operands are in flight under the MFMAs: with a single step ahead the first version of this kernel
// ran at a fifth of the matrix pipe's rate, waiting for memory.
// AVEC = true: the float4 row map above for dY (always four row tiles).  AVEC = false: the narrow last row block (e.g. 44 of 300): a lane
// loads ONE float per row tile, tile t holding the 32 consecutive columns n0 + 32 t + c, so that only TN = ceil(width / 32) tiles run.
template <int TN, bool AVEC>
__device__ __forceinline__ void wgrad_tn4_block(const float* __restrict__ dY, int64_t ld_dy, const float* __restrict__ X, int64_t ld_x, int M,
                                                int N, int K, int m_begin, int m_end, int n0, int k0, int lane, float* __restrict__ out) {
    static_assert(!AVEC || TN == 4, "the float4 row map always fills four tiles");
    constexpr int TK = 4, D = 4, NA = AVEC ? 1 : TN;
    const int col = lane & 31, half = lane >> 5;
    const int kb = k0 + 4 * col;
    const bool okb = kb < K;                                             // (K a multiple of 4: a float4 is all in or all out)
    const float* pb = X + (okb ? kb : 0);
    const float* pa[NA];
    bool oka[NA];
#pragma unroll
    for (int t = 0; t < NA; ++t) {
        const int n = AVEC ? n0 + 4 * col : n0 + 32 * t + col;
        oka[t] = n < N;
        pa[t] = dY + (oka[t] ? n : 0);
    }

    f32x16 acc[TN][TK];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int u = 0; u < TK; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

    float4 a4[D], b4[D];
    float a1[D][NA];
    // Loads are UNCONDITIONAL (clamped addresses) and land raw in the ring; invalid lanes are zeroed with a bit mask when the step
    // is USED.  (A select on the loaded value makes the compiler predicate the load itself, and masking at load time makes it wait for
    // every load right where it is issued: either way the prefetch ring drains - s_waitcnt vmcnt(0) - on every step.)
    auto keep = [](float v, uint32_t mask) __attribute__((always_inline)) { return __uint_as_float(__float_as_uint(v) & mask); };
    auto load = [&](int m, int s) __attribute__((always_inline)) {
        const int64_t r = min(m + half, M - 1);
        if (AVEC) {
            a4[s] = *reinterpret_cast<const float4*>(pa[0] + r * ld_dy);
        } else {
#pragma unroll
            for (int t = 0; t < NA; ++t) a1[s][t] = pa[t][r * ld_dy];
        }
        b4[s] = *reinterpret_cast<const float4*>(pb + r * ld_x);
    };
    auto mfma = [&](int m, int s) __attribute__((always_inline)) {
        const uint32_t live = (m + half) < m_end ? 0xffffffffu : 0u;
        const uint32_t mb = okb ? live : 0u;
        float av[TN];
        if (AVEC) {
            const uint32_t ma = oka[0] ? live : 0u;
            av[0] = keep(a4[s].x, ma), av[1] = keep(a4[s].y, ma), av[2] = keep(a4[s].z, ma), av[3] = keep(a4[s].w, ma);
        } else {
#pragma unroll
            for (int t = 0; t < TN; ++t) av[t] = keep(a1[s][t], oka[t] ? live : 0u);
        }
        const float bv[4] = {keep(b4[s].x, mb), keep(b4[s].y, mb), keep(b4[s].z, mb), keep(b4[s].w, mb)};
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int u = 0; u < TK; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[u], acc[t][u], 0, 0, 0);
    };
#pragma unroll
    for (int s = 0; s < D; ++s) load(m_begin + 2 * s, s);              // rows beyond the slab load a clamped address and count as zero
    __builtin_amdgcn_sched_barrier(0);
    for (int m = m_begin; m < m_end; m += 2 * D) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
            mfma(m + 2 * s, s);
            __builtin_amdgcn_sched_barrier(0);          // (left alone, the scheduler sinks the refill next to its use four steps later)
            load(m + 2 * (s + D), s);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // D tile: column j = lane & 31, row i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); tile (t, u) holds k = k0 + 4 j + u and
    // n = n0 + 4 i + t (AVEC) or n0 + 32 t + i
    if (okb) {
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
                const int n = AVEC ? n0 + 4 * row + t : n0 + 32 * t + row;
                if (n < N) *reinterpret_cast<float4*>(out + (int64_t)n * K + kb) = make_float4(acc[t][0][i], acc[t][1][i], acc[t][2][i], acc[t][3][i]);
            }
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wgrad_tn4_kernel(
    const float* __restrict__ dY, int64_t ld_dy, const float* __restrict__ X, int64_t ld_x, int M, int N, int K, int rows_per_slab, int nb_n,
    int nb_k, float* __restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bn = blockIdx.y / nb_k, bk = blockIdx.y - bn * nb_k;
    const int slab = blockIdx.x * 4 + wave;
    const int m_begin = slab * rows_per_slab, m_end = min(M, m_begin + rows_per_slab);
    float* out = part + (int64_t)slab * wgrad_slab_stride((int64_t)N * K);
    const int n0 = bn * 128, k0 = bk * 128, width = N - n0;             // width < 128 only in the last row block
    if (width > 96) wgrad_tn4_block<4, true>(dY, ld_dy, X, ld_x, M, N, K, m_begin, m_end, n0, k0, lane, out);
    else if (width > 64) wgrad_tn4_block<3, false>(dY, ld_dy, X, ld_x, M, N, K, m_begin, m_end, n0, k0, lane, out);
    else if (width > 32) wgrad_tn4_block<2, false>(dY, ld_dy, X, ld_x, M, N, K, m_begin, m_end, n0, k0, lane, out);
    else wgrad_tn4_block<1, false>(dY, ld_dy, X, ld_x, M, N, K, m_begin, m_end, n0, k0, lane, out);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same product on the bf16 matrix pipe with fp32 results: the exact three-way operand split of csrc/dfol_pair_split.hip (x = h + m + l,
// six of the nine piece products, fp32 accumulation) - 6/16 of the fp32 pipe's time.  v_mfma_f32_32x32x16_bf16 wants EIGHT consecutive
// k per lane and operand, and k is the row index here, so an operand register holds eight ROWS of one column: a lane loads the float4
// (columns 4c .. 4c+3) of its eight rows m0 + 8 (lane >> 5) + 0..7 - plain coalesced 16-byte loads again - and component t of the
// eight registers, split and packed, is the operand of tile t (same free row / column map as wgrad_tn4_kernel).  Per step of 16 rows
// and wavefront: 16 loads, 96 MFMAs (3072 cycles) and ~350 VALU instructions of splitting at the top of the step; the next step's rows are
// in flight under the MFMAs.
__device__ __forceinline__ void w3_split8(const float (&v)[8], u32x4& h, u32x4& m, u32x4& l) {
    uint32_t ph[8], pm[8], pl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) dfol_split3(v[j], ph[j], pm[j], pl[j]);
    h = u32x4{dfol_pack(ph[0], ph[1]), dfol_pack(ph[2], ph[3]), dfol_pack(ph[4], ph[5]), dfol_pack(ph[6], ph[7])};
    m = u32x4{dfol_pack(pm[0], pm[1]), dfol_pack(pm[2], pm[3]), dfol_pack(pm[4], pm[5]), dfol_pack(pm[6], pm[7])};
    l = u32x4{dfol_pack(pl[0], pl[1]), dfol_pack(pl[2], pl[3]), dfol_pack(pl[4], pl[5]), dfol_pack(pl[6], pl[7])};
}

// Addressing: the rows of a step come through buffer descriptors rebuilt per step from wave-uniform values (base = the step's first
// row, size = what is left of the wavefront's row range), with per-lane byte offsets that never change: no address arithmetic on the
// vector ALU, and rows past the range read as zero from the bounds check (a zero A row switches the row off in every product), so
// there is no tail code either.
// Workgroup = four wavefronts on FOUR BLOCKS OF THE SAME ROWS (consecutive blocks in row-block-major order: 2 x 2 blocks of dW for the
// pair layer); they start together and do the same work per step, so dY and X rows are fetched from HBM once per workgroup and hit
// in L1/L2 for the other wavefronts (a barrier per step to keep them aligned costs 9 % and buys nothing).  (One wavefront per block with four row ranges per workgroup, the first version, read dY twice and
// X three times for the pair layer: 13.9 GB per launch, HBM-bound at 2.96 ms.)  A last group of one or two blocks splits its rows in two
// halves over the four wavefronts; the second half's accumulators go through LDS and are added by the first half's wavefront - a
// fixed order.  (The descriptors: w3_descriptor, csrc/dfol_wgrad.h.)

// eight fp32 -> eight bf16, round to nearest even: the operand of the bf16 mode (NP = 1)
__device__ __forceinline__ u32x4 w3_rne8(const float (&v)[8]) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = dfol_rne2(v[2 * j], v[2 * j + 1]);
    return r;
}

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));       // a 16-byte load from a 4-byte aligned address

// AV: floats of dY a lane loads per row = row tiles of the block (4: 128 output rows; 2: a narrow last row block, up to 64 output rows)
// NP: pieces per operand - 3: fp32 results (six piece products); 1: the bf16 mode (operands rounded to bf16, one product, fp32 accumulation)
// ROWS: row r of the range is row src_row[r] of the table X (dfol_linear_wgrad_bias_rows_*: a feature store's table, src_row from
// dfol_store_rows_f32).  Only the address of an X row differs: a table can be larger than a buffer descriptor's 32-bit offsets reach, so the
// lane forms the 64-bit address itself and loads through it; a row past the range is not loaded at all (neither its index nor the
// table) and counts as the zero row the descriptor's bounds check gives the matrix form.  A lane reads the index of each of its rows once,
// a step before the row itself.  The instantiations without ROWS never touch src_row and compile to the code they had before it existed.
template <int AV, int NP, bool ROWS = false>
__device__ __forceinline__ void wgrad_tn3_accumulate(const float* __restrict__ dY, int64_t ld_dy, const float* __restrict__ X, int64_t ld_x,
                                                     const int32_t* __restrict__ src_row, int rows, int steps, int N, int K, int n0, int k0,
                                                     int lane, bool want_bias, f32x16 (&acc)[AV][4], float (&bs)[AV]) {
    // dY, X: first row of this wavefront's range (wave-uniform); rows: rows in the range (<= 0: nothing to add)
    // ROWS: X is the table's first row and src_row the index of the range's first row
    // bs[t] (want_bias, wave-uniform): this lane's part of the bias gradient, the sum of dY[m][n0 + AV col + t] over its rows
    const int col = lane & 31, half = lane >> 5;
    // columns beyond the matrix read a clamped column: they only feed output rows / columns that are never stored
    const int ca = min(n0 + AV * col, N - AV), cb = min(k0 + 4 * col, K - 4);
    int va[8], vb[8];                                                              // byte offsets of this lane's eight rows within a step
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        va[r] = (int)(((8 * half + r) * ld_dy + ca) * 4);
        vb[r] = (int)(((8 * half + r) * ld_x + cb) * 4);
    }
#pragma unroll
    for (int t = 0; t < AV; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;
#pragma unroll
    for (int t = 0; t < AV; ++t) bs[t] = 0.f;

    float ra[8][AV];                                                               // the step's dY and X rows: dead once the pieces are built,
    u32x4 rb[8];                                                                   // then refilled with the next step's (in flight under the MFMAs)
    int ix[ROWS ? 8 : 1];                                                          // ROWS: the table rows of the step to load next (-1: past the range)
    auto index = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < (ROWS ? 8 : 0); ++r) {
            const int row = 16 * s + 8 * half + r;
            ix[r] = row < rows ? src_row[row] : -1;
        }
    };
    auto load = [&](int s) __attribute__((always_inline)) {
        const int left = rows - 16 * s;                                            // rows of the range from this step on
        const int64_t bytes_a = left > 0 ? ((int64_t)(left - 1) * ld_dy + N) * 4 : 0, bytes_b = left > 0 ? ((int64_t)(left - 1) * ld_x + K) * 4 : 0;
        const auto da = w3_descriptor(dY + (int64_t)s * 16 * ld_dy, bytes_a), db = w3_descriptor(X + (int64_t)s * 16 * ld_x, bytes_b);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (AV == 4) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(da, va[r], 0, 0);
                ra[r][0] = __uint_as_float(v.x), ra[r][1] = __uint_as_float(v.y), ra[r][2] = __uint_as_float(v.z), ra[r][3] = __uint_as_float(v.w);
            } else {
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(da, va[r], 0, 0);
                ra[r][0] = __uint_as_float(v.x), ra[r][1] = __uint_as_float(v.y);
            }
            if constexpr (ROWS) {
                rb[r] = u32x4{0u, 0u, 0u, 0u};
                if (ix[r] >= 0) rb[r] = *reinterpret_cast<const u32x4_a4*>(X + (int64_t)ix[r] * ld_x + cb);
            } else {
                rb[r] = __builtin_amdgcn_raw_buffer_load_b128(db, vb[r], 0, 0);
            }
        }
    };
    constexpr int PA6[6] = {2, 0, 1, 1, 0, 0}, PB6[6] = {0, 2, 1, 0, 1, 0};       // (A piece, B piece): l*h, h*l, m*m, m*h, h*m, h*h
    // One step: all pieces first (a tile at a time: the split's temporaries are 32 registers per tile), then the next step's loads, then
    // 24 AV MFMAs back to back.  (Building the B pieces of column tile u + 1 between the MFMAs of tile u was tried first: with 256
    // accumulators the allocator then parks VGPRs in the accumulator file and cycles every tile through one AGPR tuple.)
    if constexpr (ROWS) index(0);
    load(0);
    if constexpr (ROWS) index(1);
    __builtin_amdgcn_sched_barrier(0);
    for (int s = 0; s < steps; ++s) {
        u32x4 ap[AV][NP], bp[4][NP];
        if (want_bias) {
#pragma unroll
            for (int t = 0; t < AV; ++t)
                bs[t] += ((ra[0][t] + ra[1][t]) + (ra[2][t] + ra[3][t])) + ((ra[4][t] + ra[5][t]) + (ra[6][t] + ra[7][t]));
        }
#pragma unroll
        for (int t = 0; t < AV; ++t) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = ra[r][t];
            if constexpr (NP == 1) ap[t][0] = w3_rne8(v);
            else w3_split8(v, ap[t][0], ap[t][1], ap[t][2]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = __uint_as_float(rb[r][u]);
            if constexpr (NP == 1) bp[u][0] = w3_rne8(v);
            else w3_split8(v, bp[u][0], bp[u][1], bp[u][2]);
            __builtin_amdgcn_sched_barrier(0);
        }
        load(s + 1);
        if constexpr (ROWS) index(s + 2);                                          // (waited for a step later, behind the pieces)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < AV; ++t)
#pragma unroll
                for (int x = NP == 1 ? 5 : 0; x < 6; ++x)                       // (the bf16 mode keeps the last product: piece 0 x piece 0)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ap[t][PA6[x]]),
                                                                        __builtin_bit_cast(bf16x8, bp[u][PB6[x]]), acc[t][u], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// eight rows' element `odd` of one 32-bit word of bf16 pairs each -> the operand's four registers (row 2j in the low half): v_perm_b32, no conversion
__device__ __forceinline__ u32x4 w3_gather8(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6, uint32_t w7, bool odd) {
    return odd ? u32x4{__builtin_amdgcn_perm(w1, w0, 0x07060302u), __builtin_amdgcn_perm(w3, w2, 0x07060302u),
                       __builtin_amdgcn_perm(w5, w4, 0x07060302u), __builtin_amdgcn_perm(w7, w6, 0x07060302u)}
               : u32x4{__builtin_amdgcn_perm(w1, w0, 0x05040100u), __builtin_amdgcn_perm(w3, w2, 0x05040100u),
                       __builtin_amdgcn_perm(w5, w4, 0x05040100u), __builtin_amdgcn_perm(w7, w6, 0x05040100u)};
}

// The bf16 mode over the indexed rows of a bf16 TABLE (a feature store built with feature_dtype="bf16": dfol_linear_wgrad_bias_rows_bf16t).
// dY is fp32 as in the first form - rounded by w3_rne8, the bias sums from the fp32 values - and X is four bf16 per row and lane through the
// ROWS form's 64-bit address, assembled into operand registers as the bf16-storage form below does it: the table holds what w3_rne8 makes of
// an fp32 feature, so every operand register has the bits the first form builds from the gathered, widened rows.  A row past the range
// loads neither its index nor the table and counts as zero.
// NP = 3 is the DEFAULT arithmetic over the same table (dfol_linear_wgrad_bias_rows_bf16t_x3): dY split by w3_split8 as in the first form, X
// as above.  A value out of a bf16 table is its own h piece - what w3_split8 makes of the widened value is (x, 0, 0) - so of the six products
// of PA6 / PB6 the three whose B piece is m or l multiply by zero and are not issued; the other three keep their order: l*h, m*h, h*h.  An
// accumulator that starts at +0 and has only +-0 added stays +0 (round to nearest: x + -x = +0, and -0 comes only of -0 + -0), so dropping
// them changes no bit of the first form's result over the gathered, widened rows.  12 AV MFMAs per step, no B-side split, half the X bytes.
template <int AV, int NP, bool ROWS = false>
__device__ __forceinline__ void wgrad_tn3_accumulate(const float* __restrict__ dY, int64_t ld_dy, const uint16_t* __restrict__ X, int64_t ld_x,
                                                     const int32_t* __restrict__ src_row, int rows, int steps, int N, int K, int n0, int k0,
                                                     int lane, bool want_bias, f32x16 (&acc)[AV][4], float (&bs)[AV]) {
    static_assert((NP == 1 || NP == 3) && ROWS, "a bf16 table under fp32 gradients is an indexed form: the bf16 mode's, or the three-piece dY's");
    const int col = lane & 31, half = lane >> 5;
    const int ca = min(n0 + AV * col, N - AV), cb = min(k0 + 4 * col, K - 4);
    int va[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) va[r] = (int)(((8 * half + r) * ld_dy + ca) * 4);
#pragma unroll
    for (int t = 0; t < AV; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;
#pragma unroll
    for (int t = 0; t < AV; ++t) bs[t] = 0.f;

    float ra[8][AV];
    u32x2 rb[8];
    int ix[8];                                                                     // the table rows of the step to load next (-1: past the range)
    auto index = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int row = 16 * s + 8 * half + r;
            ix[r] = row < rows ? src_row[row] : -1;
        }
    };
    auto load = [&](int s) __attribute__((always_inline)) {
        const int left = rows - 16 * s;
        const int64_t bytes_a = left > 0 ? ((int64_t)(left - 1) * ld_dy + N) * 4 : 0;
        const auto da = w3_descriptor(dY + (int64_t)s * 16 * ld_dy, bytes_a);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (AV == 4) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(da, va[r], 0, 0);
                ra[r][0] = __uint_as_float(v.x), ra[r][1] = __uint_as_float(v.y), ra[r][2] = __uint_as_float(v.z), ra[r][3] = __uint_as_float(v.w);
            } else {
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(da, va[r], 0, 0);
                ra[r][0] = __uint_as_float(v.x), ra[r][1] = __uint_as_float(v.y);
            }
            rb[r] = u32x2{0u, 0u};
            if (ix[r] >= 0) rb[r] = *reinterpret_cast<const u32x2*>(X + (int64_t)ix[r] * ld_x + cb);      // (8-byte aligned: ld_x % 4 == 0)
        }
    };
    index(0);
    load(0);
    index(1);
    __builtin_amdgcn_sched_barrier(0);
    for (int s = 0; s < steps; ++s) {
        u32x4 ap[AV][NP], bp[4];
        if (want_bias) {
#pragma unroll
            for (int t = 0; t < AV; ++t)
                bs[t] += ((ra[0][t] + ra[1][t]) + (ra[2][t] + ra[3][t])) + ((ra[4][t] + ra[5][t]) + (ra[6][t] + ra[7][t]));
        }
#pragma unroll
        for (int t = 0; t < AV; ++t) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = ra[r][t];
            if constexpr (NP == 1) ap[t][0] = w3_rne8(v);
            else w3_split8(v, ap[t][0], ap[t][1], ap[t][2]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            bp[u] = w3_gather8(rb[0][u >> 1], rb[1][u >> 1], rb[2][u >> 1], rb[3][u >> 1], rb[4][u >> 1], rb[5][u >> 1], rb[6][u >> 1], rb[7][u >> 1], u & 1);
        __builtin_amdgcn_sched_barrier(0);
        load(s + 1);
        index(s + 2);                                                              // (waited for a step later, behind the pieces)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < AV; ++t)
#pragma unroll
                for (int x = NP - 1; x >= 0; --x)                                 // (A piece l, m, h against the table's value: its own h piece)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ap[t][x]), __builtin_bit_cast(bf16x8, bp[u]), acc[t][u], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The same with dY and X STORED as bfloat16 (the bf16 mode's per-pair activations: dpre2 [pairs, HID2] and Z [pairs, HID1]): a lane loads
// AV resp. 4 consecutive bf16 of its eight rows (8- / 4-byte buffer loads), and an operand register pair is two rows' halves of one word
// (v_perm_b32) - no conversions, no rounding, half the bytes.  The bias sums widen the same registers to fp32.
template <int AV, int NP, bool ROWS = false>
__device__ __forceinline__ void wgrad_tn3_accumulate(const uint16_t* __restrict__ dY, int64_t ld_dy, const uint16_t* __restrict__ X, int64_t ld_x,
                                                     const int32_t* __restrict__, int rows, int steps, int N, int K, int n0, int k0, int lane,
                                                     bool want_bias, f32x16 (&acc)[AV][4], float (&bs)[AV]) {
    static_assert(NP == 1 && !ROWS, "bf16 storage belongs to the bf16 mode, and has no indexed form");
    constexpr int WA = AV / 2;                                                     // 32-bit words of dY per row and lane
    const int col = lane & 31, half = lane >> 5;
    const int ca = min(n0 + AV * col, N - AV), cb = min(k0 + 4 * col, K - 4);
    int va[8], vb[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        va[r] = (int)(((8 * half + r) * ld_dy + ca) * 2);
        vb[r] = (int)(((8 * half + r) * ld_x + cb) * 2);
    }
#pragma unroll
    for (int t = 0; t < AV; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;
#pragma unroll
    for (int t = 0; t < AV; ++t) bs[t] = 0.f;

    // A step is 16 MFMAs here (512 cycles of pipe) against the 96 of the three-piece kernel: one step of loads in flight does not cover
    // HBM latency any more, so the rows of W3B_D steps ahead are (a ring of register sets, 32 registers each).
    constexpr int D = W3B_D;
    uint32_t ra[D][8][WA];
    u32x2 rb[D][8];
    auto load = [&](int s, auto set_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(set_tag)::value;
        const int left = rows - 16 * s;
        const int64_t bytes_a = left > 0 ? ((int64_t)(left - 1) * ld_dy + N) * 2 : 0, bytes_b = left > 0 ? ((int64_t)(left - 1) * ld_x + K) * 2 : 0;
        const auto da = w3_descriptor(dY + (int64_t)s * 16 * ld_dy, bytes_a), db = w3_descriptor(X + (int64_t)s * 16 * ld_x, bytes_b);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (AV == 4) {
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(da, va[r], 0, 0);
                ra[S][r][0] = v.x, ra[S][r][WA - 1] = v.y;
            } else {
                ra[S][r][0] = __builtin_amdgcn_raw_buffer_load_b32(da, va[r], 0, 0);
            }
            rb[S][r] = __builtin_amdgcn_raw_buffer_load_b64(db, vb[r], 0, 0);
        }
    };
    auto one_step = [&](int s, auto set_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(set_tag)::value;
        u32x4 ap[AV], bp[4];
        if (want_bias) {
#pragma unroll
            for (int t = 0; t < AV; ++t) {
                float f[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) f[r] = __uint_as_float((t & 1) ? (ra[S][r][t >> 1] & 0xffff0000u) : (ra[S][r][t >> 1] << 16));
                bs[t] += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
            }
        }
#pragma unroll
        for (int t = 0; t < AV; ++t)
            ap[t] = w3_gather8(ra[S][0][t >> 1], ra[S][1][t >> 1], ra[S][2][t >> 1], ra[S][3][t >> 1], ra[S][4][t >> 1], ra[S][5][t >> 1], ra[S][6][t >> 1],
                           ra[S][7][t >> 1], t & 1);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            bp[u] = w3_gather8(rb[S][0][u >> 1], rb[S][1][u >> 1], rb[S][2][u >> 1], rb[S][3][u >> 1], rb[S][4][u >> 1], rb[S][5][u >> 1], rb[S][6][u >> 1],
                           rb[S][7][u >> 1], u & 1);
        __builtin_amdgcn_sched_barrier(0);
        load(s + D, set_tag);                                                      // (past the range: zero bytes, nothing fetched)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < AV; ++t)
                acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ap[t]), __builtin_bit_cast(bf16x8, bp[u]), acc[t][u], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    load(0, std::integral_constant<int, 0>());
    if constexpr (D > 1) load(1, std::integral_constant<int, 1>());
    if constexpr (D > 2) load(2, std::integral_constant<int, 2>());
    if constexpr (D > 3) load(3, std::integral_constant<int, 3>());
    __builtin_amdgcn_sched_barrier(0);
    for (int s = 0; s < steps; s += D) {                                           // (steps past the range multiply zero rows: exact zeros)
#if W3B_ALIGN
        // the four wavefronts of a workgroup read the SAME rows (different column blocks): kept within a ring turn of each other, the
        // second reader of a row finds it in L1 / L2.  Left free-running they drift apart and every wavefront fetches its rows from HBM:
        // 2.11 x the algorithmic bytes at 6.4 TB/s - this kernel, unlike its three-piece form, is HBM-bound.  (Wavefronts that have
        // returned do not count for s_barrier.)  Two further attempts at the byte count, both measured and dropped: handing the four row panels
        // of a 2 x 2 group through LDS (one fetch per panel and workgroup) - same FETCH_SIZE (4.65 GB per launch in isolation: the re-reads
        // were L2 hits already) and same 0.97 ms; dispatching a slab's two groups next to each other ((groups, slabs) grid) - same bytes,
        // 1.1 ms.  What the counters show as 1.65 - 2.1 x is structural: the second workgroup class reads X again and dY's 600-byte rows
        // straddle 128-byte lines.
        __builtin_amdgcn_s_barrier();
#endif
        one_step(s, std::integral_constant<int, 0>());
        if constexpr (D > 1) one_step(s + 1, std::integral_constant<int, 1>());
        if constexpr (D > 2) one_step(s + 2, std::integral_constant<int, 2>());
        if constexpr (D > 3) one_step(s + 3, std::integral_constant<int, 3>());
    }
}

template <int AV, int NP, typename TIN, bool ROWS, typename TXE = TIN>
__device__ __forceinline__ void wgrad_tn3_block(const TIN* __restrict__ dY, int64_t ld_dy, const TXE* __restrict__ X, int64_t ld_x,
                                                const int32_t* __restrict__ src_row, int rows, int steps, int N, int K, int n0, int k0, int lane,
                                                int role, float* __restrict__ lds, float* __restrict__ out, float* __restrict__ db_out) {
    // role 0: accumulate and store; 1: accumulate, add the partner's accumulators from `lds`, store; 2: accumulate into `lds` (the partner)
    // db_out (k0 == 0 wavefronts, or null): this slab's part of the bias gradient
    f32x16 acc[AV][4];
    float bs[AV];
    const bool want_bias = db_out != nullptr && k0 == 0;
    wgrad_tn3_accumulate<AV, NP, ROWS>(dY, ld_dy, X, ld_x, src_row, rows, steps, N, K, n0, k0, lane, want_bias, acc, bs);
    if (role == 2) {
#pragma unroll
        for (int t = 0; t < AV; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < 16; ++i) lds[((t * 4 + u) * 16 + i) * 64 + lane] = acc[t][u][i];
#pragma unroll
        for (int t = 0; t < AV; ++t) lds[(256 + t) * 64 + lane] = bs[t];
    }
    __syncthreads();
    if (role == 2) return;
    if (role == 1) {
#pragma unroll
        for (int t = 0; t < AV; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][u][i] += lds[((t * 4 + u) * 16 + i) * 64 + lane];
#pragma unroll
        for (int t = 0; t < AV; ++t) bs[t] += lds[(256 + t) * 64 + lane];
    }
    // D tile: column j = lane & 31, row i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); tile (t, u) holds n = n0 + AV i + t, k = k0 + 4 j + u
    const int half = lane >> 5, kb = k0 + 4 * (lane & 31);
    if (kb < K) {
#pragma unroll
        for (int t = 0; t < AV; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int n = n0 + AV * ((i & 3) + 8 * (i >> 2) + 4 * half) + t;
                if (n < N) *reinterpret_cast<float4*>(out + (int64_t)n * K + kb) = make_float4(acc[t][0][i], acc[t][1][i], acc[t][2][i], acc[t][3][i]);
            }
    }
    if (want_bias) {                                                               // lanes l and l + 32 hold the two row halves of a column
#pragma unroll
        for (int t = 0; t < AV; ++t) {
            const float other = __shfl_xor(bs[t], 32);
            const int n = n0 + AV * (lane & 31) + t;
            if (half == 0 && n < N) db_out[n] = bs[t] + other;
        }
    }
}

constexpr int W3_LDS_SLOT = 64 * (256 + 4);        // floats a row-half partner hands over: 256 accumulators and 4 bias sums per lane

// grid (row slabs, groups of four blocks); dynamic LDS: two slots when the last group splits its rows (see the launcher), else none
// ROWS: X is a table and src_row [M] names the table row of every row of the product (see wgrad_tn3_accumulate); else src_row is not read
// TXE: X's element type where it is not dY's (uint16_t under fp32 gradients: a bf16 table)
template <int NP, typename TIN = float, bool ROWS = false, typename TXE = TIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wgrad_tn3_kernel(
    const TIN* __restrict__ dY, int64_t ld_dy, const TXE* __restrict__ X, int64_t ld_x, int M, int N, int K, int rows_per_slab, int nb_k,
    int nb, float* __restrict__ part, float* __restrict__ db_part, const int32_t* __restrict__ src_row) {
    extern __shared__ float w3_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int first = blockIdx.y * 4, in_group = min(4, nb - first);               // blocks of this group
    const bool split = in_group <= 2;                                              // then wavefront w: block w % in_group, row half w / in_group
    int blk = first + wave, role = 0, half_id = 0;
    if (split) {
        half_id = wave / in_group;
        blk = first + wave - half_id * in_group;
        role = half_id >= 2 ? 3 : (half_id == 1 ? 2 : 1);                          // (one block: wavefronts 2, 3 have nothing to do)
    } else if (blk >= nb) role = 3;
    const int m_begin = blockIdx.x * rows_per_slab, m_end = min(M, m_begin + rows_per_slab);
    int rows = m_end - m_begin, steps = (rows + 15) >> 4, m_first = m_begin;
    if (split) {
        const int first_half = ((rows + 31) >> 5) << 4;                            // rows of the first half: a multiple of 16, the larger one
        steps = first_half >> 4;
        if (half_id == 1) m_first = m_begin + first_half, rows -= first_half;
        else rows = min(rows, first_half);
    }
    if (role == 3) {                                                               // (the one barrier of wgrad_tn3_block)
        __syncthreads();
        return;
    }
    const int bn = blk / nb_k, bk = blk - bn * nb_k;
    const int n0 = bn * 128, k0 = bk * 128;
    float* out = part + (int64_t)blockIdx.x * wgrad_slab_stride((int64_t)N * K);
    float* lds = w3_lds + (split ? wave - half_id * in_group : 0) * W3_LDS_SLOT;   // wavefronts w and w + in_group: the same block, one slot
    float* db_out = db_part ? db_part + (int64_t)blockIdx.x * ((N + 3) & ~3) : nullptr;
    const TIN* a = dY + (int64_t)m_first * ld_dy;
    const TXE* b = ROWS ? X : X + (int64_t)m_first * ld_x;
    const int32_t* idx = ROWS ? src_row + m_first : nullptr;
    if (N - n0 > 64) wgrad_tn3_block<4, NP, TIN, ROWS, TXE>(a, ld_dy, b, ld_x, idx, rows, steps, N, K, n0, k0, lane, role, lds, out, db_out);
    else wgrad_tn3_block<2, NP, TIN, ROWS, TXE>(a, ld_dy, b, ld_x, idx, rows, steps, N, K, n0, k0, lane, role, lds, out, db_out);
}

// Bias gradient beside the fp32-pipe kernels (the bf16x3 kernel takes it from the dY rows it loads anyway): column sums of a row slab,
// four row phases per workgroup added in a fixed order.  grid (slabs, ceil(N / 64)).
__global__ __launch_bounds__(256) void wgrad_colsum_kernel(const float* __restrict__ dY, int64_t ld_dy, int M, int N, int rows_per_slab,
                                                           float* __restrict__ db_part) {
    __shared__ float sums[4][64];
    const int c = threadIdx.x & 63, phase = threadIdx.x >> 6, n = blockIdx.y * 64 + c;
    const int m_begin = blockIdx.x * rows_per_slab, m_end = min(M, m_begin + rows_per_slab);
    float s = 0.f;
    if (n < N)
        for (int m = m_begin + phase; m < m_end; m += 4) s += dY[(int64_t)m * ld_dy + n];
    sums[phase][c] = s;
    __syncthreads();
    if (phase == 0 && n < N) db_part[(int64_t)blockIdx.x * ((N + 3) & ~3) + n] = ((sums[0][c] + sums[1][c]) + sums[2][c]) + sums[3][c];
}

// Row slabs of the bf16x3 kernel: one round of workgroups for the full groups of four blocks (a workgroup owns a CU: one wavefront per
// SIMD), at least 256 rows (16 steps) per slab.
static int wgrad_tn3_slabs(int64_t M, int nb) {
    const int full = nb / 4;
    int64_t s = full > 0 ? 256 / full : 256;
    s = std::min<int64_t>(s, (M + 255) / 256);
    return (int)std::max<int64_t>(s, 1);
}
static int wgrad_tn4_slabs(int64_t M, int nb) {
    int wgs = dfol_cdiv(768, nb);                                       // workgroups per block of dW
    const int64_t max_wgs = (M + 255) / 256;
    if (wgs > max_wgs) wgs = (int)max_wgs;
    if (wgs < 1) wgs = 1;
    return 4 * wgs;                                                     // one slab per wavefront of a workgroup
}

// Row slabs the caller sizes the workspace of dfol_linear_wgrad_f32 for (slabs x N x K floats, rounded up to 4 floats per slab): the
// launch uses this many or fewer.
extern "C" int dfol_linear_wgrad_slabs(int64_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int nb = dfol_cdiv(N, 128) * dfol_cdiv(K, 128);
    return std::max(wgrad_tn3_slabs(M, nb), wgrad_tn4_slabs(M, nb));
}

// Floats of workspace dfol_linear_wgrad_bias_f32 needs: the slabs' partial dW blocks, then their partial bias gradients
extern "C" int64_t dfol_linear_wgrad_workspace(int64_t M, int32_t N, int32_t K) {
    const int64_t slabs = dfol_linear_wgrad_slabs(M, N, K);
    return slabs * (wgrad_slab_stride((int64_t)N * K) + ((N + 3) & ~3));
}

static bool wgrad_f32_pipe_asked() {
    const char* math = getenv("DFOL_WGRAD_MATH");                       // "f32": the fp32 matrix pipe (exact products); default: bf16x3
    return math && !strcmp(math, "f32");
}

// the slabs' partial bias gradients: behind the partial dW blocks of as many slabs as the workspace is sized for
static float* wgrad_db_part(float* workspace, int64_t M, int32_t N, int32_t K) {
    return workspace + (int64_t)dfol_linear_wgrad_slabs(M, N, K) * wgrad_slab_stride((int64_t)N * K);
}

// The whole path of one instantiation of the bf16-pipe kernel: slabs, launch, both reductions (the bias partials come from the kernel).
// ROWS: X is a table (ld_x its row stride) and src_row names its rows; else src_row is not read.  `who` names the entry point's family in
// the messages.  An instantiation reserves its LDS when it is first used.
template <int NP, typename TIN, bool ROWS, typename TXE = TIN>
static int wgrad_tn3_run(const char* who, const TIN* dY, int64_t ld_dy, const TXE* X, int64_t ld_x, const int32_t* src_row, int64_t M, int32_t N,
                         int32_t K, float* workspace, float* dW, float* db, hipStream_t st) {
    DFOL_REQUIRE(16 * std::max(ld_dy, ld_x) * (int64_t)sizeof(TIN) < (1ll << 31), "%s: row stride too large (%lld)", who, (long long)std::max(ld_dy, ld_x));
    const int nb_k = dfol_cdiv(K, 128), nb = dfol_cdiv(N, 128) * nb_k, groups = dfol_cdiv(nb, 4);
    const int slabs = wgrad_tn3_slabs(M, nb);
    const int rows_per_slab = (dfol_cdiv(M, slabs) + 15) & ~15;         // sixteen rows per MFMA step
    constexpr size_t lds_two = 2 * W3_LDS_SLOT * sizeof(float);
    const size_t lds = nb % 4 == 1 || nb % 4 == 2 ? lds_two : 0;        // the last group splits its rows (two slots)
    static const hipError_t lds_ok = hipFuncSetAttribute((const void*)wgrad_tn3_kernel<NP, TIN, ROWS, TXE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_two);
    DFOL_REQUIRE(lds_ok == hipSuccess, "%s: cannot reserve 130 KB of LDS (%s)", who, hipGetErrorString(lds_ok));
    float* db_part = db ? wgrad_db_part(workspace, M, N, K) : nullptr;
    hipLaunchKernelGGL((wgrad_tn3_kernel<NP, TIN, ROWS, TXE>), dim3(slabs, groups), dim3(256), lds, st, dY, ld_dy, X, ld_x, (int)M, N, K, rows_per_slab, nb_k,
                       nb, workspace, db_part, src_row);
    DFOL_LAUNCH_CHECK(who);
    if (const int rc = wgrad_reduce(who, "reduce", workspace, slabs, (int64_t)N * K, dW, st)) return rc;
    return db ? wgrad_reduce(who, "bias reduce", db_part, slabs, (int64_t)N, db, st) : 0;
}

// one launch path for both forms: src_row == nullptr is the plain product over X's own rows; with src_row, X is a table (ld_x its row
// stride) and the caller has made sure of the bf16-pipe kernel's conditions (dfol_linear_wgrad_bias_rows_*: the other kernels have no indexed form)
static int wgrad_launch(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const int32_t* src_row, int64_t M, int32_t N, int32_t K,
                        float* workspace, float* dW, float* db, void* stream, bool bf16_mode) {
    DFOL_REQUIRE(M > 0 && M < (1ll << 31) && N > 0 && K > 0, "linear_wgrad: bad sizes M=%lld N=%d K=%d", (long long)M, N, K);
    DFOL_REQUIRE(dY && X && workspace && dW, "linear_wgrad: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const bool vec4 = N % 4 == 0 && K % 4 == 0 && ld_dy % 4 == 0 && ((uintptr_t)dY % 16 == 0);      // (X rows may be 8-byte aligned only)
    const bool f32_pipe = !bf16_mode && wgrad_f32_pipe_asked();
    if (vec4 && !f32_pipe && N >= 4 && K >= 4) {                        // fp32 results from the bf16 matrix pipe (X rows: any 4-byte alignment)
        const char* who = src_row ? "linear_wgrad_rows" : "linear_wgrad";
        if (src_row)
            return bf16_mode ? wgrad_tn3_run<1, float, true>(who, dY, ld_dy, X, ld_x, src_row, M, N, K, workspace, dW, db, st)
                             : wgrad_tn3_run<3, float, true>(who, dY, ld_dy, X, ld_x, src_row, M, N, K, workspace, dW, db, st);
        return bf16_mode ? wgrad_tn3_run<1, float, false>(who, dY, ld_dy, X, ld_x, src_row, M, N, K, workspace, dW, db, st)
                         : wgrad_tn3_run<3, float, false>(who, dY, ld_dy, X, ld_x, src_row, M, N, K, workspace, dW, db, st);
    }
    DFOL_REQUIRE(!src_row, "linear_wgrad_rows: no indexed form of the fp32-pipe kernels");
    const int nb_n = dfol_cdiv(N, 128), nb_k = dfol_cdiv(K, 128);
    const int slabs = wgrad_tn4_slabs(M, nb_n * nb_k);
    const int rows_per_slab = (dfol_cdiv(M, slabs) + 7) & ~7;           // two rows per MFMA step, four steps per ring turn
    if (vec4)
        hipLaunchKernelGGL(wgrad_tn4_kernel, dim3(slabs / 4, nb_n * nb_k), dim3(256), 0, st, dY, ld_dy, X, ld_x, (int)M, N, K, rows_per_slab, nb_n,
                           nb_k, workspace);
    else                                                                // odd widths: one float per lane and load, the four wavefronts of
        hipLaunchKernelGGL((wgrad_tn_kernel<4, 4>), dim3(slabs, dfol_cdiv(nb_n * nb_k, 4)), dim3(256), 0, st, dY, ld_dy, X, ld_x, (int)M, N, K,
                           rows_per_slab, nb_n, nb_k, workspace);      // a workgroup on four blocks of the same rows
    DFOL_LAUNCH_CHECK("linear_wgrad");
    if (const int rc = wgrad_reduce("linear_wgrad", "reduce", workspace, slabs, (int64_t)N * K, dW, st)) return rc;
    if (!db) return 0;
    float* db_part = wgrad_db_part(workspace, M, N, K);
    hipLaunchKernelGGL(wgrad_colsum_kernel, dim3(slabs, dfol_cdiv(N, 64)), dim3(256), 0, st, dY, ld_dy, (int)M, N, rows_per_slab, db_part);
    DFOL_LAUNCH_CHECK("linear_wgrad (column sums)");
    return wgrad_reduce("linear_wgrad", "bias reduce", db_part, slabs, (int64_t)N, db, st);
}

extern "C" int dfol_linear_wgrad_bias_f32(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, int64_t M, int32_t N, int32_t K,
                                          float* workspace, float* dW, float* db, void* stream) {
    return wgrad_launch(dY, ld_dy, X, ld_x, nullptr, M, N, K, workspace, dW, db, stream, false);
}

// bf16 mode (BASELINE configs[3]): both operands rounded to bf16, one product per pair, fp32 accumulation; the bias gradient stays an
// fp32 sum.  Shapes the bf16x3 kernel does not take (widths that are not multiples of 4) run in fp32 as above.
extern "C" int dfol_linear_wgrad_bias_bf16(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, int64_t M, int32_t N, int32_t K,
                                           float* workspace, float* dW, float* db, void* stream) {
    return wgrad_launch(dY, ld_dy, X, ld_x, nullptr, M, N, K, workspace, dW, db, stream, true);
}

extern "C" int dfol_linear_wgrad_f32(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, int64_t M, int32_t N, int32_t K,
                                     float* workspace, float* dW, void* stream) {
    return wgrad_launch(dY, ld_dy, X, ld_x, nullptr, M, N, K, workspace, dW, nullptr, stream, false);
}

// The weight gradient over INDEXED rows (a feature store's table read in place): row r of X is row src_row[r] of X_table.  It exists where
// the matrix form runs the bf16-pipe kernel, and gives that kernel's bits: slabs, workspace layout, reduction and bias partials are the
// same launch path's, only the address of an X row differs (wgrad_tn3_accumulate, ROWS).
// Its conditions on sizes and strides, stated once: why the form does not take them, or null when it does (f32_pipe: DFOL_WGRAD_MATH=f32)
static const char* wgrad_rows_refusal(int32_t N, int32_t K, int64_t ld_dy, int64_t ld_table, bool f32_pipe) {
    if (N < 4 || K < 4 || N % 4 != 0 || K % 4 != 0) return "N and K must be multiples of 4";
    if (ld_dy < N || ld_dy % 4 != 0) return "dY rows must be 16-byte aligned and cover N";
    if (ld_table < K) return "table rows are shorter than K";
    if (16 * std::max(ld_dy, ld_table) * 4 >= (1ll << 31)) return "row stride too large";
    if (f32_pipe) return "DFOL_WGRAD_MATH=f32 asks for the fp32 matrix pipe, which has no indexed form";
    return nullptr;
}

extern "C" int dfol_linear_wgrad_rows_supported(int32_t N, int32_t K, int64_t ld_dy, int64_t ld_table) {
    return wgrad_rows_refusal(N, K, ld_dy, ld_table, wgrad_f32_pipe_asked()) == nullptr;
}

static int wgrad_rows_launch(const float* dY, int64_t ld_dy, const float* X_table, int64_t ld_table, const int32_t* src_row, int64_t M, int32_t N,
                             int32_t K, float* workspace, float* dW, float* db, void* stream, bool bf16_mode) {
    DFOL_REQUIRE(M > 0 && M < (1ll << 31) && N > 0 && K > 0, "linear_wgrad_rows: bad sizes M=%lld N=%d K=%d", (long long)M, N, K);
    DFOL_REQUIRE(dY && X_table && src_row && workspace && dW, "linear_wgrad_rows: null pointer");
    const char* why = wgrad_rows_refusal(N, K, ld_dy, ld_table, wgrad_f32_pipe_asked());
    DFOL_REQUIRE(!why, "linear_wgrad_rows: %s (N=%d K=%d ld_dy=%lld ld_table=%lld)", why, N, K, (long long)ld_dy, (long long)ld_table);
    DFOL_REQUIRE((uintptr_t)dY % 16 == 0, "linear_wgrad_rows: dY rows must be 16-byte aligned (dY=%p)", (const void*)dY);
    DFOL_REQUIRE((uintptr_t)X_table % 4 == 0 && (uintptr_t)src_row % 4 == 0, "linear_wgrad_rows: table and index must be 4-byte aligned");
    return wgrad_launch(dY, ld_dy, X_table, ld_table, src_row, M, N, K, workspace, dW, db, stream, bf16_mode);
}

extern "C" int dfol_linear_wgrad_bias_rows_f32(const float* dY, int64_t ld_dy, const float* X_table, int64_t ld_table, const int32_t* src_row,
                                               int64_t M, int32_t N, int32_t K, float* workspace, float* dW, float* db, void* stream) {
    return wgrad_rows_launch(dY, ld_dy, X_table, ld_table, src_row, M, N, K, workspace, dW, db, stream, false);
}

extern "C" int dfol_linear_wgrad_bias_rows_bf16(const float* dY, int64_t ld_dy, const float* X_table, int64_t ld_table, const int32_t* src_row,
                                                int64_t M, int32_t N, int32_t K, float* workspace, float* dW, float* db, void* stream) {
    return wgrad_rows_launch(dY, ld_dy, X_table, ld_table, src_row, M, N, K, workspace, dW, db, stream, true);
}

// The bf16 mode's weight gradient over the indexed rows of a bf16 TABLE (a feature store built with feature_dtype="bf16"): dY fp32, row r of X
// is row src_row[r] of X_table_bf16 (ld_table in elements, a multiple of 4: 8-byte rows).  Bit for bit dfol_linear_wgrad_bias_bf16 over the
// gathered rows widened to fp32; slabs, workspace layout and reductions are that launch path's.
static const char* wgrad_rows_bf16t_refusal(int32_t N, int32_t K, int64_t ld_dy, int64_t ld_table) {
    if (const char* why = wgrad_rows_refusal(N, K, ld_dy, ld_table, false)) return why;      // (the bf16 mode never asks for the fp32 pipe)
    if (ld_table % 4 != 0) return "table rows must be 8-byte aligned (ld_table % 4 == 0)";
    return nullptr;
}

extern "C" int dfol_linear_wgrad_rows_bf16t_supported(int32_t N, int32_t K, int64_t ld_dy, int64_t ld_table) {
    return wgrad_rows_bf16t_refusal(N, K, ld_dy, ld_table) == nullptr;
}

extern "C" int dfol_linear_wgrad_bias_rows_bf16t(const float* dY, int64_t ld_dy, const void* X_table_bf16, int64_t ld_table, const int32_t* src_row,
                                                 int64_t M, int32_t N, int32_t K, float* workspace, float* dW, float* db, void* stream) {
    DFOL_REQUIRE(M > 0 && M < (1ll << 31) && N > 0 && K > 0, "linear_wgrad_rows_bf16t: bad sizes M=%lld N=%d K=%d", (long long)M, N, K);
    DFOL_REQUIRE(dY && X_table_bf16 && src_row && workspace && dW, "linear_wgrad_rows_bf16t: null pointer");
    const char* why = wgrad_rows_bf16t_refusal(N, K, ld_dy, ld_table);
    DFOL_REQUIRE(!why, "linear_wgrad_rows_bf16t: %s (N=%d K=%d ld_dy=%lld ld_table=%lld)", why, N, K, (long long)ld_dy, (long long)ld_table);
    DFOL_REQUIRE((uintptr_t)dY % 16 == 0, "linear_wgrad_rows_bf16t: dY rows must be 16-byte aligned (dY=%p)", (const void*)dY);
    DFOL_REQUIRE((uintptr_t)X_table_bf16 % 8 == 0 && (uintptr_t)src_row % 4 == 0, "linear_wgrad_rows_bf16t: the table must be 8-byte and the index 4-byte aligned");
    return wgrad_tn3_run<1, float, true, uint16_t>("linear_wgrad_rows_bf16t", dY, ld_dy, (const uint16_t*)X_table_bf16, ld_table, src_row, M, N, K, workspace,
                                                   dW, db, (hipStream_t)stream);
}

// The DEFAULT arithmetic's weight gradient over the indexed rows of a bf16 TABLE: dY fp32 in three bf16 pieces, the table's values their own
// one piece, three products per pair (wgrad_tn3_accumulate, NP = 3 over uint16_t X).  Bit for bit dfol_linear_wgrad_bias_f32 over the gathered
// rows widened to fp32 where that runs the bf16-pipe kernel; slabs, workspace layout and reductions are that launch path's.  The fp32 pipe
// (DFOL_WGRAD_MATH=f32) has no indexed form: the predicate says 0 and the entry point refuses.
extern "C" int dfol_linear_wgrad_rows_bf16t_x3_supported(int32_t N, int32_t K, int64_t ld_dy, int64_t ld_table) {
    return wgrad_rows_bf16t_refusal(N, K, ld_dy, ld_table) == nullptr && !wgrad_f32_pipe_asked();
}

extern "C" int dfol_linear_wgrad_bias_rows_bf16t_x3(const float* dY, int64_t ld_dy, const void* X_table_bf16, int64_t ld_table, const int32_t* src_row,
                                                    int64_t M, int32_t N, int32_t K, float* workspace, float* dW, float* db, void* stream) {
    DFOL_REQUIRE(M > 0 && M < (1ll << 31) && N > 0 && K > 0, "linear_wgrad_rows_bf16t_x3: bad sizes M=%lld N=%d K=%d", (long long)M, N, K);
    DFOL_REQUIRE(dY && X_table_bf16 && src_row && workspace && dW, "linear_wgrad_rows_bf16t_x3: null pointer");
    const char* why = wgrad_rows_bf16t_refusal(N, K, ld_dy, ld_table);
    if (!why && wgrad_f32_pipe_asked()) why = "DFOL_WGRAD_MATH=f32 asks for the fp32 matrix pipe, which has no indexed form";
    DFOL_REQUIRE(!why, "linear_wgrad_rows_bf16t_x3: %s (N=%d K=%d ld_dy=%lld ld_table=%lld)", why, N, K, (long long)ld_dy, (long long)ld_table);
    DFOL_REQUIRE((uintptr_t)dY % 16 == 0, "linear_wgrad_rows_bf16t_x3: dY rows must be 16-byte aligned (dY=%p)", (const void*)dY);
    DFOL_REQUIRE((uintptr_t)X_table_bf16 % 8 == 0 && (uintptr_t)src_row % 4 == 0, "linear_wgrad_rows_bf16t_x3: the table must be 8-byte and the index 4-byte aligned");
    return wgrad_tn3_run<3, float, true, uint16_t>("linear_wgrad_rows_bf16t_x3", dY, ld_dy, (const uint16_t*)X_table_bf16, ld_table, src_row, M, N, K,
                                                   workspace, dW, db, (hipStream_t)stream);
}

// bf16 mode with bf16 STORAGE of both operands (the per-pair activations dpre2 [M, N] and Z [M, K] as bfloat16, rows 4-byte / 8-byte
// aligned: ld_dy % 2 == 0, ld_x % 4 == 0 in elements, N and K multiples of 4): one product per pair, fp32 accumulation, fp32 dW and db.
extern "C" int dfol_linear_wgrad_bias_bf16_bf16(const void* dY_bf16, int64_t ld_dy, const void* X_bf16, int64_t ld_x, int64_t M, int32_t N, int32_t K,
                                                float* workspace, float* dW, float* db, void* stream) {
    DFOL_REQUIRE(M > 0 && M < (1ll << 31) && N >= 4 && K >= 4 && N % 4 == 0 && K % 4 == 0, "linear_wgrad_bf16_bf16: bad sizes M=%lld N=%d K=%d (N, K multiples of 4)",
                 (long long)M, N, K);
    DFOL_REQUIRE(dY_bf16 && X_bf16 && workspace && dW, "linear_wgrad_bf16_bf16: null pointer");
    DFOL_REQUIRE(ld_dy % 4 == 0 && ld_x % 4 == 0 && ((uintptr_t)dY_bf16 % 8 == 0) && ((uintptr_t)X_bf16 % 8 == 0), "linear_wgrad_bf16_bf16: rows must be 8-byte aligned");
    return wgrad_tn3_run<1, uint16_t, false>("linear_wgrad_bf16_bf16", (const uint16_t*)dY_bf16, ld_dy, (const uint16_t*)X_bf16, ld_x, nullptr, M, N, K, workspace, dW,
                                             db, (hipStream_t)stream);
}
