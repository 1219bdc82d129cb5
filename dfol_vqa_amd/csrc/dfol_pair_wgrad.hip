// Round 4: the pair layer's weight gradient with dpre2 PRODUCED in the kernel (the logit layer's backward folded in, like
// dfol_pair_dz_fused_f32 does for the input gradient):   dW2[j][c] = sum_r dpre2[r][j] Z[r][c],   db2[j] = sum_r dpre2[r][j],
// dpre2[r][j] = dx[r] E[p(r)][j] h (1 - h), h = Sigmoid(pre2[r][j]).  pre2 and Z are read ONCE (the bf16x3 kernel of csrc/dfol_dense_wgrad.hip reads Z once per
// workgroup class and dpre2 - which no longer exists - on top: 1.6 x the algorithmic bytes), and the operands are two fp16 pieces, three
// products on v_mfma_f32_32x32x16_f16 instead of six bf16 ones.
//
// One workgroup (8 wavefronts, two per SIMD) per row slab, ALL of dW2 in its accumulators: wavefront (a, b) owns the 5 x 2 tiles of 32 x 32
// at rows 160 a .. and columns 64 b .. (160 accumulator registers), H2 <= 320, H1 <= 256.  The operands go through LDS: per macro step of
// 32 rows, thread (column quad c, row octet o) loads the four columns of its eight rows (plain 16-byte loads), builds dpre2 resp. takes Z,
// splits into fp16 pieces and writes, per column, the 16-byte MFMA operand entry (eight consecutive rows = eight consecutive k of the
// MFMA) of both pieces; every wavefront then reads its tiles' entries (conflict-free ds_read_b128).  Two LDS buffers (2 x 72 KB), one
// barrier per macro step; the next macro step's rows are in flight under the MFMAs.
// A row's gradient has no natural scale and the contraction runs over the rows, so ONE power of two S for the whole launch (from the
// caller: S max_r |dx[r]| max|E[p(r)]| / 4 in [2^13, 2^14)) scales dpre2 into fp16's range: an element's error is
// max(2^-23 |a|, 2^-39 max_r(|dx[r]| max|E[p(r)]|)) - rows that far below the largest do not move the sum.  Z is split unscaled (ELU outputs).
#include "dfol_common.h"
#include "dfol_split.h"
#include "dfol_wgrad.h"

#include <type_traits>

constexpr int PW_TA = 10, PW_TB = 8;                                   // 32-wide tiles of H2 (<= 320) and of H1 (<= 256)
constexpr int PW_A_ENT = 2 * 2 * PW_TA * 64, PW_B_ENT = 2 * 2 * PW_TB * 64;   // 16-byte entries per buffer: [k-step][piece][tile][lane]
constexpr int PW_BUF = PW_A_ENT + PW_B_ENT;

__device__ __forceinline__ void pw_split8(const float (&v)[8], u32x4& h, u32x4& l) {
    uint32_t hh[4], ll[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dfol_split2h(v[2 * j], v[2 * j + 1], hh[j], ll[j]);
    h = u32x4{hh[0], hh[1], hh[2], hh[3]};
    l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}

// CPT: columns of dpre2 per thread - 3 when H2 is a multiple of 3 (HID2 = 300: 100 x 4 = 400 building threads with 24 prefetched registers
// each; with 4 - 300 threads, 32 registers - the allocator runs out under the MFMAs and spills a prefetched row right behind its load).
//
// Schedule (second version; the first ran "build all of step s, barrier, multiply step s" and took the SUM of the two phases - 1.2 ms
// + 0.77 ms at 256 x 100 objects - because every wavefront of the CU was in the same phase): the MFMAs of step s are interleaved, in
// the instruction stream of every wavefront, with the building of step s + 1 into the other LDS buffer - two 32 x 32 tile rows of MFMAs
// (12 instructions, 384 cycles of pipe), then one chunk of vector work (a pair of dpre2 rows, or the Z columns), and so on - so the
// SIMD's two wavefronts find each other's gaps.  A pair of rows leaves for LDS as soon as it is built (4-byte pieces of the 16-byte
// operand entries) and its registers are refilled at once with the same rows of step s + 2: one register set is both the prefetch ring
// and the work space.
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
// SUMS: the sums of the logit layer's backward from the same pass (every h and dx is in registers here): per thread the running sums of
// dx h (dE of the current predicate) and of dpre2 (db2) over its rows; the dE sums are flushed where the thread's rows cross into the
// next predicate - its own first row past the boundary, or, for threads whose rows of the boundary step all lie before it, the step
// after - into partials indexed by (slab + predicate, row octet), which pair_sums_reduce_kernel adds in a fixed order.  Needs every
// predicate to own at least 32 rows (or none): a macro step then holds at most one boundary (the launcher's caller checks 64;
// tests/test_pair_wgrad_sums_shapes_gpu.py holds predicates of exactly 32, 33, 40 and 63 rows to the same bounds as the 64-row ones).
// BIO (the bf16 mode): pre2 and Z are rows of bfloat16 (8-byte aligned rows, strides in elements), four columns of dpre2 per thread, ONE
// bf16 piece per operand and one product on v_mfma_f32_32x32x16_bf16; dpre2 is rounded to bfloat16 exactly as dfol_pair_logit_bwd_bf16
// stores it (no scaling: bf16 has fp32's exponent range; `scale` is not read).
// MULTI (several readers of one trunk - relate hops, option slots - in ONE pass): dpre2[r][j] = h (1 - h) sum_k dx_k[r] E_k[p(r)][j], k < nr <= PW_MAXR;
// reader k's dx at G + k g_stride, its embedding rows at E + k e_stride, one row -> predicate map and one scale for all.  Only the
// coefficient changes - gs e[t] becomes ((gs_0 e_0[t] + gs_1 e_1[t]) + gs_2 e_2[t]) + gs_3 e_3[t], absent readers entering as exact zeros (one
// reader: the bits of the kernel without MULTI) - and the schedule stays.  The embedding rows of the step's predicate, all readers, are
// staged in the LDS the sums of SUMS would occupy, [column][reader], and read where the coefficient is formed (one ds_read_b128 per column:
// no nr x CPT registers under the MFMAs); two slots: the rows of the NEXT step's predicate are written one step ahead, where the predicate
// changes, and the step's closing barrier publishes them.  Octets across a predicate boundary or cut by the slab's end look their rows
// up one by one, once per reader, as before.
constexpr int PW_MAXR = 4;
template <int CPT, bool SUMS, bool BIO = false, bool MULTI = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void pair_wgrad_fused_kernel(
    const void* __restrict__ P2v, int64_t ld_p2, const float* __restrict__ G, const int32_t* __restrict__ RP, const int64_t* __restrict__ pred_off,
    const float* __restrict__ E, int64_t ld_e, const float* __restrict__ scale, const void* __restrict__ Zv, int64_t ld_z, int M, int H2, int H1,
    int rows_per_slab, float* __restrict__ part, float* __restrict__ de_part, float* __restrict__ db_part, int nr, int64_t g_stride,
    int64_t e_stride) {
    static_assert(!BIO || CPT == 4, "bf16 storage: four columns (8 bytes) per thread and row");
    static_assert(!MULTI || (!SUMS && !BIO), "several readers: fp32 storage, the sums come from the readers' own passes");
    typedef typename std::conditional<BIO, uint16_t, float>::type TIN;
    const TIN* __restrict__ P2 = reinterpret_cast<const TIN*>(P2v);
    const TIN* __restrict__ Z = reinterpret_cast<const TIN*>(Zv);
    constexpr int EB = sizeof(TIN), NPC = BIO ? 1 : 2;                // bytes per stored element; pieces per operand
    constexpr int A_ENT = 2 * NPC * PW_TA * 64, B_ENT = 2 * NPC * PW_TB * 64, BUFK = A_ENT + B_ENT;      // 16-byte entries: [k-step][piece][tile][lane]
    extern __shared__ __attribute__((aligned(16))) u32x4 pw_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m_begin = blockIdx.x * rows_per_slab, m_end = min(M, m_begin + rows_per_slab);
    const int steps = (m_end - m_begin + 31) >> 5;
    const int QA = H2 / CPT, QB = H1 >> 1;
    const float S = BIO ? 1.0f : scale[0], invS = BIO ? 1.0f : scale[1];

    // Roles per macro step of 32 rows.  dpre2: thread (column group ca, row octet oa) for tid < 4 QA - eight rows x CPT columns, the
    // expensive part (a Sigmoid derivative per element).  Z: thread (column pair cz, row octet oz) for tid < 4 QB - eight rows x two columns.
    const bool is_a = tid < 4 * QA;
    const int ca = is_a ? tid % QA : 0, oa = is_a ? tid / QA : 0;
    const bool is_z = tid < 4 * QB;
    const int cz = is_z ? tid % QB : 0, oz = is_z ? tid / QB : 0;

    for (int i = tid; i < 2 * BUFK; i += 512) pw_lds[i] = u32x4{0u, 0u, 0u, 0u};      // (columns past the matrices stay zero for good)

    f32x16 acc[5][2];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

    // The rows of a macro step come through buffer descriptors rebuilt per step from wave-uniform values (base = the step's first row,
    // size = what is left of the slab), with per-lane byte offsets that never change and the row within the octet as the scalar offset:
    // no 64-bit address arithmetic on the vector ALU, and rows past the slab read as zero (dx = 0 switches such a row off).
    typename std::conditional<BIO, u32x2, typename std::conditional<CPT == 3, u32x3, u32x4>::type>::type xa[8];
    typename std::conditional<BIO, uint32_t, u32x2>::type xz[8];
    // The predicate of the step's first row and the row its range ends at, wave-uniform (the rows of a predicate are contiguous and
    // row_pred is non-decreasing): an octet that ends before that row reads the predicate's embedding columns through a uniform base; the
    // few octets at a boundary look their rows up one by one.
    int p_cur = 0, end_cur = 0;                                        // (M < 2^31)
    if (steps > 0) {
        p_cur = __builtin_amdgcn_readfirstlane(RP[m_begin]);
        end_cur = __builtin_amdgcn_readfirstlane((int)pred_off[p_cur + 1]);
    }
    // The thread's constants (byte offsets of its loads, its columns) live in LDS and are re-read where they are used: registers that would
    // otherwise sit idle under the MFMAs, where accumulators + operand fragments + the row ring fill the 256 of a wavefront.
    int* cst = reinterpret_cast<int*>(pw_lds + 2 * BUFK) + tid;       // [2][512] words, then (SUMS) the threads' running sums [2 CPT][512]
    const int rs_p = (int)(ld_p2 * EB), rs_z = (int)(ld_z * EB);
    // the 16-byte LDS entry of column `col` (tile col >> 5, row col & 31 of the MFMA operand) for the eight rows of octet o
    auto entry = [&](int col, int o, int tiles) __attribute__((always_inline)) { return ((o >> 1) * NPC * tiles + (col >> 5)) * 64 + (col & 31) + 32 * (o & 1); };
    cst[0] = ca | (oa << 16);                                          // (two words per thread; everything else is derived where it is used)
    cst[512] = cz | (oz << 16);
    auto k_oa = [&]() __attribute__((always_inline)) { return cst[0] >> 16; };
    auto k_col0 = [&]() __attribute__((always_inline)) { return CPT * (cst[0] & 0xffff); };                    // the thread's first column of dpre2
    auto k_goff = [&]() __attribute__((always_inline)) { return 32 * (cst[0] >> 16); };                        // byte offset of its octet's dx
    auto k_voff_a = [&]() __attribute__((always_inline)) { const int w = cst[0]; return (8 * (w >> 16) * (int)ld_p2 + CPT * (w & 0xffff)) * EB; };
    auto k_voff_z = [&]() __attribute__((always_inline)) { const int w = cst[512]; return (8 * (w >> 16) * (int)ld_z + 2 * (w & 0xffff)) * EB; };
    auto k_at_z = [&]() __attribute__((always_inline)) { const int w = cst[512]; return A_ENT + entry(2 * (w & 0xffff), w >> 16, PW_TB); };   // entry of its first Z column

    struct Desc { __amdgpu_buffer_rsrc_t p, z, g; };
    auto descriptors = [&](int s) __attribute__((always_inline)) {     // step s (past the slab: empty ranges, every load returns zero)
        const int first = m_begin + 32 * s, left = max(m_end - first, 0);
        Desc d;
        d.p = w3_descriptor(P2 + (int64_t)first * ld_p2, left > 0 ? ((int64_t)(left - 1) * ld_p2 + H2) * EB : 0);
        d.z = w3_descriptor(Z + (int64_t)first * ld_z, left > 0 ? ((int64_t)(left - 1) * ld_z + H1) * EB : 0);
        d.g = w3_descriptor(G + first, (int64_t)left * 4);
        return d;
    };
    auto load_a = [&](const Desc& d, int i) __attribute__((always_inline)) {           // row i of the thread's octet
        const int voff_a = k_voff_a();
        if constexpr (BIO) xa[i] = __builtin_amdgcn_raw_buffer_load_b64(d.p, voff_a, i * rs_p, 0);
        else if constexpr (CPT == 3) xa[i] = __builtin_amdgcn_raw_buffer_load_b96(d.p, voff_a, i * rs_p, 0);
        else xa[i] = __builtin_amdgcn_raw_buffer_load_b128(d.p, voff_a, i * rs_p, 0);
    };
    auto load_z = [&](const Desc& d) __attribute__((always_inline)) {
        const int voff_z = k_voff_z();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (BIO) xz[i] = __builtin_amdgcn_raw_buffer_load_b32(d.z, voff_z, i * rs_z, 0);
            else xz[i] = __builtin_amdgcn_raw_buffer_load_b64(d.z, voff_z, i * rs_z, 0);
        }
    };

    // ---- building step s (its rows are in xa / xz) into `buf`, a chunk at a time; `next`: the descriptors of step s + 1, whose rows refill
    // the registers as they are released
    // SUMS: the running sums live in LDS (the accumulators leave no register that survives the MFMAs: held in registers they were
    // spilled to scratch and reloaded four times a step, 2.44 ms against 1.77 for the kernel without them) and are read, added to and
    // written back by every pair of rows
    float* sums = reinterpret_cast<float*>(pw_lds + 2 * BUFK) + 1024 + tid;       // [2 CPT][512]: dE sums, then db2 sums
    if constexpr (SUMS) {
#pragma unroll
        for (int t = 0; t < 2 * CPT; ++t) sums[512 * t] = 0.f;
    }
    auto flush_de = [&](int p) __attribute__((always_inline)) {        // this thread's dE sums of predicate p -> partial row (slab + p, octet); cleared
        if constexpr (SUMS) {
            float* o = de_part + (((int64_t)blockIdx.x + p) * 4 + k_oa()) * H2 + k_col0();
#pragma unroll
            for (int t = 0; t < CPT; ++t) o[t] = sums[512 * t] * invS, sums[512 * t] = 0.f;
        }
    };
    bool same = false;
    float ev[MULTI ? 1 : CPT];
    u32x2 gq;                                                       // dx of the row pair that comes next
    // MULTI: the staged embedding rows [2 slots][320 columns] x {reader 0..3} behind the constant words, `slot` holding the rows of p_cur;
    // then the readers' dx of two steps, [step parity][32 rows] x {reader 0..3} (absent readers, rows past the slab: zeros), written one step
    // ahead by 128 threads: eight dx registers per thread prefetched under the MFMAs, as the one reader's two are, do not fit
    float4* etab = reinterpret_cast<float4*>(pw_lds + 2 * BUFK + 256);
    float4* dxs = etab + 2 * 32 * PW_TA;
    int slot = 0;
    float gnext = 0.f;
    // (both stagings address through wave-uniform descriptors and the lane number taken where it is needed - v_mbcnt - so that no per-thread
    // address survives the MFMAs; loads past a descriptor's range return zero)
    auto lane_now = []() __attribute__((always_inline)) { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); };
    auto fetch_g = [&](int sn) __attribute__((always_inline)) {        // wavefront q < 4, lane < 32: reader q's dx of row `lane` of step sn
        if (wave < PW_MAXR) {
            const int first = m_begin + 32 * sn, left = min(max(m_end - first, 0), 32);
            const auto dg = w3_descriptor(G + (int64_t)min(wave, nr - 1) * g_stride + first, wave < nr ? (int64_t)left * 4 : 0);
            gnext = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(dg, 4 * lane_now(), 0, 0));
        }
    };
    auto put_g = [&](int sn) __attribute__((always_inline)) {
        const int l = lane_now();
        if (wave < PW_MAXR && l < 32) reinterpret_cast<float*>(dxs)[(sn & 1) * 32 * PW_MAXR + PW_MAXR * l + wave] = gnext;
    };
    auto stage = [&](int p, int sl) __attribute__((always_inline)) {   // thread j < H2: column j of predicate p's rows, every reader
        if (wave < PW_TA / 2) {
            const int j = 64 * wave + lane_now();
            float e4[PW_MAXR];
#pragma unroll
            for (int q = 0; q < PW_MAXR; ++q) {
                const auto de = w3_descriptor(E + (int64_t)min(q, nr - 1) * e_stride + (int64_t)p * ld_e, q < nr ? (int64_t)H2 * 4 : 0);
                e4[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(de, 4 * j, 0, 0));
            }
            etab[sl * (32 * PW_TA) + j] = make_float4(e4[0], e4[1], e4[2], e4[3]);
        }
    };
    auto lookahead = [&](int sn) __attribute__((always_inline)) {      // step sn opens under another predicate than p_cur: its rows -> the other slot
        if (sn < steps) {
            int pn = p_cur, en = end_cur;
            while (m_begin + 32 * sn >= en) {
                ++pn;
                en = __builtin_amdgcn_readfirstlane((int)pred_off[pn + 1]);
            }
            if (pn != p_cur) stage(pn, slot ^ 1);
        }
    };
    auto begin_a = [&](int s, const Desc& d) __attribute__((always_inline)) {          // before the first pair of rows
        if (is_a) {
            const int goff = k_goff(), col0 = k_col0();
            const int first = m_begin + 32 * s + (goff >> 2);         // the octet's first row
            same = first + 7 < m_end && first + 7 < end_cur;          // (all eight rows exist and belong to p_cur)
            if constexpr (!MULTI) {
#pragma unroll
                for (int t = 0; t < CPT; ++t) ev[t] = 0.f;
                if (same) {
#pragma unroll
                    for (int t = 0; t < CPT; ++t) ev[t] = E[(int64_t)p_cur * ld_e + col0 + t];
                }
                gq = __builtin_amdgcn_raw_buffer_load_b64(d.g, goff, 0, 0);
            }
        }
    };
    auto pair_a = [&](int s, int k, const Desc& d, const Desc& next, uint32_t* __restrict__ buf32) __attribute__((always_inline)) {   // rows 2 k, 2 k + 1
        if (is_a) {
            const int goff = k_goff(), col0 = k_col0(), o = k_oa();
            const int first = m_begin + 32 * s + (goff >> 2);
            float v[2][CPT];
            float sde[SUMS ? CPT : 1], sdb[SUMS ? CPT : 1];            // this pair's share of the running sums (added to LDS once, below)
#pragma unroll
            for (int t = 0; t < (SUMS ? CPT : 1); ++t) sde[t] = sdb[t] = 0.f;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = 2 * k + r;
                float e[CPT];
#pragma unroll
                for (int t = 0; t < CPT; ++t) e[t] = ev[MULTI ? 0 : t];
                if (!MULTI && !same) {                                 // (an octet across two predicates, or cut by the slab's end)
                    const float* er = E + (int64_t)RP[min(first + i, m_end - 1)] * ld_e + col0;
#pragma unroll
                    for (int t = 0; t < CPT; ++t) e[t] = er[t];
                }
                const float gs = MULTI ? 0.f : __uint_as_float(gq[r]) * S;      // (rows past the slab were read as zero)
                float cf[MULTI ? CPT : 1];                             // MULTI: the row's coefficients sum_k gs_k e_k[t], readers in order
                if constexpr (MULTI) {
                    if (r == 1) __builtin_amdgcn_sched_barrier(0);     // (a row at a time: both rows' staged operands at once cost a ring row its registers)
                    const float4 g4 = dxs[(s & 1) * 32 + 8 * o + i];
                    const float gm[PW_MAXR] = {g4.x * S, g4.y * S, g4.z * S, g4.w * S};
                    if (same) {
#pragma unroll
                        for (int t = 0; t < CPT; ++t) {
                            // (four columns per thread: a column at a time - the four staged entries read at once cost a ring row its registers)
                            if (CPT == 4 && t > 0) __builtin_amdgcn_sched_barrier(0);
                            const float4 e4 = etab[slot * (32 * PW_TA) + col0 + t];
                            cf[t] = fmaf(gm[3], e4.w, fmaf(gm[2], e4.z, fmaf(gm[1], e4.y, gm[0] * e4.x)));
                        }
                    } else {                                           // (an octet across two predicates, or cut by the slab's end)
                        const float* er = E + (int64_t)RP[min(first + i, m_end - 1)] * ld_e + col0;
#pragma unroll
                        for (int t = 0; t < CPT; ++t) cf[t] = gm[0] * er[t];
#pragma unroll
                        for (int q = 1; q < PW_MAXR; ++q)
                            if (q < nr) {
                                __builtin_amdgcn_sched_barrier(0);     // (a reader at a time: all readers' rows at once cost a ring row its registers)
#pragma unroll
                                for (int t = 0; t < CPT; ++t) cf[t] = fmaf(gm[q], er[(int64_t)q * e_stride + t], cf[t]);
                            }
                    }
                }
                if constexpr (SUMS) {
                    if (!same) {                                       // this thread's first row past the predicate's end: its sums so far belong to p_cur
                        const int rr = first + i;
                        if (rr >= end_cur && (i == 0 || rr - 1 < end_cur)) {
#pragma unroll
                            for (int t = 0; t < CPT; ++t) sums[512 * t] += sde[t], sde[t] = 0.f;       // (the pair's first row, if it lies before the end)
                            flush_de(p_cur);
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < CPT; ++t) {
                    float xv;
                    if constexpr (BIO) xv = __uint_as_float((t & 1) ? (xa[i][t >> 1] & 0xffff0000u) : (xa[i][t >> 1] << 16));
                    else xv = __uint_as_float(xa[i][t]);
                    const float hh = dfol_sigmoid_hw(xv);
                    if constexpr (BIO) v[r][t] = __uint_as_float(dfol_rne2(gs * e[t] * hh * (1.0f - hh), 0.f) << 16);      // (the value dfol_pair_logit_bwd_bf16 stores)
                    else if constexpr (MULTI) v[r][t] = cf[t] * (hh * (1.0f - hh));
                    else v[r][t] = (gs * e[t]) * (hh * (1.0f - hh));
                    if constexpr (SUMS) {
                        sde[t] = fmaf(gs, hh, sde[t]);
                        sdb[t] += v[r][t];
                    }
                }
            }
            if constexpr (SUMS) {
#pragma unroll
                for (int t = 0; t < CPT; ++t) sums[512 * t] += sde[t], sums[512 * (CPT + t)] += sdb[t];
            }
            if constexpr (!MULTI) {
                if (k < 3) gq = __builtin_amdgcn_raw_buffer_load_b64(d.g, goff, 8 * (k + 1), 0);
            }
            if constexpr (!MULTI) {
                load_a(next, 2 * k);                                   // the same rows of the next step: in flight for a whole step
                load_a(next, 2 * k + 1);
            }
#pragma unroll
            for (int t = 0; t < CPT; ++t) {
                const int at = entry(col0 + t, o, PW_TA) * 4 + k;      // 4-byte piece k of the entry: rows 2 k, 2 k + 1
                if constexpr (BIO) {
                    buf32[at] = (__float_as_uint(v[0][t]) >> 16) | (__float_as_uint(v[1][t]) & 0xffff0000u);      // (rounded above: the high halves are the bf16 bits)
                } else {
                    uint32_t h, l;
                    dfol_split2h(v[0][t], v[1][t], h, l);
                    buf32[at] = h;
                    buf32[at + PW_TA * 64 * 4] = l;
                }
            }
            if constexpr (MULTI) {                                     // (after the pair has left: with the pair's values still held, four columns cost a ring row its registers)
                load_a(next, 2 * k);
                load_a(next, 2 * k + 1);
            }
        }
    };
    auto columns_z = [&](const Desc& next, u32x4* __restrict__ buf) __attribute__((always_inline)) {
        if (is_z) {
            const int at = k_at_z();
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if constexpr (BIO) {                                   // eight rows' halfword c of one word each -> the entry's four words (row 2 j in the low half)
                    u32x4 en;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        en[j] = c ? ((xz[2 * j] >> 16) | (xz[2 * j + 1] & 0xffff0000u)) : ((xz[2 * j] & 0xffffu) | (xz[2 * j + 1] << 16));
                    buf[at + c] = en;
                } else {
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = __uint_as_float(xz[i][c]);
                    u32x4 h, l;
                    pw_split8(v, h, l);
                    buf[at + c] = h;
                    buf[at + c + PW_TB * 64] = l;
                }
            }
            load_z(next);
        }
    };
    const int ta0 = 5 * (wave >> 2), tb0 = 2 * (wave & 3);
    // one tile row of the step's MFMAs: k-step ks, A tile t against both B tiles (fragments read just before)
    auto tile_row = [&](const u32x4* __restrict__ buf, int ks, int t) __attribute__((always_inline)) {
        const u32x4* Ab = buf + ks * NPC * PW_TA * 64 + lane;
        const u32x4* Bb = buf + A_ENT + ks * NPC * PW_TB * 64 + lane;
        if constexpr (BIO) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, Ab[(ta0 + t) * 64]);
#pragma unroll
            for (int u = 0; u < 2; ++u)
                acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, Bb[(tb0 + u) * 64]), acc[t][u], 0, 0, 0);
            return;
        }
        const f16x8 ah = __builtin_bit_cast(f16x8, Ab[(ta0 + t) * 64]), al = __builtin_bit_cast(f16x8, Ab[((NPC - 1) * PW_TA + ta0 + t) * 64]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {                                  // smallest terms first
            const f16x8 bh = __builtin_bit_cast(f16x8, Bb[(tb0 + u) * 64]), bl = __builtin_bit_cast(f16x8, Bb[((NPC - 1) * PW_TB + tb0 + u) * 64]);
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t][u], 0, 0, 0);
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t][u], 0, 0, 0);
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t][u], 0, 0, 0);
        }
    };
    auto fence = []() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };

    // prologue: step 0 is built on its own (nothing to multiply yet); its chunks already refill the ring with step 1
    if (steps > 0) {
        const Desc d0 = descriptors(0), d1 = descriptors(1);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (is_a) load_a(d0, i);
        if (is_z) load_z(d0);
        if constexpr (MULTI) {
            stage(p_cur, 0);
            lookahead(1);
            fetch_g(0), put_g(0);
            fetch_g(1), put_g(1);
        }
        __syncthreads();                                               // the zeroed buffers
        begin_a(0, d0);
#pragma unroll
        for (int k = 0; k < 4; ++k) pair_a(0, k, d0, d1, reinterpret_cast<uint32_t*>(pw_lds));
        columns_z(d1, pw_lds);
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const u32x4* cur = pw_lds + (s & 1) * BUFK;
        u32x4* nxt = pw_lds + ((s + 1) & 1) * BUFK;
        uint32_t* nxt32 = reinterpret_cast<uint32_t*>(nxt);
        const bool more = s + 1 < steps;                               // (uniform) is there a step s + 1 to build
        const int p_old = p_cur, end_old = end_cur;
        while (more && m_begin + 32 * (s + 1) >= end_cur) {            // (scalar; predicates without rows are stepped over)
            ++p_cur;
            end_cur = __builtin_amdgcn_readfirstlane((int)pred_off[p_cur + 1]);
        }
        if constexpr (SUMS) {
            // the predicate ended inside step s: the threads whose octet of step s reached its end have flushed there, the others flush now
            if (p_cur != p_old && is_a && m_begin + 32 * s + 8 * k_oa() + 7 < end_old) flush_de(p_old);
        }
        if constexpr (MULTI) {
            if (p_cur != p_old) slot ^= 1;                             // (its rows were staged a step ago; this step's barrier publishes the next)
            lookahead(s + 2);
        }
        const Desc d1 = descriptors(s + 1), d2 = descriptors(s + 2);
        if (more) begin_a(s + 1, d1);
        fence();
        tile_row(cur, 0, 0); tile_row(cur, 0, 1);
        fence();
        if (more) pair_a(s + 1, 0, d1, d2, nxt32);
        fence();
        tile_row(cur, 0, 2); tile_row(cur, 0, 3);
        fence();
        if (more) pair_a(s + 1, 1, d1, d2, nxt32);
        fence();
        tile_row(cur, 0, 4); tile_row(cur, 1, 0);
        fence();
        if (more) pair_a(s + 1, 2, d1, d2, nxt32);
        fence();
        tile_row(cur, 1, 1); tile_row(cur, 1, 2);
        fence();
        if (more) pair_a(s + 1, 3, d1, d2, nxt32);
        if constexpr (MULTI) fetch_g(s + 2);                           // (in flight under the last two tile rows only)
        fence();
        tile_row(cur, 1, 3);
        fence();
        if (more) columns_z(d2, nxt);
        fence();
        tile_row(cur, 1, 4);
        fence();
        if constexpr (MULTI) put_g(s + 2);
        __syncthreads();                                               // step s + 1 is complete in LDS; everyone is past the MFMAs of step s
    }

    if constexpr (SUMS) {
        if (steps > 0 && is_a) {
            const bool crossed = m_begin + 32 * (steps - 1) + 8 * k_oa() + 7 >= end_cur;      // (this thread's sums already belong to the next predicate)
            if (!crossed) flush_de(p_cur);
            if (end_cur < m_end) {                                     // (uniform) the slab's last rows open another predicate: its partial row is written by everyone
                int p_nxt = p_cur + 1;
                while ((int)pred_off[p_nxt + 1] <= end_cur) ++p_nxt;   // (predicates without rows)
                flush_de(__builtin_amdgcn_readfirstlane(p_nxt));
            }
        }
        // A slab WITHOUT rows (above 65 536 rows the rounding of rows_per_slab to 32 can leave whole slabs past M) writes its zero sums too:
        // pair_sums_reduce_kernel adds the db2 partial rows of EVERY slab, and the workspace is not cleared.  (Its dE partial rows are not
        // read: the reduce takes only the slabs that hold rows of the predicate.)
        if (is_a) {
            float* o = db_part + ((int64_t)blockIdx.x * 4 + k_oa()) * H2 + k_col0();
#pragma unroll
            for (int t = 0; t < CPT; ++t) o[t] = sums[512 * (CPT + t)] * invS;
        }
    }
    // D tile: column j = lane & 31, row i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int64_t stride = wgrad_slab_stride((int64_t)H2 * H1);
    float* out = part + (int64_t)blockIdx.x * stride;
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = 32 * (tb0 + u) + (lane & 31);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int n = 32 * (ta0 + t) + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                if (n < H2 && k < H1) out[(int64_t)n * H1 + k] = acc[t][u][i] * invS;
            }
        }
}

static int pw_slabs(int64_t M) { return (int)std::max<int64_t>(1, std::min<int64_t>(256, (M + 255) / 256)); }
static int pw_rows_per_slab(int64_t M) { return (dfol_cdiv(M, pw_slabs(M)) + 31) & ~31; }      // (a macro step is 32 rows)

extern "C" int64_t dfol_pair_wgrad_fused_workspace(int64_t M, int32_t H2, int32_t H1) {
    if (M <= 0 || H2 <= 0 || H1 <= 0) return 0;
    return (int64_t)pw_slabs(M) * wgrad_slab_stride((int64_t)H2 * H1);
}

// The partial sums of pair_wgrad_fused_kernel<.., true> in a fixed order.  Block p < P: dE[p][:] from the partial rows (slab + p, octet) of
// the slabs that hold rows of p, and dbe[p] = the sum of dx over p's rows; blocks P .. P + 7: db2 from every slab's four octet rows.
__global__ __launch_bounds__(320) void pair_sums_reduce_kernel(const float* __restrict__ de_part, const float* __restrict__ db_part,
                                                               const float* __restrict__ dx, const int64_t* __restrict__ pred_off, int P, int H2,
                                                               int slabs, int rows_per_slab, float* __restrict__ dE, int64_t ld_de,
                                                               float* __restrict__ dbe, float* __restrict__ db2) {
    __shared__ float red[320];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (p >= P) {                                                      // db2: 8 blocks of 40 columns, 8 row phases each (one thread walking all 4 x slabs rows of a column took 0.25 ms)
        const int c = (p - P) * 40 + tid % 40, ph = tid / 40;
        float acc = 0.f;
        if (c < H2)
            for (int r = ph; r < slabs * 4; r += 8) acc += db_part[(int64_t)r * H2 + c];
        red[tid] = acc;
        __syncthreads();
        if (ph == 0 && c < H2) {
            float t = 0.f;
            for (int i = 0; i < 8; ++i) t += red[i * 40 + tid];
            db2[c] = t;
        }
        return;
    }
    const int64_t r0 = pred_off[p], r1 = pred_off[p + 1];
    float acc = 0.f;
    if (r1 > r0 && tid < H2) {
        const int s0 = (int)(r0 / rows_per_slab), s1 = (int)((r1 - 1) / rows_per_slab);
        for (int s = s0; s <= s1; ++s)
            for (int o = 0; o < 4; ++o) acc += de_part[(((int64_t)s + p) * 4 + o) * H2 + tid];
    }
    if (tid < H2) dE[(int64_t)p * ld_de + tid] = acc;
    if (dbe) {
        float g = 0.f;
        for (int64_t r = r0 + tid; r < r1; r += 320) g += dx[r];
        red[tid] = g;
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            for (int i = 0; i < 320; ++i) t += red[i];
            dbe[p] = t;
        }
    }
}

// floats of workspace for dfol_pair_wgrad_fused_sums_f32: the slabs' dW2 partials, then the dE partial rows ((slabs + P) x 4 x HID2)
// and the db2 partial rows (slabs x 4 x HID2)
extern "C" int64_t dfol_pair_wgrad_fused_sums_workspace(int64_t M, int32_t H2, int32_t H1, int32_t P) {
    if (M <= 0 || H2 <= 0 || H1 <= 0 || P < 0) return 0;
    const int64_t slabs = pw_slabs(M);
    return slabs * wgrad_slab_stride((int64_t)H2 * H1) + (2 * slabs + P) * 4 * (int64_t)H2;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Several readers of one trunk in ONE weight-gradient pass (pair_wgrad_fused_kernel<.., MULTI>): dW2 = sum_k dpre2_k^T Z with pre2 and Z read
// once instead of once per reader.  The readers' own sums (dE, dbe, db2) stay with dfol_pair_logit_bwd_sums_f32.

// The launch's scale without a host sync: the largest row bound sum_k |dx_k[r]| emax_k[p(r)] / 4 (formed as tall_row_scale_multi_kernel forms a
// row's, csrc/dfol_dense_tall.hip) as the bits of a non-negative float - their order is the integers' order and a maximum does not depend
// on the order of its updates, so the atomic keeps the run repeatable - then {S, 1 / S} of it.
__global__ __launch_bounds__(256) void pair_wgrad_multi_bound_kernel(const float* __restrict__ dx, int64_t dx_stride, const int32_t* __restrict__ row_pred,
                                                                     const float* __restrict__ emax, int P, int nr, int M,
                                                                     uint32_t* __restrict__ bound_max) {
    __shared__ float wmax[4];
    float m = 0.f;
    for (int r = blockIdx.x * 256 + (int)threadIdx.x; r < M; r += gridDim.x * 256) {
        const int p = row_pred[r];
        float bound = 0.f;
#pragma unroll
        for (int q = 0; q < PW_MAXR; ++q) {
            const float g = (p >= 0 && q < nr) ? dx[(int64_t)q * dx_stride + r] : 0.f;
            bound += fabsf(g) * (q < nr ? emax[(int64_t)q * P + max(p, 0)] : 0.f) * 0.25f;
        }
        if (bound > 0.f && bound < 3.0e38f) m = fmaxf(m, bound);         // (a non-finite bound leaves the scale alone; the products show the NaN)
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        if (m > 0.f) atomicMax(bound_max, __float_as_uint(m));
    }
}
__global__ void pair_wgrad_multi_scale_kernel(const float* __restrict__ bound_max, float* __restrict__ scale) {
    const int e = dfol_scale_exp(bound_max[0]);
    scale[0] = ldexpf(1.0f, e);
    scale[1] = ldexpf(1.0f, -e);
}

// scale [3] (device): {S, 1 / S}, then the bound itself; dx [nr][dx_stride >= M], emax [nr][P] = max_j |E_k[p][j]|, row_pred [M] (< 0: no gradient)
extern "C" int dfol_pair_wgrad_multi_scale_f32(const float* dx, int64_t dx_stride, int32_t nr, const int32_t* row_pred, const float* emax, int32_t P,
                                               int64_t M, float* scale, void* stream) {
    DFOL_REQUIRE(nr >= 1 && nr <= PW_MAXR && P >= 1 && M > 0 && M < (1ll << 31) - 64 && dx_stride >= M,
                 "pair_wgrad_multi_scale: %d readers (1..%d), P=%d, M=%lld, dx_stride=%lld", nr, PW_MAXR, P, (long long)M, (long long)dx_stride);
    DFOL_REQUIRE(dx && row_pred && emax && scale, "pair_wgrad_multi_scale: null pointer");
    hipStream_t st = (hipStream_t)stream;
    DFOL_REQUIRE(hipMemsetAsync(scale + 2, 0, 4, st) == hipSuccess, "pair_wgrad_multi_scale: hipMemsetAsync failed");
    hipLaunchKernelGGL(pair_wgrad_multi_bound_kernel, dim3((unsigned)std::min<int64_t>(dfol_cdiv(M, 256), 1024)), dim3(256), 0, st, dx, dx_stride, row_pred, emax, P,
                       nr, (int)M, reinterpret_cast<uint32_t*>(scale + 2));
    hipLaunchKernelGGL(pair_wgrad_multi_scale_kernel, dim3(1), dim3(1), 0, st, (const float*)(scale + 2), scale);
    DFOL_LAUNCH_CHECK("pair_wgrad_multi_scale");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The launch path of every form of pair_wgrad_fused_kernel.  The operands every form takes, as the entry points get them:
struct PwArgs {
    const void* pre2; int64_t ld_p2; const float* dx; const int32_t* row_pred; const int64_t* pred_off; const float* E; int64_t ld_e;
    const float* scale; const void* Z; int64_t ld_z, M; int32_t H2, H1; float *workspace, *dW;
};

// sizes, strides and alignment; `who` names the entry points in the message; bio: bf16 storage (8-byte aligned rows, `scale` is not read)
static int pw_check(const char* who, const PwArgs& a, bool bio) {
    DFOL_REQUIRE(a.M > 0 && a.M < (1ll << 31) - 64 && a.H2 >= 4 && a.H1 >= 4 && a.H2 % 4 == 0 && a.H1 % 4 == 0 && a.H2 <= 32 * PW_TA && a.H1 <= 32 * PW_TB,
                 "%s: bad sizes M=%lld H2=%d H1=%d (multiples of 4, H2 <= %d, H1 <= %d)", who, (long long)a.M, a.H2, a.H1, 32 * PW_TA, 32 * PW_TB);
    DFOL_REQUIRE(a.pre2 && a.dx && a.row_pred && a.pred_off && a.E && (a.scale || bio) && a.Z && a.workspace && a.dW, "%s: null pointer", who);
    DFOL_REQUIRE(a.ld_p2 >= a.H2 && a.ld_z >= a.H1 && a.ld_e >= a.H2, "%s: row strides ld_p2=%lld ld_z=%lld ld_e=%lld must cover H2=%d, H1=%d, H2", who,
                 (long long)a.ld_p2, (long long)a.ld_z, (long long)a.ld_e, a.H2, a.H1);
    DFOL_REQUIRE(a.ld_p2 % 4 == 0 && a.ld_z % 4 == 0 && a.ld_e % 4 == 0 && ((uintptr_t)a.pre2 % (bio ? 8 : 16) == 0) && ((uintptr_t)a.Z % (bio ? 8 : 16) == 0) &&
                 ((uintptr_t)a.E % 16 == 0), "%s: rows of pre2, Z and E must be 16-byte (bf16 storage: 8-byte) aligned", who);
    DFOL_REQUIRE(8 * std::max(a.ld_p2, a.ld_z) * 4 * 4 < (1ll << 31), "%s: row stride too large (%lld)", who, (long long)std::max(a.ld_p2, a.ld_z));
    return 0;
}

// Dynamic LDS: two operand buffers, 2 + 6 words per thread (fp32 storage with CPT = 4 and the sums - 2 + 8 words per thread - does not fit;
// two slots of 320 x 4 staged floats fit the 12 KB behind the constant words).  bf16 storage: one piece per operand, the two buffers are half the size.
constexpr size_t pw_lds_bytes(bool bio) { return bio ? (size_t)PW_BUF * 16 + (2 + 8) * 512 * 4 : (size_t)2 * PW_BUF * 16 + (2 + 6) * 512 * 4; }
static_assert(2 * 32 * PW_TA * PW_MAXR * 4 <= 6 * 512 * 4, "the staged embedding rows must fit behind the constant words");

// One instantiation (it reserves its LDS when it is first used): one workgroup per slab, then the slabs' dW2 blocks added up.
// de_part, db_part: the partial rows of SUMS; nr, g_stride, e_stride: the readers of MULTI
template <int CPT, bool SUMS, bool BIO, bool MULTI>
static int pw_run(const char* who, const PwArgs& a, float* de_part, float* db_part, int nr, int64_t g_stride, int64_t e_stride, hipStream_t st) {
    constexpr size_t lds = pw_lds_bytes(BIO);
    static const hipError_t ok = hipFuncSetAttribute((const void*)pair_wgrad_fused_kernel<CPT, SUMS, BIO, MULTI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    DFOL_REQUIRE(ok == hipSuccess, "%s: cannot reserve %zu bytes of LDS (%s)", who, lds, hipGetErrorString(ok));
    const int slabs = pw_slabs(a.M);
    hipLaunchKernelGGL((pair_wgrad_fused_kernel<CPT, SUMS, BIO, MULTI>), dim3(slabs), dim3(512), lds, st, a.pre2, a.ld_p2, a.dx, a.row_pred, a.pred_off, a.E, a.ld_e,
                       a.scale, a.Z, a.ld_z, (int)a.M, a.H2, a.H1, pw_rows_per_slab(a.M), a.workspace, de_part, db_part, nr, g_stride, e_stride);
    DFOL_LAUNCH_CHECK(who);
    return wgrad_reduce(who, "reduce", a.workspace, slabs, (int64_t)a.H2 * a.H1, a.dW, st);
}

static int pw_launch(const void* pre2, int64_t ld_p2, const float* dx, const int32_t* row_pred, const int64_t* pred_off, int32_t P, const float* E,
                     int64_t ld_e, const float* scale, const void* Z, int64_t ld_z, int64_t M, int32_t H2, int32_t H1, float* workspace, float* dW,
                     float* dE, int64_t ld_de, float* dbe, float* db2, bool sums, void* stream, bool bio = false) {
    const char* who = "pair_wgrad_fused";
    const PwArgs a = {pre2, ld_p2, dx, row_pred, pred_off, E, ld_e, scale, Z, ld_z, M, H2, H1, workspace, dW};
    if (const int rc = pw_check(who, a, bio)) return rc;
    const int slabs = pw_slabs(M);
    float* de_part = workspace + slabs * wgrad_slab_stride((int64_t)H2 * H1);
    float* db_part = de_part + ((int64_t)slabs + P) * 4 * H2;
    hipStream_t st = (hipStream_t)stream;
    DFOL_REQUIRE(sums || !bio, "pair_wgrad_fused (bf16 storage): only the sums form exists");
    DFOL_REQUIRE(!sums || bio || H2 % 3 == 0, "pair_wgrad_fused_sums: HID2=%d must be a multiple of 3 (the running sums of four columns per thread do not fit the LDS)", H2);
    // three columns of dpre2 per thread where H2 allows it (4 (H2 / 3) <= 427 threads build dpre2); bf16 storage: always four
    const int rc = bio           ? pw_run<4, true, true, false>(who, a, de_part, db_part, 0, 0, 0, st)
                   : H2 % 3 != 0 ? pw_run<4, false, false, false>(who, a, de_part, db_part, 0, 0, 0, st)
                   : sums        ? pw_run<3, true, false, false>(who, a, de_part, db_part, 0, 0, 0, st)
                                 : pw_run<3, false, false, false>(who, a, de_part, db_part, 0, 0, 0, st);
    if (rc || !sums) return rc;
    hipLaunchKernelGGL(pair_sums_reduce_kernel, dim3(P + 8), dim3(320), 0, st, (const float*)de_part, (const float*)db_part, dx, pred_off, P, H2, slabs,
                       pw_rows_per_slab(M), dE, ld_de, dbe, db2);
    DFOL_LAUNCH_CHECK("pair_wgrad_fused (sums reduce)");
    return 0;
}

// scale: device pointer to {S, 1 / S}, S a power of two with S max_r(|dx[r]| max|E[row_pred[r]]|) / 4 <= 2^14 (see above)
// row_pred [M]: NON-DECREASING valid rows of E (the pair rows of a predicate are contiguous), pred_off [P + 1]: the first pair row of every
// predicate (row_pred[r] = p for pred_off[p] <= r < pred_off[p + 1], pred_off[P] = M); a row without a gradient carries dx = 0.
// (The bias gradient db2 - the column sums of dpre2 - comes from dfol_pair_logit_bwd_f32's db2 output: that kernel has the registers for it.)
extern "C" int dfol_pair_wgrad_fused_f32(const float* pre2, int64_t ld_p2, const float* dx, const int32_t* row_pred, const int64_t* pred_off,
                                         const float* E, int64_t ld_e, const float* scale, const float* Z, int64_t ld_z, int64_t M, int32_t H2,
                                         int32_t H1, float* workspace, float* dW, void* stream) {
    return pw_launch(pre2, ld_p2, dx, row_pred, pred_off, 0, E, ld_e, scale, Z, ld_z, M, H2, H1, workspace, dW, nullptr, 0, nullptr, nullptr, false, stream);
}

// ... and the sums of the logit layer's backward from the same pass (no separate pass over pre2): dE [P, ld_de], dbe [P] (or NULL),
// db2 [HID2].  EVERY predicate must own at least 64 pair rows or none (the caller checks; dfol_pair_logit_bwd_sums_f32 otherwise);
// workspace: dfol_pair_wgrad_fused_sums_workspace floats.
extern "C" int dfol_pair_wgrad_fused_sums_f32(const float* pre2, int64_t ld_p2, const float* dx, const int32_t* row_pred, const int64_t* pred_off,
                                              int32_t P, const float* E, int64_t ld_e, const float* scale, const float* Z, int64_t ld_z, int64_t M,
                                              int32_t H2, int32_t H1, float* workspace, float* dW, float* dE, int64_t ld_de, float* dbe, float* db2,
                                              void* stream) {
    DFOL_REQUIRE(P > 0 && dE && db2 && ld_de >= H2 && H2 <= 320, "pair_wgrad_fused_sums: bad arguments P=%d", P);
    return pw_launch(pre2, ld_p2, dx, row_pred, pred_off, P, E, ld_e, scale, Z, ld_z, M, H2, H1, workspace, dW, dE, ld_de, dbe, db2, true, stream);
}

// ... over bf16-STORED pre2 and Z (the bf16 mode; strides in elements, multiples of 4, 8-byte aligned rows): one bf16 piece per operand,
// dpre2 rounded as dfol_pair_logit_bwd_bf16 stores it; db2 = the column sums of those rounded values.  HID2 % 4 == 0 is enough here.
extern "C" int dfol_pair_wgrad_fused_sums_bf16(const void* pre2_bf16, int64_t ld_p2, const float* dx, const int32_t* row_pred, const int64_t* pred_off,
                                               int32_t P, const float* E, int64_t ld_e, const void* Z_bf16, int64_t ld_z, int64_t M, int32_t H2,
                                               int32_t H1, float* workspace, float* dW, float* dE, int64_t ld_de, float* dbe, float* db2, void* stream) {
    DFOL_REQUIRE(P > 0 && dE && db2 && ld_de >= H2 && H2 <= 320, "pair_wgrad_fused_sums_bf16: bad arguments P=%d", P);
    return pw_launch(pre2_bf16, ld_p2, dx, row_pred, pred_off, P, E, ld_e, nullptr, Z_bf16, ld_z, M, H2, H1, workspace, dW, dE, ld_de, dbe, db2, true, stream, true);
}

// dx [nr][dx_stride >= M], E [nr][P][ld_e] (reader k's rows at E + k P ld_e); row_pred, pred_off, scale, workspace and the size rules as
// dfol_pair_wgrad_fused_f32 (scale from the bound of the SUM: dfol_pair_wgrad_multi_scale_f32); 1 <= nr <= 4, more readers: further launches, added
extern "C" int dfol_pair_wgrad_fused_multi_f32(const float* pre2, int64_t ld_p2, const float* dx, int64_t dx_stride, int32_t nr, const int32_t* row_pred,
                                               const int64_t* pred_off, const float* E, int64_t ld_e, int32_t P, const float* scale, const float* Z,
                                               int64_t ld_z, int64_t M, int32_t H2, int32_t H1, float* workspace, float* dW, void* stream) {
    const char* who = "pair_wgrad_fused_multi";
    DFOL_REQUIRE(nr >= 1 && nr <= PW_MAXR && P >= 1, "pair_wgrad_fused_multi: %d readers (1..%d), P=%d", nr, PW_MAXR, P);
    const PwArgs a = {pre2, ld_p2, dx, row_pred, pred_off, E, ld_e, scale, Z, ld_z, M, H2, H1, workspace, dW};
    if (const int rc = pw_check(who, a, false)) return rc;
    DFOL_REQUIRE(dx_stride >= M, "pair_wgrad_fused_multi: dx_stride=%lld < M=%lld", (long long)dx_stride, (long long)M);
    const int64_t e_stride = (int64_t)P * ld_e;
    hipStream_t st = (hipStream_t)stream;
    return H2 % 3 == 0 ? pw_run<3, false, false, true>(who, a, nullptr, nullptr, nr, dx_stride, e_stride, st)
                       : pw_run<4, false, false, true>(who, a, nullptr, nullptr, nr, dx_stride, e_stride, st);
}
