// Fused pair MLP with the second layer on the fp16 matrix pipe at fp32 accuracy, THREE products per fp32 product (gfx950).
//
// Round 3's kernel (csrc/dfol_pair_split.hip) cuts every fp32 operand into three bf16 pieces and issues six piece products per fp32
// product: 0.55 of the bf16 pipe executed, 0.09 in algorithmic flops, and three rounds of schedule work moved it by < 3 %.  The lever
// is the arithmetic: fp16 carries 11 significand bits against bf16's 8, so TWO pieces x = h + l (h = fp16(x), l = fp16(x - h), both
// rounded to nearest even; x - h is exact in fp32) hold 22 - 23 bits, and the three products  al*wh + ah*wl + ah*wh  on
// v_mfma_f32_16x16x32_f16 (fp32 accumulation, the same 2.5 PFLOP/s as bf16) leave out only al*wl <= 2^-22 |a w|.
//
// fp16 has a narrow exponent range, and this is where the accuracy is decided (measured, tools/lab/split_accuracy.hip ->
// profiles/r04_split_accuracy_lab.txt, K = 256 dot products of ELU activations with U(-1/16, 1/16) weights, error against float64):
//   * the low piece of a value below 2^-3 is SUBNORMAL in fp16.  The matrix pipe keeps subnormal operands (probe in the same lab: a
//     2^-20 input survives); a pipe that flushed them would be off by 1e-4.  A subnormal low piece still has an absolute error of
//     2^-25, so an operand's error is max(2^-22 |x|, 2^-25): harmless for activations of order 1, but weights of order 1/16 would
//     carry 2^-21 relative.  unscaled weights: mean error 3.1e-7 (the fp32 FMA chain: 1.5e-7, bf16x3: 1.25e-7);
//   * so every ROW of W2 is scaled by a power of two 2^e_r that puts its largest magnitude into [2^13, 2^14) (exact; chosen by the pack
//     kernel on the device, no host round trip, overflow impossible for finite weights), and the epilogue folds 2^-e_r into the
//     multiplier of the Sigmoid's exponent (the product is there anyway).  scaled weights: mean error 1.0e-7 - BELOW the fp32 FMA chain
//     and the bf16x3 kernel, because the MFMA rounds once per 32 products;
//   * activations are ELU outputs in (-1, inf): they are split unscaled and saturate at 6e4 (fp16's largest finite value is 65504).
//     The first layer is fed by Sigmoid outputs and box geometry, |z| <= sum |W1| ~ 1036 |w|: an activation of 6e4 needs weights of
//     magnitude 58.  The clamp costs nothing (it is the third operand of the v_med3 that implements the ELU's select).
//
// W2 image (dfol_pair_pack_w2_f16x2): per 32 k (one MFMA's depth) a 40 KB chunk [2 pieces][320 rows][4 k-groups] x 16 bytes, rows >=
// HID2 zero, the four 8-element k-groups of row r stored at group kq ^ dfol_swz(r) (64-byte rows: every ds_read_b128 of a B
// fragment is bank-conflict-free), copied to LDS verbatim by LDS-DMA; after the chunks 320 floats -log2(e) 2^-e_r (the Sigmoid's
// per-column multiplier) and the 320 exponents.
//
// Schedule: the ping-pong of the bf16x3 kernel (one 8-wavefront workgroup per CU; in every tick one half runs a chunk's MFMAs - 114 now,
// not 228 - while the other half loads U / V rows, requests the next W2 chunk and builds its A pieces).
#include "dfol_common.h"
#include "dfol_split.h"

#include <stdlib.h>

#include <type_traits>

// -DDFOL_PAIR_TRACE: clock64 stamps of one wavefront per half in a few workgroups (tools/lab/trace_pair.py reads them)
#ifdef DFOL_PAIR_TRACE
__device__ long long dfol_h2_trace_buf[8 * 8 * 64];
#define TRACE(slot)                                                                                                  \
    do {                                                                                                             \
        if (trace_on && lane == 0) dfol_h2_trace_buf[(trace_blk * 8 + wave) * 64 + (slot)] = clock64();              \
    } while (0)
#else
#define TRACE(slot)
#endif

// U / V rows of chunk c + 1 requested at the top of the multiply tick of chunk c (1) or at the top of their own build tick (0)
#ifndef DFOL_H2_PREFETCH
#define DFOL_H2_PREFETCH 1
#endif
// tiles of B fragments requested ahead of the MFMAs that use them (a tile's six MFMAs are 96 cycles of the pipe: less than an LDS round trip
// under load, so one tile ahead - the bf16x3 kernel's distance, with twelve MFMAs per tile - leaves the reads exposed)
#ifndef DFOL_H2_BDEPTH
#define DFOL_H2_BDEPTH 2
#endif
// the same distance for the one-piece kernel (NP = 1): a tile is two MFMAs there, 32 cycles of the pipe, so the same time ahead is more tiles
// (four fragments in flight are 20 registers, fewer than the 24 of the two-piece form).  NOT MEASURED against 2 or 3: the value follows
// from that arithmetic alone.  Cross-compiled, NP = 1 <19> takes 240 / 244 / 248 VGPRs at depth 2 / 3 / 4, no scratch at any of them.
#ifndef DFOL_H1_BDEPTH
#define DFOL_H1_BDEPTH 4
#endif
// Y's chunk requests as inline asm (1): in flight across the build tick's closing barrier
#ifndef DFOL_H2_DMA_ASM
#define DFOL_H2_DMA_ASM 1
#endif
// lab switch for the TRAIN variant (tools/lab/time_train_fwd.py): bit 0 = no Z stores, bit 1 = no pre2 stores (what each costs)
#ifndef DFOL_H2T_SKIP
#define DFOL_H2T_SKIP 0
#endif
// Y's request for the next W2 chunk: 0 = at the top of its build tick, 1 = after its A pieces are built
#ifndef DFOL_H2_DMA_LATE
#define DFOL_H2_DMA_LATE 0
#endif


namespace {

constexpr float H2_NL2E = -1.44269504088896340736f;         // -log2(e)
constexpr int H2_CH = 32;                                   // K per chunk = one v_mfma_f32_16x16x32_f16
constexpr int H2_ROWS = 320, H2_TILES = 20;                 // rows (hidden columns) of the packed image
constexpr int H2_PIECES = 2 * H2_ROWS * 4;                  // 16-byte pieces per chunk: 2560 = 40 KB
constexpr int H1_PIECES = H2_ROWS * 4;                      // ... of the one-piece image (pair_math "f16"): 1280 = 20 KB
constexpr float H2_AMAX = 60000.0f;                         // activations saturate here (fp16 max 65504); in units of 1 / ln 2 (see make_a): ELU outputs of 41 589
constexpr float H2_L2E = 1.44269504088896340736f;           // log2(e) = 1 / ln 2
constexpr float H2_LN2 = 0.69314718055994530942f;

// The ELU's negative branch in the kernel's units: z' = z / ln 2 comes in (UV and the geometry weights are pre-multiplied by log2(e)), and
// (e^min(z, 0) - 1) / ln 2 = (2^min(z', 0) - 1) / ln 2 goes out - the hardware exponential with the CLAMP output modifier (2^z' clamped to
// [0, 1]: exactly 1 for z' >= 0, +inf included) and one fused multiply-add.  TWO instructions per element where round 4 had four (v_med3 for
// min(z, 0), v_mul by log2(e), v_exp, v_add -1): a build tick is paced by its instruction COUNT - one issue slot per MFMA of the SIMD's
// other wavefront - so the sixteen elements of a chunk cost 32 slots less.  The factor ln 2 is folded into W2 by the pack kernel.
__device__ __forceinline__ float h2_elu_neg(float zs) {
    const float p = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(zs), 0.0f, 1.0f);        // (folds into v_exp_f32 ... clamp)
    return fmaf(p, H2_L2E, -H2_L2E);
}

// The k of a 32-chunk that k-group kq (a lane's kh) holds at position e = 0..7 of its MFMA operand register: 16 (e >> 2) + 4 kq + (e & 3).
// The order of k inside a chunk is free as long as A and B agree; this one makes the A operand coincide with the C / D layout of an MFMA
// whose ROWS are k: a lane's four accumulator elements of the two geometry MFMAs of a chunk (rows 4 kh + e of k-tile t) are exactly its
// eight A elements, so the first layer's geometry term comes out of the matrix pipe in place (see make_a).
__host__ __device__ __forceinline__ constexpr int h2_kperm(int kq, int e) { return 16 * (e >> 2) + 4 * kq + (e & 3); }

// x - float(h.lo) / x - float(h.hi) in one instruction (v_fma_mix_f32: fma with per-source fp16 / fp32 selection): the residual of the split
template <bool HI>
__device__ __forceinline__ float h2_resid(float x, uint32_t hpair) {
    float r;
    if (HI) asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpair), "v"(x));
    else asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpair), "v"(x));
    return r;
}

// One wavefront per row of W2: e_r puts the row's largest magnitude into [2^13, 2^14); tail[r] = -log2(e) 2^-e_r, tail[320 + r] = e_r
__global__ void h2_row_scale_kernel(const float* __restrict__ W2, int64_t ld_w2, int HID2, int HID1, float* __restrict__ tail) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= H2_ROWS) return;
    float m = 0.f;
    if (r < HID2)
        for (int k = lane; k < HID1; k += 64) m = fmaxf(m, fabsf(W2[(int64_t)r * ld_w2 + k] * H2_LN2));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    const int e = dfol_scale_exp(m);
    if (lane == 0) {
        tail[r] = ldexpf(H2_NL2E, -e);
        reinterpret_cast<int32_t*>(tail)[H2_ROWS + r] = e;
    }
}

// One thread per 16-byte piece of the packed image.  NP = 2: [hi pieces][lo pieces] per chunk; NP = 1: the hi pieces alone (the same bits).
template <int NP>
__global__ void h2_pack_w2_kernel(const float* __restrict__ W2, int64_t ld_w2, int HID2, int HID1, const float* __restrict__ tail,
                                  u32x4* __restrict__ out) {
    constexpr int PIECES = NP * H2_ROWS * 4;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (HID1 / H2_CH) * PIECES) return;
    const int c = idx / PIECES, rem = idx - c * PIECES;
    const int p = rem / (H2_ROWS * 4), rr = rem - p * H2_ROWS * 4, r = rr >> 2, slot = rr & 3;
    const int kq = slot ^ dfol_swz(r);
    const int e = reinterpret_cast<const int32_t*>(tail)[H2_ROWS + r];
    uint32_t piece[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float w0 = 0.f, w1 = 0.f;
        if (r < HID2) {
            // (times ln 2: the kernel feeds the second layer ELU outputs in units of 1 / ln 2 - see make_a; one rounding per weight)
            w0 = ldexpf(W2[(int64_t)r * ld_w2 + c * H2_CH + h2_kperm(kq, 2 * j)] * H2_LN2, e);
            w1 = ldexpf(W2[(int64_t)r * ld_w2 + c * H2_CH + h2_kperm(kq, 2 * j + 1)] * H2_LN2, e);
        }
        uint32_t h, l;
        dfol_split2h(w0, w1, h, l);
        piece[j] = p == 0 ? h : l;
    }
    out[idx] = u32x4{piece[0], piece[1], piece[2], piece[3]};
}

// TRAIN (round 6): the same kernel as the FORWARD of a train step's pair MLP (trainer.py:429-442 over classifier_oracle.py:145-156) - what the
// backward needs leaves the registers on the way: the first hidden layer Z (multiplied back from the kernel's units of 1 / ln 2: one v_mul per
// element of the build), the pair geometry, the second layer's pre-activations pre2 and the first reader's raw logits; no relation tile is written.  Replaces dfol_pair_hidden1_fwd_f32 + the tall product over Z (Z written, then read again: 5.2 GB).
struct H2Train {
    float* Z;                       // [pairs, HID1]
    float* pre2;                    // [pairs, ld_pre2]
    int64_t ld_pre2;
    float* geo;                     // [pairs, 4]
    float* x;                       // [K, ld_x]: x[k][row] = Sigmoid(pre2[row]) . E[req_col[k][image(row)]]  (no bias)
    int64_t ld_x;
    const int64_t* pair_off;        // [Q]: first pair row of every image
};

// One 8-wavefront workgroup per CU owns 256 ordered pairs (s != o, row-major in s: util.py:87-103) of one image at a time; a wavefront owns
// 32 of them (two 16-slot tiles) and all NB16 column tiles (2 x NB16 accumulator tiles: 152 registers at NB16 = 19).  A workgroup runs
// wg_tiles consecutive pair tiles (tile = image * tiles_per_image + tb, the order of the T = 1 grid) one after the other: the geometry
// weights are staged once, the epilogue's rows once per image, and the next tile's start runs under the current one's end (see the tile loop).
// NP: fp16 pieces per operand.  2 = the three products above (fp32 accuracy); 1 = the opt-in reduced mode (pair_math "f16": A = fp16(a), the
// one-piece W2 image, ONE product per MAC - 38 MFMAs and 19 fragment reads per chunk, 20 KB chunk buffers; everything else is the same body).
template <int NB16, bool TBF16, bool TRAIN = false, int NP = 2>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void pair_ll32h_kernel(
    const float* UV_ /* not __restrict__: see load_uv */, int64_t ld_uv_, int HID1, const float* __restrict__ pos_, int64_t ld_pos_,
    const float* __restrict__ Wg_, const u32x4* __restrict__ W2h_, const float* __restrict__ b2_, int HID2,
    const float* __restrict__ E_, int64_t ld_e, const float* __restrict__ be, const int32_t* __restrict__ n_obj,
    const int32_t* __restrict__ obj_off, int Q, int tiles_per_image, int wg_tiles, const int32_t* __restrict__ req_col,
    const int32_t* __restrict__ req_tile, const uint8_t* __restrict__ req_orient, int K, int NS, float dflt,
    void* __restrict__ tiles_v, H2Train tr) {
    constexpr int MT = 2, WAVES = 8;
    constexpr int ROWS = NB16 * 16, T = WAVES * 64, SLOTS = MT * 16 * WAVES;
    static_assert(NB16 > 16 && NB16 <= H2_TILES, "geometry");
    static_assert(NP == 2 || (NP == 1 && !TRAIN), "pieces per operand (the train forward keeps both)");
    constexpr int PIECES = NP * H2_ROWS * 4;                                  // 16-byte pieces of a W2 chunk
    __shared__ __attribute__((aligned(16))) u32x4 Bs[2 * PIECES];             // two W2 chunks, all pieces (40 KB each; NP = 1: 20 KB)
    __shared__ __attribute__((aligned(16))) u32x4 WgA[(256 / H2_CH) * 2 * 64];      // the geometry weights as MFMA A fragments: [chunk][k-tile][lane], 16 KB
    constexpr int STAGE_FLOATS = 8192;                          // the epilogue's bias / multiplier / embedding rows (32 KB)
    __shared__ __attribute__((aligned(16))) float stage[STAGE_FLOATS];

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#ifdef DFOL_PAIR_TRACE
    const int trace_b0 = 3000 / wg_tiles, trace_step = 500 / wg_tiles > 0 ? 500 / wg_tiles : 1;      // (the stamps of a block's LAST tile stay)
    const int trace_blk = ((int)blockIdx.x - trace_b0) / trace_step;
    const bool trace_on = (int)blockIdx.x >= trace_b0 && ((int)blockIdx.x - trace_b0) % trace_step == 0 && trace_blk < 8;
#endif
    const int nchunk = HID1 / H2_CH, lastc = nchunk - 1;
    const int tile_end = (int)min((int64_t)blockIdx.x * wg_tiles + wg_tiles, (int64_t)Q * tiles_per_image);
    // W2 chunk 0 -> buffer 0 by all 512 threads (the first tile's request: it lands under the geometry arithmetic and the staging below)
    auto dma_chunk0_all = [&](const u32x4* W2h) __attribute__((always_inline)) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int i = 0; i < (PIECES + T - 1) / T; ++i)              // (NP = 1: 2.5 passes - the last one by the wavefronts 0-3)
            if (PIECES % T == 0 || T * i + wave * 64 < PIECES)      // (wave-uniform)
                __builtin_amdgcn_global_load_lds(W2h + T * i + tid, (__attribute__((address_space(3))) void*)&Bs[T * i + wave * 64], 16, 0, 0);
    };
    bool started = false;           // a tile has run: WgA is staged, stage[] holds the rows of image stage_q, the buffers hold W2 chunks
    bool b0 = false;                // buffer 0 holds chunk 0 again: half X requested it at the end of the previous tile (W2 is the same for every tile)
    int stage_q = -1;
    for (int tile = (int)blockIdx.x * wg_tiles; tile < tile_end; tile = TRAIN ? tile_end : tile + 1) {       // (TRAIN: one tile, see the launcher)
        // (A tile without work is skipped by the whole workgroup - the tests below are uniform - so no barrier goes unmatched.)
        const int q = tile / tiles_per_image, tb = tile - q * tiles_per_image;
        const int n = n_obj[q], npairs = n * (n - 1);
        if (tb * SLOTS >= npairs) continue;
        bool any = TRAIN;                                           // (training keeps every pair's activations, requested or not)
        for (int k = 0; k < K; ++k) any |= req_col[(int64_t)k * Q + q] >= 0;
        if (!any) continue;
        const int64_t prow0 = TRAIN ? tr.pair_off[q] : 0;           // the image's first pair row
        // The operands and the lane's coordinates, made opaque per tile (empty asm, no instruction): left alone, the compiler hoists every
        // address derived from them out of the tile loop - the lane's 64-bit row, chunk and embedding addresses, SGPR pairs of the DMA
        // groups - and keeps them live across the multiply ticks, where the 152 accumulator registers leave no room: 285 spilled VGPRs
        // at NB16 = 19.  Recomputed per tile they cost what they cost at one tile per workgroup.  (The same reason for the opaque copies
        // in the first tile's staging, the end-of-tile request and the epilogue's fallback reads.)
        const u32x4* W2h = W2h_;
        const float *Wg = Wg_, *b2 = b2_, *E = E_, *UV = UV_, *pos = pos_;
        int64_t ld_uv = ld_uv_, ld_pos = ld_pos_;
        asm volatile("" : "+s"(W2h), "+s"(Wg), "+s"(b2), "+s"(E));
        asm volatile("" : "+s"(UV), "+s"(pos), "+s"(ld_uv), "+s"(ld_pos));
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, kh = lane >> 4, r16 = lane & 15;
        const float* cf = reinterpret_cast<const float*>(W2h + (int64_t)nchunk * PIECES);      // -log2(e) 2^-e_r per hidden column

        TRACE(0);
        // chunk 0 is requested before anything else: it lands under the geometry arithmetic below
        if (!started) dma_chunk0_all(W2h);
        const int first = obj_off[q];
        // The pair geometry {distance, angle, sign dx, sign dy} (batch_gqa_boxfeatures_pipeline.py:263-279) as the B fragment of the geometry
        // MFMAs (make_a): 32 contraction slots, twelve in use - [0..3] geo_h, [4..7] geo_l (meeting wg_h), [8..11] geo_h (meeting wg_l)
        u32x4 geoB[MT];
        // U / V rows as 32-bit byte offsets from the image's first row (a scalar base: the loads take the saddr + voffset form; 64-bit per-lane
        // pointers cost 16 registers that the prefetched rows need)
        const char* img_uv = reinterpret_cast<const char*>(UV + (int64_t)first * ld_uv);
        uint32_t uoff[MT], voff[MT];
        uint32_t zoff[MT];                                          // TRAIN: byte offset of the slot's Z row piece from the image's first row (~0: no such pair)
        // (run before the barrier that closes the previous tile: X's under Y's last multiply and epilogue)
        auto slot_geometry = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int e_slot = tb * SLOTS + wave * (MT * 16) + m * 16 + r16;
                const bool valid = e_slot < npairs;
                zoff[m] = (TRAIN && valid) ? (uint32_t)(e_slot * HID1 + 4 * kh) * 4u : 0xffffffffu;
                // (n >= 2 here; dfol_offdiag_slot written out: selecting e_slot before the division changes the kernel's code)
                const int s = valid ? e_slot / (n - 1) : 0, oo_ = valid ? e_slot - s * (n - 1) : 0, o = oo_ + (oo_ >= s);
                const float4 g = dfol_pair_geometry(pos + (int64_t)(first + s) * ld_pos, pos + (int64_t)(first + o) * ld_pos);
                uint32_t gh01, gl01, gh23, gl23;
                dfol_split2h(g.x, g.y, gh01, gl01);
                dfol_split2h(g.z, g.w, gh23, gl23);
                if (TRAIN && valid && kh == 0) *reinterpret_cast<floatx4*>(tr.geo + (prow0 + e_slot) * 4) = floatx4{g.x, g.y, g.z, g.w};
                geoB[m] = kh == 0 ? u32x4{gh01, gh23, gl01, gl23} : (kh == 1 ? u32x4{gh01, gh23, 0u, 0u} : u32x4{0u, 0u, 0u, 0u});
                uoff[m] = (uint32_t)(s * (int)ld_uv + 4 * kh) * 4u;          // the lane's k of a chunk: 16 t + 4 kh + 0..3, t = 0, 1 (h2_kperm)
                voff[m] = (uint32_t)(o * (int)ld_uv + HID1 + 4 * kh) * 4u;
            }
        };
        constexpr int SR = STAGE_FLOATS / ROWS - 2;                 // embedding rows that fit into stage[]
        const int Kc = K < SR ? K : SR;
        floatx4 acc[MT][NB16];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < NB16; ++i) acc[m][i] = floatx4{0.f, 0.f, 0.f, 0.f};

        // The whole chunk c -> chunk buffer `buf`, requested by the 4 wavefronts of one half, w = the wavefront's quarter (10 passes of 256
        // pieces; a wavefront's 64 pieces of a pass are 1 KiB of contiguous LDS: wave-uniform base, the hardware adds lane * 16 bytes)
        // (a wavefront copies a CONTIGUOUS 10 KiB quarter of the chunk, 1 KiB per request, and the requests use the instruction's immediate
        // offset - it advances the global and the LDS address alike - so one pointer / M0 setting serves four requests: three settings per chunk
        // instead of ten.  Y's build tick is paced by its instruction count, and every request used to come with five address instructions.)
        auto dma_chunk = [&](int c, int buf, int w, int ln) __attribute__((always_inline)) {
            constexpr int PER_WAVE = PIECES / 4;                                    // 16-byte pieces of a wavefront's quarter (640 = ten requests; NP = 1: 320 = five)
            const u32x4* src = W2h + (int64_t)c * PIECES + w * PER_WAVE + ln;
            u32x4* dst = &Bs[buf * PIECES + w * PER_WAVE];
#pragma unroll
            for (int g = 0; g < PER_WAVE / 64; g += 4) {
#if DFOL_H2_DMA_ASM
                // (inline asm: the compiler does not know these requests, so the barrier that closes the build tick does not drain them - they land
                // under Y's multiply tick, whose closing s_waitcnt vmcnt(0) is theirs)
                const uint32_t d = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(dst + 64 * g);
                const u32x4* sp = src + 64 * g;
                // (ONE asm block per group, M0 in its clobber list: the compiler may write M0 itself - the builtin form at the kernel's top, readlane /
                // movrel - and must neither place such a write between the group's requests nor assume M0 keeps its earlier value: ADVICE r5)
                // (the target keeps M0 reserved - the compiler sets it right before each of its own uses - so clang warns about the clobber; it is still
                // recorded as a definition of M0, which is what the pass that merges identical M0 settings looks at)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
                const uint32_t m0v = __builtin_amdgcn_readfirstlane(d);
                const int rem = PER_WAVE / 64 - g;                      // requests of this group (compile-time after unrolling): 4, 4, 2; NP = 1: 4, 1
                if (rem >= 4)
                    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\tglobal_load_lds_dwordx4 %0, off offset:1024\n\t"
                                 "global_load_lds_dwordx4 %0, off offset:2048\n\tglobal_load_lds_dwordx4 %0, off offset:3072" ::"v"(sp), "s"(m0v) : "memory", "m0");
                else if (rem == 3)
                    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\tglobal_load_lds_dwordx4 %0, off offset:1024\n\t"
                                 "global_load_lds_dwordx4 %0, off offset:2048" ::"v"(sp), "s"(m0v) : "memory", "m0");
                else if (rem == 2)
                    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\tglobal_load_lds_dwordx4 %0, off offset:1024" ::"v"(sp), "s"(m0v) : "memory", "m0");
                else
                    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(sp), "s"(m0v) : "memory", "m0");
#pragma clang diagnostic pop
#else
                auto d = (__attribute__((address_space(3))) void*)(dst + 64 * g);
                __builtin_amdgcn_global_load_lds(src + 64 * g, d, 16, 0, 0);
                if (g + 1 < PER_WAVE / 64) __builtin_amdgcn_global_load_lds(src + 64 * g, d, 16, 1024, 0);
                if (g + 2 < PER_WAVE / 64) __builtin_amdgcn_global_load_lds(src + 64 * g, d, 16, 2048, 0);
                if (g + 3 < PER_WAVE / 64) __builtin_amdgcn_global_load_lds(src + 64 * g, d, 16, 3072, 0);
#endif
            }
        };
        // A pieces of a chunk for the lane's slots: k = 32 c + 8 kh + 0..7.  Two ADJACENT k of one slot form every packed-math pair
        // (U, V and the transposed geometry weights are contiguous in k): no register shuffles.
        floatx4 ru[MT][2], rv[MT][2];                                    // [slot][half]: the lane's 8 first-layer terms of a chunk
        auto load_uv = [&](int c) __attribute__((always_inline)) {
            // (UV is deliberately not a __restrict__ pointer: loads through a noalias readonly pointer are free to move, and the compiler sinks
            // the rows requested at the top of a multiply tick below the tick's closing barrier, to their first use - the prefetch then
            // prefetches nothing; loads that may alias the kernel's stores stay on their side of the barrier's release fence)
            // the chunk's offset stays in a scalar register (readfirstlane: loop strength reduction otherwise turns the four row addresses into
            // 64-bit per-lane induction variables - 8 registers that spill); the pointer keeps its global address space (a pointer rebuilt
            // from an integer is a FLAT one: flat loads also count in lgkmcnt, and the multiply tick's waits for B fragments would wait for them)
            const char* base = img_uv + (uint32_t)__builtin_amdgcn_readfirstlane(H2_CH * 4 * c);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int half = 0; half < 2; ++half) {                  // (k-tile t = half: 16 k = 64 bytes further)
                    ru[m][half] = *reinterpret_cast<const floatx4*>(base + uoff[m] + 64 * half);
                    rv[m][half] = *reinterpret_cast<const floatx4*>(base + voff[m] + 64 * half);
                }
        };
        u32x4 ap[MT][NP];                                               // [slot][piece h, l]
        // A pieces of chunk c.  The first layer's sums z = U[s] + V[o] + Wg geo(s, o) come out of the matrix pipe: per k-tile t (16 k) one MFMA
        // per slot tile with the geometry weights as A (rows = k), the pair geometry as B (columns = slots) and U + V as the C operand - twelve
        // contraction slots hold the three piece products wg_h geo_h + wg_h geo_l + wg_l geo_h.  With the k order of h2_kperm its result
        // registers ARE the lane's A elements of the main product (slot r16, k = 16 t + 4 kh + e): four MFMAs replace 32 packed FMAs and eight LDS
        // reads per chunk.  Then nn.ELU with the saturation - med3(z, e^min(z, 0) - 1, AMAX) = z in (0, AMAX], e^z - 1 for z <= 0 (e^z - 1 >= z),
        // AMAX beyond - and the split.
        auto make_a = [&](int c) __attribute__((always_inline)) {
            floatx4 z[MT][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f16x8 wa = __builtin_bit_cast(f16x8, WgA[(2 * c + t) * 64 + lane]);
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    z[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, __builtin_bit_cast(f16x8, geoB[m]), ru[m][t] + rv[m][t], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int jp = 0; jp < 2; ++jp) {
                        const float z0 = z[m][t][2 * jp], z1 = z[m][t][2 * jp + 1];
                        const float a0 = __builtin_amdgcn_fmed3f(z0, h2_elu_neg(z0), H2_AMAX);
                        const float a1 = __builtin_amdgcn_fmed3f(z1, h2_elu_neg(z1), H2_AMAX);
                        const uint32_t hh = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a0, a1}, f16x2));
                        ap[m][0][2 * t + jp] = hh;
                        if constexpr (NP == 2)
                            ap[m][1][2 * t + jp] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){h2_resid<false>(a0, hh), h2_resid<true>(a1, hh)}, f16x2));
                        if (TRAIN) z[m][t][2 * jp] = a0 * H2_LN2, z[m][t][2 * jp + 1] = a1 * H2_LN2;       // the activations themselves, back in plain units
                    }
            if (TRAIN && !(DFOL_H2T_SKIP & 1)) {
                // the lane's four consecutive k of k-tile t of chunk c (h2_kperm: 32 c + 16 t + 4 kh + 0..3): one 16-byte store; the sixteen lanes
                // kh = 0..3 x t = 0, 1 of a slot cover 128 contiguous bytes of its row per chunk
                char* zimg = reinterpret_cast<char*>(tr.Z + prow0 * HID1) + (uint32_t)__builtin_amdgcn_readfirstlane(H2_CH * 4 * c);
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    if (zoff[m] != 0xffffffffu) {
#pragma unroll
                        for (int t = 0; t < 2; ++t) *reinterpret_cast<floatx4*>(zimg + zoff[m] + 64 * t) = z[m][t];
                    }
            }
        };
        const int boff = r16 * 4 + (kh ^ dfol_swz(r16));                  // the lane's 16-byte piece inside a 16-row block
        int bbase = boff;                                               // + the chunk buffer's offset
        auto load_b = [&](int i, f16x8 (&b)[NP]) __attribute__((always_inline)) {
#pragma unroll
            for (int p = 0; p < NP; ++p) b[p] = __builtin_bit_cast(f16x8, Bs[bbase + i * 64 + p * H2_ROWS * 4]);
        };
        // The MFMAs of a chunk: the B fragments of tile i+1 are requested before the MFMAs of tile i, and the scheduler may not move anything
        // across tiles (left alone it hoists the reads of all tiles to the top and spills).  The three products of one accumulator are issued
        // back to back, smallest first: a dependent MFMA takes its C operand from the previous result without a register-file read.
        constexpr int PA3[3] = {1, 0, 0}, PB3[3] = {0, 1, 0};           // al wh, ah wl, ah wh
        auto chunk_mfma = [&]() __attribute__((always_inline)) {
            constexpr int D = NP == 2 ? DFOL_H2_BDEPTH : DFOL_H1_BDEPTH;  // tiles of B fragments in flight ahead of the MFMAs
            f16x8 bq[D + 1][NP];
#pragma unroll
            for (int d = 0; d < D; ++d) load_b(d, bq[d]);
#pragma unroll
            for (int i = 0; i < NB16; ++i) {
                if (i + D < NB16) load_b(i + D, bq[(i + D) % (D + 1)]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
#pragma unroll
                    for (int x = NP == 2 ? 0 : 2; x < 3; ++x)   // (one piece: ah wh alone)
                        acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, ap[m][PA3[x]]), bq[i % (D + 1)][PB3[x]], acc[m][i], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        // The tile's start.  The pair geometry is computed BEFORE the barrier that closes the previous tile (it touches no LDS): X's under Y's
        // last multiply and epilogue.
        slot_geometry();
        if (started) {
            __syncthreads();                                    // the previous tile is done: its readers of stage[] and of both chunk buffers
            if (!b0) dma_chunk0_all(W2h);
        } else {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            for (int i = tid; i < (HID1 / 16) * 64; i += T) {   // A fragment of k-tile i / 64 (16 consecutive k): lane (row k' = r16, khh) holds slots 8 khh ..
                const int kt = i >> 6, ln = i & 63, khh = ln >> 4;
                u32x4 frag = {0u, 0u, 0u, 0u};
                if (khh < 2) {
                    const float4 g = *reinterpret_cast<const float4*>(Wg + (kt * 16 + (ln & 15)) * 4);
                    uint32_t h01, l01, h23, l23;                    // (times log2(e): the first layer's sums come out in units of ln 2, as UV holds them)
                    dfol_split2h(g.x * H2_L2E, g.y * H2_L2E, h01, l01);
                    dfol_split2h(g.z * H2_L2E, g.w * H2_L2E, h23, l23);
                    frag = khh == 0 ? u32x4{h01, h23, h01, h23} : u32x4{l01, l23, 0u, 0u};      // [0..3] wg_h, [4..7] wg_h, [8..11] wg_l
                }
                WgA[i] = frag;
            }
        }
        // the epilogue's rows (the barrier below publishes them), once per image: row 0 the hidden bias times -log2(e), row 1 the per-column
        // multiplier -log2(e) 2^-e_r, then the requested embedding rows.  Padding columns get bias -1e30: Sigmoid exactly 0.
        if (q != stage_q) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            for (int i = tid; i < ROWS; i += T) {
                stage[i] = H2_NL2E * (i < HID2 ? b2[i] : -1.0e30f);     // Sigmoid(x + b) = 1 / (1 + 2^(-L2E x - L2E b))
                stage[ROWS + i] = i < HID2 ? cf[i] : 0.f;
            }
            for (int k = 0; k < Kc; ++k) {
                const int col = req_col[(int64_t)k * Q + q];
                for (int i = tid; i < ROWS; i += T) stage[ROWS * (2 + k) + i] = (col >= 0 && i < HID2) ? E[(int64_t)col * ld_e + i] : 0.f;
            }
        }
        // LDS-DMA completion is tracked by vmcnt of the ISSUING wavefront only; a workgroup barrier does not wait for it by itself
        __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
        __syncthreads();                                        // WgA, the staged epilogue rows and chunk 0 visible

        // chunk 0 of the next tile requested at the end of this one: buffer 0 must be free after X's last multiply (lastc odd)
        const bool pf = (lastc & 1) && tile + 1 < tile_end;
        // Tick tau: half X (wavefronts 0-3) builds chunk tau/2 on even ticks and multiplies it on the next; half Y (4-7) does the same one
        // tick later.  Chunk c is read in ticks 2c+1 (X) and 2c+2 (Y); its buffer is refilled with chunk c+2 by Y during its build tick 2c+3
        // and Y drains that DMA at the end of its multiply tick 2c+4, one tick before X needs it.  Chunk 1 goes into the free second buffer
        // in Y's idle tick 0.  Each half runs its own copy of the loop (plain straight-line bodies for the register allocator); the barriers
        // pair up by count: X executes 2 per chunk, Y one idle tick first and none after its last multiply.
        auto run_half = [&](auto y_tag) __attribute__((always_inline)) {
            constexpr bool Y = decltype(y_tag)::value;
            TRACE(1);
            if (Y) {
                if (nchunk > 1) dma_chunk(1, 1, wave - 4, lane);
                if (DFOL_H2_PREFETCH) load_uv(0);
                __syncthreads();                                // tick 0: X builds chunk 0
            } else if (DFOL_H2_PREFETCH) {
                load_uv(0);
            }
            TRACE(2);
            for (int c = 0; c < nchunk; ++c) {
                if (!DFOL_H2_PREFETCH) load_uv(c);
                // The U / V rows of this chunk have landed - spelled out, and TIED to the registers: an s_waitcnt whose in-out operands are the
                // rows, so that nothing that reads them can be scheduled above it.  (The compiler's own wait in front of their first use went
                // missing on some paths once the explicit drain at the end of Y's multiply tick covered the loop's back edge, and a bare
                // s_waitcnt builtin does not order the VALU instructions around it: cold launches then built A pieces from registers the loads
                // had not reached - tools/lab/stress_pair.py, tools/lab/diag_pair.py.)  Nothing else is in flight here: it costs nothing.
                if (DFOL_H2_PREFETCH) {
                    floatx4 t0 = ru[0][0], t1 = ru[0][1], t2 = ru[1][0], t3 = ru[1][1], t4 = rv[0][0], t5 = rv[0][1], t6 = rv[1][0], t7 = rv[1][1];
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3), "+v"(t4), "+v"(t5), "+v"(t6), "+v"(t7));
                    ru[0][0] = t0, ru[0][1] = t1, ru[1][0] = t2, ru[1][1] = t3, rv[0][0] = t4, rv[0][1] = t5, rv[1][0] = t6, rv[1][1] = t7;
                }
                TRACE(40 + c);
                if (Y && !DFOL_H2_DMA_LATE && c >= 1 && c < lastc) dma_chunk(c + 1, (c + 1) & 1, wave - 4, lane);
                TRACE(50 + c);
                make_a(c);
                // the A pieces are pure register arithmetic: without these fences the compiler sinks them below the barrier, in front of the
                // MFMAs of the multiply tick - the IR-level sinking into the block that uses them (the empty asm pins the values here), and
                // the machine scheduler (sched_barrier)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(ap[m][p]));
                __builtin_amdgcn_sched_barrier(0);
                if (Y && DFOL_H2_DMA_LATE && c >= 1 && c < lastc) dma_chunk(c + 1, (c + 1) & 1, wave - 4, lane);
                TRACE(3 + 4 * c);
                // end of the build tick.  (__syncthreads() carries a release fence, for which the compiler drains the chunk request Y has just
                // issued - vmcnt(0) in front of the barrier.  Two ways around that wait were built and measured slower: the bare s_barrier
                // instruction for Y, the DMA landing under its multiply tick (1.27 ms against 1.19: its LDS writes compete with the multiply tick's
                // fragment reads), and THREE chunk buffers with the request two chunks ahead, drained at the top of Y's next build tick
                // (1.28 ms against 1.16: a chunk takes more than a tick - ~3.5 k cycles - to arrive from L2 when every CU streams the 320 KB
                // image, so the wait only moves).)
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
                TRACE(4 + 4 * c);
                bbase = boff + (c & 1) * PIECES;
                if (DFOL_H2_PREFETCH && c < lastc) load_uv(c + 1);      // lands under the MFMAs
                chunk_mfma();
                if (Y) __builtin_amdgcn_s_waitcnt(0x0F70);      // the chunk requested in the build tick has landed
                TRACE(5 + 4 * c);
                if (!Y || c < lastc) __syncthreads();           // end of the multiply tick (Y's last one has no partner)
                TRACE(6 + 4 * c);
            }
            // X past its last barrier: chunk 0 of the next tile -> buffer 0, whose last reader (Y's multiply of chunk lastc - 1) is behind that
            // barrier; it lands under X's epilogue and Y's last multiply (buffer 1).  X's wait before the next tile's first barrier drains it.
            if (!Y && pf) {
                int ln = lane;                              // (opaque: see the tile's start)
                asm volatile("" : "+v"(ln));
                dma_chunk(0, 0, wave, ln);
            }
        };
        // (Round 5 also measured the form WITHOUT ping-pong - all eight wavefronts build a chunk, barrier, all eight multiply it: 1167 - 1184 us
        // against 1144 - 1150; the SIMD's two wavefronts then multiply one after the other - the older one is served first - at 20.6 cycles per
        // MFMA, profiles/r05_pair_h2_trace.txt.)
        if (wave < 4) run_half(std::false_type());
        else run_half(std::true_type());

        // Epilogue: Sigmoid of the hidden layer (the row scale of W2 folded into the exponent's multiplier), dot products with the requested
        // embedding rows (16-lane DPP reduction), LogSigmoid, straight into the [s][o] (or [o][s]) tile the Relate kernel reads.
        const int64_t tile_sz = (int64_t)NS * NS;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < NB16; ++i) {
                const float bv = stage[i * 16 + r16], cm = stage[ROWS + i * 16 + r16];
                if (TRAIN && !(DFOL_H2T_SKIP & 2)) {
                    // pre2 = acc 2^-e_r + b2 = -ln 2 (acc cm + bv): column 16 i + r16 of the rows 4 kh + e of slot tile m (sixteen lanes = 64 contiguous
                    // bytes of a row; the next column tile's store continues them).  (Staged through the free chunk buffers for 16-byte stores along the
                    // rows, two forms: 2.28 and 2.06 ms per launch against 1.97 for these dword stores - tools/lab/time_train_fwd.py.)
                    const int colp = i * 16 + r16;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ee = tb * SLOTS + wave * (MT * 16) + m * 16 + 4 * kh + e;
                        // (a scalar base per image + a 32-bit lane offset: the saddr form of the store, no 64-bit multiply per element)
                        if (colp < HID2 && ee < npairs)
                            *reinterpret_cast<float*>(reinterpret_cast<char*>(tr.pre2 + prow0 * tr.ld_pre2) + (uint32_t)(ee * (int)tr.ld_pre2 + colp) * 4u) =
                                -H2_LN2 * fmaf(acc[m][i][e], cm, bv);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[m][i][e] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fmaf(acc[m][i][e], cm, bv)));
            }
        for (int k = 0; k < K; ++k) {
            const int col = req_col[(int64_t)k * Q + q];
            if (col < 0) continue;
            float vm[MT];                                           // the logit of slot 4 kh + r16 of slot tile m, in the lanes r16 < 4
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float part[4] = {0.f, 0.f, 0.f, 0.f};
                if (k < Kc) {
                    const float* erow = stage + ROWS * (2 + k) + r16;
#pragma unroll
                    for (int i = 0; i < NB16; ++i) {
                        const float ev = erow[i * 16];
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[e] = fmaf(acc[m][i][e], ev, part[e]);
                    }
                } else {
                    const float* erow = E + (int64_t)col * ld_e;
                    int c16 = r16;                              // (opaque: see the tile's start)
                    asm volatile("" : "+v"(c16));
#pragma unroll
                    for (int i = 0; i < NB16; ++i) {
                        const float ev = erow[min(i * 16 + c16, HID2 - 1)];     // padding columns: activation is exactly 0
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[e] = fmaf(acc[m][i][e], ev, part[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) part[e] = dfol_group_sum<16>(part[e]);
                vm[m] = r16 == 0 ? part[0] : (r16 == 1 ? part[1] : (r16 == 2 ? part[2] : part[3]));
            }
            // One store instruction for the wavefront's 32 slots - consecutive ordered pairs, i.e. mostly consecutive floats of a tile row: the
            // lanes r16 = 4..7 take the second slot tile's logits from the lanes r16 - 4 (DPP row_shr:4), so a kh group writes slots 4 kh + 0..3
            // of both tiles.  (One instruction per slot tile wrote two misaligned 64-byte runs: 23 MB of WRITE_SIZE for 10 MB of tiles.)
            const float shifted = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(vm[1]), 0x114, 0xF, 0xF, false));
            if (r16 < 8) {
                const int hi = r16 >> 2;
                const float v = hi ? shifted : vm[0];
                const int ee = tb * SLOTS + wave * (MT * 16) + hi * 16 + 4 * kh + (r16 & 3);
                if (ee < npairs) {
                    if (TRAIN) {                                          // the reader's raw logit of this pair row (its bias and LogSigmoid stay with the caller)
                        tr.x[(int64_t)k * tr.ld_x + prow0 + ee] = v;
                        continue;
                    }
                    int ss, oo;
                    dfol_offdiag_slot_rcp(ee, n, ss, oo);
                    const float x = v + (be ? be[col] : 0.f);
                    const float val = fminf(x, 0.f) - dfol_log(1.0f + dfol_exp(-fabsf(x)));        // nn.LogSigmoid (the diagonal keeps the caller's fill)
                    const int64_t at = (int64_t)req_tile[(int64_t)k * Q + q] * tile_sz +
                                       ((req_orient && req_orient[(int64_t)k * Q + q]) ? (int64_t)oo * NS + ss : (int64_t)ss * NS + oo);
                    if (TBF16) {
                        uint32_t u = __float_as_uint(val);
                        u += 0x7fffu + ((u >> 16) & 1u);                 // round to nearest even
                        reinterpret_cast<uint16_t*>(tiles_v)[at] = (uint16_t)(u >> 16);
                    } else {
                        reinterpret_cast<float*>(tiles_v)[at] = val;
                    }
                }
            }
        }
        TRACE(60);
        started = true;
        stage_q = q;
        b0 = pf;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // a chunk request for a tile that turned out to have no work
}

// The range check of pair_ll32h_kernel, outside it (its build tick is paced by its instruction count: the same test inside cost 4 %).  A pair's
// ELU input z[k] = U[s][k] + V[o][k] + Wg[k] . geo(s, o) saturates above H2_AMAX (units of 1 / ln 2).  Per image and hidden unit k this kernel
// bounds it from above by  max_s U[s][k] + max_o V[o][k] + |Wg[k]| . (dmax, pi / 2, 1, 1),  dmax = the diagonal of the box that holds the
// image's centres - reached by a real pair unless the two maxima belong to the same object - and ORs DFOL_RANGE_PAIR_SATURATED into the
// caller's status word when the bound passes H2_AMAX or is NaN.  One workgroup per image; 16-byte loads, four row groups side by side and four
// rows of each in flight (the pair kernel reads the same rows next, so this pass also warms L2 / MALL for it).
__global__ __launch_bounds__(512) void h2_uv_range_kernel(const float* __restrict__ UV, int64_t ld_uv, int HID1, const float* __restrict__ pos,
                                                          int64_t ld_pos, const float* __restrict__ Wg, const int32_t* __restrict__ n_obj,
                                                          const int32_t* __restrict__ obj_off, uint32_t* __restrict__ status) {
    // thread t: four columns 4 (t % G) .. of the rows t / G, t / G + R, ... (G = 2 HID1 / 4 threads cover a 2 HID1-float row with 16-byte loads,
    // R = 512 / G row groups walk the image's rows side by side: 128 threads x 4 row groups at HID1 = 256)
    __shared__ float4 part[512];
    __shared__ float box[4][8];
    const int q = blockIdx.x, n = n_obj[q], first = obj_off[q], t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (n < 2) return;
    const int G = (2 * HID1) / 4, R = 512 / G, cg = t % G, rg = t / G;          // (HID1 a multiple of 32, <= 256: G in {16, .., 128} divides 512)
    float4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    bool nan = false;
    const float* base = UV + (int64_t)first * ld_uv + 4 * cg;
    auto take = [&](const float4 a) {
        nan |= (a.x != a.x) | (a.y != a.y) | (a.z != a.z) | (a.w != a.w);
        m.x = fmaxf(m.x, a.x), m.y = fmaxf(m.y, a.y), m.z = fmaxf(m.z, a.z), m.w = fmaxf(m.w, a.w);
    };
    int o = rg;
    for (; o + 3 * R < n; o += 4 * R) {
        const float4 a = *reinterpret_cast<const float4*>(base + (int64_t)o * ld_uv), b = *reinterpret_cast<const float4*>(base + (int64_t)(o + R) * ld_uv);
        const float4 c = *reinterpret_cast<const float4*>(base + (int64_t)(o + 2 * R) * ld_uv), d = *reinterpret_cast<const float4*>(base + (int64_t)(o + 3 * R) * ld_uv);
        take(a), take(b), take(c), take(d);
    }
    for (; o < n; o += R) take(*reinterpret_cast<const float4*>(base + (int64_t)o * ld_uv));
    if (nan) m.x = NAN;
    part[t] = m;
    float lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
    for (int i = t; i < n; i += 512) {
        const float* p = pos + (int64_t)(first + i) * ld_pos;
        const float cx = p[0] + p[2] / 2.0f, cy = p[1] + p[3] / 2.0f;
        lox = fminf(lox, cx), hix = fmaxf(hix, cx), loy = fminf(loy, cy), hiy = fmaxf(hiy, cy);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        lox = fminf(lox, __shfl_xor(lox, s, 64)), hix = fmaxf(hix, __shfl_xor(hix, s, 64));
        loy = fminf(loy, __shfl_xor(loy, s, 64)), hiy = fmaxf(hiy, __shfl_xor(hiy, s, 64));
    }
    if (lane == 0) box[0][wave] = lox, box[1][wave] = hix, box[2][wave] = loy, box[3][wave] = hiy;
    __syncthreads();
    if (t < HID1) {                                                              // hidden unit k = t: U column k, V column HID1 + k
#pragma unroll
        for (int w = 0; w < 8; ++w) lox = fminf(lox, box[0][w]), hix = fmaxf(hix, box[1][w]), loy = fminf(loy, box[2][w]), hiy = fmaxf(hiy, box[3][w]);
        const float* pf = reinterpret_cast<const float*>(part);
        float mu = -INFINITY, mv = -INFINITY;
        bool bad = false;
        for (int r = 0; r < R; ++r) {                                            // (a NaN travels in component x of its thread's partial)
            const float u = pf[(r * G + t / 4) * 4 + (t & 3)], v = pf[(r * G + (HID1 + t) / 4) * 4 + (t & 3)];
            const float ux = pf[(r * G + t / 4) * 4], vx = pf[(r * G + (HID1 + t) / 4) * 4];
            bad |= (ux != ux) | (vx != vx);
            mu = fmaxf(mu, u), mv = fmaxf(mv, v);
        }
        const float dmax = sqrtf((hix - lox) * (hix - lox) + (hiy - loy) * (hiy - loy));
        const float4 g = *reinterpret_cast<const float4*>(Wg + t * 4);
        const float geo = H2_L2E * (fabsf(g.x) * dmax + fabsf(g.y) * 1.57079632679489661923f + fabsf(g.z) + fabsf(g.w));
        const float bound = mu + mv + geo;
        if (bad || !(bound <= H2_AMAX)) atomicOr(status, (uint32_t)DFOL_RANGE_PAIR_SATURATED);
    }
}


// ---- the attribute head: the fused body with an OBJECT per slot --------------------------------------------------------------------
// The attribute MLP is the relation MLP after its first layer (516 -> 256 -> 300 -> concepts, ELU then Sigmoid), so its head runs the same
// second layer: per 128-object tile the eight chunks of the packed W2 image through LDS, A pieces built from the object's own row of
// first-layer PRE-activations (no geometry product, no U[s] + V[o]), the three piece products, Sigmoid in registers, dot products with the
// requested embedding rows, LogSigmoid into ll[p][o].  The hidden table [O, HID2] never exists.
//   * four wavefronts, two 16-slot tiles each (the pair kernel's chunk_mfma shape: 2 x NB16 accumulator tiles): 128 slots per workgroup,
//     200 workgroups at 256 x 100 objects.  No ping-pong: the build is one row load, an ELU and a split per element; the next chunk's
//     DMA and rows are requested behind the barrier that publishes the current chunk and land under its MFMAs (one barrier per chunk).
//   * the rows come in plain units (the first layer is the ordinary dense kernel without activation): one multiply by log2(e) per
//     element puts them into the units of h2_elu_neg and of the packed image (which carries the factor ln 2).
//   * a tile straddles images (three at N = 100, up to 128 at N = 1), and the request table is per predicate, in any order: per window of
//     AH_CAP predicates the workgroup collects those whose image meets the tile (image range by binary search in obj_off), stages up to SR
//     embedding rows (more: read from global memory, same values in the same order) and every wavefront runs the dot products of the
//     entries that meet its 32 slots.  Cells that no object owns (no-op tokens, columns >= n) get the default in a grid-stride pass.
//   * activations saturate at H2_AMAX as in the pair kernel; an element beyond it (or NaN) ORs DFOL_RANGE_X_OVERFLOW into the status
//     word - the bit the dense second layer raised for the same input.
constexpr int AH_WAVES = 4, AH_MT = 2, AH_T = AH_WAVES * 64, AH_SLOTS = AH_WAVES * AH_MT * 16, AH_CAP = 512;

template <int NB16>
__global__ __launch_bounds__(AH_T) void attr_head_h2_kernel(const float* pre1, int64_t ld_pre1, int HID1, const u32x4* __restrict__ W2h,
                                                            const float* __restrict__ b2, int HID2, const float* __restrict__ E, int64_t ld_e,
                                                            const float* __restrict__ be, const int32_t* __restrict__ obj_off, int Q, int O,
                                                            const int32_t* __restrict__ pred_q, const int32_t* __restrict__ pred_col, int P, int NS,
                                                            float dflt, float* __restrict__ ll, uint32_t* __restrict__ status) {
    constexpr int MT = AH_MT, ROWS = NB16 * 16, T = AH_T;
    static_assert(NB16 > 16 && NB16 <= H2_TILES, "geometry");
    __shared__ __attribute__((aligned(16))) u32x4 Bs[2 * H2_PIECES];          // two W2 chunks, both pieces (40 KB each)
    constexpr int STAGE_FLOATS = 8192;                                        // bias / multiplier / embedding rows (32 KB)
    __shared__ __attribute__((aligned(16))) float stage[STAGE_FLOATS];
    __shared__ int32_t ent[4][AH_CAP];                                        // a window's entries: predicate, column, first and end object of its image
    __shared__ int ent_n;
    __shared__ int img_cnt[2];
    constexpr int SR = STAGE_FLOATS / ROWS - 2;

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, kh = lane >> 4, r16 = lane & 15;
    const int nchunk = HID1 / H2_CH;
    const float* cf = reinterpret_cast<const float*>(W2h + (int64_t)nchunk * H2_PIECES);      // -log2(e) 2^-e_r per hidden column

    auto fill_defaults = [&]() {      // cells without an object: the default (disjoint from the cells the dot products write)
        for (int64_t idx = (int64_t)blockIdx.x * T + tid; idx < (int64_t)P * NS; idx += (int64_t)gridDim.x * T) {
            const int p = (int)(idx / NS), o = (int)(idx - (int64_t)p * NS), q = pred_q[p];
            if (pred_col[p] < 0 || o >= obj_off[q + 1] - obj_off[q]) ll[idx] = dflt;
        }
    };
    const int g0 = blockIdx.x * AH_SLOTS;
    if (g0 >= O) {                                                            // (uniform: the launcher's one workgroup of a batch without objects)
        fill_defaults();
        return;
    }

    auto dma_chunk = [&](int c, int buf) __attribute__((always_inline)) {      // all 256 threads: ten requests of 4 KiB, a wavefront's 1 KiB contiguous
#pragma unroll
        for (int i = 0; i < H2_PIECES / T; ++i)
            __builtin_amdgcn_global_load_lds(W2h + (int64_t)c * H2_PIECES + T * i + tid,
                                             (__attribute__((address_space(3))) void*)&Bs[buf * H2_PIECES + T * i + wave * 64], 16, 0, 0);
    };
    dma_chunk(0, 0);
    // the lane's rows: slot r16 of the wavefront's slot tile m, k = 32 c + 16 t + 4 kh + 0..3 (h2_kperm); slots past the last object repeat it
    const float* row[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) row[m] = pre1 + (int64_t)min(g0 + wave * (MT * 16) + m * 16 + r16, O - 1) * ld_pre1 + 4 * kh;
    floatx4 ra[MT][2];
    auto load_rows = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) ra[m][t] = *reinterpret_cast<const floatx4*>(row[m] + H2_CH * c + 16 * t);
    };
    load_rows(0);
    // (chunk 0 and the first rows are in flight: the default cells and the tile's image range cost their own latency only)
    fill_defaults();
    // the images of the tile's first and last object: the largest q with obj_off[q] <= g = the number of q in [1, Q) with obj_off[q] <= g
    // (an image without objects is never chosen), counted by all threads at once - a binary search is eight dependent trips to L2
    if (tid < 2) img_cnt[tid] = 0;
    __syncthreads();
    {
        const int g_last = min(g0 + AH_SLOTS, O) - 1;
        int c_lo = 0, c_hi = 0;
        for (int q = 1 + tid; q < Q; q += T) {
            const int f = obj_off[q];
            c_lo += f <= g0, c_hi += f <= g_last;
        }
        if (c_lo) atomicAdd(&img_cnt[0], c_lo);
        if (c_hi) atomicAdd(&img_cnt[1], c_hi);
    }
    for (int i = tid; i < ROWS; i += T) {
        stage[i] = H2_NL2E * (i < HID2 ? b2[i] : -1.0e30f);                  // Sigmoid(x + b) = 1 / (1 + 2^(-L2E x - L2E b)); padding columns: exactly 0
        stage[ROWS + i] = i < HID2 ? cf[i] : 0.f;
    }

    floatx4 acc[MT][NB16];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < NB16; ++i) acc[m][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    u32x4 ap[MT][2];                                                         // [slot tile][piece h, l]
    bool bad = false;
    const int boff = r16 * 4 + (kh ^ dfol_swz(r16));                         // the lane's 16-byte piece inside a 16-row block
    constexpr int PA3[3] = {1, 0, 0}, PB3[3] = {0, 1, 0};                    // al wh, ah wl, ah wh
    for (int c = 0; c < nchunk; ++c) {
        // chunk c (requested one iteration ago, under the MFMAs of chunk c - 1) and the rows have landed; behind the barrier every
        // wavefront's part of it is visible and nobody reads the other buffer any more
        __builtin_amdgcn_s_waitcnt(0x0F70);                                  // vmcnt(0): LDS-DMA completion is tracked per issuing wavefront
        __syncthreads();
        if (c + 1 < nchunk) dma_chunk(c + 1, (c + 1) & 1);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int jp = 0; jp < 2; ++jp) {
                    const float z0 = ra[m][t][2 * jp] * H2_L2E, z1 = ra[m][t][2 * jp + 1] * H2_L2E;
                    bad |= !(z0 <= H2_AMAX) | !(z1 <= H2_AMAX);
                    const float a0 = __builtin_amdgcn_fmed3f(z0, h2_elu_neg(z0), H2_AMAX);
                    const float a1 = __builtin_amdgcn_fmed3f(z1, h2_elu_neg(z1), H2_AMAX);
                    const uint32_t hh = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a0, a1}, f16x2));
                    const uint32_t lw = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){h2_resid<false>(a0, hh), h2_resid<true>(a1, hh)}, f16x2));
                    ap[m][0][2 * t + jp] = hh;
                    ap[m][1][2 * t + jp] = lw;
                }
        if (c + 1 < nchunk) load_rows(c + 1);
        const int bbase = boff + (c & 1) * H2_PIECES;
        constexpr int D = DFOL_H2_BDEPTH;
        f16x8 bq[D + 1][2];
        auto load_b = [&](int i, f16x8(&b)[2]) __attribute__((always_inline)) {
#pragma unroll
            for (int p = 0; p < 2; ++p) b[p] = __builtin_bit_cast(f16x8, Bs[bbase + i * 64 + p * H2_ROWS * 4]);
        };
#pragma unroll
        for (int d = 0; d < D; ++d) load_b(d, bq[d]);
#pragma unroll
        for (int i = 0; i < NB16; ++i) {
            if (i + D < NB16) load_b(i + D, bq[(i + D) % (D + 1)]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, ap[m][PA3[x]]), bq[i % (D + 1)][PB3[x]], acc[m][i], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (status && __any(bad) && lane == 0) atomicOr(status, (uint32_t)DFOL_RANGE_X_OVERFLOW);

    // Sigmoid of the hidden layer (the row scale of W2 folded into the exponent's multiplier)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < NB16; ++i) {
            const float bv = stage[i * 16 + r16], cm = stage[ROWS + i * 16 + r16];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m][i][e] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fmaf(acc[m][i][e], cm, bv)));
        }
    const int q_lo = img_cnt[0], q_hi = img_cnt[1];                          // (published by the chunk loop's barriers)
    const int w0 = g0 + wave * (MT * 16);                                    // the wavefront's first object
    for (int pw = 0; pw < P; pw += AH_CAP) {
        __syncthreads();                                                     // the previous window's readers of ent[] and stage[] are done
        if (tid == 0) ent_n = 0;
        __syncthreads();
        for (int p = pw + tid; p < min(pw + AH_CAP, P); p += T) {
            const int q = pred_q[p], col = pred_col[p];
            if (col >= 0 && q >= q_lo && q <= q_hi) {
                const int j = atomicAdd(&ent_n, 1);                          // (any order: every entry writes its own cells, staged or not the same values)
                ent[0][j] = p, ent[1][j] = col, ent[2][j] = obj_off[q], ent[3][j] = obj_off[q + 1];
            }
        }
        __syncthreads();
        const int n_ent = ent_n;
        if (n_ent == 0) continue;                                            // (uniform)
        const int n_st = n_ent < SR ? n_ent : SR;
        for (int j = 0; j < n_st; ++j) {
            const float* erow = E + (int64_t)ent[1][j] * ld_e;
            for (int i = tid; i < ROWS; i += T) stage[ROWS * (2 + j) + i] = i < HID2 ? erow[i] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < n_ent; ++j) {
            const int first = __builtin_amdgcn_readfirstlane(ent[2][j]), end = __builtin_amdgcn_readfirstlane(ent[3][j]);
            if (end <= w0 || first >= w0 + MT * 16) continue;               // none of this wavefront's objects belongs to the entry's image
            const int p = __builtin_amdgcn_readfirstlane(ent[0][j]), col = __builtin_amdgcn_readfirstlane(ent[1][j]);
            float vm[MT];                                                    // the logit of slot 4 kh + r16 of slot tile m, in the lanes r16 < 4
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float part[4] = {0.f, 0.f, 0.f, 0.f};
                if (j < SR) {
                    const float* erow = stage + ROWS * (2 + j) + r16;
#pragma unroll
                    for (int i = 0; i < NB16; ++i) {
                        const float ev = erow[i * 16];
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[e] = fmaf(acc[m][i][e], ev, part[e]);
                    }
                } else {
                    const float* erow = E + (int64_t)col * ld_e;
#pragma unroll
                    for (int i = 0; i < NB16; ++i) {
                        const float ev = i * 16 + r16 < HID2 ? erow[i * 16 + r16] : 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[e] = fmaf(acc[m][i][e], ev, part[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) part[e] = dfol_group_sum<16>(part[e]);
                vm[m] = r16 == 0 ? part[0] : (r16 == 1 ? part[1] : (r16 == 2 ? part[2] : part[3]));
            }
            // lanes r16 = 4..7 take the second slot tile's logits from the lanes r16 - 4 (DPP row_shr:4): one store for the wavefront's 32 objects
            const float shifted = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(vm[1]), 0x114, 0xF, 0xF, false));
            if (r16 < 8) {
                const int hi = r16 >> 2;
                const int g = w0 + hi * 16 + 4 * kh + (r16 & 3);
                if (g >= first && g < end && g - first < NS) {
                    const float x = (hi ? shifted : vm[0]) + (be ? be[col] : 0.f);
                    ll[(int64_t)p * NS + (g - first)] = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));       // nn.LogSigmoid, as attr_ll_kernel writes it
                }
            }
        }
    }
}

}  // namespace

#ifdef DFOL_PAIR_TRACE
extern "C" int dfol_pair_h2_trace_read(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dfol_h2_trace_buf), sizeof(dfol_h2_trace_buf)); }
#endif

// Pair tiles per workgroup of pair_ll32h_kernel.  DFOL_PAIR_TILES overrides it (read at every launch: the lab's sweep, the tests' T = 1 vs T
// comparisons); the grid stays ~Q * tiles_per_image / T workgroups deep, several per CU, so the other lane's kernels still find CUs.
#ifndef DFOL_H2_WG_TILES
#define DFOL_H2_WG_TILES 4
#endif
static int h2_wg_tiles() {
    const char* e = getenv("DFOL_PAIR_TILES");
    const int t = e ? atoi(e) : DFOL_H2_WG_TILES;
    return t < 1 ? 1 : (t > 64 ? 64 : t);
}

extern "C" int64_t dfol_pair_w2_f16x2_bytes(int32_t HID1) { return (int64_t)(HID1 / H2_CH) * H2_PIECES * 16 + 2 * H2_ROWS * 4; }
extern "C" int64_t dfol_pair_w2_f16_bytes(int32_t HID1) { return (int64_t)(HID1 / H2_CH) * H1_PIECES * 16 + 2 * H2_ROWS * 4; }

// NP = 2: the two-piece image; NP = 1: its hi pieces alone (same row scales, same tail)
template <int NP>
static int h2_pack_w2(const char* name, const float* W2, int64_t ld_w2, int32_t HID2, int32_t HID1, void* W2_split, void* stream) {
    DFOL_REQUIRE(HID1 > 0 && HID1 <= 256 && HID1 % H2_CH == 0, "%s: HID1=%d must be a multiple of %d, <= 256", name, HID1, H2_CH);
    DFOL_REQUIRE(HID2 > 256 && HID2 <= 320, "%s: HID2=%d must be in (256, 320]", name, HID2);
    DFOL_REQUIRE(W2 && W2_split && ld_w2 >= HID1, "%s: null pointer or ld_w2 < HID1", name);
    DFOL_REQUIRE((uintptr_t)W2_split % 16 == 0, "%s: output must be 16-byte aligned", name);
    const int total = (HID1 / H2_CH) * NP * H2_ROWS * 4;
    float* tail = reinterpret_cast<float*>(reinterpret_cast<u32x4*>(W2_split) + total);
    hipLaunchKernelGGL(h2_row_scale_kernel, dim3(H2_ROWS / 4), dim3(256), 0, (hipStream_t)stream, W2, ld_w2, HID2, HID1, tail);
    hipLaunchKernelGGL(h2_pack_w2_kernel<NP>, dim3(dfol_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, W2, ld_w2, HID2, HID1, (const float*)tail,
                       (u32x4*)W2_split);
    DFOL_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int dfol_pair_pack_w2_f16x2(const float* W2, int64_t ld_w2, int32_t HID2, int32_t HID1, void* W2_split, void* stream) {
    return h2_pack_w2<2>("pair_pack_w2_f16x2", W2, ld_w2, HID2, HID1, W2_split, stream);
}

extern "C" int dfol_pair_pack_w2_f16(const float* W2, int64_t ld_w2, int32_t HID2, int32_t HID1, void* W2_split, void* stream) {
    return h2_pack_w2<1>("pair_pack_w2_f16", W2, ld_w2, HID2, HID1, W2_split, stream);
}

// dfol_pair_ll_h2_f32 (NP = 2) and dfol_pair_ll_h1_f32 (NP = 1): the same checks, the same range kernel in front, the same grid
template <int NP>
static int h2_pair_ll(const char* name, const float* UV, int64_t ld_uv, int32_t HID1, const float* pos, int64_t ld_pos, const float* Wg,
                      const void* W2_split, const float* b2, int32_t HID2, const float* E, int64_t ld_e, const float* be, const int32_t* n_obj,
                      const int32_t* obj_off, int32_t Q, int32_t max_n, const int32_t* req_col, const int32_t* req_tile, const uint8_t* req_orient,
                      int32_t K, int32_t NS, float default_ll, int32_t tile_dtype, void* tiles_v, void* stream) {
    DFOL_REQUIRE(tile_dtype == DFOL_TILE_F32 || (tile_dtype == DFOL_TILE_BF16 && NS % 8 == 0), "%s: tile_dtype=%d (bf16 tiles need NS %% 8 == 0)", name, tile_dtype);
    DFOL_REQUIRE(Q >= 0 && K >= 0 && NS > 0 && NS % 4 == 0 && max_n >= 0 && max_n <= NS, "%s: bad sizes Q=%d K=%d NS=%d max_n=%d", name, Q, K, NS, max_n);
    DFOL_REQUIRE(HID1 > 0 && HID1 <= 256 && HID1 % H2_CH == 0 && ld_uv % 4 == 0, "%s: HID1=%d must be a multiple of %d, <= 256, UV rows 16-byte aligned", name, HID1, H2_CH);
    DFOL_REQUIRE(HID2 > 256 && HID2 <= 320, "%s: HID2=%d must be in (256, 320]", name, HID2);
    DFOL_REQUIRE(max_n <= DFOL_OFFDIAG_RCP_MAX_N, "%s: max_n=%d is above %d objects per image, the range of the epilogue's reciprocal pair decode (dfol_common.h)",
                 name, max_n, DFOL_OFFDIAG_RCP_MAX_N);
    if (Q == 0 || K == 0 || max_n < 2) return 0;
    DFOL_REQUIRE(UV && pos && Wg && W2_split && b2 && E && n_obj && obj_off && req_col && req_tile && tiles_v, "%s: null pointer", name);
    DFOL_REQUIRE(((uintptr_t)UV % 16 == 0) && ((uintptr_t)W2_split % 16 == 0) && ((uintptr_t)Wg % 16 == 0), "%s: operands must be 16-byte aligned", name);
    hipStream_t st = (hipStream_t)stream;
    const int tpi = dfol_cdiv((int64_t)max_n * (max_n - 1), 256);
    DFOL_REQUIRE((int64_t)Q * tpi < ((int64_t)1 << 31), "%s: too many tiles", name);
    DFOL_REQUIRE((int64_t)max_n * ld_uv * 4 < ((int64_t)1 << 31), "%s: an image's U / V rows must span less than 2 GB", name);
    const int wgt = h2_wg_tiles();
    const dim3 grid((unsigned)dfol_cdiv((int64_t)Q * tpi, wgt));
    if (uint32_t* status = dfol_range_status_ptr())           // (dfol_set_range_status: saturated ELU outputs are reported, not answered with)
        hipLaunchKernelGGL(h2_uv_range_kernel, dim3((unsigned)Q), dim3(512), 0, st, UV, ld_uv, HID1, pos, ld_pos, Wg, n_obj, obj_off, status);
    const H2Train none = {nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr};
#define DFOL_PAIR32H(NBV, BF)                                                                                                       \
    hipLaunchKernelGGL((pair_ll32h_kernel<NBV, BF, false, NP>), grid, dim3(512), 0, st, UV, ld_uv, HID1, pos, ld_pos, Wg, (const u32x4*)W2_split, b2, HID2, \
                       E, ld_e, be, n_obj, obj_off, Q, tpi, wgt, req_col, req_tile, req_orient, K, NS, default_ll, tiles_v, none)
    if (HID2 <= 272) { if (tile_dtype == DFOL_TILE_BF16) DFOL_PAIR32H(17, true); else DFOL_PAIR32H(17, false); }
    else if (HID2 <= 288) { if (tile_dtype == DFOL_TILE_BF16) DFOL_PAIR32H(18, true); else DFOL_PAIR32H(18, false); }
    else if (HID2 <= 304) { if (tile_dtype == DFOL_TILE_BF16) DFOL_PAIR32H(19, true); else DFOL_PAIR32H(19, false); }
    else { if (tile_dtype == DFOL_TILE_BF16) DFOL_PAIR32H(20, true); else DFOL_PAIR32H(20, false); }
#undef DFOL_PAIR32H
    DFOL_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int dfol_pair_ll_h2_f32(const float* UV, int64_t ld_uv, int32_t HID1, const float* pos, int64_t ld_pos, const float* Wg,
                                   const void* W2_split, const float* b2, int32_t HID2, const float* E, int64_t ld_e,
                                   const float* be, const int32_t* n_obj, const int32_t* obj_off, int32_t Q, int32_t max_n,
                                   const int32_t* req_col, const int32_t* req_tile, const uint8_t* req_orient, int32_t K,
                                   int32_t NS, float default_ll, int32_t tile_dtype, void* tiles_v, void* stream) {
    return h2_pair_ll<2>("pair_ll_h2", UV, ld_uv, HID1, pos, ld_pos, Wg, W2_split, b2, HID2, E, ld_e, be, n_obj, obj_off, Q, max_n, req_col, req_tile, req_orient, K,
                         NS, default_ll, tile_dtype, tiles_v, stream);
}

// The opt-in reduced-precision form (pair_math "f16"): ONE fp16 product per MAC on the dfol_pair_pack_w2_f16 image.
extern "C" int dfol_pair_ll_h1_f32(const float* UV, int64_t ld_uv, int32_t HID1, const float* pos, int64_t ld_pos, const float* Wg,
                                   const void* W2_f16, const float* b2, int32_t HID2, const float* E, int64_t ld_e,
                                   const float* be, const int32_t* n_obj, const int32_t* obj_off, int32_t Q, int32_t max_n,
                                   const int32_t* req_col, const int32_t* req_tile, const uint8_t* req_orient, int32_t K,
                                   int32_t NS, float default_ll, int32_t tile_dtype, void* tiles_v, void* stream) {
    return h2_pair_ll<1>("pair_ll_h1", UV, ld_uv, HID1, pos, ld_pos, Wg, W2_f16, b2, HID2, E, ld_e, be, n_obj, obj_off, Q, max_n, req_col, req_tile, req_orient, K,
                         NS, default_ll, tile_dtype, tiles_v, stream);
}


// The forward of a train step's pair MLP in ONE launch (round 6): per ordered pair of every image, Z = ELU(U[s] + V[o] + Wg geo), pre2 = W2 Z + b2, the pair geometry and, for K reader slots, the raw logits
// x[k][row] = Sigmoid(pre2[row]) . E[req_row[k][image]] (req_row < 0: that image has no reader in slot k; its x entries are left alone).
// Same arithmetic as dfol_pair_ll_h2_f32 (two fp16 pieces per operand, three products, fp32 accumulation).
extern "C" int dfol_pair_train_fwd_h2_f32(const float* UV, int64_t ld_uv, int32_t HID1, const float* pos, int64_t ld_pos, const float* Wg,
                                          const void* W2_split, const float* b2, int32_t HID2, const float* E, int64_t ld_e, const int32_t* n_obj,
                                          const int32_t* obj_off, const int64_t* pair_off, int32_t Q, int32_t max_n, const int32_t* req_row, int32_t K,
                                          float* Z, float* pre2, int64_t ld_pre2, float* geo, float* x, int64_t ld_x, void* stream) {
    DFOL_REQUIRE(Q >= 0 && K >= 0 && max_n >= 0, "pair_train_fwd_h2: bad sizes Q=%d K=%d max_n=%d", Q, K, max_n);
    DFOL_REQUIRE(HID1 > 0 && HID1 <= 256 && HID1 % H2_CH == 0 && ld_uv % 4 == 0, "pair_train_fwd_h2: HID1=%d must be a multiple of %d, <= 256, UV rows 16-byte aligned", HID1, H2_CH);
    DFOL_REQUIRE(HID2 > 256 && HID2 <= 320 && ld_pre2 >= HID2, "pair_train_fwd_h2: HID2=%d must be in (256, 320], ld_pre2 >= HID2", HID2);
    if (Q == 0 || max_n < 2) return 0;
    DFOL_REQUIRE(UV && pos && Wg && W2_split && b2 && n_obj && obj_off && pair_off && Z && pre2 && geo && (K == 0 || (E && req_row && x)), "pair_train_fwd_h2: null pointer");
    DFOL_REQUIRE(((uintptr_t)UV % 16 == 0) && ((uintptr_t)W2_split % 16 == 0) && ((uintptr_t)Wg % 16 == 0) && ((uintptr_t)Z % 16 == 0) && ((uintptr_t)geo % 16 == 0),
                 "pair_train_fwd_h2: operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int tpi = dfol_cdiv((int64_t)max_n * (max_n - 1), 256);
    DFOL_REQUIRE((int64_t)Q * tpi < ((int64_t)1 << 31), "pair_train_fwd_h2: too many tiles");
    DFOL_REQUIRE((int64_t)max_n * ld_uv * 4 < ((int64_t)1 << 31) && (int64_t)max_n * (max_n - 1) * HID1 * 4 < ((int64_t)1 << 32) - 1,
                 "pair_train_fwd_h2: an image's rows must span less than 2 GB (U | V) / 4 GB (Z)");
    if (uint32_t* status = dfol_range_status_ptr())
        hipLaunchKernelGGL(h2_uv_range_kernel, dim3((unsigned)Q), dim3(512), 0, st, UV, ld_uv, HID1, pos, ld_pos, Wg, n_obj, obj_off, status);
    const H2Train tr = {Z, pre2, ld_pre2, geo, x, ld_x, pair_off};
    // (one tile per workgroup: the TRAIN instantiation keeps the loop-free body - with a back edge its register allocation spills 33
    // VGPRs at NB16 = 19 instead of 5, on top of the Z / pre2 stores that already bound it)
    const int wgt = 1;
    const dim3 grid((unsigned)Q * tpi);
#define DFOL_PAIR32T(NBV)                                                                                                                    \
    hipLaunchKernelGGL((pair_ll32h_kernel<NBV, false, true>), grid, dim3(512), 0, st, UV, ld_uv, HID1, pos, ld_pos, Wg, (const u32x4*)W2_split, b2, HID2, \
                       E, ld_e, (const float*)nullptr, n_obj, obj_off, Q, tpi, wgt, req_row, (const int32_t*)nullptr, (const uint8_t*)nullptr, K, 4, 0.f,      \
                       (void*)nullptr, tr)
    if (HID2 <= 272) DFOL_PAIR32T(17);
    else if (HID2 <= 288) DFOL_PAIR32T(18);
    else if (HID2 <= 304) DFOL_PAIR32T(19);
    else DFOL_PAIR32T(20);
#undef DFOL_PAIR32T
    DFOL_LAUNCH_CHECK("pair_train_fwd_h2");
    return 0;
}


// The attribute head without its hidden table (include/dfol_vqa.h).  pre1: the first layer's pre-activations in plain units.
extern "C" int dfol_attr_head_h2_f32(const float* pre1, int64_t ld_pre1, int32_t HID1, const void* W2_split, const float* b2, int32_t HID2,
                                     const float* E, int64_t ld_e, const float* be, const int32_t* obj_off, int32_t Q, int32_t O,
                                     const int32_t* pred_q, const int32_t* pred_col, int32_t P, int32_t NS, float default_ll, float* ll, void* stream) {
    DFOL_REQUIRE(P >= 0 && Q >= 0 && O >= 0 && NS > 0 && NS % 4 == 0, "attr_head_h2: bad sizes P=%d Q=%d O=%d NS=%d", P, Q, O, NS);
    DFOL_REQUIRE(HID1 > 0 && HID1 <= 256 && HID1 % H2_CH == 0 && ld_pre1 % 4 == 0 && ld_pre1 >= HID1,
                 "attr_head_h2: HID1=%d must be a multiple of %d, <= 256, rows 16-byte aligned", HID1, H2_CH);
    DFOL_REQUIRE(HID2 > 256 && HID2 <= 320, "attr_head_h2: HID2=%d must be in (256, 320]", HID2);
    if (P == 0) return 0;
    DFOL_REQUIRE(obj_off && pred_q && pred_col && ll && Q > 0, "attr_head_h2: null pointer (or requests without images)");
    DFOL_REQUIRE(O == 0 || (pre1 && W2_split && b2 && E), "attr_head_h2: null pointer");
    DFOL_REQUIRE(((uintptr_t)pre1 % 16 == 0) && ((uintptr_t)W2_split % 16 == 0), "attr_head_h2: operands must be 16-byte aligned");
    const dim3 grid((unsigned)(O > 0 ? dfol_cdiv(O, AH_SLOTS) : 1));
    uint32_t* status = dfol_range_status_ptr();
#define DFOL_ATTR_HEAD(NBV)                                                                                                                      \
    hipLaunchKernelGGL((attr_head_h2_kernel<NBV>), grid, dim3(AH_T), 0, (hipStream_t)stream, pre1, ld_pre1, HID1, (const u32x4*)W2_split, b2, HID2, E, \
                       ld_e, be, obj_off, Q, O, pred_q, pred_col, P, NS, default_ll, ll, status)
    if (HID2 <= 272) DFOL_ATTR_HEAD(17);
    else if (HID2 <= 288) DFOL_ATTR_HEAD(18);
    else if (HID2 <= 304) DFOL_ATTR_HEAD(19);
    else DFOL_ATTR_HEAD(20);
#undef DFOL_ATTR_HEAD
    DFOL_LAUNCH_CHECK("attr_head_h2");
    return 0;
}
