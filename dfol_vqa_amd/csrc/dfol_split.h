// Operand formats of the 16-bit matrix-pipe kernels (gfx950).  A weight packer (dfol_linear_pack_w_*, dfol_pair_pack_w2_*) writes
// an operand image with these helpers and the kernel that reads it splits its own operand with the same ones: the two sides must
// agree bit for bit, so each format is defined here once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- LDS k-group swizzle --------------------------------------------------------------------------------------------------------
// A row of a B tile is four 16-byte k-groups; k-group kq of row r is stored at group kq ^ dfol_swz(r), dfol_swz = {0,3,2,1}[(r >> 2) & 3].
// A ds_read_b128 is served in four groups of 16 lanes, and a lane group of an MFMA fragment read mixes rows {0-3, 12-15} of k-group kh
// with rows {4-11} of k-group kh + 1 (or kh - 1); with the swizzle those 16 (row, group) pairs cover all 64 banks exactly once, so every
// fragment read is conflict-free and a packed image can be copied to LDS verbatim, without padding.
__device__ __forceinline__ int dfol_swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }

// ---- three bf16 pieces: x = h + m + l exactly ---------------------------------------------------------------------------------------
// h = top 16 bits of x, m = top 16 bits of x - h, l = x - h - m: 8 + 8 + 8 mantissa bits, all subtractions exact.  Each piece comes back
// as the fp32 whose low 16 bits are (or can be taken as) zero: the bf16 piece is the top half.  A product a w is accumulated (fp32, by the
// MFMA) as the six piece products of order <= 2^-16: al wh + ah wl + am wm + am wh + ah wm + ah wh; the three dropped ones are below
// 2^-23 |a w|, the rounding error of one fp32 FMA on the same product.  The exponent range is fp32's.
__device__ __forceinline__ void dfol_split3(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
    h = __float_as_uint(x);
    const float r = x - __uint_as_float(h & 0xffff0000u);
    m = __float_as_uint(r);
    l = __float_as_uint(r - __uint_as_float(m & 0xffff0000u));
}
// {top half of x0, top half of x1} as one register (element 0 in the low half)
__device__ __forceinline__ uint32_t dfol_pack(uint32_t x0, uint32_t x1) { return __builtin_amdgcn_perm(x1, x0, 0x07060302u); }

// 8 consecutive fp32 -> the three 8 x bf16 pieces
__device__ __forceinline__ void dfol_split3x8(const float4& a, const float4& b, u32x4& h, u32x4& m, u32x4& l) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t ph[8], pm[8], pl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) dfol_split3(v[j], ph[j], pm[j], pl[j]);
    h = u32x4{dfol_pack(ph[0], ph[1]), dfol_pack(ph[2], ph[3]), dfol_pack(ph[4], ph[5]), dfol_pack(ph[6], ph[7])};
    m = u32x4{dfol_pack(pm[0], pm[1]), dfol_pack(pm[2], pm[3]), dfol_pack(pm[4], pm[5]), dfol_pack(pm[6], pm[7])};
    l = u32x4{dfol_pack(pl[0], pl[1]), dfol_pack(pl[2], pl[3]), dfol_pack(pl[4], pl[5]), dfol_pack(pl[6], pl[7])};
}

// ---- two fp16 pieces: x = h + l ----------------------------------------------------------------------------------------------------
// h = fp16(x), l = fp16(x - h), both rounded to nearest even; x - h is exact in fp32.  (x0, x1) = (h0 + l0, h1 + l1) up to 2^-22 |x|, and
// 2^-25 absolute below 2^-3, where the low piece is subnormal in fp16 (the matrix pipe keeps subnormal operands).  Three products
// xl wh + xh wl + xh wh leave out xl wl <= 2^-22 |x w|.  |x| > 65504 overflows fp16 (the high piece is inf, the products NaN).
// v_cvt_pk_f16_f32, two v_cvt_f32_f16, v_pk_add_f32, v_cvt_pk_f16_f32.
__device__ __forceinline__ void dfol_split2h(float x0, float x1, uint32_t& h, uint32_t& l) {
    const f32x2 x = {x0, x1};
    const f16x2 hh = __builtin_convertvector(x, f16x2);
    const f32x2 r = x - __builtin_convertvector(hh, f32x2);
    h = __builtin_bit_cast(uint32_t, hh);
    l = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
}
// 8 consecutive fp32 -> the two 8 x fp16 pieces
__device__ __forceinline__ void dfol_split2hx8(const float4& a, const float4& b, u32x4& h, u32x4& l) {
    uint32_t hh[4], ll[4];
    dfol_split2h(a.x, a.y, hh[0], ll[0]);
    dfol_split2h(a.z, a.w, hh[1], ll[1]);
    dfol_split2h(b.x, b.y, hh[2], ll[2]);
    dfol_split2h(b.z, b.w, hh[3], ll[3]);
    h = u32x4{hh[0], hh[1], hh[2], hh[3]};
    l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}

// ---- bf16 storage ------------------------------------------------------------------------------------------------------------------
// two fp32 -> two bf16, round to nearest even (v_cvt_pk_bf16_f32; element 0 in the low half): the operand and storage form of the bf16 mode
__device__ __forceinline__ uint32_t dfol_rne2(float x0, float x1) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{x0, x1}, bf16x2)); }
// four bf16 (two registers) -> four fp32 (exact)
__device__ __forceinline__ float4 dfol_widen(const u32x2& v) {
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}
// (four fp32 as loaded: the same call for either storage)
__device__ __forceinline__ float4 dfol_widen(const floatx4& v) { return make_float4(v.x, v.y, v.z, v.w); }

// ---- power-of-two scales for the fp16 pieces ---------------------------------------------------------------------------------------
// fp16 has a narrow exponent range: a row (or a launch) whose largest magnitude is m is scaled by 2^e, e = 14 - x for m = f 2^x,
// f in [0.5, 1), which puts m 2^e into [2^13, 2^14) (exact), so that the low pieces are normal fp16 numbers.  e is clamped to
// [-100, 100] (2^e and 2^-e stay normal fp32 numbers); e = 0 when m is zero or not finite (a NaN or inf operand shows in the products).
__device__ __forceinline__ int dfol_scale_exp(float m) {
    int e = 0;
    if (m > 0.f && m < 3.0e38f) {
        int x;
        (void)frexpf(m, &x);
        e = 14 - x;
        e = e < -100 ? -100 : (e > 100 ? 100 : e);
    }
    return e;
}
