// The device-resident object-feature store's kernels (dfol_vqa_amd/feature_store.py).  The gather: the [O, F + 6] object matrix of a batch, which
// BatchGQABoxFeaturesCollator.collate_object_features builds on the host from the chunk files and ships over PCIe (822 KB per question at
// 100 objects x 2048 features), written on the device from a store that holds the corpus' features, boxes and image sizes.
//
//   out[obj_off[i] + j] = [features[slot[i]][j][0:F], W, H, x1, y1, x2 - x1, y2 - y1]       j < obj_off[i + 1] - obj_off[i]
//
// A pure copy, bound by HBM: one workgroup column per image, a wavefront per row (8 KB at F = 2048), 16-byte loads with four in flight per
// lane.  Output rows have a stride of F + 6 floats, so they are 16-byte aligned at best every other row: the store width (16, 8 or 4 bytes)
// follows the row's actual address, which is uniform over the wavefront.  The two subtractions are single fp32 subtractions, as numpy's on
// the host, so the matrix is bit-equal to the collator's.  No LDS, no atomics.
//
// The index form (a `direct` store): the same batch as O row numbers into the store's [S * max_obj, F] table and its six box columns - 28 bytes
// per object instead of 4 (F + 6) - for the consumer that reads the table's rows itself (dfol_linear_wide_rows_h2_f32).
//
// The cached form (a `featurized` store): the batch's object matrix [O, W + 4] from the cached OUTPUT of a frozen featurizer for every table
// row - the indexed rows of the cache beside their box positions, one launch instead of the featurizer's products (store_objects_kernel).
//
// The bf16 form (a store built with feature_dtype="bf16"): the table holds every feature rounded to bfloat16 by dfol_rne2 - the rounding the
// bf16 mode's first product and weight gradient apply to an fp32 feature anyway (round_bf16_kernel, at upload) - and the gather widens the
// stored values exactly to the same [O, F + 6] fp32 matrix (gather_object_rows_bf16_kernel); boxes and sizes stay fp32.
#include "dfol_common.h"
#include "dfol_split.h"

namespace {

constexpr int ST_WAVES = 4;                 // wavefronts of a workgroup = rows in flight per workgroup
constexpr int ST_TARGET_WAVES = 4096;       // wavefronts of a launch when the batch has the rows for it: 16 per CU

template <int SW>
__device__ __forceinline__ void st_store(float* d, const float4& v) {
    if (SW == 4) {
        *reinterpret_cast<float4*>(d) = v;
    } else if (SW == 2) {
        *reinterpret_cast<float2*>(d) = make_float2(v.x, v.y);
        *reinterpret_cast<float2*>(d + 2) = make_float2(v.z, v.w);
    } else {
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}

// n4 16-byte pieces of one row, the wavefront's lanes side by side; SW = floats per store instruction
template <int SW>
__device__ __forceinline__ void st_copy_row(const float4* __restrict__ src, float* __restrict__ dst, int n4, int lane) {
    int c = lane;
    for (; c + 192 < n4; c += 256) {
        const float4 a = src[c], b = src[c + 64], e = src[c + 128], f = src[c + 192];
        st_store<SW>(dst + 4 * c, a);
        st_store<SW>(dst + 4 * (c + 64), b);
        st_store<SW>(dst + 4 * (c + 128), e);
        st_store<SW>(dst + 4 * (c + 192), f);
    }
    for (; c < n4; c += 64) st_store<SW>(dst + 4 * c, src[c]);
}

// grid (I, row slices): workgroup (i, y) writes the rows j = 4 y + wave, + 4 gridDim.y, ... of image i
template <bool VEC>
__global__ __launch_bounds__(ST_WAVES * 64) void gather_object_rows_kernel(const float* __restrict__ feats, const float* __restrict__ boxes,
                                                                           const float* __restrict__ sizes, const int32_t* __restrict__ slot,
                                                                           const int32_t* __restrict__ obj_off, int max_obj, int F,
                                                                           float* __restrict__ out, int64_t ld_out) {
    const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = obj_off[i];
    const int n = min(obj_off[i + 1] - first, max_obj);              // (an image has at most max_obj rows in the store)
    const int s = slot[i];
    const int64_t img = (int64_t)s * max_obj;
    for (int j = blockIdx.y * ST_WAVES + wave; j < n; j += gridDim.y * ST_WAVES) {
        const float* src = feats + (img + j) * F;
        float* dst = out + (int64_t)(first + j) * ld_out;
        if (VEC) {
            const float4* src4 = reinterpret_cast<const float4*>(src);
            const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15);
            if (mis == 0)
                st_copy_row<4>(src4, dst, F >> 2, lane);
            else if (mis == 8)
                st_copy_row<2>(src4, dst, F >> 2, lane);
            else
                st_copy_row<1>(src4, dst, F >> 2, lane);
        } else {
            for (int c = lane; c < F; c += 64) dst[c] = src[c];
        }
        if (lane < 6) {                                              // [W, H, x, y, w, h]  (batch_gqa_boxfeatures_pipeline.py:57-71)
            const float* b = boxes + (img + j) * 4;
            float v;
            if (lane < 2)
                v = sizes[2 * (int64_t)s + lane];
            else if (lane < 4)
                v = b[lane - 2];
            else
                v = b[lane - 2] - b[lane - 4];
            dst[F + lane] = v;
        }
    }
}

// The bf16 table's row: n4 8-byte pieces (four bf16) widened exactly to 16 bytes of fp32 each, four loads in flight per lane as st_copy_row
template <int SW>
__device__ __forceinline__ void st_widen_row(const u32x2* __restrict__ src, float* __restrict__ dst, int n4, int lane) {
    int c = lane;
    for (; c + 192 < n4; c += 256) {
        const u32x2 a = src[c], b = src[c + 64], e = src[c + 128], f = src[c + 192];
        st_store<SW>(dst + 4 * c, dfol_widen(a));
        st_store<SW>(dst + 4 * (c + 64), dfol_widen(b));
        st_store<SW>(dst + 4 * (c + 128), dfol_widen(e));
        st_store<SW>(dst + 4 * (c + 192), dfol_widen(f));
    }
    for (; c < n4; c += 64) st_store<SW>(dst + 4 * c, dfol_widen(src[c]));
}

// gather_object_rows_kernel over a bf16 table (F % 4 == 0, rows 8-byte aligned): same grid, same output rows, same box columns
__global__ __launch_bounds__(ST_WAVES * 64) void gather_object_rows_bf16_kernel(const uint16_t* __restrict__ feats, const float* __restrict__ boxes,
                                                                                const float* __restrict__ sizes, const int32_t* __restrict__ slot,
                                                                                const int32_t* __restrict__ obj_off, int max_obj, int F,
                                                                                float* __restrict__ out, int64_t ld_out) {
    const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = obj_off[i];
    const int n = min(obj_off[i + 1] - first, max_obj);
    const int s = slot[i];
    const int64_t img = (int64_t)s * max_obj;
    for (int j = blockIdx.y * ST_WAVES + wave; j < n; j += gridDim.y * ST_WAVES) {
        const u32x2* src = reinterpret_cast<const u32x2*>(feats + (img + j) * F);
        float* dst = out + (int64_t)(first + j) * ld_out;
        const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15);
        if (mis == 0)
            st_widen_row<4>(src, dst, F >> 2, lane);
        else if (mis == 8)
            st_widen_row<2>(src, dst, F >> 2, lane);
        else
            st_widen_row<1>(src, dst, F >> 2, lane);
        if (lane < 6) {                                              // (the fp32 gather's six columns by its own subtractions)
            const float* b = boxes + (img + j) * 4;
            float v;
            if (lane < 2)
                v = sizes[2 * (int64_t)s + lane];
            else if (lane < 4)
                v = b[lane - 2];
            else
                v = b[lane - 2] - b[lane - 4];
            dst[F + lane] = v;
        }
    }
}

// dst[i] = bf16(src[i]), round to nearest even by dfol_rne2 - the dense kernels' own rounding; a thread takes two elements (one 4-byte store),
// the last thread of an odd count one
constexpr int RB_THREADS = 256;

__global__ __launch_bounds__(RB_THREADS) void round_bf16_kernel(const float* __restrict__ src, int64_t n, uint16_t* __restrict__ dst) {
    const int64_t step = (int64_t)gridDim.x * RB_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; 2 * p < n; p += step) {
        const int64_t e = 2 * p;
        if (e + 1 < n)
            *reinterpret_cast<uint32_t*>(dst + e) = dfol_rne2(src[e], src[e + 1]);
        else
            dst[e] = (uint16_t)dfol_rne2(src[e], 0.f);
    }
}

// The certificate of a bf16 table whose every value is an fp16 value (dfol_store_bf16_is_f16): a grid-stride pass that clears *flag (set to
// a non-zero value by the caller) when an element is not finite or does not survive the conversion to fp16 and back.  Such a table's low
// fp16 piece is +0 everywhere, which is what the wide kernel's two-product form stands on (csrc/dfol_dense_wide.hip, TWO).
__global__ __launch_bounds__(RB_THREADS) void bf16_is_f16_kernel(const uint16_t* __restrict__ t, int64_t n, uint32_t* __restrict__ flag) {
    const int64_t step = (int64_t)gridDim.x * RB_THREADS;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; i < n; i += step) {
        const float x = __uint_as_float((uint32_t)t[i] << 16);
        const float back = (float)(_Float16)x;                        // (inf beyond 65504, NaN stays NaN)
        bad |= !(fabsf(x) <= 65504.0f) || !(back == x);
    }
    if (bad) atomicAnd(flag, 0u);
}

// grid (I, row slices of SR_THREADS): thread (i, j) writes row obj_off[i] + j - its table row and (W, H, x1, y1, x2 - x1, y2 - y1), the gather's own
// six values by the gather's own subtractions
constexpr int SR_THREADS = 128;

__global__ __launch_bounds__(SR_THREADS) void store_rows_kernel(const float* __restrict__ boxes, const float* __restrict__ sizes,
                                                                const int32_t* __restrict__ slot, const int32_t* __restrict__ obj_off, int max_obj,
                                                                int32_t* __restrict__ src_row, float* __restrict__ box6) {
    const int i = blockIdx.x, j = blockIdx.y * SR_THREADS + threadIdx.x;
    const int first = obj_off[i];
    const int n = min(obj_off[i + 1] - first, max_obj);              // (an image has at most max_obj rows in the store)
    if (j >= n) return;
    const int s = slot[i];
    const int64_t row = (int64_t)s * max_obj + j;                    // (< 2^31: the host checked S * max_obj)
    const float* b = boxes + row * 4;
    const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    src_row[first + j] = (int32_t)row;
    float* d = box6 + (int64_t)(first + j) * 6;
    d[0] = sizes[2 * (int64_t)s], d[1] = sizes[2 * (int64_t)s + 1];
    d[2] = x1, d[3] = y1, d[4] = x2 - x1, d[5] = y2 - y1;
}

// The cached form (a `featurized` store): object row r = [cache[src_row[r]][0:W], box positions of box6[r]] - the featurizer's output for a
// frozen featurizer, read back instead of recomputed.  As the gather: a pure copy, a wavefront per row and 16-byte loads; rows of W <= 128
// take LPR = 8 .. 32 lanes each (a power of two >= W / 4: one 16-byte piece per lane), 64 / LPR rows per wavefront.  An output row starts
// at any multiple of 4 bytes, so the store width follows the row's address (uniform over the row's lanes).  Lanes 0 .. 3 of a row write
// its position columns by dfol_box_position, box_positions_kernel's arithmetic.  src_row is trusted, as in wide_h2_kernel<ROWS>.
template <bool VEC>
__global__ __launch_bounds__(ST_WAVES * 64) void store_objects_kernel(const float* __restrict__ cache, int64_t ld_cache,
                                                                      const int32_t* __restrict__ src_row, const float* __restrict__ box6, int O,
                                                                      int W, int lpr, float* __restrict__ out, int64_t ld_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rpw = 64 / lpr, sub = lane / lpr, l = lane & (lpr - 1);
    const int64_t step = (int64_t)gridDim.x * ST_WAVES * rpw;
    for (int64_t r = ((int64_t)blockIdx.x * ST_WAVES + wave) * rpw + sub; r < O; r += step) {
        const float* src = cache + (int64_t)src_row[r] * ld_cache;
        float* dst = out + r * ld_out;
        if (VEC) {
            const float4* src4 = reinterpret_cast<const float4*>(src);
            const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15);
            const int n4 = W >> 2;
            if (lpr == 64) {
                if (mis == 0)
                    st_copy_row<4>(src4, dst, n4, lane);
                else if (mis == 8)
                    st_copy_row<2>(src4, dst, n4, lane);
                else
                    st_copy_row<1>(src4, dst, n4, lane);
            } else if (l < n4) {                                     // (n4 <= lpr: the host chose lpr so)
                const float4 v = src4[l];
                if (mis == 0)
                    st_store<4>(dst + 4 * l, v);
                else if (mis == 8)
                    st_store<2>(dst + 4 * l, v);
                else
                    st_store<1>(dst + 4 * l, v);
            }
            if (l < (W & 3)) dst[4 * n4 + l] = src[4 * n4 + l];      // (a table whose row stride, but not W, is a multiple of four floats)
        } else {
            for (int c = l; c < W; c += lpr) dst[c] = src[c];
        }
        if (l < 4) dst[W + l] = dfol_box_position(box6 + r * 6, l);
    }
}

}  // namespace

extern "C" int dfol_store_objects_f32(const float* cache, int64_t ld_cache, const int32_t* src_row, const float* box6, int32_t O, int32_t W, float* out,
                                      int64_t ld_out, void* stream) {
    DFOL_REQUIRE(O >= 0 && W > 0 && ld_cache >= W, "store_objects: bad sizes O=%d W=%d ld_cache=%lld", O, W, (long long)ld_cache);
    DFOL_REQUIRE(ld_out >= (int64_t)W + 4, "store_objects: ld_out=%lld is less than W + 4 = %d", (long long)ld_out, W + 4);
    if (O == 0) return 0;
    DFOL_REQUIRE(cache && src_row && box6 && out, "store_objects: null pointer");
    int lpr = 8;                                                     // lanes per row: a 16-byte piece each up to W = 128, then the whole wavefront
    while (lpr < 64 && 4 * lpr < W) lpr *= 2;
    const int waves = dfol_cdiv(O, 64 / lpr);
    int blocks = dfol_cdiv(waves, ST_WAVES);
    blocks = blocks < ST_TARGET_WAVES / ST_WAVES ? blocks : ST_TARGET_WAVES / ST_WAVES;
    const dim3 grid(blocks), block(ST_WAVES * 64);
    const bool vec = ld_cache % 4 == 0 && (reinterpret_cast<uintptr_t>(cache) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(store_objects_kernel<true>, grid, block, 0, (hipStream_t)stream, cache, ld_cache, src_row, box6, O, W, lpr, out, ld_out);
    else
        hipLaunchKernelGGL(store_objects_kernel<false>, grid, block, 0, (hipStream_t)stream, cache, ld_cache, src_row, box6, O, W, lpr, out, ld_out);
    DFOL_LAUNCH_CHECK("store_objects");
    return 0;
}

extern "C" int dfol_store_rows_f32(const float* store_boxes, const float* store_sizes, const int32_t* slot, const int32_t* obj_off, int32_t I, int32_t S,
                                   int32_t max_obj, int32_t* src_row, float* box6, void* stream) {
    DFOL_REQUIRE(I >= 0 && S > 0 && max_obj > 0, "store_rows: bad sizes I=%d S=%d max_obj=%d", I, S, max_obj);
    DFOL_REQUIRE((int64_t)S * max_obj < (1ll << 31), "store_rows: S * max_obj = %lld rows do not fit the int32 row numbers (< 2^31)",
                 (long long)S * max_obj);
    if (I == 0) return 0;
    DFOL_REQUIRE(store_boxes && store_sizes && slot && obj_off && src_row && box6, "store_rows: null pointer");
    const int slices = dfol_cdiv(max_obj, SR_THREADS);
    DFOL_REQUIRE(slices <= 65535, "store_rows: max_obj=%d is more than a launch's %d rows per image", max_obj, 65535 * SR_THREADS);
    hipLaunchKernelGGL(store_rows_kernel, dim3(I, slices), dim3(SR_THREADS), 0, (hipStream_t)stream, store_boxes, store_sizes, slot, obj_off, max_obj,
                       src_row, box6);
    DFOL_LAUNCH_CHECK("store_rows");
    return 0;
}

extern "C" int dfol_store_round_bf16(const float* src, int64_t n, void* dst, void* stream) {
    DFOL_REQUIRE(n >= 0, "store_round_bf16: bad size n=%lld", (long long)n);
    if (n == 0) return 0;
    DFOL_REQUIRE(src && dst, "store_round_bf16: null pointer");
    DFOL_REQUIRE((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0, "store_round_bf16: src and dst must be 4-byte aligned");
    int64_t blocks = ((n + 1) / 2 + RB_THREADS - 1) / RB_THREADS;
    blocks = blocks < 8192 ? blocks : 8192;
    hipLaunchKernelGGL(round_bf16_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), 0, (hipStream_t)stream, src, n, static_cast<uint16_t*>(dst));
    DFOL_LAUNCH_CHECK("store_round_bf16");
    return 0;
}

extern "C" int dfol_store_bf16_is_f16(const void* table_bf16, int64_t n, void* flag_out, void* stream) {
    DFOL_REQUIRE(n >= 0, "store_bf16_is_f16: bad size n=%lld", (long long)n);
    DFOL_REQUIRE(flag_out, "store_bf16_is_f16: null pointer");
    if (n == 0) return 0;
    DFOL_REQUIRE(table_bf16, "store_bf16_is_f16: null pointer");
    DFOL_REQUIRE((uintptr_t)table_bf16 % 2 == 0 && (uintptr_t)flag_out % 4 == 0, "store_bf16_is_f16: the table must be 2-byte and the flag 4-byte aligned");
    int64_t blocks = (n + RB_THREADS - 1) / RB_THREADS;
    blocks = blocks < 8192 ? blocks : 8192;
    hipLaunchKernelGGL(bf16_is_f16_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), 0, (hipStream_t)stream, static_cast<const uint16_t*>(table_bf16), n,
                       static_cast<uint32_t*>(flag_out));
    DFOL_LAUNCH_CHECK("store_bf16_is_f16");
    return 0;
}

extern "C" int dfol_gather_object_rows_bf16_f32(const void* store_features_bf16, const float* store_boxes, const float* store_sizes, const int32_t* slot,
                                                const int32_t* obj_off, int32_t I, int32_t max_obj, int32_t F, float* out, int64_t ld_out,
                                                void* stream) {
    DFOL_REQUIRE(I >= 0 && F > 0 && max_obj > 0, "gather_object_rows_bf16: bad sizes I=%d max_obj=%d F=%d", I, max_obj, F);
    DFOL_REQUIRE(F % 4 == 0, "gather_object_rows_bf16: F=%d must be a multiple of 4 (8-byte rows of bfloat16)", F);
    DFOL_REQUIRE(ld_out >= (int64_t)F + 6, "gather_object_rows_bf16: ld_out=%lld is less than F + 6 = %d", (long long)ld_out, F + 6);
    if (I == 0) return 0;
    DFOL_REQUIRE(store_features_bf16 && store_boxes && store_sizes && slot && obj_off && out, "gather_object_rows_bf16: null pointer");
    DFOL_REQUIRE((uintptr_t)store_features_bf16 % 8 == 0, "gather_object_rows_bf16: the table must be 8-byte aligned");
    const int rows = dfol_cdiv(max_obj, ST_WAVES);
    int slices = dfol_cdiv(ST_TARGET_WAVES / ST_WAVES, I);
    slices = slices < rows ? slices : rows;
    slices = slices < 65535 ? slices : 65535;
    hipLaunchKernelGGL(gather_object_rows_bf16_kernel, dim3(I, slices), dim3(ST_WAVES * 64), 0, (hipStream_t)stream,
                       static_cast<const uint16_t*>(store_features_bf16), store_boxes, store_sizes, slot, obj_off, max_obj, F, out, ld_out);
    DFOL_LAUNCH_CHECK("gather_object_rows_bf16");
    return 0;
}

extern "C" int dfol_gather_object_rows_f32(const float* store_features, const float* store_boxes, const float* store_sizes, const int32_t* slot,
                                           const int32_t* obj_off, int32_t I, int32_t max_obj, int32_t F, float* out, int64_t ld_out,
                                           void* stream) {
    DFOL_REQUIRE(I >= 0 && F > 0 && max_obj > 0, "gather_object_rows: bad sizes I=%d max_obj=%d F=%d", I, max_obj, F);
    DFOL_REQUIRE(ld_out >= (int64_t)F + 6, "gather_object_rows: ld_out=%lld is less than F + 6 = %d", (long long)ld_out, F + 6);
    if (I == 0) return 0;
    DFOL_REQUIRE(store_features && store_boxes && store_sizes && slot && obj_off && out, "gather_object_rows: null pointer");
    const int rows = dfol_cdiv(max_obj, ST_WAVES);
    int slices = dfol_cdiv(ST_TARGET_WAVES / ST_WAVES, I);
    slices = slices < rows ? slices : rows;
    slices = slices < 65535 ? slices : 65535;
    const dim3 grid(I, slices), block(ST_WAVES * 64);
    const bool vec = F % 4 == 0 && (reinterpret_cast<uintptr_t>(store_features) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(gather_object_rows_kernel<true>, grid, block, 0, (hipStream_t)stream, store_features, store_boxes, store_sizes, slot,
                           obj_off, max_obj, F, out, ld_out);
    else
        hipLaunchKernelGGL(gather_object_rows_kernel<false>, grid, block, 0, (hipStream_t)stream, store_features, store_boxes, store_sizes, slot,
                           obj_off, max_obj, F, out, ld_out);
    DFOL_LAUNCH_CHECK("gather_object_rows");
    return 0;
}
