// Scene-graph supervision, the relation side's input: the rows of the LISTED (subject, object) pairs of a batch
// (batch_gqa_boxfeatures_pipeline.py:225-279 for the indices meta_data['object_pairs'] lists, offset per image :238-249) and their backward.
//   scene_pair_rows_kernel      out[p] = [obj[s_p], obj[o_p], dist, angle, sign(xo - xs), sign(yo - ys)], one wavefront per pair row; the last four
//                               columns of an object row are its box (x, y, w, h):  dx = xs + ws / 2 - xo - wo / 2, dy likewise,
//                               dist = sqrt(dx dx + dy dy), angle = asin(dy / max(dist, 1e-10))  - interpreter.build_scene_graph's expressions,
//                               term for term and without contraction, so the two gathered blocks and the two signs are the tensor ops' bits
//   scene_pair_rows_bwd_kernel  d_obj[t] = sum of the g blocks the by-object list names for t, in the list's order: one wavefront per object row,
//                               its lanes side by side over the D columns, each walking the whole segment - however long - front to back.
// No atomics; the order of every sum is the list's (sorted by object, then pair number, subject block before object block): two runs give the same
// bits, and a pair row appended behind the real ones (a padded batch) does not move the real ones' places in it.  The four geometry columns carry
// no gradient back: they come from the box columns, which feed no parameter.  An index outside its range is clamped, never followed.
#include "dfol_common.h"

namespace {

constexpr int SP_WAVES = 4, SP_T = SP_WAVES * 64;

__device__ __forceinline__ float sp_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : (v == v ? 0.f : v)); }   // torch.sign; a NaN stays one

// [dist, angle, side x, side y] of subject box s and object box o, each (x, y, w, h)
__device__ __forceinline__ float4 sp_geometry(const float* __restrict__ s, const float* __restrict__ o) {
#pragma clang fp contract(off)
    const float dx = ((s[0] + s[2] / 2.0f) - o[0]) - o[2] / 2.0f;
    const float dy = ((s[1] + s[3] / 2.0f) - o[1]) - o[3] / 2.0f;
    const float xx = dx * dx, yy = dy * dy;
    const float dist = sqrtf(xx + yy);
    return make_float4(dist, asinf(dy / fmaxf(dist, 1e-10f)), sp_sign(o[0] - s[0]), sp_sign(o[1] - s[1]));
}

__global__ __launch_bounds__(SP_T) void scene_pair_rows_kernel(const float* __restrict__ obj, int64_t ld_obj, int O, int D, const int32_t* __restrict__ pair_s,
                                                               const int32_t* __restrict__ pair_o, int P, float* __restrict__ out, int64_t ld_out, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (p >= P) return;
    const int s = min(max(pair_s[p], 0), O - 1), o = min(max(pair_o[p], 0), O - 1);
    const float* rs = obj + (int64_t)s * ld_obj;
    const float* ro = obj + (int64_t)o * ld_obj;
    float* w = out + p * ld_out;
    if (vec) {                                                       // D % 4 == 0 and every row 16-byte aligned: 16 B per lane
        for (int c = lane * 4; c < D; c += 256) {
            *reinterpret_cast<float4*>(w + c) = *reinterpret_cast<const float4*>(rs + c);
            *reinterpret_cast<float4*>(w + D + c) = *reinterpret_cast<const float4*>(ro + c);
        }
    } else {
        const int D4 = ld_obj % 4 == 0 && (reinterpret_cast<uintptr_t>(obj) & 15) == 0 ? D & ~3 : 0;      // aligned loads, scalar stores and tail
        for (int c = lane * 4; c < D4; c += 256) {
            const float4 a = *reinterpret_cast<const float4*>(rs + c), b = *reinterpret_cast<const float4*>(ro + c);
            w[c] = a.x, w[c + 1] = a.y, w[c + 2] = a.z, w[c + 3] = a.w;
            w[D + c] = b.x, w[D + c + 1] = b.y, w[D + c + 2] = b.z, w[D + c + 3] = b.w;
        }
        for (int c = D4 + lane; c < D; c += 64) {
            w[c] = rs[c];
            w[D + c] = ro[c];
        }
    }
    if (lane == 0) {
        const float4 g = sp_geometry(rs + D - 4, ro + D - 4);
        w[2 * D] = g.x, w[2 * D + 1] = g.y, w[2 * D + 2] = g.z, w[2 * D + 3] = g.w;
    }
}

__global__ __launch_bounds__(SP_T) void scene_pair_rows_bwd_kernel(const float* __restrict__ g, int64_t ld_g, int P, int D, const int32_t* __restrict__ seg_off,
                                                                   const int32_t* __restrict__ slot, int O, float* __restrict__ d_obj, int64_t ld_d, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (t >= O) return;
    const int n_slots = 2 * P;
    const int k0 = min(max(seg_off[t], 0), n_slots), k1 = min(max(seg_off[t + 1], k0), n_slots);
    float* w = d_obj + t * ld_d;
    if (vec) {
        for (int c = lane * 4; c < D; c += 256) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = k0; k < k1; ++k) {
                const int e = min(max(slot[k], 0), n_slots - 1);     // 2 pair + (0: its subject block, 1: its object block)
                const float4 v = *reinterpret_cast<const float4*>(g + (int64_t)(e >> 1) * ld_g + (e & 1) * D + c);
                acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
            }
            *reinterpret_cast<float4*>(w + c) = acc;
        }
    } else {
        for (int c = lane; c < D; c += 64) {
            float acc = 0.f;
            for (int k = k0; k < k1; ++k) {
                const int e = min(max(slot[k], 0), n_slots - 1);
                acc += g[(int64_t)(e >> 1) * ld_g + (e & 1) * D + c];
            }
            w[c] = acc;
        }
    }
}

inline bool sp_aligned(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

}  // namespace

extern "C" int dfol_scene_pair_rows_f32(const float* obj, int64_t ld_obj, int32_t O, int32_t D, const int32_t* pair_s, const int32_t* pair_o, int32_t P,
                                        float* out, int64_t ld_out, void* stream) {
    DFOL_REQUIRE(O >= 0 && P >= 0 && D >= 4 && ld_obj >= D && ld_out >= 2 * (int64_t)D + 4, "scene_pair_rows: bad sizes O=%d P=%d D=%d ld_obj=%lld ld_out=%lld",
                 O, P, D, (long long)ld_obj, (long long)ld_out);
    if (P == 0) return 0;
    DFOL_REQUIRE(O >= 1, "scene_pair_rows: %d pairs over no object", P);
    DFOL_REQUIRE(obj && pair_s && pair_o && out, "scene_pair_rows: null pointer");
    const int vec = D % 4 == 0 && sp_aligned(obj, ld_obj) && sp_aligned(out, ld_out) ? 1 : 0;
    hipLaunchKernelGGL(scene_pair_rows_kernel, dim3((unsigned)dfol_cdiv(P, SP_WAVES)), dim3(SP_T), 0, (hipStream_t)stream, obj, ld_obj, O, D, pair_s, pair_o,
                       P, out, ld_out, vec);
    DFOL_LAUNCH_CHECK("scene_pair_rows");
    return 0;
}

extern "C" int dfol_scene_pair_rows_bwd_f32(const float* g, int64_t ld_g, int32_t P, int32_t D, const int32_t* seg_off, const int32_t* slot, int32_t O,
                                            float* d_obj, int64_t ld_d, void* stream) {
    DFOL_REQUIRE(O >= 0 && P >= 0 && P < (1 << 30) && D >= 1 && ld_d >= D && ld_g >= 2 * (int64_t)D, "scene_pair_rows_bwd: bad sizes O=%d P=%d D=%d ld_g=%lld ld_d=%lld",
                 O, P, D, (long long)ld_g, (long long)ld_d);
    if (O == 0) return 0;
    DFOL_REQUIRE(seg_off && d_obj && (P == 0 || (g && slot)), "scene_pair_rows_bwd: null pointer");
    const int vec = D % 4 == 0 && sp_aligned(d_obj, ld_d) && (P == 0 || sp_aligned(g, ld_g)) ? 1 : 0;
    hipLaunchKernelGGL(scene_pair_rows_bwd_kernel, dim3((unsigned)dfol_cdiv(O, SP_WAVES)), dim3(SP_T), 0, (hipStream_t)stream, g, ld_g, P, D, seg_off, slot, O,
                       d_obj, ld_d, vec);
    DFOL_LAUNCH_CHECK("scene_pair_rows_bwd");
    return 0;
}
