// Scene-graph supervision (operator `scene`, batch_gqa_ops.py:883-902; the loss trainer.py:235-256, the metric :265-275): the weighted BCE of
// ALL concept columns of the embedding layer against dense targets, without any [M, C] array in HBM.
//   z = h E[cols]^T + b[cols],  lp = LogSigmoid(z),  p = e^lp,  l1p = LogSigmoid(-z) (= lp - z = log(1 - p) without the rounded 1 - p)
//   loss = sum -w (t max(lp, -100) + (1 - t) max(l1p, -100))          torch binary_cross_entropy(p, t, weight = w, reduction = 'sum')
//   num  = sum w [(t + a) > 0] [t != a],  den = sum w [(t + a) > 0],  a = [lp > thr]
//   dz   = g w (p - t) p (1 - p) / max(p (1 - p), 1e-12)               autograd through BCE, exp and LogSigmoid; 0 once saturated
// Three kernels rebuild the same z tile (64 rows x 32 columns; the h row block and the gathered E rows sit in LDS as fp32 over the whole padded
// K, every wavefront splits its own fragments in registers):
//   scene_fwd_kernel       a workgroup owns a row block and a slab of column tiles; three partial sums per workgroup, added by an ordered pass
//   scene_bwd_rows_kernel  a workgroup owns a row block and walks ALL column tiles: dh = dz E[cols] accumulates in its registers
//   scene_bwd_cols_kernel  a workgroup owns a column tile and walks a slab of row blocks: dE = dz^T h and db = sum_rows dz in its registers;
//                          more than one slab leaves partial outputs that an ordered pass adds
// No atomics on any sum: two runs give the same bits.  Arithmetic: z from two fp16 pieces per operand and three products
// (dfol_split2h; h is a Sigmoid output, E is split unscaled and an element beyond fp16's range is reported through the range word); the
// backward products from three bf16 pieces per operand and six products (dfol_split3: dz has no natural scale).
// The z tile's dz goes through a 9 KB LDS tile to become an MFMA operand; it never reaches HBM.
#include "dfol_common.h"
#include "dfol_split.h"

namespace {

constexpr int SC_BM = 64, SC_BN = 32, SC_T = 256, SC_DP = 36;   // rows / columns of a z tile, threads, pitch of the dz tile
constexpr int SC_MAXH = 320;                                    // the widest hidden row (dfol_attr_head_h2_f32's HID2 limit)
constexpr int SC_HT = SC_MAXH / 16 / 4;                         // 16-column tiles of an [*, H] output per wavefront (tiles w, w + 4, ...)
constexpr int SC_MAX_SLABS = 16;

__host__ __device__ inline int sc_kp(int K) { return (K + 31) / 32 * 32; }
inline size_t sc_lds_bytes(int K) { return ((size_t)(SC_BM + SC_BN) * (sc_kp(K) + 4) + SC_BM * SC_DP + 16) * sizeof(float); }

// R rows of a [*, K] fp32 matrix (rows idx[row0 + r] of it when idx is given, clamped to [0, n_src)) into dst [R][pitch], zero beyond nrows and K.
// Returns true if an element is beyond fp16's largest finite value or NaN.
__device__ __forceinline__ bool sc_stage(float* __restrict__ dst, int pitch, int KP, const float* __restrict__ src, int64_t ld, const int32_t* __restrict__ idx,
                                         int n_src, int row0, int nrows, int R, int K, int vec) {
    bool bad = false;
    const int q = KP >> 2;
    for (int i = threadIdx.x; i < R * q; i += SC_T) {
        const int r = i / q, k = (i - r * q) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int gr = row0 + r;
        if (gr < nrows && k < K) {
            const int sr = idx ? min(max(idx[gr], 0), n_src - 1) : gr;
            const float* p = src + (int64_t)sr * ld + k;
            if (vec && k + 4 <= K) v = *reinterpret_cast<const float4*>(p);
            else {
                v.x = p[0];
                if (k + 1 < K) v.y = p[1];
                if (k + 2 < K) v.z = p[2];
                if (k + 3 < K) v.w = p[3];
            }
            bad |= !(fabsf(v.x) <= 65504.f) || !(fabsf(v.y) <= 65504.f) || !(fabsf(v.z) <= 65504.f) || !(fabsf(v.w) <= 65504.f);
        }
        *reinterpret_cast<float4*>(dst + r * pitch + k) = v;
    }
    return bad;
}

// Eight consecutive k of an MFMA fragment from an fp32 LDS tile: element (r, k) at s[r * pitch + k] (KCONT) or at s[k * pitch + r]
template <bool KCONT>
__device__ __forceinline__ void sc_frag(const float* __restrict__ s, int pitch, int r, int k, float4& a, float4& b) {
    if (KCONT) {
        a = *reinterpret_cast<const float4*>(s + r * pitch + k);
        b = *reinterpret_cast<const float4*>(s + r * pitch + k + 4);
    } else {
        const float* p = s + k * pitch + r;
        a = make_float4(p[0], p[pitch], p[2 * pitch], p[3 * pitch]);
        b = make_float4(p[4 * pitch], p[5 * pitch], p[6 * pitch], p[7 * pitch]);
    }
}
struct ScP3 { u32x4 p[3]; };
template <bool KCONT>
__device__ __forceinline__ ScP3 sc_frag3(const float* __restrict__ s, int pitch, int r, int k) {
    float4 a, b;
    sc_frag<KCONT>(s, pitch, r, k, a, b);
    ScP3 o;
    dfol_split3x8(a, b, o.p[0], o.p[1], o.p[2]);
    return o;
}
// acc += A B on three bf16 pieces each: six products, smallest first (csrc/dfol_dense_split.hip)
__device__ __forceinline__ floatx4 sc_mfma6(const ScP3& a, const ScP3& b, floatx4 acc) {
    constexpr int PA6[6] = {2, 0, 1, 1, 0, 0}, PB6[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int x = 0; x < 6; ++x)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a.p[PA6[x]]), __builtin_bit_cast(bf16x8, b.p[PB6[x]]), acc, 0, 0, 0);
    return acc;
}

// z tile without the bias: wavefront `wave` owns rows 16 wave .. + 15 and both 16-column tiles.  acc[j][e]: row 16 wave + 4 kh + e, column 16 j + r16.
__device__ __forceinline__ void sc_z_tile(const float* __restrict__ Hs, const float* __restrict__ Es, int pitch, int KP, int wave, int kh, int r16, floatx4 (&acc)[2]) {
    acc[0] = acc[1] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < KP; k0 += 32) {
        float4 x0, x1;
        u32x4 ah, al;
        sc_frag<true>(Hs, pitch, wave * 16 + r16, k0 + kh * 8, x0, x1);
        dfol_split2hx8(x0, x1, ah, al);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32x4 bh, bl;
            sc_frag<true>(Es, pitch, j * 16 + r16, k0 + kh * 8, x0, x1);
            dfol_split2hx8(x0, x1, bh, bl);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, al), __builtin_bit_cast(f16x8, bh), acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, bl), acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, bh), acc[j], 0, 0, 0);
        }
    }
}

// lp = LogSigmoid(z) and l1p = LogSigmoid(-z) from one shared log1p term (libm forms: the sums are compared with float64)
__device__ __forceinline__ void sc_point(float z, float& lp, float& l1p) {
    const float L = log1pf(expf(-fabsf(z)));
    lp = fminf(z, 0.f) - L;
    l1p = fminf(-z, 0.f) - L;
}
// dz / g:  w (p - t) p q / max(p q, 1e-12) with q = 1 - p = e^l1p and p - t = (1 - t) p - t q (no cancellation at either end); +0 where w is 0
__device__ __forceinline__ float sc_dz(float z, float t, float w) {
    float lp, l1p;
    sc_point(z, lp, l1p);
    const float p = expf(lp), q = expf(l1p), pq = p * q;
    return w == 0.f ? 0.f : w * ((1.f - t) * p - t * q) * (pq / fmaxf(pq, 1e-12f));
}

// The z tile's dz into the LDS tile Dz [SC_BM][SC_DP] (row, column); 0 outside [M, C]
__device__ __forceinline__ void sc_dz_tile(const floatx4 (&acc)[2], float* __restrict__ Dz, const float* __restrict__ bias, const int32_t* __restrict__ cols,
                                           int n_src, const float* __restrict__ tgt, const float* __restrict__ wgt, float g, int row0, int col0, int M, int C,
                                           int wave, int kh, int r16) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cl = j * 16 + r16, col = col0 + cl;
        const float bj = (bias && col < C) ? bias[min(max(cols[col], 0), n_src - 1)] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rl = wave * 16 + kh * 4 + e, row = row0 + rl;
            float d = 0.f;
            if (row < M && col < C) {
                const int64_t at = (int64_t)row * C + col;
                const float w = wgt[at];
                d = sc_dz(acc[j][e] + bj, tgt[at], w);
                d = w == 0.f ? 0.f : g * d;
            }
            Dz[rl * SC_DP + cl] = d;
        }
    }
}

__global__ __launch_bounds__(SC_T) void scene_fwd_kernel(const float* __restrict__ h, int64_t ldh, int M, int K, const float* __restrict__ E, int64_t lde,
                                                          int n_src, const float* __restrict__ bias, const int32_t* __restrict__ cols, int C,
                                                          const float* __restrict__ tgt, const float* __restrict__ wgt, float thr, int tiles_per_slab,
                                                          float* __restrict__ partials, uint32_t* __restrict__ status, int vec_h, int vec_e) {
    extern __shared__ __attribute__((aligned(16))) float sc_lds[];
    const int KP = sc_kp(K), pitch = KP + 4;
    float* Hs = sc_lds;
    float* Es = Hs + SC_BM * pitch;
    float* red = Es + SC_BN * pitch + SC_BM * SC_DP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 4, r16 = lane & 15;
    const int row0 = blockIdx.x * SC_BM, ntiles = (C + SC_BN - 1) / SC_BN;
    const int t0 = blockIdx.y * tiles_per_slab, t1 = min(t0 + tiles_per_slab, ntiles);

    bool bad = sc_stage(Hs, pitch, KP, h, ldh, nullptr, M, row0, M, SC_BM, K, vec_h);
    float loss = 0.f, num = 0.f, den = 0.f;
    for (int ct = t0; ct < t1; ++ct) {
        const int col0 = ct * SC_BN;
        __syncthreads();                                     // the previous tile's fragments are read
        bad |= sc_stage(Es, pitch, KP, E, lde, cols, n_src, col0, C, SC_BN, K, vec_e);
        __syncthreads();
        floatx4 acc[2];
        sc_z_tile(Hs, Es, pitch, KP, wave, kh, r16, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = col0 + j * 16 + r16;
            const float bj = (bias && col < C) ? bias[min(max(cols[col], 0), n_src - 1)] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = row0 + wave * 16 + kh * 4 + e;
                if (row < M && col < C) {
                    const int64_t at = (int64_t)row * C + col;
                    const float t = tgt[at], w = wgt[at];
                    float lp, l1p;
                    sc_point(acc[j][e] + bj, lp, l1p);
                    loss -= w * (t * fmaxf(lp, -100.f) + (1.f - t) * fmaxf(l1p, -100.f));
                    const float a = lp > thr ? 1.f : 0.f;
                    if (t + a > 0.f) {
                        den += w;
                        if (t != a) num += w;
                    }
                }
            }
        }
    }
    if (status != nullptr && __any(bad) && lane == 0) atomicOr(status, (uint32_t)DFOL_RANGE_X_OVERFLOW);
    loss = dfol_wave_sum(loss);
    num = dfol_wave_sum(num);
    den = dfol_wave_sum(den);
    if (lane == 0) {
        red[wave * 3 + 0] = loss;
        red[wave * 3 + 1] = num;
        red[wave * 3 + 2] = den;
    }
    __syncthreads();
    if (tid < 3) {
        const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[wg * 3 + tid] = ((red[tid] + red[3 + tid]) + red[6 + tid]) + red[9 + tid];
    }
}

// out[c] = sum_i partials[i][c], c < 3: one workgroup, thread t adds i = t, t + 256, ... in order (in double), then a fixed tree
__global__ __launch_bounds__(SC_T) void scene_sum3_kernel(const float* __restrict__ partials, int64_t n, float* __restrict__ out) {
    __shared__ double sm[3][SC_T];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += SC_T)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += (double)partials[i * 3 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) sm[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int w = SC_T / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int c = 0; c < 3; ++c) sm[c][threadIdx.x] += sm[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[threadIdx.x] = (float)sm[threadIdx.x][0];
}

__global__ __launch_bounds__(SC_T) void scene_bwd_rows_kernel(const float* __restrict__ gp, const float* __restrict__ h, int64_t ldh, int M, int K,
                                                               const float* __restrict__ E, int64_t lde, int n_src, const float* __restrict__ bias,
                                                               const int32_t* __restrict__ cols, int C, const float* __restrict__ tgt,
                                                               const float* __restrict__ wgt, float* __restrict__ dh, int64_t lddh, int vec_h, int vec_e) {
    extern __shared__ __attribute__((aligned(16))) float sc_lds[];
    const int KP = sc_kp(K), pitch = KP + 4, KT = KP / 16;
    float* Hs = sc_lds;
    float* Es = Hs + SC_BM * pitch;
    float* Dz = Es + SC_BN * pitch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 4, r16 = lane & 15;
    const int row0 = blockIdx.x * SC_BM, ntiles = (C + SC_BN - 1) / SC_BN;
    const float g = gp[0];

    (void)sc_stage(Hs, pitch, KP, h, ldh, nullptr, M, row0, M, SC_BM, K, vec_h);
    floatx4 out[4][SC_HT];                                   // dh rows 16 rt + ..., columns 16 (wave + 4 u) + ...
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int u = 0; u < SC_HT; ++u) out[rt][u] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int ct = 0; ct < ntiles; ++ct) {
        const int col0 = ct * SC_BN;
        __syncthreads();                                     // the previous tile's E rows and dz are read
        (void)sc_stage(Es, pitch, KP, E, lde, cols, n_src, col0, C, SC_BN, K, vec_e);
        __syncthreads();
        floatx4 acc[2];
        sc_z_tile(Hs, Es, pitch, KP, wave, kh, r16, acc);
        sc_dz_tile(acc, Dz, bias, cols, n_src, tgt, wgt, g, row0, col0, M, C, wave, kh, r16);
        __syncthreads();
        // dh [64, K] += dz [64, 32] E [32, K]: one k-step over the tile's 32 columns; A = dz (k contiguous), B = E rows (k strided)
        ScP3 a[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) a[rt] = sc_frag3<true>(Dz, SC_DP, rt * 16 + r16, kh * 8);
#pragma unroll
        for (int u = 0; u < SC_HT; ++u) {
            const int ht = wave + 4 * u;
            if (ht < KT) {
                const ScP3 b = sc_frag3<false>(Es, pitch, ht * 16 + r16, kh * 8);
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) out[rt][u] = sc_mfma6(a[rt], b, out[rt][u]);
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int u = 0; u < SC_HT; ++u) {
            const int hc = (wave + 4 * u) * 16 + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = row0 + rt * 16 + kh * 4 + e;
                if (row < M && hc < K) dh[(int64_t)row * lddh + hc] = out[rt][u][e];
            }
        }
}

__global__ __launch_bounds__(SC_T) void scene_bwd_cols_kernel(const float* __restrict__ gp, const float* __restrict__ h, int64_t ldh, int M, int K,
                                                               const float* __restrict__ E, int64_t lde, int n_src, const float* __restrict__ bias,
                                                               const int32_t* __restrict__ cols, int C, const float* __restrict__ tgt,
                                                               const float* __restrict__ wgt, int blocks_per_slab, float* __restrict__ dE,
                                                               float* __restrict__ db, int64_t slab_stride, int vec_h, int vec_e) {
    extern __shared__ __attribute__((aligned(16))) float sc_lds[];
    const int KP = sc_kp(K), pitch = KP + 4, KT = KP / 16;
    float* Hs = sc_lds;
    float* Es = Hs + SC_BM * pitch;
    float* Dz = Es + SC_BN * pitch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 4, r16 = lane & 15;
    const int col0 = blockIdx.x * SC_BN, nblocks = (M + SC_BM - 1) / SC_BM;
    const int b0 = blockIdx.y * blocks_per_slab, b1 = min(b0 + blocks_per_slab, nblocks);
    const float g = gp[0];
    dE += (int64_t)blockIdx.y * slab_stride;
    db += (int64_t)blockIdx.y * slab_stride;

    (void)sc_stage(Es, pitch, KP, E, lde, cols, n_src, col0, C, SC_BN, K, vec_e);
    floatx4 out[2][SC_HT];                                   // dE rows (columns of z) 16 nt + ..., columns 16 (wave + 4 u) + ...
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int u = 0; u < SC_HT; ++u) out[nt][u] = floatx4{0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    for (int rb = b0; rb < b1; ++rb) {
        const int row0 = rb * SC_BM;
        __syncthreads();                                     // the previous block's h rows and dz are read
        (void)sc_stage(Hs, pitch, KP, h, ldh, nullptr, M, row0, M, SC_BM, K, vec_h);
        __syncthreads();
        floatx4 acc[2];
        sc_z_tile(Hs, Es, pitch, KP, wave, kh, r16, acc);
        sc_dz_tile(acc, Dz, bias, cols, n_src, tgt, wgt, g, row0, col0, M, C, wave, kh, r16);
        __syncthreads();
        if (tid < SC_BN)
            for (int m = 0; m < SC_BM; ++m) dbs += Dz[m * SC_DP + tid];
        // dE [32, K] += dz^T [32, 64] h [64, K]: two k-steps over the block's 64 rows; both operands k strided
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            ScP3 a[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) a[nt] = sc_frag3<false>(Dz, SC_DP, nt * 16 + r16, ks * 32 + kh * 8);
#pragma unroll
            for (int u = 0; u < SC_HT; ++u) {
                const int ht = wave + 4 * u;
                if (ht < KT) {
                    const ScP3 b = sc_frag3<false>(Hs, pitch, ht * 16 + r16, ks * 32 + kh * 8);
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) out[nt][u] = sc_mfma6(a[nt], b, out[nt][u]);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int u = 0; u < SC_HT; ++u) {
            const int hc = (wave + 4 * u) * 16 + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = col0 + nt * 16 + kh * 4 + e;
                if (col < C && hc < K) dE[(int64_t)col * K + hc] = out[nt][u][e];
            }
        }
    if (tid < SC_BN && col0 + tid < C) db[col0 + tid] = dbs;
}

// out[i] = part[0][i] + part[1][i] + ... in that order
__global__ void scene_sum_slabs_kernel(const float* __restrict__ part, int64_t stride, int slabs, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int k = 1; k < slabs; ++k) s += part[(int64_t)k * stride + i];
    out[i] = s;
}

inline int sc_vec(const float* p, int64_t ld) { return ((uintptr_t)p % 16 == 0 && ld % 4 == 0) ? 1 : 0; }
constexpr int SC_FWD_SLAB = 8;                                // column tiles per forward workgroup (256 columns)
// slabs of row blocks of the column kernel: enough workgroups to cover the chip, at most SC_MAX_SLABS partial outputs
inline void sc_cols_slabs(int32_t M, int32_t C, int& slabs, int& per) {
    const int rb = dfol_cdiv(M, SC_BM), cb = dfol_cdiv(C, SC_BN);
    int want = 512 / (cb > 0 ? cb : 1);
    want = want < 1 ? 1 : (want > SC_MAX_SLABS ? SC_MAX_SLABS : want);
    if (want > rb) want = rb > 0 ? rb : 1;
    per = rb > 0 ? dfol_cdiv(rb, want) : 1;
    slabs = rb > 0 ? dfol_cdiv(rb, per) : 1;
}

template <class Kern>
inline bool sc_lds_ok(Kern kern, size_t bytes) {
    return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

int sc_check(const char* name, int32_t M, int32_t H, int32_t C, int32_t C_all, int64_t ldh, int64_t lde) {
    DFOL_REQUIRE(M >= 0 && C >= 0 && C_all >= 0, "%s: bad sizes M=%d C=%d C_all=%d", name, M, C, C_all);
    DFOL_REQUIRE(dfol_scene_bce_supported(M, H, C), "%s: H=%d is not in [1, %d] (dfol_scene_bce_supported)", name, H, SC_MAXH);
    DFOL_REQUIRE(ldh >= H && lde >= H, "%s: row strides %lld, %lld below H=%d", name, (long long)ldh, (long long)lde, H);
    DFOL_REQUIRE(C == 0 || C_all > 0, "%s: columns without embedding rows", name);
    return 0;
}

}  // namespace

extern "C" int dfol_scene_bce_supported(int32_t M, int32_t H, int32_t C) { return (M >= 0 && C >= 0 && H >= 1 && H <= SC_MAXH) ? 1 : 0; }

extern "C" int64_t dfol_scene_bce_fwd_workspace(int32_t M, int32_t H, int32_t C) {
    if (M <= 0 || C <= 0) return 0;
    return (int64_t)dfol_cdiv(M, SC_BM) * dfol_cdiv(dfol_cdiv(C, SC_BN), SC_FWD_SLAB) * 3;
}

extern "C" int64_t dfol_scene_bce_bwd_cols_workspace(int32_t M, int32_t H, int32_t C) {
    if (M <= 0 || C <= 0) return 0;
    int slabs, per;
    sc_cols_slabs(M, C, slabs, per);
    return slabs > 1 ? (int64_t)slabs * ((int64_t)C * H + C) : 0;
}

extern "C" int dfol_scene_bce_fwd_f32(const float* h, int64_t ldh, int32_t M, int32_t H, const float* emb_w, int64_t lde, int32_t C_all, const float* emb_b,
                                      const int32_t* cols, int32_t C, const float* target, const float* weight, float thr, float* workspace,
                                      float* sums, void* stream) {
    if (int rc = sc_check("scene_bce_fwd", M, H, C, C_all, ldh, lde)) return rc;
    DFOL_REQUIRE(sums, "scene_bce_fwd: null output");
    hipStream_t st = (hipStream_t)stream;
    if (M == 0 || C == 0) {
        DFOL_REQUIRE(hipMemsetAsync(sums, 0, 3 * sizeof(float), st) == hipSuccess, "scene_bce_fwd: memset failed");
        return 0;
    }
    DFOL_REQUIRE(h && emb_w && cols && target && weight && workspace, "scene_bce_fwd: null pointer");
    const size_t lds = sc_lds_bytes(H);
    static const bool ok = sc_lds_ok(scene_fwd_kernel, sc_lds_bytes(SC_MAXH));
    DFOL_REQUIRE(ok, "scene_bce_fwd: cannot reserve %zu bytes of LDS", sc_lds_bytes(SC_MAXH));
    const int tps = SC_FWD_SLAB;
    const dim3 grid(dfol_cdiv(M, SC_BM), dfol_cdiv(dfol_cdiv(C, SC_BN), tps));
    hipLaunchKernelGGL(scene_fwd_kernel, grid, dim3(SC_T), lds, st, h, ldh, M, H, emb_w, lde, C_all, emb_b, cols, C, target, weight, thr, tps, workspace,
                       dfol_range_status_ptr(), sc_vec(h, ldh), sc_vec(emb_w, lde));
    DFOL_LAUNCH_CHECK("scene_bce_fwd");
    hipLaunchKernelGGL(scene_sum3_kernel, dim3(1), dim3(SC_T), 0, st, workspace, (int64_t)grid.x * grid.y, sums);
    DFOL_LAUNCH_CHECK("scene_bce_fwd (sum)");
    return 0;
}

extern "C" int dfol_scene_bce_bwd_rows_f32(const float* g, const float* h, int64_t ldh, int32_t M, int32_t H, const float* emb_w, int64_t lde, int32_t C_all,
                                           const float* emb_b, const int32_t* cols, int32_t C, const float* target, const float* weight, float* dh,
                                           int64_t ld_dh, void* stream) {
    if (int rc = sc_check("scene_bce_bwd_rows", M, H, C, C_all, ldh, lde)) return rc;
    if (M == 0) return 0;
    DFOL_REQUIRE(dh && ld_dh >= H, "scene_bce_bwd_rows: null output or row stride below H");
    hipStream_t st = (hipStream_t)stream;
    if (C == 0) {
        DFOL_REQUIRE(hipMemset2DAsync(dh, ld_dh * sizeof(float), 0, (size_t)H * sizeof(float), M, st) == hipSuccess, "scene_bce_bwd_rows: memset failed");
        return 0;
    }
    DFOL_REQUIRE(g && h && emb_w && cols && target && weight, "scene_bce_bwd_rows: null pointer");
    static const bool ok = sc_lds_ok(scene_bwd_rows_kernel, sc_lds_bytes(SC_MAXH));
    DFOL_REQUIRE(ok, "scene_bce_bwd_rows: cannot reserve %zu bytes of LDS", sc_lds_bytes(SC_MAXH));
    hipLaunchKernelGGL(scene_bwd_rows_kernel, dim3(dfol_cdiv(M, SC_BM)), dim3(SC_T), sc_lds_bytes(H), st, g, h, ldh, M, H, emb_w, lde, C_all, emb_b, cols, C,
                       target, weight, dh, ld_dh, sc_vec(h, ldh), sc_vec(emb_w, lde));
    DFOL_LAUNCH_CHECK("scene_bce_bwd_rows");
    return 0;
}

extern "C" int dfol_scene_bce_bwd_cols_f32(const float* g, const float* h, int64_t ldh, int32_t M, int32_t H, const float* emb_w, int64_t lde, int32_t C_all,
                                           const float* emb_b, const int32_t* cols, int32_t C, const float* target, const float* weight, float* workspace,
                                           float* dE, float* db, void* stream) {
    if (int rc = sc_check("scene_bce_bwd_cols", M, H, C, C_all, ldh, lde)) return rc;
    if (C == 0) return 0;
    DFOL_REQUIRE(dE && db, "scene_bce_bwd_cols: null output");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)C * H;
    if (M == 0) {
        DFOL_REQUIRE(hipMemsetAsync(dE, 0, n * sizeof(float), st) == hipSuccess && hipMemsetAsync(db, 0, (size_t)C * sizeof(float), st) == hipSuccess,
                     "scene_bce_bwd_cols: memset failed");
        return 0;
    }
    DFOL_REQUIRE(g && h && emb_w && cols && target && weight, "scene_bce_bwd_cols: null pointer");
    int slabs, per;
    sc_cols_slabs(M, C, slabs, per);
    DFOL_REQUIRE(slabs == 1 || workspace, "scene_bce_bwd_cols: %d slabs need the workspace of dfol_scene_bce_bwd_cols_workspace", slabs);
    static const bool ok = sc_lds_ok(scene_bwd_cols_kernel, sc_lds_bytes(SC_MAXH));
    DFOL_REQUIRE(ok, "scene_bce_bwd_cols: cannot reserve %zu bytes of LDS", sc_lds_bytes(SC_MAXH));
    // one slab writes the outputs; several write [slab][C H | C] partial outputs (the two at the same slab stride) for the ordered pass
    float* oE = slabs == 1 ? dE : workspace;
    float* ob = slabs == 1 ? db : workspace + n;
    hipLaunchKernelGGL(scene_bwd_cols_kernel, dim3(dfol_cdiv(C, SC_BN), slabs), dim3(SC_T), sc_lds_bytes(H), st, g, h, ldh, M, H, emb_w, lde, C_all, emb_b,
                       cols, C, target, weight, per, oE, ob, slabs == 1 ? (int64_t)0 : n + C, sc_vec(h, ldh), sc_vec(emb_w, lde));
    DFOL_LAUNCH_CHECK("scene_bce_bwd_cols");
    if (slabs > 1) {
        hipLaunchKernelGGL(scene_sum_slabs_kernel, dim3(dfol_cdiv(n, 256)), dim3(256), 0, st, workspace, n + C, slabs, n, dE);
        hipLaunchKernelGGL(scene_sum_slabs_kernel, dim3(dfol_cdiv(C, 256)), dim3(256), 0, st, workspace + n, n + C, slabs, (int64_t)C, db);
        DFOL_LAUNCH_CHECK("scene_bce_bwd_cols (sum)");
    }
    return 0;
}
