// What the two weight-gradient files share: the dense TN product (csrc/dfol_dense_wgrad.hip) and the fused weight gradient of the pair
// layer (csrc/dfol_pair_wgrad.hip) both cut the rows into slabs, write one partial block per slab and add the blocks in a fixed order.
#pragma once

#include "dfol_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Floats from one slab's partial block of `elems` results to the next: slabs start 16-byte aligned (the padding floats are never stored)
__host__ __device__ __forceinline__ int64_t wgrad_slab_stride(int64_t elems) { return (elems + 3) & ~(int64_t)3; }

// A buffer descriptor over `bytes` bytes from `base`, both wave-uniform
// (every input through readfirstlane: hipcc wraps each buffer load in a waterfall loop unless the descriptor is provably wave-uniform)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t w3_descriptor(const void* base, int64_t bytes) {
    const uint64_t p = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    const int n = __builtin_amdgcn_readfirstlane((int)(bytes < 0x7fffffff ? bytes : 0x7fffffff));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}

namespace {      // (the library is built without relocatable device code: each file that includes this compiles its own copy of the kernel)

// dW[e] = sum over the slabs in a fixed order: a workgroup takes 16 groups of four elements x 16 slab phases (phase p adds slabs p,
// p + 16, ... in order), then the phases are added in order.  (One thread per element group walking all slabs, the first version, was
// 75 workgroups of serial loads for the pair layer.)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int slabs, int64_t elems, float* __restrict__ dW) {
    __shared__ float4 sums[16][16];
    const int g = threadIdx.x & 15, phase = threadIdx.x >> 4;
    const int64_t e = ((int64_t)blockIdx.x * 16 + g) * 4;
    const int64_t stride = wgrad_slab_stride(elems);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < elems)
        for (int i = phase; i < slabs; i += 16) {
            const float4 v = *reinterpret_cast<const float4*>(part + (int64_t)i * stride + e);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    sums[phase][g] = s;
    __syncthreads();
    if (phase != 0 || e >= elems) return;
#pragma unroll
    for (int p = 1; p < 16; ++p) {
        const float4 v = sums[p][g];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (e + 4 <= elems) *reinterpret_cast<float4*>(dW + e) = s;
    else {
        const float t[4] = {s.x, s.y, s.z, s.w};
        for (int64_t k = e; k < elems; ++k) dW[k] = t[k - e];
    }
}

}  // namespace

// out [elems] = the partial blocks of `slabs` slabs added up; `who` and `what` name the launch in the message of a failure
static int wgrad_reduce(const char* who, const char* what, const float* part, int slabs, int64_t elems, float* out, hipStream_t st) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(dfol_cdiv(dfol_cdiv(elems, 4), 16)), dim3(256), 0, st, part, slabs, elems, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) dfol_set_error("%s (%s): launch failed: %s", who, what, hipGetErrorString(e));
    return e != hipSuccess ? 2 : 0;                        // (DFOL_LAUNCH_CHECK's status)
}
