// The row walk of the forward RMS norms over [M, D] bf16 rows (csrc/gemma.hip, csrc/t5.hip, csrc/dcae.hip): LPR lanes per
// row (a power of two dividing D / 8, at most 64), two passes over the row (the second re-reads it from L1), fp32 inside.
//   pass 1: ss = sum of squares of what Pre makes of each loaded 8-chunk of x;
//   pass 2: v = Pre's row * rsqrt(ss / D + eps), then Post finishes the chunk from (v, w) with its own rounding points.
// Pre  : void operator()(float* v, int64_t off) const   -- the chunk of x at element offset `off`, changed in place
//        const bf16_t* src(const bf16_t* x) const        -- the row matrix pass 2 reads (x, or what operator() stored)
// Post : void operator()(float* v, const float* w, int64_t off, int col) const   -- v = x * rs in, the output chunk out
//        out_t: the type of y -- RowOutInPlace where y may be a matrix Post reads (Gemma's post-norms write the residual
//        stream they add), RowOutApart (__restrict__: the loads of the next chunk need not wait for the store) where not
#pragma once
#include "common.hpp"

namespace {

typedef bf16_t* RowOutInPlace;
typedef bf16_t* __restrict__ RowOutApart;

struct RowIdentity {
    __device__ __forceinline__ void operator()(float*, int64_t) const {}
    __device__ __forceinline__ const bf16_t* src(const bf16_t* x) const { return x; }
};

template <class Pre, class Post>
__global__ __launch_bounds__(256) void rownorm_lpr_kernel(int M, int D, int lpr, float eps, const bf16_t* __restrict__ x,
                                                          const bf16_t* __restrict__ w, typename Post::out_t y, Pre pre, Post post) {
    const int rows_per_block = 256 / lpr;
    const int r = blockIdx.x * rows_per_block + threadIdx.x / lpr;
    const int l = threadIdx.x & (lpr - 1);
    const int nch = D >> 3;
    const bool live = r < M;
    const int64_t ro = (int64_t)(live ? r : 0) * D;
    float ss = 0.f;
    if (live) {
        for (int c = l; c < nch; c += lpr) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + ro + c * 8), v);
            pre(v, ro + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
        }
    }
    for (int o = 1; o < lpr; o <<= 1) ss += __shfl_xor(ss, o, 64);
    if (!live) return;
    const float rs = 1.0f / sqrtf(ss / (float)D + eps);
    const bf16_t* src = pre.src(x);
    for (int c = l; c < nch; c += lpr) {
        float v[8], wv[8];
        unpack8(*reinterpret_cast<const u32x4*>(src + ro + c * 8), v);
        unpack8(*reinterpret_cast<const u32x4*>(w + c * 8), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= rs;
        post(v, wv, ro + c * 8, c * 8);
        *reinterpret_cast<u32x4*>(y + ro + c * 8) = pack8(v);
    }
}

template <class Pre, class Post>
int launch_rownorm_lpr(int M, int D, float eps, const void* x, const void* w, void* y, Pre pre, Post post, hipStream_t stream) {
    int lpr = 1;
    while (lpr < 64 && ((D >> 3) % (lpr * 2)) == 0) lpr *= 2;
    const int rows_per_block = 256 / lpr;
    hipLaunchKernelGGL((rownorm_lpr_kernel<Pre, Post>), dim3((unsigned)((M + rows_per_block - 1) / rows_per_block)), dim3(256), 0,
                       stream, M, D, lpr, eps, (const bf16_t*)x, (const bf16_t*)w, (typename Post::out_t)y, pre, post);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // namespace
