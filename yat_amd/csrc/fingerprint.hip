// Position-sensitive 64-bit fingerprint of a device buffer (include/yat_hip.h yat_fingerprint_u64): the sum mod 2^64 of one
// splitmix64 term per 32-bit word, keyed by the word's global index.  A streaming read: 16-B loads per lane, four in flight,
// grid-stride over <= 2048 workgroups; partial sums per lane, per wave (shuffles), per workgroup (LDS), then ONE 64-bit
// vector atomic add per workgroup.  Integer addition is associative, so the value does not depend on the grid, on the
// arrival order of the atomics or on how the buffer is cut into calls.
#include "common.hpp"
#include "../../include/yat_hip.h"

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_MAX_BLOCKS = 2048;
constexpr int FP_UNROLL = 4;

__device__ __forceinline__ uint64_t fp_term(uint64_t g, uint32_t w) {
    uint64_t z = ((g << 32) ^ (g >> 32) ^ (uint64_t)w) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t fp_term4(uint64_t g, const u32x4& v) {
    return fp_term(g, v[0]) + fp_term(g + 1, v[1]) + fp_term(g + 2, v[2]) + fp_term(g + 3, v[3]);
}

// buf: the first word; head: words before the first 16-byte boundary (0..3, <= n_words); the body is nvec 16-byte vectors from
// there and the rest (< 4 words) is the tail.  Head and tail words are taken one per lane by workgroup 0.
__global__ void __launch_bounds__(FP_THREADS)
fingerprint_kernel(int64_t n_words, const uint32_t* __restrict__ buf, uint64_t word_offset, int head, unsigned long long* out) {
    const int64_t nvec = (n_words - head) >> 2;
    const u32x4* body = reinterpret_cast<const u32x4*>(buf + head);
    const uint64_t g0 = word_offset + (uint64_t)head;
    const int64_t stride = (int64_t)gridDim.x * FP_THREADS;
    int64_t i = (int64_t)blockIdx.x * FP_THREADS + threadIdx.x;
    uint64_t sum = 0;
    for (; i + (FP_UNROLL - 1) * stride < nvec; i += FP_UNROLL * stride) {
        u32x4 v[FP_UNROLL];
#pragma unroll
        for (int u = 0; u < FP_UNROLL; ++u) v[u] = body[i + u * stride];
#pragma unroll
        for (int u = 0; u < FP_UNROLL; ++u) sum += fp_term4(g0 + 4 * (uint64_t)(i + u * stride), v[u]);
    }
    for (; i < nvec; i += stride) sum += fp_term4(g0 + 4 * (uint64_t)i, body[i]);
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + (nvec << 2);                 // first word behind the body
        const int t = threadIdx.x;
        if (t < head) sum += fp_term(word_offset + (uint64_t)t, buf[t]);
        else if (t - head < n_words - tail0) sum += fp_term(word_offset + (uint64_t)(tail0 + t - head), buf[tail0 + t - head]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, o, 64);
    __shared__ unsigned long long red[FP_THREADS / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < FP_THREADS / 64; ++w) s += red[w];
        atomicAdd(out, s);
    }
}

}  // namespace

extern "C" int yat_fingerprint_u64(int64_t n_words, const void* buf, uint64_t word_offset, uint64_t* out, int accumulate,
                                   yat_stream_t stream) {
    if (n_words <= 0 || !buf || !out || ((uintptr_t)buf & 3) || ((uintptr_t)out & 7)) return YAT_EINVAL;
    if (!accumulate) {
        const hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    int64_t head = (int64_t)((16 - ((uintptr_t)buf & 15)) & 15) >> 2;
    if (head > n_words) head = n_words;
    const int64_t nvec = (n_words - head) >> 2;
    int64_t blocks = (nvec + FP_THREADS - 1) / FP_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > FP_MAX_BLOCKS ? FP_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(fingerprint_kernel, dim3((unsigned)blocks), dim3(FP_THREADS), 0, (hipStream_t)stream, n_words,
                       (const uint32_t*)buf, word_offset, (int)head, (unsigned long long*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}
