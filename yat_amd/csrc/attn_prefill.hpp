// What the forward-only prefill attention kernels share (csrc/vae_kl.hip, csrc/gemma.hip, csrc/t5.hip): the LDS fragment
// reads of the two K / V image layouts, the Q-fragment prologue, one step of the lazy-rescale online softmax and the
// normalise-and-store epilogue.  Each kernel keeps what is its own: staging, head and strip mapping, tile counts, the
// logit transform and the mask.  (csrc/sdpa.hip, the training path, is built with its own flags and has its own copies.)
//
// Every product is issued with swapped operands so the query sits on lane & 15 and the key / output column on the
// accumulator's (lane >> 4, register) slot: the probability accumulators are directly the B operand of P V, and the softmax
// state of a query (m, l) lives in the four lanes that share lane & 15.
#pragma once
#include "common.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LAZY_LOG2 = 8.0f;                   // rescale threshold in log2 units (P <= 2^8, exact in fp32 / bf16)

// ---- images with 256-byte rows: [32 keys][128 columns], K row-swizzled, V swizzled for the transposed read
__device__ __forceinline__ bf16x8 frag_row256(const char* lds, int row0, int ks, int lane) {
    const uint32_t r = row0 + (lane & 15);
    const uint32_t c = (ks * 4 + (lane >> 4)) ^ (r & 15);
    return lds_read8(lds, r * 256 + c * 16);
}
// operand in ACCUMULATOR k order from a TR image: idx = col0 + (lane & 15); k slot (g, j): row 4g + j (j < 4), 16 + 4g + j - 4
__device__ __forceinline__ bf16x8 frag_tr256(const char* lds, int col0, int lane) {
    const uint32_t g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const uint32_t col = col0 + 4 * p;
    const uint32_t r0 = 4 * g + q, r1 = r0 + 16;
    const uint32_t c0 = (col >> 3) ^ ((r0 & 7) << 1), c1 = (col >> 3) ^ ((r1 & 7) << 1);
    return cat4(lds_read_tr4(lds, r0 * 256 + c0 * 16 + (p & 1) * 8), lds_read_tr4(lds, r1 * 256 + c1 * 16 + (p & 1) * 8));
}

// ---- images with 128-byte rows: [64 keys][64 columns].  K image: 16-byte chunk c of key row r lives at chunk
// c ^ ((r >> 1) & 7) (swz128); V image: at chunk c ^ (((r >> 1) & 3) << 1) (an even XOR: the two chunks a 16-lane group of
// the transposed read covers stay adjacent)
__device__ __forceinline__ bf16x8 frag_row128(const char* lds, int row0, int ks, int lane) {
    const uint32_t r = row0 + (lane & 15);
    return lds_read8(lds, r * 128 + swz128(r, ks * 4 + (lane >> 4)) * 16);
}
__device__ __forceinline__ bf16x8 frag_tr128(const char* lds, int row0, int col0, int lane) {
    const uint32_t g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const uint32_t col = col0 + 4 * p;
    const uint32_t r0 = row0 + 4 * g + q, r1 = r0 + 16;
    const uint32_t c0 = (col >> 3) ^ (((r0 >> 1) & 3) << 1), c1 = (col >> 3) ^ (((r1 >> 1) & 3) << 1);
    return cat4(lds_read_tr4(lds, r0 * 128 + c0 * 16 + (p & 1) * 8), lds_read_tr4(lds, r1 * 128 + c1 * 16 + (p & 1) * 8));
}

__device__ __forceinline__ bf16x8 acc_to_frag(const f32x4& a, const f32x4& b) {
    bf16x8 r;
    r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
    r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    return r;
}
__device__ __forceinline__ float group_max(float v) {         // across the 4 lane groups that share lane & 15
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// The KS fragments of this lane's query: `q_row` is the query's row at its head's first column, a dead query reads as zeros.
template <int KS>
__device__ __forceinline__ void load_q_frags(bf16x8 (&qf)[KS], const bf16_t* q_row, bool live, int g) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.0f;
        if (live) z = *reinterpret_cast<const bf16x8*>(q_row + ks * 32 + 8 * g);
        qf[ks] = z;
    }
}

// One tile of 32 keys: the masked logits s -> the probabilities as the B operand of P V, with m, l and o brought up to date;
// the caller issues the P V products.  The logits are in units of 1 / ce log2: exp2 takes (s - m) * ce.  o is rescaled only
// when some query's maximum grew by more than LAZY_LOG2 (wave-uniform; after the first tiles: rare), so P may reach 2^8.
// With ce = 1.0f (logits already in log2 units) every expression below is exact and the constant folds away.
template <int DT>
__device__ __forceinline__ bf16x8 online_softmax_step(f32x4 (&s)[2], float& m, float& l, f32x4 (&o)[DT], float ce) {
    float t = -1e30f;
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) t = fmaxf(t, s[nj][r]);
    const float mx = group_max(t);
    if (__builtin_amdgcn_ballot_w64(mx > m + LAZY_LOG2 / ce) != 0) {
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * ce);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
    }
    const float nm2 = -m * ce;
    float rs = 0.f;
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = rbf(__builtin_amdgcn_exp2f(__builtin_fmaf(s[nj][r], ce, nm2)));
            s[nj][r] = e;
            rs += e;
        }
    l += group_sum(rs);
    return acc_to_frag(s[0], s[1]);
}

// o / l of this lane's query to its output row (`out_row` at its head's first column).
template <int DT>
__device__ __forceinline__ void store_o(bf16_t* out_row, const f32x4 (&o)[DT], float l, int g) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<u32x2*>(out_row + dt * 16 + 4 * g) = pack4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
}

}  // namespace
