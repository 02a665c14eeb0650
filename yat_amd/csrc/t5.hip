// T5 v1.1 encoder kernels (transformers T5EncoderModel, the text encoder of PixArt-Sigma: pipe.encode_prompt at
// train_pixart_sigma.py:68-74,97-108).  Forward only, bf16 activations, fp32 arithmetic inside every kernel.  The text side
// runs PACKED as in csrc/gemma.hip: the B prompts are the row ranges [off[b], off[b+1]) of one [rows, .] matrix and no pad row
// exists (the reference pads on the right and masks the pad keys; the position bias depends on the distance only).  The
// projections run on yat_gemm_bf16, the gather on yat_embed_rows (scale 1) and the gated GELU on yat_geglu (yat_amd/t5.py);
// what the encoder needs beyond them:
//
//   rmsnorm     y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps)))            T5LayerNorm: TWO roundings, no mean, no bias, no 1 + w
//               s = bf16(residual + x) stored, y = norm(s) with a residual   the block's h = h + sublayer(.) and the next norm
//   attention   bidirectional, unscaled, with the learned relative-position bias looked up by key - query distance (below)
#include "attn_prefill.hpp"
#include "rownorm_lpr.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------- rmsnorm
// The row walk is csrc/rownorm_lpr.hpp's.  With a residual the first pass stores the rounded sum and the second pass reads it
// back: every 16-byte chunk is written and re-read by the same lane, so `sum` may be `res` itself.
struct T5NormPre {
    const bf16_t* res;
    bf16_t* sum;
    __device__ __forceinline__ void operator()(float* v, int64_t off) const {
        if (!res) return;
        float rv[8];
        unpack8(*reinterpret_cast<const u32x4*>(res + off), rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = rbf(rv[e] + v[e]);
        *reinterpret_cast<u32x4*>(sum + off) = pack8(v);
    }
    __device__ __forceinline__ const bf16_t* src(const bf16_t* x) const { return res ? sum : x; }
};
struct T5NormPost {                                        // T5LayerNorm: TWO roundings
    typedef RowOutApart out_t;
    __device__ __forceinline__ void operator()(float* v, const float* w, int64_t, int) const {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = w[e] * rbf(v[e]);
    }
};

// ----------------------------------------------------------------------------------------------------------- attention
// Flash-style prefill over packed prompts, head dim 64.  Grid = (query tiles of 64, head, prompt); a workgroup is 4 waves, wave
// = one 16-query strip, holding its Q fragments (2) and its O accumulator (16 x 64 fp32 = 4 MFMA tiles) in registers.  K / V
// arrive by LDS-DMA in tiles of 64 keys, two stages (tile t + 1 lands while tile t is consumed, one barrier per tile): a stage
// is K then V, each a [64 keys][64 columns] image with 128-byte rows -- K swizzled for the row read of S = K Q^T, V for the
// transposed ds_read_b64_tr_b16 read.  8 KiB per matrix, 32 KiB for the two stages; the head's slice of the bias table sits
// beside them once per workgroup as fp32 in log2 units (4 KiB): 36 KiB, four workgroups per CU.  Every product is issued with
// swapped operands so the query sits on lane & 15 (csrc/gemma.hip): the probability accumulators are directly the B operand
// of P V and the online softmax stays in registers.  The kernel does no bucket arithmetic: the logit of (query i, key j) gets
// table[(j - i) + max_len - 1].  Keys past the prompt's end are masked in the last tile only (a 32-key half wholly past it is
// skipped); a query tile past the end exits before any barrier.
constexpr int TA_DH = 64, TA_KT = 64, TA_NW = 4, TA_QT = 16 * TA_NW;
constexpr int TA_MAT = TA_KT * TA_DH * 2, TA_STAGE = 2 * TA_MAT;       // K (or V) of one stage; K then V
constexpr int TA_MAX_LEN = 512;
constexpr int TA_BIAS = 2 * TA_MAX_LEN * 4;                             // 2 * max_len - 1 fp32 entries
constexpr int TA_LDS = 2 * TA_STAGE + TA_BIAS;
struct T5AttnP {
    int rows, ld, ldo, max_len;
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    const bf16_t* bias;
    const int* off;
    bf16_t* out;
};

__global__ __launch_bounds__(TA_NW * 64) void t5_attn_kernel(T5AttnP p) {
    constexpr int KS = TA_DH / 32, DT = TA_DH / 16;
    constexpr int PIECES = (TA_MAT / 1024) / TA_NW;            // 1-KiB DMA pieces (8 key rows) per wave per matrix
    __shared__ __attribute__((aligned(16))) char smem[TA_LDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int b = blockIdx.z, head = blockIdx.y;
    const int prow0 = min(max(p.off[b], 0), p.rows), prow1 = min(max(p.off[b + 1], prow0), p.rows);
    const int len = min(prow1 - prow0, p.max_len);
    const int q0 = blockIdx.x * TA_QT;
    if (q0 >= len) return;                                     // (the whole workgroup, before any barrier)
    const int sq0 = q0 + wave * 16;                            // this wave's strip
    const bf16_t* kb = p.k + head * TA_DH;
    const bf16_t* vb = p.v + head * TA_DH;

    auto stage = [&](int k0, char* base) {
        const uint64_t bytes = (uint64_t)(len - k0) * p.ld * 2;          // rows past the prompt's end read as zeros
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb + (int64_t)(prow0 + k0) * p.ld, bytes);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb + (int64_t)(prow0 + k0) * p.ld, bytes);
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int pc = j * TA_NW + wave;
            const int row = pc * 8 + (lane >> 3), slot = lane & 7;
            const int ck = slot ^ ((row >> 1) & 7), cv = slot ^ (((row >> 1) & 3) << 1);
            lds_dma16(rk, (YAT_LDS void*)(base + pc * 1024), (uint32_t)((row * p.ld + ck * 8) * 2));
            lds_dma16(rv, (YAT_LDS void*)(base + TA_MAT + pc * 1024), (uint32_t)((row * p.ld + cv * 8) * 2));
        }
    };
    stage(0, smem);

    const int nbias = 2 * p.max_len - 1;
    float* bl = reinterpret_cast<float*>(smem + 2 * TA_STAGE);
    {
        const bf16_t* bh = p.bias + (int64_t)head * nbias;
        for (int i = threadIdx.x; i < nbias; i += TA_NW * 64) bl[i] = bf2f(bh[i]) * LOG2E;
    }

    bf16x8 qf[KS];
    load_q_frags<KS>(qf, p.q + (int64_t)(prow0 + sq0 + li) * p.ld + head * TA_DH, sq0 + li < len, g);
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;                                 // running maximum in log2 units, row sum
    const bool wave_live = sq0 < len;                          // a strip wholly past the end only stages and meets the barriers
    const int dbase = p.max_len - 1 - (sq0 + li);              // table index of key j for this lane's query: j + dbase

    const int ntiles = (len + TA_KT - 1) / TA_KT;
    for (int it = 0; it < ntiles; ++it) {
        const int k0 = it * TA_KT;
        char* cur = smem + (it & 1) * TA_STAGE;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                       // tile `it` (and the bias) landed for every wave; the other stage is free
        if (it + 1 < ntiles) stage(k0 + TA_KT, smem + ((it + 1) & 1) * TA_STAGE);
        if (!wave_live) continue;
        const char* Ks = cur;
        const char* Vs = cur + TA_MAT;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int kh0 = k0 + h * 32;
            if (kh0 >= len) break;                             // uniform: this half lies wholly past the prompt's end
            f32x4 s[2];
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                s[nj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s[nj] = mfma16(frag_row128(Ks, h * 32 + nj * 16, ks, lane), qf[ks], s[nj]);
            }
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kj = kh0 + nj * 16 + 4 * g + r;
                    const int bi = min(max(kj + dbase, 0), nbias - 1);     // (a dead query's index may leave the table)
                    s[nj][r] = __builtin_fmaf(s[nj][r], LOG2E, bl[bi]);
                }
            if (kh0 + 32 > len) {                              // uniform: the prompt ends inside this half
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kh0 + nj * 16 + 4 * g + r >= len) s[nj][r] = -1e30f;
            }
            const bf16x8 pf = online_softmax_step<DT>(s, m, l, o, 1.0f);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(frag_tr128(Vs, h * 32, dt * 16, lane), pf, o[dt]);
        }
    }
    const int qi = sq0 + li;
    if (qi < len) store_o<DT>(p.out + (int64_t)(prow0 + qi) * p.ldo + head * TA_DH, o, l, g);
}

}  // namespace

extern "C" {

int yat_t5_rmsnorm(int M, int D, float eps, const void* x, const void* w, const void* residual, void* sum_out, void* y,
                   yat_stream_t stream) {
    if (M <= 0 || D <= 0 || (D & 7) || !(eps >= 0.f) || !x || !w || !y || (residual && !sum_out)) return YAT_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)residual | (uintptr_t)sum_out) & 15) return YAT_EINVAL;
    return launch_rownorm_lpr(M, D, eps, x, w, y, T5NormPre{(const bf16_t*)residual, (bf16_t*)sum_out}, T5NormPost{},
                              (hipStream_t)stream);
}

int yat_t5_attn_fwd(int B, int rows, int H, int dh, int max_len, const void* qkv, int ld, int q_off, int k_off, int v_off,
                    const void* bias_rel, const void* row_offsets, void* out, int ldo, yat_stream_t stream) {
    if (dh != TA_DH || H < 1 || H > 65535 || max_len <= 0 || max_len > TA_MAX_LEN) return YAT_EINVAL;
    if (B <= 0 || B > 65535 || rows <= 0 || !qkv || !bias_rel || !row_offsets || !out) return YAT_EINVAL;
    if ((ld & 7) || (ldo & 7) || ((q_off | k_off | v_off) & 7) || q_off < 0 || k_off < 0 || v_off < 0 || ld <= 0 || ldo <= 0)
        return YAT_EINVAL;
    const int64_t width = (int64_t)H * dh;
    if (q_off + width > ld || k_off + width > ld || v_off + width > ld || width > ldo) return YAT_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)out) & 15 || ((uintptr_t)row_offsets & 3) || ((uintptr_t)bias_rel & 1)) return YAT_EINVAL;
    if ((int64_t)TA_MAX_LEN * ld * 2 > 0x7fffffffll) return YAT_EINVAL;              // a prompt's K / V block: one buffer resource
    T5AttnP p{};
    p.rows = rows; p.ld = ld; p.ldo = ldo; p.max_len = max_len;
    p.q = (const bf16_t*)qkv + q_off; p.k = (const bf16_t*)qkv + k_off; p.v = (const bf16_t*)qkv + v_off;
    p.bias = (const bf16_t*)bias_rel; p.off = (const int*)row_offsets; p.out = (bf16_t*)out;
    hipLaunchKernelGGL(t5_attn_kernel, dim3((unsigned)((max_len + TA_QT - 1) / TA_QT), (unsigned)H, (unsigned)B), dim3(TA_NW * 64),
                       0, (hipStream_t)stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
