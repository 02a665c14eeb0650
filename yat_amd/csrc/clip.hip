// CLIP text-encoder kernels (transformers CLIPTextModelWithProjection: CLIP-L and OpenCLIP bigG, `text_encoder` and
// `text_encoder_2` of the SD3.5 pipe; pipe.encode_prompt at train_sd35.py:79-92,113-118).  Forward only, bf16 activations, fp32
// arithmetic inside every kernel.  The text side runs PACKED as in csrc/gemma.hip and csrc/t5.hip: the B prompts are the row
// ranges [off[b], off[b+1]) of one [rows, .] matrix.  The model is causal, so a row depends on the earlier rows of its own
// prompt only.  The projections run on yat_gemm_bf16 with its bias epilogue (yat_amd/clip.py); what the encoder needs beyond it:
//
//   embed       out[r] = bf16(token_table[ids[r]] + pos_table[pos[r]])          CLIPTextEmbeddings: one add, one rounding
//   layernorm   y = bf16((x - mean) * rstd * w + b)                              nn.LayerNorm: ONE rounding, variance from (x - mean)^2
//               s = bf16(residual + x) stored, y = LN(s) with a residual         the block's h = h + sublayer(.) and the next norm
//   act         quick-GELU x * sigmoid(1.702 x) or exact (erf) GELU              after fc1 + bias: the module's two roundings
//   attention   causal, scaled, head dim 64 (below)
#include "attn_prefill.hpp"

namespace {

// --------------------------------------------------------------------------------------------------------------- embed
__global__ __launch_bounds__(256) void clip_embed_kernel(int64_t nchunk, int nch, int vocab, int npos, const int* __restrict__ ids,
                                                         const int* __restrict__ pos, const bf16_t* __restrict__ tok,
                                                         const bf16_t* __restrict__ ptab, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    const int64_t r = i / nch;
    const int c = (int)(i - r * nch);
    const int id = ids[r], p = pos[r];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (id >= 0 && id < vocab && p >= 0 && p < npos) {    // (the host rejects such a row; never gather through one)
        float t[8];
        unpack8(*reinterpret_cast<const u32x4*>(tok + ((int64_t)id * nch + c) * 8), v);
        unpack8(*reinterpret_cast<const u32x4*>(ptab + ((int64_t)p * nch + c) * 8), t);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += t[e];
    }
    *reinterpret_cast<u32x4*>(out + i * 8) = pack8(v);
}

// ----------------------------------------------------------------------------------------------------------- layernorm
// LPR lanes per row (a power of two dividing D / 8, at most 64), three passes over the row (the second and third re-read it
// from L1): the sum, the sum of (x - mean)^2, the output.  With a residual the first pass stores the rounded sum and the later
// passes read it back: every 16-byte chunk is written and re-read by the same lane, so `sum` may be `res` itself.
__global__ __launch_bounds__(256) void clip_layernorm_kernel(int M, int D, int lpr, float eps, const bf16_t* __restrict__ x,
                                                             const bf16_t* __restrict__ w, const bf16_t* __restrict__ bias,
                                                             const bf16_t* res, bf16_t* sum, bf16_t* __restrict__ y) {
    const int rows_per_block = 256 / lpr;
    const int r = blockIdx.x * rows_per_block + threadIdx.x / lpr;
    const int l = threadIdx.x & (lpr - 1);
    const int nch = D >> 3;
    const bool live = r < M;
    const int64_t ro = (int64_t)(live ? r : 0) * D;
    float s1 = 0.f;
    if (live) {
        for (int c = l; c < nch; c += lpr) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + ro + c * 8), v);
            if (res) {
                float rv[8];
                unpack8(*reinterpret_cast<const u32x4*>(res + ro + c * 8), rv);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = rbf(rv[e] + v[e]);
                *reinterpret_cast<u32x4*>(sum + ro + c * 8) = pack8(v);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s1 += v[e];
        }
    }
    for (int o = 1; o < lpr; o <<= 1) s1 += __shfl_xor(s1, o, 64);
    const float mean = s1 / (float)D;
    const bf16_t* src = res ? sum : x;
    float s2 = 0.f;
    if (live) {
        for (int c = l; c < nch; c += lpr) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4*>(src + ro + c * 8), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[e] - mean;
                s2 = __builtin_fmaf(d, d, s2);
            }
        }
    }
    for (int o = 1; o < lpr; o <<= 1) s2 += __shfl_xor(s2, o, 64);
    if (!live) return;
    const float rs = 1.0f / sqrtf(s2 / (float)D + eps);
    for (int c = l; c < nch; c += lpr) {
        float v[8], wv[8], bv[8];
        unpack8(*reinterpret_cast<const u32x4*>(src + ro + c * 8), v);
        unpack8(*reinterpret_cast<const u32x4*>(w + c * 8), wv);
        unpack8(*reinterpret_cast<const u32x4*>(bias + c * 8), bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf((v[e] - mean) * rs, wv[e], bv[e]);
        *reinterpret_cast<u32x4*>(y + ro + c * 8) = pack8(v);
    }
}

// ----------------------------------------------------------------------------------------------------------------- act
template <int KIND>
__global__ __launch_bounds__(256) void clip_act_kernel(int64_t nchunk, const bf16_t* x, bf16_t* y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    float v[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + i * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (KIND == 1) v[e] = v[e] * sigmoid_f(1.702f * v[e]);                    // QuickGELUActivation
        else v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752f));      // GELUActivation (erf)
    }
    *reinterpret_cast<u32x4*>(y + i * 8) = pack8(v);
}

// ----------------------------------------------------------------------------------------------------------- attention
// Flash-style prefill over packed prompts, head dim 64, with the staging of csrc/t5.hip: grid = (query tiles of 64, head,
// prompt); a workgroup is 4 waves, wave = one 16-query strip, holding its Q fragments (2) and its O accumulator (16 x 64 fp32 =
// 4 MFMA tiles) in registers.  K / V arrive by LDS-DMA in tiles of 64 keys, two stages (tile t + 1 lands while tile t is
// consumed, one barrier per tile): a stage is K then V, each a [64 keys][64 columns] image with 128-byte rows -- K swizzled for
// the row read of S = K Q^T, V for the transposed ds_read_b64_tr_b16 read.  8 KiB per matrix, 32 KiB for the two stages.  Every
// product is issued with swapped operands so the query sits on lane & 15 (csrc/gemma.hip).  The logit is q . k * scale, taken
// to log2 units in one multiply.  Causality as in csrc/gemma.hip: a query tile is as wide as a key tile, so it walks the key
// tiles up to its own and stages none above; a 32-key half wholly above a wave's strip is skipped and only a half the diagonal
// crosses is masked per element.  Keys past the prompt's end are above every live query: the same mask drops them, and their
// rows read as zeros through the buffer bound.  A query tile past the end exits before any barrier.
constexpr int CA_DH = 64, CA_KT = 64, CA_NW = 4, CA_QT = 16 * CA_NW;
constexpr int CA_MAT = CA_KT * CA_DH * 2, CA_STAGE = 2 * CA_MAT;       // K (or V) of one stage; K then V
constexpr int CA_MAX_LEN = 512;
constexpr int CA_LDS = 2 * CA_STAGE;
static_assert(CA_QT == CA_KT, "a query tile must lie inside one key tile");
struct ClipAttnP {
    int rows, ld, ldo, max_len;
    float scale;
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    const int* off;
    bf16_t* out;
};

__global__ __launch_bounds__(CA_NW * 64) void clip_attn_kernel(ClipAttnP p) {
    constexpr int KS = CA_DH / 32, DT = CA_DH / 16;
    constexpr int PIECES = (CA_MAT / 1024) / CA_NW;            // 1-KiB DMA pieces (8 key rows) per wave per matrix
    __shared__ __attribute__((aligned(16))) char smem[CA_LDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int b = blockIdx.z, head = blockIdx.y;
    const int prow0 = min(max(p.off[b], 0), p.rows), prow1 = min(max(p.off[b + 1], prow0), p.rows);
    const int len = min(prow1 - prow0, p.max_len);
    const int q0 = blockIdx.x * CA_QT;
    if (q0 >= len) return;                                     // (the whole workgroup, before any barrier)
    const int sq0 = q0 + wave * 16;                            // this wave's strip
    const bf16_t* kb = p.k + head * CA_DH;
    const bf16_t* vb = p.v + head * CA_DH;

    auto stage = [&](int k0, char* base) {
        const uint64_t bytes = (uint64_t)(len - k0) * p.ld * 2;          // rows past the prompt's end read as zeros
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb + (int64_t)(prow0 + k0) * p.ld, bytes);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb + (int64_t)(prow0 + k0) * p.ld, bytes);
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int pc = j * CA_NW + wave;
            const int row = pc * 8 + (lane >> 3), slot = lane & 7;
            const int ck = slot ^ ((row >> 1) & 7), cv = slot ^ (((row >> 1) & 3) << 1);
            lds_dma16(rk, (YAT_LDS void*)(base + pc * 1024), (uint32_t)((row * p.ld + ck * 8) * 2));
            lds_dma16(rv, (YAT_LDS void*)(base + CA_MAT + pc * 1024), (uint32_t)((row * p.ld + cv * 8) * 2));
        }
    };
    stage(0, smem);

    bf16x8 qf[KS];
    load_q_frags<KS>(qf, p.q + (int64_t)(prow0 + sq0 + li) * p.ld + head * CA_DH, sq0 + li < len, g);
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;                                 // running maximum in log2 units, row sum
    const bool wave_live = sq0 < len;                          // a strip wholly past the end only stages and meets the barriers
    const float c_lin = p.scale * LOG2E;

    const int ntiles = q0 / CA_KT + 1;                         // the last one holds the diagonal
    for (int it = 0; it < ntiles; ++it) {
        const int k0 = it * CA_KT;
        char* cur = smem + (it & 1) * CA_STAGE;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                       // tile `it` landed for every wave; the other stage is free
        if (it + 1 < ntiles) stage(k0 + CA_KT, smem + ((it + 1) & 1) * CA_STAGE);
        if (!wave_live) continue;
        const char* Ks = cur;
        const char* Vs = cur + CA_MAT;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int kh0 = k0 + h * 32;
            if (kh0 > sq0 + 15) break;                         // wave-uniform: this half lies above the whole strip
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
                for (int r = 0; r < 4; ++r) s[nj][r] *= c_lin;
            if (kh0 + 31 > sq0) {                              // uniform: the diagonal crosses this half
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kh0 + nj * 16 + 4 * g + r > sq0 + li) s[nj][r] = -1e30f;
            }
            const bf16x8 pf = online_softmax_step<DT>(s, m, l, o, 1.0f);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(frag_tr128(Vs, h * 32, dt * 16, lane), pf, o[dt]);
        }
    }
    const int qi = sq0 + li;
    if (qi < len) store_o<DT>(p.out + (int64_t)(prow0 + qi) * p.ldo + head * CA_DH, o, l, g);
}

}  // namespace

extern "C" {

int yat_clip_embed(int rows, int D, int vocab, int npos, const void* ids, const void* positions, const void* token_table,
                   const void* pos_table, void* out, yat_stream_t stream) {
    if (rows <= 0 || D <= 0 || (D & 7) || vocab <= 0 || npos <= 0 || !ids || !positions || !token_table || !pos_table || !out)
        return YAT_EINVAL;
    if (((uintptr_t)token_table | (uintptr_t)pos_table | (uintptr_t)out) & 15 || (((uintptr_t)ids | (uintptr_t)positions) & 3))
        return YAT_EINVAL;
    const int64_t nchunk = (int64_t)rows * (D / 8);
    if ((nchunk + 255) / 256 > 0x7fffffffll) return YAT_EINVAL;
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nchunk, D / 8,
                       vocab, npos, (const int*)ids, (const int*)positions, (const bf16_t*)token_table, (const bf16_t*)pos_table,
                       (bf16_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_clip_layernorm(int M, int D, float eps, const void* x, const void* w, const void* b, const void* residual, void* sum_out,
                       void* y, yat_stream_t stream) {
    if (M <= 0 || D <= 0 || (D & 7) || !(eps >= 0.f) || !x || !w || !b || !y || (residual && !sum_out)) return YAT_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b | (uintptr_t)y | (uintptr_t)residual | (uintptr_t)sum_out) & 15) return YAT_EINVAL;
    int lpr = 1;
    while (lpr < 64 && ((D >> 3) % (lpr * 2)) == 0) lpr *= 2;
    const int rows_per_block = 256 / lpr;
    hipLaunchKernelGGL(clip_layernorm_kernel, dim3((unsigned)((M + rows_per_block - 1) / rows_per_block)), dim3(256), 0,
                       (hipStream_t)stream, M, D, lpr, eps, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b,
                       (const bf16_t*)residual, (bf16_t*)(residual ? sum_out : nullptr), (bf16_t*)y);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_clip_act(int64_t n, int kind, const void* x, void* y, yat_stream_t stream) {
    if (n <= 0 || (n & 7) || (kind != 1 && kind != 2) || !x || !y) return YAT_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y) & 15) return YAT_EINVAL;
    const int64_t nchunk = n / 8;
    if ((nchunk + 255) / 256 > 0x7fffffffll) return YAT_EINVAL;
    const dim3 grid((unsigned)((nchunk + 255) / 256));
    if (kind == 1)
        hipLaunchKernelGGL(clip_act_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, nchunk, (const bf16_t*)x, (bf16_t*)y);
    else
        hipLaunchKernelGGL(clip_act_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, nchunk, (const bf16_t*)x, (bf16_t*)y);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_clip_attn_fwd(int B, int rows, int H, int dh, int max_len, const void* qkv, int ld, int q_off, int k_off, int v_off,
                      float scale, const void* row_offsets, void* out, int ldo, yat_stream_t stream) {
    if (dh != CA_DH || H < 1 || H > 65535 || max_len <= 0 || max_len > CA_MAX_LEN) return YAT_EINVAL;
    if (B <= 0 || B > 65535 || rows <= 0 || !qkv || !row_offsets || !out || !(scale > 0.f) || !(scale < 1e30f)) return YAT_EINVAL;
    if ((ld & 7) || (ldo & 7) || ((q_off | k_off | v_off) & 7) || q_off < 0 || k_off < 0 || v_off < 0 || ld <= 0 || ldo <= 0)
        return YAT_EINVAL;
    const int64_t width = (int64_t)H * dh;
    if (q_off + width > ld || k_off + width > ld || v_off + width > ld || width > ldo) return YAT_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)out) & 15 || ((uintptr_t)row_offsets & 3)) return YAT_EINVAL;
    if ((int64_t)CA_MAX_LEN * ld * 2 > 0x7fffffffll) return YAT_EINVAL;              // a prompt's K / V block: one buffer resource
    ClipAttnP p{};
    p.rows = rows; p.ld = ld; p.ldo = ldo; p.max_len = max_len; p.scale = scale;
    p.q = (const bf16_t*)qkv + q_off; p.k = (const bf16_t*)qkv + k_off; p.v = (const bf16_t*)qkv + v_off;
    p.off = (const int*)row_offsets; p.out = (bf16_t*)out;
    hipLaunchKernelGGL(clip_attn_kernel, dim3((unsigned)((max_len + CA_QT - 1) / CA_QT), (unsigned)H, (unsigned)B), dim3(CA_NW * 64),
                       0, (hipStream_t)stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
