// Gemma-2 text-encoder kernels (transformers Gemma2Model, the text encoder of SANA: train_sana.py:84-94,113-129 and
// common/trainer.py:307-308 through SanaPipeline.encode_prompt).  Forward only, bf16 activations, fp32 arithmetic inside every
// kernel.  The text side runs PACKED: the B prompts are the row ranges [off[b], off[b+1]) of one [rows, .] matrix and no pad
// row exists (the reference pads on the right and the model is causal: a real token never sees a pad).  The projections run
// on yat_gemm_bf16 (yat_amd/gemma2.py); what the encoder needs beyond it:
//
//   embed_rows  out[r, :] = bf16(table[ids[r], :] * scale)            embed_tokens times bf16(sqrt(hidden))
//   rmsnorm     y = bf16(x * rsqrt(mean(x^2) + eps) * (1 + w))         Gemma2RMSNorm: ONE rounding (yat_rmsnorm_fwd rounds before
//               y = bf16(residual + y) with a residual                 the weight); the block's post-norm + add in one pass
//   rope_qk     x' = bf16(bf16(x cos) + bf16(rotate_half(x) sin))      apply_rotary_pos_emb on the q and k column blocks, in place
//   geglu       out = bf16(bf16(gelu_tanh(gate)) * up)                 Gemma2MLP's act_fn(gate_proj(x)) * up_proj(x)
//   attention   causal, grouped-query, soft-capped softmax attention at head dim 256 (below)
#include "attn_prefill.hpp"
#include "rownorm_lpr.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------- embed_rows
__global__ __launch_bounds__(256) void embed_rows_kernel(int64_t nchunk, int nch, int vocab, const int* __restrict__ ids,
                                                         const bf16_t* __restrict__ table, float scale, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    const int64_t r = i / nch;
    const int c = (int)(i - r * nch);
    const int id = ids[r];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (id >= 0 && id < vocab) {                          // (the host rejects such an id; never gather through one)
        unpack8(*reinterpret_cast<const u32x4*>(table + ((int64_t)id * nch + c) * 8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= scale;
    }
    *reinterpret_cast<u32x4*>(out + i * 8) = pack8(v);
}

// ------------------------------------------------------------------------------------------------------------- rmsnorm
// The row walk is csrc/rownorm_lpr.hpp's; Gemma2RMSNorm finishes an element with ONE rounding and 1 + w, then the residual add.
struct GemmaNormPost {
    typedef RowOutInPlace out_t;                           // y may be res
    const bf16_t* res;
    __device__ __forceinline__ void operator()(float* v, const float* w, int64_t off, int) const {
        float rv[8];
        if (res) unpack8(*reinterpret_cast<const u32x4*>(res + off), rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = v[e] * (1.0f + w[e]);
            if (res) t = rv[e] + rbf(t);
            v[e] = t;
        }
    }
};

// ------------------------------------------------------------------------------------------------------------- rope_qk
// thread = (row, head, 8-column chunk c of the lower half): rotates columns [8c, 8c + 8) and [dh/2 + 8c, dh/2 + 8c + 8).
__global__ __launch_bounds__(256) void rope_qk_kernel(int64_t nthread, int heads, int dh, int max_len, bf16_t* qkv, int ld,
                                                      const int* __restrict__ pos, const bf16_t* __restrict__ cs,
                                                      const bf16_t* __restrict__ sn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nthread) return;
    const int nc = dh >> 4, half = dh >> 1;
    const int c = (int)(i % nc);
    const int h = (int)((i / nc) % heads);
    const int64_t r = i / ((int64_t)nc * heads);
    const int p = pos[r];
    if (p < 0 || p >= max_len) return;
    bf16_t* x = qkv + r * ld + h * dh + c * 8;
    const bf16_t* cp = cs + (int64_t)p * dh + c * 8;
    const bf16_t* sp = sn + (int64_t)p * dh + c * 8;
    float a[8], b[8], c1[8], c2[8], s1[8], s2[8];
    unpack8(*reinterpret_cast<const u32x4*>(x), a);
    unpack8(*reinterpret_cast<const u32x4*>(x + half), b);
    unpack8(*reinterpret_cast<const u32x4*>(cp), c1);
    unpack8(*reinterpret_cast<const u32x4*>(cp + half), c2);
    unpack8(*reinterpret_cast<const u32x4*>(sp), s1);
    unpack8(*reinterpret_cast<const u32x4*>(sp + half), s2);
    float lo[8], hi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {                         // rotate_half(x) = cat(-x2, x1)
        lo[e] = rbf(a[e] * c1[e]) + rbf(-b[e] * s1[e]);
        hi[e] = rbf(b[e] * c2[e]) + rbf(a[e] * s2[e]);
    }
    *reinterpret_cast<u32x4*>(x) = pack8(lo);
    *reinterpret_cast<u32x4*>(x + half) = pack8(hi);
}

// --------------------------------------------------------------------------------------------------------------- geglu
__global__ __launch_bounds__(256) void geglu_kernel(int64_t nchunk, int nch, const bf16_t* __restrict__ gate,
                                                    const bf16_t* __restrict__ up, int ld, bf16_t* __restrict__ out, int ldo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    const int64_t r = i / nch;
    const int c = (int)(i - r * nch) * 8;
    float g[8], u[8];
    unpack8(*reinterpret_cast<const u32x4*>(gate + r * ld + c), g);
    unpack8(*reinterpret_cast<const u32x4*>(up + r * ld + c), u);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = rbf(gelu_tanh_f(g[e])) * u[e];
    *reinterpret_cast<u32x4*>(out + r * ldo + c) = pack8(g);
}

// ----------------------------------------------------------------------------------------------------------- attention
// Flash-style prefill over packed prompts, head dim 256.  Grid = (query tiles, kv head x head groups, prompt).  A workgroup
// serves HPW query heads of ONE kv head for its tile of 16 * (NW / HPW) queries: wave = (head, 16-query strip), so a staged
// K / V tile is read from memory once for all of them.  Each wave holds its strip's Q fragments (8) and its O accumulator
// (16 x 256 fp32 = 16 MFMA tiles, 64 VGPRs) in registers.  K / V arrive by LDS-DMA in tiles of 64 keys, two stages (tile t + 1
// lands while tile t is consumed, one barrier per tile): a stage holds K then V, each as 2 halves (32 keys) x 2 column
// blocks of the [32 keys][128 columns] images of csrc/vae_kl.hip -- K row-swizzled (read as rows for S = K Q^T), V swizzled
// for the transposed ds_read_b64_tr_b16 read.  64 KiB per stage, 128 KiB in all: one workgroup per CU.  Every product is
// issued with swapped operands so the query sits on lane & 15: the probability accumulators are directly the B operand of
// P V, and the online softmax stays in registers.  Causality: a query tile lies inside one key tile (its size divides 64), so
// the key tiles above the diagonal are never staged, only the last (diagonal) tile is masked, and a 32-key half that lies
// wholly above a wave's strip is skipped.  Keys past the prompt's end are above every live query: the same mask drops them.
constexpr int GA_DH = 256, GA_KT = 64, GA_SUB = 32 * 256;       // one [32][128] bf16 image = 8 KiB
constexpr int GA_MAT = 4 * GA_SUB, GA_STAGE = 2 * GA_MAT;       // K (or V) of one stage; K then V
constexpr int GA_LDS = 2 * GA_STAGE;
constexpr int GA_MAX_LEN = 1024;
struct GemmaAttnP {
    int rows, Hq, G, ld, ldo, max_len;
    float scale, cap;
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    const int* off;
    bf16_t* out;
};

template <int NW, int HPW>
__global__ __launch_bounds__(NW * 64) void gemma_attn_kernel(GemmaAttnP p) {
    constexpr int STRIPS = NW / HPW, QT = 16 * STRIPS, KS = GA_DH / 32, DT = GA_DH / 16;
    constexpr int PIECES = 32 / NW;                            // 1-KiB DMA pieces per wave per matrix
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int b = blockIdx.z;
    const int prow0 = min(max(p.off[b], 0), p.rows), prow1 = min(max(p.off[b + 1], prow0), p.rows);
    const int len = min(prow1 - prow0, p.max_len);             // (as csrc/t5.hip, csrc/clip.hip: rows past max_len stay as they are)
    const int q0 = blockIdx.x * QT;
    if (q0 >= len) return;                                     // (the whole workgroup, before any barrier)
    const int groups = p.G / HPW;
    const int kvh = blockIdx.y / groups;
    const int head = kvh * p.G + (blockIdx.y % groups) * HPW + wave / STRIPS;
    const int sq0 = q0 + (wave % STRIPS) * 16;                 // this wave's strip
    const bf16_t* kb = p.k + kvh * GA_DH;
    const bf16_t* vb = p.v + kvh * GA_DH;

    auto stage = [&](int k0, char* base) {
        const uint64_t bytes = (uint64_t)(len - k0) * p.ld * 2;          // rows past the prompt's end read as zeros
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb + (int64_t)(prow0 + k0) * p.ld, bytes);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb + (int64_t)(prow0 + k0) * p.ld, bytes);
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int pc = j * NW + wave, img = pc >> 3, db = img & 1;
            const int r = (pc & 7) * 4 + (lane >> 4), slot = lane & 15;
            const int row = (img >> 1) * 32 + r;
            const int ck = db * 16 + (slot ^ (r & 15)), cv = db * 16 + (slot ^ ((r & 7) << 1));
            lds_dma16(rk, (YAT_LDS void*)(base + pc * 1024), (uint32_t)((row * p.ld + ck * 8) * 2));
            lds_dma16(rv, (YAT_LDS void*)(base + GA_MAT + pc * 1024), (uint32_t)((row * p.ld + cv * 8) * 2));
        }
    };
    stage(0, smem);

    bf16x8 qf[KS];
    load_q_frags<KS>(qf, p.q + (int64_t)(prow0 + sq0 + li) * p.ld + head * GA_DH, sq0 + li < len, g);
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;                                 // running maximum in log2 units, row sum
    const bool capped = p.cap > 0.f;
    // logit in log2 units: t = s * c_lin (no cap), or c_cap * tanh(s * scale / cap) with tanh(y) = 1 - 2 / (1 + e^(2y))
    const float c_lin = p.scale * LOG2E;
    const float c_exp = capped ? 2.0f * LOG2E * p.scale / p.cap : 0.f;
    const float c_cap = p.cap * LOG2E;

    const int ntiles = q0 / GA_KT + 1;                         // the last one holds the diagonal
    for (int it = 0; it < ntiles; ++it) {
        const int k0 = it * GA_KT;
        char* cur = smem + (it & 1) * GA_STAGE;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                       // tile `it` landed for every wave; the other stage is free
        if (it + 1 < ntiles) stage(k0 + GA_KT, smem + ((it + 1) & 1) * GA_STAGE);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int kh0 = k0 + h * 32;
            if (kh0 > sq0 + 15) break;                         // wave-uniform: this half lies above the whole strip
            const char* Ks = cur + h * 2 * GA_SUB;
            const char* Vs = cur + GA_MAT + h * 2 * GA_SUB;
            f32x4 s[2];
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                s[nj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    s[nj] = mfma16(frag_row256(Ks + (ks / 4) * GA_SUB, nj * 16, ks % 4, lane), qf[ks], s[nj]);
            }
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = s[nj][r];
                    s[nj][r] = capped ? c_cap * (1.0f - 2.0f * fast_rcp(1.0f + __builtin_amdgcn_exp2f(x * c_exp))) : x * c_lin;
                }
            if (kh0 + 31 > sq0) {                              // uniform: the diagonal crosses this half
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kh0 + nj * 16 + 4 * g + r > sq0 + li) s[nj][r] = -1e30f;
            }
            const bf16x8 pf = online_softmax_step<DT>(s, m, l, o, 1.0f);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(frag_tr256(Vs + (dt / 8) * GA_SUB, (dt % 8) * 16, lane), pf, o[dt]);
        }
    }
    const int qi = sq0 + li;
    if (qi < len) store_o<DT>(p.out + (int64_t)(prow0 + qi) * p.ldo + head * GA_DH, o, l, g);
}

template <int NW, int HPW>
int launch_gemma_attn(const GemmaAttnP& p, int B, int Hkv, int max_len, hipStream_t stream) {
    constexpr int QT = 16 * (NW / HPW);
    static bool attr_set = false;
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute((const void*)gemma_attn_kernel<NW, HPW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, GA_LDS);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    hipLaunchKernelGGL((gemma_attn_kernel<NW, HPW>), dim3((unsigned)((max_len + QT - 1) / QT), (unsigned)(Hkv * (p.G / HPW)),
                       (unsigned)B), dim3(NW * 64), GA_LDS, stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // namespace

extern "C" {

int yat_embed_rows(int rows, int D, int vocab, const void* ids, const void* table, float scale, void* out, yat_stream_t stream) {
    if (rows <= 0 || D <= 0 || (D & 7) || vocab <= 0 || !ids || !table || !out) return YAT_EINVAL;
    if (((uintptr_t)table | (uintptr_t)out) & 15 || ((uintptr_t)ids & 3)) return YAT_EINVAL;
    const int64_t nchunk = (int64_t)rows * (D / 8);
    if ((nchunk + 255) / 256 > 0x7fffffffll) return YAT_EINVAL;
    hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nchunk, D / 8,
                       vocab, (const int*)ids, (const bf16_t*)table, scale, (bf16_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_gemma_rmsnorm(int M, int D, float eps, const void* x, const void* w, const void* residual, void* y, yat_stream_t stream) {
    if (M <= 0 || D <= 0 || (D & 7) || !(eps >= 0.f) || !x || !w || !y) return YAT_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)residual) & 15) return YAT_EINVAL;
    return launch_rownorm_lpr(M, D, eps, x, w, y, RowIdentity{}, GemmaNormPost{(const bf16_t*)residual}, (hipStream_t)stream);
}

int yat_rope_qk(int rows, int heads, int dh, int max_len, void* qkv, int ld, const void* positions, const void* cos_table,
                const void* sin_table, yat_stream_t stream) {
    if (rows <= 0 || heads <= 0 || dh <= 0 || (dh & 15) || max_len <= 0 || !qkv || !positions || !cos_table || !sin_table)
        return YAT_EINVAL;
    if ((ld & 7) || (int64_t)heads * dh > ld) return YAT_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)cos_table | (uintptr_t)sin_table) & 15 || ((uintptr_t)positions & 3)) return YAT_EINVAL;
    const int64_t nthread = (int64_t)rows * heads * (dh / 16);
    if ((nthread + 255) / 256 > 0x7fffffffll) return YAT_EINVAL;
    hipLaunchKernelGGL(rope_qk_kernel, dim3((unsigned)((nthread + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nthread, heads,
                       dh, max_len, (bf16_t*)qkv, ld, (const int*)positions, (const bf16_t*)cos_table, (const bf16_t*)sin_table);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_geglu(int M, int N, const void* gate, const void* up, int ld, void* out, int ldo, yat_stream_t stream) {
    if (M <= 0 || N <= 0 || (N & 7) || (ld & 7) || (ldo & 7) || ld < N || ldo < N || !gate || !up || !out) return YAT_EINVAL;
    if (((uintptr_t)gate | (uintptr_t)up | (uintptr_t)out) & 15) return YAT_EINVAL;
    const int64_t nchunk = (int64_t)M * (N / 8);
    if ((nchunk + 255) / 256 > 0x7fffffffll) return YAT_EINVAL;
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nchunk, N / 8,
                       (const bf16_t*)gate, (const bf16_t*)up, ld, (bf16_t*)out, ldo);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_gemma_attn_fwd(int B, int rows, int Hq, int Hkv, int dh, int max_len, float scale, float softcap, const void* qkv,
                       int ld, int q_off, int k_off, int v_off, const void* row_offsets, void* out, int ldo,
                       yat_stream_t stream) {
    if (dh != GA_DH || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || max_len <= 0 || max_len > GA_MAX_LEN) return YAT_EINVAL;
    if (B <= 0 || B > 65535 || rows <= 0 || !qkv || !row_offsets || !out || !(scale > 0.f) || !(softcap >= 0.f)) return YAT_EINVAL;
    if ((ld & 7) || (ldo & 7) || ((q_off | k_off | v_off) & 7) || q_off < 0 || k_off < 0 || v_off < 0) return YAT_EINVAL;
    if ((int64_t)q_off + (int64_t)Hq * dh > ld || (int64_t)k_off + (int64_t)Hkv * dh > ld ||
        (int64_t)v_off + (int64_t)Hkv * dh > ld || (int64_t)Hq * dh > ldo)
        return YAT_EINVAL;
    if (((uintptr_t)qkv | (uintptr_t)out) & 15 || ((uintptr_t)row_offsets & 3)) return YAT_EINVAL;
    if ((int64_t)GA_MAX_LEN * ld * 2 > 0x7fffffffll || Hq > 65535) return YAT_EINVAL;   // a prompt's K / V block: one buffer resource
    GemmaAttnP p{};
    p.rows = rows; p.Hq = Hq; p.G = Hq / Hkv; p.ld = ld; p.ldo = ldo; p.max_len = max_len; p.scale = scale; p.cap = softcap;
    p.q = (const bf16_t*)qkv + q_off; p.k = (const bf16_t*)qkv + k_off; p.v = (const bf16_t*)qkv + v_off;
    p.off = (const int*)row_offsets; p.out = (bf16_t*)out;
    hipStream_t st = (hipStream_t)stream;
    if (p.G % 8 == 0) return launch_gemma_attn<8, 8>(p, B, Hkv, max_len, st);
    if (p.G % 4 == 0) return launch_gemma_attn<4, 4>(p, B, Hkv, max_len, st);
    if (p.G % 2 == 0) return launch_gemma_attn<4, 2>(p, B, Hkv, max_len, st);
    return launch_gemma_attn<4, 1>(p, B, Hkv, max_len, st);
}

}  // extern "C"
