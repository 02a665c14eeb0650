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
#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------- rmsnorm
// LPR lanes per row as in gemma_rmsnorm_kernel.  With a residual the first pass stores the rounded sum and the second pass
// reads it back: every 16-byte chunk is written and re-read by the same lane, so `sum` may be `res` itself.
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(int M, int D, int lpr, float eps, const bf16_t* __restrict__ x,
                                                         const bf16_t* __restrict__ w, const bf16_t* res, bf16_t* sum,
                                                         bf16_t* __restrict__ y) {
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
            if (res) {
                float rv[8];
                unpack8(*reinterpret_cast<const u32x4*>(res + ro + c * 8), rv);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = rbf(rv[e] + v[e]);
                *reinterpret_cast<u32x4*>(sum + ro + c * 8) = pack8(v);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
        }
    }
    for (int o = 1; o < lpr; o <<= 1) ss += __shfl_xor(ss, o, 64);
    if (!live) return;
    const float rs = 1.0f / sqrtf(ss / (float)D + eps);
    const bf16_t* src = res ? sum : x;
    for (int c = l; c < nch; c += lpr) {
        float v[8], wv[8];
        unpack8(*reinterpret_cast<const u32x4*>(src + ro + c * 8), v);
        unpack8(*reinterpret_cast<const u32x4*>(w + c * 8), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = wv[e] * rbf(v[e] * rs);
        *reinterpret_cast<u32x4*>(y + ro + c * 8) = pack8(v);
    }
}

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
constexpr float TA_LOG2E = 1.4426950408889634f;
constexpr float TA_LAZY_LOG2 = 8.0f;                                   // rescale threshold in log2 units (P <= 2^8)

struct T5AttnP {
    int rows, ld, ldo, max_len;
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    const bf16_t* bias;
    const int* off;
    bf16_t* out;
};

// K image: 16-byte chunk c of key row r lives at chunk c ^ ((r >> 1) & 7) (swz128); V image: at chunk c ^ (((r >> 1) & 3) << 1)
// (an even XOR: the two chunks a 16-lane group of the transposed read covers stay adjacent)
__device__ __forceinline__ bf16x8 ta_frag_row(const char* lds, int row0, int ks, int lane) {
    const uint32_t r = row0 + (lane & 15);
    return lds_read8(lds, r * 128 + swz128(r, ks * 4 + (lane >> 4)) * 16);
}
// operand in ACCUMULATOR k order from the V image: idx = col0 + (lane & 15); k slot (g, j): row 4g + j (j < 4), 16 + 4g + j - 4
__device__ __forceinline__ bf16x8 ta_frag_tr(const char* lds, int row0, int col0, int lane) {
    const uint32_t g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const uint32_t col = col0 + 4 * p;
    const uint32_t r0 = row0 + 4 * g + q, r1 = r0 + 16;
    const uint32_t c0 = (col >> 3) ^ (((r0 >> 1) & 3) << 1), c1 = (col >> 3) ^ (((r1 >> 1) & 3) << 1);
    return cat4(lds_read_tr4(lds, r0 * 128 + c0 * 16 + (p & 1) * 8), lds_read_tr4(lds, r1 * 128 + c1 * 16 + (p & 1) * 8));
}
__device__ __forceinline__ bf16x8 ta_acc_to_frag(const f32x4& a, const f32x4& b) {
    bf16x8 r;
    r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
    r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    return r;
}
__device__ __forceinline__ float ta_group_max(float v) {      // across the 4 lane groups that share lane & 15
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float ta_group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

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
        for (int i = threadIdx.x; i < nbias; i += TA_NW * 64) bl[i] = bf2f(bh[i]) * TA_LOG2E;
    }

    bf16x8 qf[KS];
    {
        const int qi = sq0 + li;
        const bf16_t* qp = p.q + (int64_t)(prow0 + qi) * p.ld + head * TA_DH + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 z;
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.0f;
            if (qi < len) z = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
            qf[ks] = z;
        }
    }
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
                for (int ks = 0; ks < KS; ++ks) s[nj] = mfma16(ta_frag_row(Ks, h * 32 + nj * 16, ks, lane), qf[ks], s[nj]);
            }
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kj = kh0 + nj * 16 + 4 * g + r;
                    const int bi = min(max(kj + dbase, 0), nbias - 1);     // (a dead query's index may leave the table)
                    s[nj][r] = __builtin_fmaf(s[nj][r], TA_LOG2E, bl[bi]);
                }
            if (kh0 + 32 > len) {                              // uniform: the prompt ends inside this half
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kh0 + nj * 16 + 4 * g + r >= len) s[nj][r] = -1e30f;
            }
            float t = -1e30f;
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 4; ++r) t = fmaxf(t, s[nj][r]);
            const float mx = ta_group_max(t);
            if (__builtin_amdgcn_ballot_w64(mx > m + TA_LAZY_LOG2) != 0) {     // uniform; after the first tiles: rare
                const float mn = fmaxf(m, mx);
                const float alpha = __builtin_amdgcn_exp2f(m - mn);
                m = mn;
                l *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
            }
            float rs = 0.f;
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = rbf(__builtin_amdgcn_exp2f(s[nj][r] - m));
                    s[nj][r] = e;
                    rs += e;
                }
            l += ta_group_sum(rs);
            const bf16x8 pf = ta_acc_to_frag(s[0], s[1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(ta_frag_tr(Vs, h * 32, dt * 16, lane), pf, o[dt]);
        }
    }
    const int qi = sq0 + li;
    if (qi < len) {
        const float inv = 1.0f / l;
        bf16_t* op = p.out + (int64_t)(prow0 + qi) * p.ldo + head * TA_DH;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            *reinterpret_cast<u32x2*>(op + dt * 16 + 4 * g) =
                pack4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

}  // namespace

extern "C" {

int yat_t5_rmsnorm(int M, int D, float eps, const void* x, const void* w, const void* residual, void* sum_out, void* y,
                   yat_stream_t stream) {
    if (M <= 0 || D <= 0 || (D & 7) || !(eps >= 0.f) || !x || !w || !y || (residual && !sum_out)) return YAT_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)residual | (uintptr_t)sum_out) & 15) return YAT_EINVAL;
    int lpr = 1;
    while (lpr < 64 && ((D >> 3) % (lpr * 2)) == 0) lpr *= 2;
    const int rows_per_block = 256 / lpr;
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)((M + rows_per_block - 1) / rows_per_block)), dim3(256), 0,
                       (hipStream_t)stream, M, D, lpr, eps, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)residual,
                       (bf16_t*)sum_out, (bf16_t*)y);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
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
