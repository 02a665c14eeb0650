// AutoencoderKL decoder kernels (diffusers AutoencoderKL, the VAE of PixArt-Sigma and SD3.5: train_pixart_sigma.py:137-144,
// train_sd35.py:150-156).  Forward only, bf16 activations in NHWC (token-major) layout, fp32 arithmetic inside every kernel.
// The 3x3 convs, the 1x1 convs / Linears and the postprocess reuse the DC-AE and GEMM entry points (yat_amd/autoencoder_kl.py);
// what the KL decoder needs beyond them:
//
//   groupnorm   nn.GroupNorm(G, C, eps) (+ the SiLU module after it) over NHWC.  Three launches, no atomics, fixed order:
//               partial  one workgroup per (image, slab of GN_SLAB pixels): per-group sums of (x - K_g) and (x - K_g)^2 in
//                        fp32, K_g = the group's first value in the image (a shifted sum: the group's spread sets the scale of
//                        the sums, not its offset, so E[x^2] - E[x]^2 does not cancel);
//               finish   one workgroup per (group, image): the slab partials in a fixed tree order -> K, mean - K, rstd;
//               apply    y = bf16(((x - K) - (mean - K)) * rstd * w + b), then bf16(silu(y)) with silu = 1.
//   attention   F.scaled_dot_product_attention(q, k, v) with one head of dh in {64, 512}, no mask (the mid-block Attention):
//               flash-style, scores and the online softmax in fp32, P rounded to bf16 for the P V product, fp32 accumulation;
//               the row sum adds the same rounded P, so the weights that multiply V sum to one exactly.
#include "attn_prefill.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------- groupnorm
constexpr int GN_SLAB = 512;          // pixels per partial workgroup
constexpr int GN_MAX_C = 2048;        // C / 8 chunks <= 256 threads

inline int gn_slabs(int HW) { return (HW + GN_SLAB - 1) / GN_SLAB; }
// workspace: slab partials [B, nslab, G, 2], padded to 16 bytes, then the statistics [B, G, 4]
inline uint64_t gn_part_floats(int B, int HW, int G) { return ((uint64_t)B * gn_slabs(HW) * G * 2 + 3) & ~(uint64_t)3; }

// thread = (pixel row r, 8-channel chunk c): rows = 256 / (C / 8) pixels in flight per iteration
__global__ __launch_bounds__(256) void gn_partial_kernel(int HW, int C, int G, const bf16_t* __restrict__ x,
                                                         float* __restrict__ part) {
    const int slab = blockIdx.x, b = blockIdx.y, nslab = gridDim.x;
    const int nch = C >> 3, rows = 256 / nch, cg = C / G;
    const int tid = threadIdx.x, c = tid % nch, r = tid / nch;
    const bf16_t* xb = x + (int64_t)b * HW * C;
    float k[8], s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        k[e] = bf2f(xb[((c * 8 + e) / cg) * cg]);
        s1[e] = 0.f;
        s2[e] = 0.f;
    }
    if (r < rows) {
        const int p1 = min(HW, (slab + 1) * GN_SLAB);
        for (int p = slab * GN_SLAB + r; p < p1; p += rows) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4*>(xb + (int64_t)p * C + c * 8), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[e] - k[e];
                s1[e] += d;
                s2[e] = __builtin_fmaf(d, d, s2[e]);
            }
        }
    }
    // this workgroup's rows, then the group's channels, in order (LDS [row][C])
    __shared__ float rs1[GN_MAX_C], rs2[GN_MAX_C];
    if (r < rows) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            rs1[r * C + c * 8 + e] = s1[e];
            rs2[r * C + c * 8 + e] = s2[e];
        }
    }
    __syncthreads();
    for (int g = tid; g < G; g += 256) {
        float a = 0.f, q = 0.f;
        for (int rr = 0; rr < rows; ++rr)
            for (int j = 0; j < cg; ++j) {
                a += rs1[rr * C + g * cg + j];
                q += rs2[rr * C + g * cg + j];
            }
        float* o = part + (((int64_t)b * nslab + slab) * G + g) * 2;
        o[0] = a;
        o[1] = q;
    }
}

__global__ __launch_bounds__(256) void gn_finish_kernel(int HW, int C, int G, int nslab, float eps, const bf16_t* __restrict__ x,
                                                        const float* __restrict__ part, float* __restrict__ stats) {
    __shared__ float t1[256], t2[256];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, cg = C / G;
    float a = 0.f, q = 0.f;
    for (int i = tid; i < nslab; i += 256) {
        const float* pp = part + (((int64_t)b * nslab + i) * G + g) * 2;
        a += pp[0];
        q += pp[1];
    }
    t1[tid] = a;
    t2[tid] = q;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            t1[tid] += t1[tid + s];
            t2[tid] += t2[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float n = (float)HW * (float)cg;
        const float m1 = t1[0] / n;                               // mean - K
        const float var = fmaxf(t2[0] / n - m1 * m1, 0.f);        // biased, as nn.GroupNorm
        // (K, mean - K, rstd): the apply pass forms (x - K) - (mean - K), exact up to the last subtraction -- K + m1 rounded to
        // fp32 would carry an error of |mean| * 2^-24, which is not small against the spread when mean >> std.  K is kept
        // here because the apply pass may overwrite x (y aliasing x).
        float* st = stats + ((int64_t)b * G + g) * 4;
        st[0] = bf2f(x[(int64_t)b * HW * C + g * cg]);
        st[1] = m1;
        st[2] = 1.0f / sqrtf(var + eps);
        st[3] = 0.f;
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(int64_t nchunk, int HW, int C, int G, const bf16_t* x,
                                                       const bf16_t* __restrict__ w, const bf16_t* __restrict__ bias,
                                                       const float* __restrict__ stats, int silu, bf16_t* y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    const int nch = C >> 3, cg = C / G;
    const int64_t pix = i / nch;
    const int c0 = (int)(i - pix * nch) * 8;
    const int b = (int)(pix / HW);
    float v[8], wv[8], bv[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + i * 8), v);
    unpack8(*reinterpret_cast<const u32x4*>(w + c0), wv);
    unpack8(*reinterpret_cast<const u32x4*>(bias + c0), bv);
    const float* st = stats + (int64_t)b * G * 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const f32x4 sg = *reinterpret_cast<const f32x4*>(st + 4 * ((c0 + e) / cg));     // K, mean - K, rstd
        float t = rbf(__builtin_fmaf(((v[e] - sg[0]) - sg[1]) * sg[2], wv[e], bv[e]));
        if (silu) t = rbf(silu_f(t));
        v[e] = t;
    }
    *reinterpret_cast<u32x4*>(y + i * 8) = pack8(v);
}

// ---------------------------------------------------------------------------------------------------------- attention
// Workgroup = 64 queries (4 waves x 16), loop over 32-key tiles, two LDS stages (tile t+1 lands while tile t is consumed, one
// barrier per tile).  Each wave holds its 16 queries' Q fragments (dh / 32 of them) and the whole O accumulator (16 x dh fp32
// = dh / 16 MFMA tiles: 128 VGPRs at dh 512) in registers.  The K and V tiles are kept as dh / 128 images of [32 keys][128
// columns] each in the layouts of csrc/sdpa.hip: K row-swizzled (read as rows for S = K Q^T), V swizzled for the transposed
// ds_read_b64_tr_b16 read (the P V operand in the accumulator's k order).  Every product is issued with swapped operands so
// the query sits on lane & 15: the probability accumulators are directly the B operand of P V.
//   dh 512: stage = (K + V) 32 x 512 bf16 = 64 KiB, two stages = 128 KiB -> one workgroup per CU.
constexpr int AT_KEYS = 32;
constexpr int AT_SUB = AT_KEYS * 256;               // one [32][128] bf16 image

struct AttnP {
    int N, ld, ldo;
    float scale;
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    bf16_t* out;
};

template <int DH>
__global__ __launch_bounds__(256) void vae_attn_kernel(AttnP p) {
    constexpr int KS = DH / 32, DT = DH / 16, DB = (DH + 127) / 128;
    constexpr int IMG = DB * AT_SUB, STAGE = 2 * IMG;          // K images, then V images
    constexpr int PIECES = DB * AT_SUB / 1024 / 4;             // 1-KiB DMA pieces per wave per matrix
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * 64 + wave * 16;
    const int64_t row0 = (int64_t)b * p.N, rowl = row0 + p.N;

    // this lane's byte offsets (relative to the tile's first row) for its pieces of the K and V images
    uint32_t ok[PIECES], ov[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int pc = j * 4 + wave, db = pc / 8, r = (pc % 8) * 4 + (lane >> 4), slot = lane & 15;
        const int ck = db * 16 + (slot ^ (r & 15)), cv = db * 16 + (slot ^ ((r & 7) << 1));
        ok[j] = ck * 8 < DH ? (uint32_t)((r * p.ld + ck * 8) * 2) : YAT_OOB;
        ov[j] = cv * 8 < DH ? (uint32_t)((r * p.ld + cv * 8) * 2) : YAT_OOB;
    }
    auto stage = [&](int k0, char* base) {
        const int64_t rows = rowl - (row0 + k0);
        const uint64_t bytes = (uint64_t)rows * p.ld * 2;
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(p.k + (row0 + k0) * p.ld, bytes);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(p.v + (row0 + k0) * p.ld, bytes);
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int pc = j * 4 + wave;
            lds_dma16(rk, (YAT_LDS void*)(base + pc * 1024), ok[j]);
            lds_dma16(rv, (YAT_LDS void*)(base + IMG + pc * 1024), ov[j]);
        }
    };
    stage(0, smem);

    bf16x8 qf[KS];
    {
        const int64_t qr = row0 + q0 + li;
        load_q_frags<KS>(qf, p.q + qr * p.ld, qr < rowl, g);
    }
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;
    const float ce = p.scale * LOG2E;                   // exp2 argument = s * ce - m * ce on the raw scores

    int it = 0;
    for (int k0 = 0; k0 < p.N; k0 += AT_KEYS, ++it) {
        char* cur = smem + (it & 1) * STAGE;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // tile `it` landed for every wave; the other stage is free
        if (k0 + AT_KEYS < p.N) stage(k0 + AT_KEYS, smem + ((it + 1) & 1) * STAGE);
        const char* Ks = cur;
        const char* Vs = cur + IMG;

        f32x4 s[2];
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) {
            s[nj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                s[nj] = mfma16(frag_row256(Ks + (ks / 4) * AT_SUB, nj * 16, ks % 4, lane), qf[ks], s[nj]);
        }
        if (k0 + AT_KEYS > p.N) {                          // uniform: keys past N in the last tile vanish from the softmax
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + nj * 16 + 4 * g + r >= p.N) s[nj][r] = -1e30f;
        }
        const bf16x8 pf = online_softmax_step<DT>(s, m, l, o, ce);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(frag_tr256(Vs + (dt / 8) * AT_SUB, (dt % 8) * 16, lane), pf, o[dt]);
    }
    const int qi = q0 + li;
    if (qi < p.N) store_o<DT>(p.out + (row0 + qi) * p.ldo, o, l, g);
}

template <int DH>
int launch_attn(const AttnP& p, int B, hipStream_t stream) {
    constexpr int LDS = 2 * 2 * ((DH + 127) / 128) * AT_SUB;
    static bool attr_set = false;
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute((const void*)vae_attn_kernel<DH>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    hipLaunchKernelGGL(vae_attn_kernel<DH>, dim3((unsigned)((p.N + 63) / 64), (unsigned)B), dim3(256), LDS, stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // namespace

extern "C" {

uint64_t yat_vae_groupnorm_workspace_bytes(int B, int HW, int C, int G) {
    if (B <= 0 || HW <= 0 || G <= 0) return 0;
    (void)C;
    return (gn_part_floats(B, HW, G) + (uint64_t)B * G * 4) * sizeof(float);
}

int yat_vae_groupnorm(int B, int HW, int C, int G, float eps, const void* x, const void* w, const void* b, int silu, void* y,
                      void* workspace, yat_stream_t stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || G <= 0 || (C & 7) || C > GN_MAX_C || C % G || !(eps >= 0.f)) return YAT_EINVAL;
    if (silu != 0 && silu != 1) return YAT_EINVAL;
    if (!x || !w || !b || !y || !workspace) return YAT_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b | (uintptr_t)y | (uintptr_t)workspace) & 15) return YAT_EINVAL;
    if (B > 65535 || G > 65535 || (int64_t)B * HW * C / 8 / 256 >= 0x7fffffffll) return YAT_EINVAL;
    const int nslab = gn_slabs(HW);
    float* part = (float*)workspace;
    float* stats = part + gn_part_floats(B, HW, G);
    hipLaunchKernelGGL(gn_partial_kernel, dim3((unsigned)nslab, (unsigned)B), dim3(256), 0, (hipStream_t)stream, HW, C, G,
                       (const bf16_t*)x, part);
    YAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_finish_kernel, dim3((unsigned)G, (unsigned)B), dim3(256), 0, (hipStream_t)stream, HW, C, G, nslab, eps,
                       (const bf16_t*)x, (const float*)part, stats);
    YAT_CHECK_LAUNCH();
    const int64_t nchunk = (int64_t)B * HW * (C / 8);
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nchunk, HW, C,
                       G, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (const float*)stats, silu, (bf16_t*)y);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_vae_attn_fwd(int B, int N, int dh, const void* q, const void* k, const void* v, int ld, void* out, int ldo,
                     yat_stream_t stream) {
    if (dh != 64 && dh != 512) return YAT_EINVAL;
    if (B <= 0 || N <= 0 || B > 65535 || !q || !k || !v || !out) return YAT_EINVAL;
    if (ld < dh || ldo < dh || (ld & 7) || (ldo & 7)) return YAT_EINVAL;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return YAT_EINVAL;
    if ((int64_t)B * N * ld > 0x3fffffffll) return YAT_EINVAL;     // byte offsets of the buffer resources stay below 2 GiB
    AttnP p{};
    p.N = N; p.ld = ld; p.ldo = ldo; p.scale = 1.0f / sqrtf((float)dh);
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.out = (bf16_t*)out;
    return dh == 512 ? launch_attn<512>(p, B, (hipStream_t)stream) : launch_attn<64>(p, B, (hipStream_t)stream);
}

}  // extern "C"
