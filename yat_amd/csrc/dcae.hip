// DC-AE decoder kernels (diffusers AutoencoderDC, the VAE that SanaModel.validate decodes with: train_sana.py:153-157).
// Forward only, bf16 activations in NHWC (token-major) layout, fp32 arithmetic inside every kernel.
//
//   conv3x3         dense 3x3 convolution, pad 1, as an implicit GEMM on MFMA: M = output pixels, N = Cout, K = 9 Cin
//                   (weights re-packed by the host to [Cout, 3, 3, Cin] so that K is contiguous).  Optional, fused: a
//                   nearest x2 upsample of the input in the address math (DCUpBlock2d, interpolate mode), bias, SiLU
//                   (ResBlock conv1), one of the two channel-repeat shortcuts (Decoder.conv_in, DCUpBlock2d) and a
//                   residual add.  Cout <= 4 (the RGB conv_out) takes a direct kernel instead of a 128-wide MFMA tile.
//   msla_aggregate  SanaMultiscaleAttentionProjection: depthwise 5x5 (pad 2) + grouped 1x1 (32 -> 32 per group), one pass.
//   rmsnorm_bias    diffusers RMSNorm(eps, elementwise_affine, bias) with its bf16 rounding, + residual, + ReLU.
//   image_to_uint8  VaeImageProcessor.postprocess: (x / 2 + 0.5).clamp(0, 1) in bf16, then numpy's round(x * 255).
#include "dcae_conv.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------- conv3x3
// The tile, its B operand, fragment reads and K loop are dcae_conv.hpp (shared with the encoder convs, dcae_enc.hip); this
// file adds the decoder's A-operand address math (optional nearest x2 upsample) and its epilogue.
struct ConvP {
    const bf16_t* x;      // [B, Hin, Win, Cin]
    const bf16_t* w;      // [Cout, 9 * Cin]
    const bf16_t* bias;   // [Cout] or null
    const bf16_t* sc;     // shortcut source or null
    const bf16_t* res;    // [B, H, W, Cout] or null
    bf16_t* y;            // [B, H, W, Cout] (NCHW for the direct kernel when nchw)
    int B, H, W, Cin, Cout, Hin, Win, up, silu, sc_mode, sc_ch, sc_rep, nchw;
    int M, K, nbm, nbn;
    uint64_t x_bytes, w_bytes;
};

template <bool TAPU>
__device__ __forceinline__ void conv_stage_a(const ConvP& p, __amdgpu_buffer_rsrc_t rx, char* lds, int k0, int wave,
                                             const int (&rb)[4], const int (&ry)[4], const int (&rxx)[4], const int (&cc)[4]) {
    int tapu = 0, ciu = 0;
    if (TAPU) {                                        // Cin % 64 == 0: the whole K-tile lies in one tap
        tapu = k0 / p.Cin;
        ciu = k0 - tapu * p.Cin;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int piece = j * 4 + wave;
        const int kg = k0 + cc[j] * 8;
        int tap, ci;
        if (TAPU) {
            tap = tapu;
            ci = ciu + cc[j] * 8;
        } else {
            tap = kg / p.Cin;
            ci = kg - tap * p.Cin;
        }
        const int t3 = tap / 3;
        int iy = ry[j] + t3 - 1, ix = rxx[j] + (tap - 3 * t3) - 1;
        const bool ok = kg < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        if (p.up) {
            iy >>= 1;
            ix >>= 1;
        }
        const uint32_t voff = ok ? (uint32_t)((((int64_t)(rb[j] + iy) * p.Win + ix) * p.Cin + ci) * 2) : YAT_OOB;
        lds_dma16(rx, (YAT_LDS void*)(lds + piece * 1024), voff);
    }
}

// epilogue of 4 consecutive output channels n..n+3 of pixel m:
// +bias -> bf16 -> [SiLU -> bf16] -> [+ shortcut -> bf16] -> [+ residual -> bf16]
__device__ __forceinline__ void conv_epilogue(const ConvP& p, float (&v)[4], int m, int n) {
    if (p.bias) {
        float bb[4];
        unpack4(*reinterpret_cast<const u32x2*>(p.bias + n), bb);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bb[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
    if (p.silu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(silu_f(v[e]));
    }
    if (p.sc_mode == 1) {                    // repeat_interleave(z, rep, dim=C): channel c adds z[c // rep]
        const bf16_t* s = p.sc + (int64_t)m * p.sc_ch;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] + bf2f(s[(n + e) / p.sc_rep]));
    } else if (p.sc_mode == 2) {             // pixel_shuffle(repeat_interleave(x, rep), 2) from the half-resolution input
        const int hw = p.H * p.W, b = m / hw, pix = m - b * hw, oy = pix / p.W, ox = pix - oy * p.W;
        const bf16_t* s = p.sc + (((int64_t)b * (p.H >> 1) + (oy >> 1)) * (p.W >> 1) + (ox >> 1)) * p.sc_ch;
        const int sub = 2 * (oy & 1) + (ox & 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] + bf2f(s[(4 * (n + e) + sub) / p.sc_rep]));
    }
    if (p.res) {
        float r[4];
        unpack4(*reinterpret_cast<const u32x2*>(p.res + (int64_t)m * p.Cout + n), r);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] + r[e]);
    }
    *reinterpret_cast<u32x2*>(p.y + (int64_t)m * p.Cout + n) = pack4(v[0], v[1], v[2], v[3]);
}

template <bool TAPU>
__global__ __launch_bounds__(256, 2) void conv3x3_mfma_kernel(ConvP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    int m0, n0;
    conv_tile_origin(p.nbm, p.nbn, m0, n0);

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

    // this lane's four A rows (output pixels) and the source chunk each of its LDS slots holds
    int rb[4], ry[4], rxx[4], cc[4];
    const int hw = p.H * p.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (j * 4 + wave) * 8 + (lane >> 3);
        const int m = m0 + r;
        cc[j] = swz128(r, lane & 7);
        if (m < p.M) {
            const int b = m / hw, pix = m - b * hw, oy = pix / p.W;
            rb[j] = b * p.Hin;
            ry[j] = oy;
            rxx[j] = pix - oy * p.W;
        } else {
            rb[j] = 0;
            ry[j] = -4;                                  // every tap out of range -> zeros
            rxx[j] = 0;
        }
    }

    f32x4 acc[4][4];
    conv_mainloop(smem, rw, p.Cout, p.K, n0, wave, lane, acc,
                  [&](char* lds, int k0) { conv_stage_a<TAPU>(p, rx, lds, k0, wave, rb, ry, rxx, cc); });

    // lane owns pixel m = .. + (lane & 15) and output channels n = .. + 4 (lane >> 4) + 0..3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= p.Cout) continue;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            conv_epilogue(p, v, m, n);
        }
    }
}

// Cout <= 4 (Decoder.conv_out, C0 -> RGB): one output pixel per thread, all Cout channels, the weights broadcast from
// LDS.  The input is read once per tap in 16-B chunks (neighbouring threads share rows through L1 / L2) instead of being
// staged into a 128-wide MFMA tile of which 3 columns would be used.
constexpr int SMALL_COUT = 4;

__global__ __launch_bounds__(256) void conv3x3_small_kernel(ConvP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* wl = reinterpret_cast<bf16_t*>(smem);
    const int nw = p.Cout * p.K;                               // multiple of 8 (Cin % 8 == 0)
    for (int i = threadIdx.x * 8; i < nw; i += 256 * 8)
        *reinterpret_cast<u32x4*>(wl + i) = *reinterpret_cast<const u32x4*>(p.w + i);
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= p.M) return;
    const int hw = p.H * p.W, b = m / hw, pix = m - b * hw, oy = pix / p.W, ox = pix - oy * p.W;
    float acc[SMALL_COUT] = {0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        if ((unsigned)iy >= (unsigned)p.H || (unsigned)ix >= (unsigned)p.W) continue;
        if (p.up) {
            iy >>= 1;
            ix >>= 1;
        }
        const bf16_t* xp = p.x + (((int64_t)b * p.Hin + iy) * p.Win + ix) * p.Cin;
        for (int c = 0; c < p.Cin; c += 8) {
            float xv[8];
            unpack8(*reinterpret_cast<const u32x4*>(xp + c), xv);
#pragma unroll
            for (int co = 0; co < SMALL_COUT; ++co) {
                if (co < p.Cout) {
                    float wv[8];
                    unpack8(*reinterpret_cast<const u32x4*>(wl + co * p.K + tap * p.Cin + c), wv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[co] = __builtin_fmaf(xv[e], wv[e], acc[co]);
                }
            }
        }
    }
#pragma unroll
    for (int co = 0; co < SMALL_COUT; ++co) {
        if (co >= p.Cout) break;
        float v = acc[co];
        if (p.bias) v += bf2f(p.bias[co]);
        v = rbf(v);
        if (p.silu) v = rbf(silu_f(v));
        if (p.res) v = rbf(v + bf2f(p.res[(int64_t)m * p.Cout + co]));
        const int64_t o = p.nchw ? ((int64_t)b * p.Cout + co) * hw + pix : (int64_t)m * p.Cout + co;
        p.y[o] = f2bf(v);
    }
}

// ------------------------------------------------------------------------------------------------------ msla_aggregate
// One workgroup = 64 pixels of one image row x one 32-channel group.  Thread (pixel px, chunk q of 8 channels):
//   t[c] = bf16( sum_{5x5 taps} w_dw[c, tap] x[pixel + tap, c] )         (proj_in, depthwise, pad 2, no bias)
//   y[o] = bf16( sum_{i < 32} w_pw[g*32 + o, i] t[g*32 + i] )             (proj_out, groups of 32 -> 32, no bias)
// t goes through LDS so that each thread's 8 outputs can read the group's 32 inputs.
constexpr int MS_PIX = 64;

__global__ __launch_bounds__(256) void msla_aggregate_kernel(int H, int W, int C3, const bf16_t* __restrict__ x,
                                                             const bf16_t* __restrict__ wdw, const bf16_t* __restrict__ wpw,
                                                             bf16_t* __restrict__ y) {
    __shared__ float s_wdw[32 * 25];
    __shared__ float s_wpw[32 * 33];
    __shared__ float s_t[MS_PIX * 33];
    const int g = blockIdx.z, row = blockIdx.y;             // row = b * H + oy
    const int b = row / H, oy = row - b * H;
    const int tid = threadIdx.x;
    for (int i = tid; i < 32 * 25; i += 256) s_wdw[i] = bf2f(wdw[(int64_t)g * 32 * 25 + i]);
    for (int i = tid; i < 32 * 32; i += 256) s_wpw[(i >> 5) * 33 + (i & 31)] = bf2f(wpw[(int64_t)g * 32 * 32 + i]);
    __syncthreads();
    const int px = tid >> 2, q = tid & 3;
    const int ox = blockIdx.x * MS_PIX + px;
    const int c0 = g * 32 + q * 8;
    if (ox < W) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int dy = -2; dy <= 2; ++dy) {
            const int iy = oy + dy;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int ix = ox + dx;
                if ((unsigned)ix >= (unsigned)W) continue;
                float xv[8];
                unpack8(*reinterpret_cast<const u32x4*>(x + (((int64_t)b * H + iy) * W + ix) * C3 + c0), xv);
                const int tap = (dy + 2) * 5 + (dx + 2);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(s_wdw[(q * 8 + e) * 25 + tap], xv[e], acc[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s_t[px * 33 + q * 8 + e] = rbf(acc[e]);
    }
    __syncthreads();
    if (ox >= W) return;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float s = 0.f;
#pragma unroll 8
        for (int i = 0; i < 32; ++i) s = __builtin_fmaf(s_wpw[(q * 8 + e) * 33 + i], s_t[px * 33 + i], s);
        o[e] = s;
    }
    *reinterpret_cast<u32x4*>(y + (((int64_t)b * H + oy) * W + ox) * C3 + c0) = pack8(o);
}

// -------------------------------------------------------------------------------------------------------- rmsnorm_bias
// LPR lanes per row (a power of two dividing D / 8, at most 64); two passes over the row (the second re-reads it from L1).
__global__ __launch_bounds__(256) void rmsnorm_bias_kernel(int M, int D, int lpr, float eps, const bf16_t* __restrict__ x,
                                                           const bf16_t* __restrict__ w, const bf16_t* __restrict__ bias,
                                                           const bf16_t* res, int relu, bf16_t* y) {
    const int rows_per_block = 256 / lpr;
    const int r = blockIdx.x * rows_per_block + threadIdx.x / lpr;
    const int l = threadIdx.x & (lpr - 1);
    const int nch = D >> 3;
    const bool live = r < M;
    const bf16_t* xr = x + (int64_t)(live ? r : 0) * D;
    float ss = 0.f;
    if (live) {
        for (int c = l; c < nch; c += lpr) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
        }
    }
    for (int o = 1; o < lpr; o <<= 1) ss += __shfl_xor(ss, o, 64);
    if (!live) return;
    const float rs = 1.0f / sqrtf(ss / (float)D + eps);
    for (int c = l; c < nch; c += lpr) {
        float v[8], wv[8], bv[8];
        unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
        unpack8(*reinterpret_cast<const u32x4*>(w + c * 8), wv);
        if (bias) unpack8(*reinterpret_cast<const u32x4*>(bias + c * 8), bv);
        float rv[8];
        if (res) unpack8(*reinterpret_cast<const u32x4*>(res + (int64_t)r * D + c * 8), rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = rbf(rbf(v[e] * rs) * wv[e]);
            if (bias) t = rbf(t + bv[e]);
            if (res) t = rbf(t + rv[e]);
            if (relu) t = fmaxf(t, 0.f);
            v[e] = t;
        }
        *reinterpret_cast<u32x4*>(y + (int64_t)r * D + c * 8) = pack8(v);
    }
}

// ------------------------------------------------------------------------------------------------------ image_to_uint8
__global__ __launch_bounds__(256) void image_to_uint8_kernel(int64_t n, const bf16_t* __restrict__ x, uint8_t* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float h = rbf(bf2f(x[i]) * 0.5f);
    const float p = fminf(fmaxf(rbf(h + 0.5f), 0.f), 1.f);
    y[i] = (uint8_t)__builtin_rintf(p * 255.0f);          // round half to even, as numpy's round
}

}  // namespace

extern "C" {

int yat_dcae_conv3x3(int B, int H, int W, int Cin, int Cout, int upsample, int silu, const void* x, const void* w,
                     const void* bias, int shortcut_mode, const void* shortcut, int shortcut_channels, const void* residual,
                     int out_nchw, void* y, yat_stream_t stream) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 7) || !x || !w || !y) return YAT_EINVAL;
    if (upsample != 0 && upsample != 1) return YAT_EINVAL;
    if (silu != 0 && silu != 1) return YAT_EINVAL;
    if (out_nchw != 0 && out_nchw != 1) return YAT_EINVAL;
    if (upsample && ((H | W) & 1)) return YAT_EINVAL;
    const bool small = Cout <= SMALL_COUT;
    if (!small && ((Cout & 3) || out_nchw)) return YAT_EINVAL;
    ConvP p{};
    p.sc_rep = 1;
    if (shortcut_mode == 1) {
        if (!shortcut || shortcut_channels <= 0 || Cout % shortcut_channels) return YAT_EINVAL;
        p.sc_rep = Cout / shortcut_channels;
    } else if (shortcut_mode == 2) {
        if (!shortcut || shortcut_channels <= 0 || ((H | W) & 1) || (4 * Cout) % shortcut_channels) return YAT_EINVAL;
        p.sc_rep = 4 * Cout / shortcut_channels;
    } else if (shortcut_mode != 0) {
        return YAT_EINVAL;
    }
    if (small && shortcut_mode) return YAT_EINVAL;
    const int Hin = upsample ? H / 2 : H, Win = upsample ? W / 2 : W;
    const int64_t M = (int64_t)B * H * W;
    const uint64_t x_bytes = (uint64_t)B * Hin * Win * Cin * 2, w_bytes = (uint64_t)Cout * 9 * Cin * 2;
    if (M > 0x7fffffffll || x_bytes > 0x7fffffffull || w_bytes > 0x7fffffffull) return YAT_EINVAL;
    if (small && w_bytes > 65536) return YAT_EINVAL;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.bias = (const bf16_t*)bias; p.sc = (const bf16_t*)shortcut;
    p.res = (const bf16_t*)residual; p.y = (bf16_t*)y;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.Hin = Hin; p.Win = Win; p.up = upsample; p.silu = silu;
    p.sc_mode = shortcut_mode; p.sc_ch = shortcut_channels; p.nchw = out_nchw;
    p.M = (int)M; p.K = 9 * Cin; p.x_bytes = x_bytes; p.w_bytes = w_bytes;
    if (small) {
        hipLaunchKernelGGL(conv3x3_small_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), (unsigned)w_bytes,
                           (hipStream_t)stream, p);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    }
    p.nbm = (int)((M + CBM - 1) / CBM);
    p.nbn = (Cout + CBN - 1) / CBN;
    if ((int64_t)p.nbm * p.nbn > 0x7fffffffll) return YAT_EINVAL;
    const dim3 grid((unsigned)(p.nbm * p.nbn));
    if (Cin % 64 == 0)
        hipLaunchKernelGGL(conv3x3_mfma_kernel<true>, grid, dim3(256), CLDS, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(conv3x3_mfma_kernel<false>, grid, dim3(256), CLDS, (hipStream_t)stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_dcae_msla_aggregate(int B, int H, int W, int C3, const void* qkv, const void* w_dw, const void* w_pw, void* out,
                            yat_stream_t stream) {
    if (B <= 0 || H <= 0 || W <= 0 || C3 <= 0 || (C3 & 31) || !qkv || !w_dw || !w_pw || !out) return YAT_EINVAL;
    if ((int64_t)B * H > 65535 || C3 / 32 > 65535) return YAT_EINVAL;
    hipLaunchKernelGGL(msla_aggregate_kernel, dim3((W + MS_PIX - 1) / MS_PIX, B * H, C3 / 32), dim3(256), 0,
                       (hipStream_t)stream, H, W, C3, (const bf16_t*)qkv, (const bf16_t*)w_dw, (const bf16_t*)w_pw,
                       (bf16_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_dcae_rmsnorm_bias(int M, int D, float eps, const void* x, const void* w, const void* b, const void* residual,
                          int relu, void* y, yat_stream_t stream) {
    if (M <= 0 || D <= 0 || (D & 7) || !(eps >= 0.f) || !x || !w || !y || (relu != 0 && relu != 1)) return YAT_EINVAL;
    int lpr = 1;
    while (lpr < 64 && ((D >> 3) % (lpr * 2)) == 0) lpr *= 2;
    const int rows_per_block = 256 / lpr;
    hipLaunchKernelGGL(rmsnorm_bias_kernel, dim3((unsigned)((M + rows_per_block - 1) / rows_per_block)), dim3(256), 0,
                       (hipStream_t)stream, M, D, lpr, eps, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b,
                       (const bf16_t*)residual, relu, (bf16_t*)y);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_dcae_image_to_uint8(int64_t n, const void* x, void* out, yat_stream_t stream) {
    if (n <= 0 || n > 0x7fffffffll || !x || !out) return YAT_EINVAL;
    hipLaunchKernelGGL(image_to_uint8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       (const bf16_t*)x, (uint8_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
