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
#include "rownorm_lpr.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------- conv3x3
// The kernel is dcae_conv.hpp's (stride 1, pad 1, with or without the nearest x2 upsample of the input); this file adds the
// decoder's epilogue and the direct kernel for Cout <= 4.
//
// epilogue of 4 consecutive output channels n..n+3 of pixel m:
// +bias -> bf16 -> [SiLU -> bf16] -> [+ shortcut -> bf16] -> [+ residual -> bf16]
struct conv_epilogue {
    const bf16_t* bias;   // [Cout] or null
    const bf16_t* sc;     // shortcut source or null
    const bf16_t* res;    // [B, H, W, Cout] or null
    bf16_t* y;            // [B, H, W, Cout] (NCHW for the direct kernel when nchw)
    int silu, sc_mode, sc_ch, sc_rep;

    __device__ __forceinline__ void operator()(const ConvGeom& g, float (&v)[4], int m, int n) const {
        if (bias) {
            float bb[4];
            unpack4(*reinterpret_cast<const u32x2*>(bias + n), bb);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bb[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
        if (silu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rbf(silu_f(v[e]));
        }
        if (sc_mode == 1) {                    // repeat_interleave(z, rep, dim=C): channel c adds z[c // rep]
            const bf16_t* s = sc + (int64_t)m * sc_ch;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] + bf2f(s[(n + e) / sc_rep]));
        } else if (sc_mode == 2) {             // pixel_shuffle(repeat_interleave(x, rep), 2) from the half-resolution input
            int b, oy, ox;
            conv_pixel(g, m, b, oy, ox);
            const bf16_t* s = sc + (((int64_t)b * (g.Ho >> 1) + (oy >> 1)) * (g.Wo >> 1) + (ox >> 1)) * sc_ch;
            const int sub = 2 * (oy & 1) + (ox & 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] + bf2f(s[(4 * (n + e) + sub) / sc_rep]));
        }
        if (res) {
            float r[4];
            unpack4(*reinterpret_cast<const u32x2*>(res + (int64_t)m * g.Cout + n), r);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] + r[e]);
        }
        *reinterpret_cast<u32x2*>(y + (int64_t)m * g.Cout + n) = pack4(v[0], v[1], v[2], v[3]);
    }
};

// Cout <= 4 (Decoder.conv_out, C0 -> RGB): one output pixel per thread, all Cout channels, the weights broadcast from
// LDS.  The input is read once per tap in 16-B chunks (neighbouring threads share rows through L1 / L2) instead of being
// staged into a 128-wide MFMA tile of which 3 columns would be used.
constexpr int SMALL_COUT = 4;

__global__ __launch_bounds__(256) void conv3x3_small_kernel(ConvGeom g, conv_epilogue e, int nchw) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* wl = reinterpret_cast<bf16_t*>(smem);
    const int nw = g.Cout * g.K;                               // multiple of 8 (Cin % 8 == 0)
    for (int i = threadIdx.x * 8; i < nw; i += 256 * 8)
        *reinterpret_cast<u32x4*>(wl + i) = *reinterpret_cast<const u32x4*>(g.w + i);
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= g.M) return;
    const int hw = g.Ho * g.Wo, b = m / hw, pix = m - b * hw, oy = pix / g.Wo, ox = pix - oy * g.Wo;
    float acc[SMALL_COUT] = {0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        if ((unsigned)iy >= (unsigned)g.Ho || (unsigned)ix >= (unsigned)g.Wo) continue;
        if (g.up) {
            iy >>= 1;
            ix >>= 1;
        }
        const bf16_t* xp = g.x + (((int64_t)b * g.H + iy) * g.W + ix) * g.Cin;
        for (int c = 0; c < g.Cin; c += 8) {
            float xv[8];
            unpack8(*reinterpret_cast<const u32x4*>(xp + c), xv);
#pragma unroll
            for (int co = 0; co < SMALL_COUT; ++co) {
                if (co < g.Cout) {
                    float wv[8];
                    unpack8(*reinterpret_cast<const u32x4*>(wl + co * g.K + tap * g.Cin + c), wv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[co] = __builtin_fmaf(xv[e], wv[e], acc[co]);
                }
            }
        }
    }
#pragma unroll
    for (int co = 0; co < SMALL_COUT; ++co) {
        if (co >= g.Cout) break;
        float v = acc[co];
        if (e.bias) v += bf2f(e.bias[co]);
        v = rbf(v);
        if (e.silu) v = rbf(silu_f(v));
        if (e.res) v = rbf(v + bf2f(e.res[(int64_t)m * g.Cout + co]));
        const int64_t o = nchw ? ((int64_t)b * g.Cout + co) * hw + pix : (int64_t)m * g.Cout + co;
        e.y[o] = f2bf(v);
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
// The row walk is csrc/rownorm_lpr.hpp's; diffusers' RMSNorm rounds the normalised value, the weight product, the bias add and
// the residual add each on its own.
struct RmsnormBiasPost {
    typedef RowOutInPlace out_t;                           // y may be res
    const bf16_t* bias;
    const bf16_t* res;
    int relu;
    __device__ __forceinline__ void operator()(float* v, const float* w, int64_t off, int col) const {
        float bv[8], rv[8];
        if (bias) unpack8(*reinterpret_cast<const u32x4*>(bias + col), bv);
        if (res) unpack8(*reinterpret_cast<const u32x4*>(res + off), rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = rbf(rbf(v[e]) * w[e]);
            if (bias) t = rbf(t + bv[e]);
            if (res) t = rbf(t + rv[e]);
            if (relu) t = fmaxf(t, 0.f);
            v[e] = t;
        }
    }
};

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
    if (!y) return YAT_EINVAL;
    if (upsample != 0 && upsample != 1) return YAT_EINVAL;
    if (silu != 0 && silu != 1) return YAT_EINVAL;
    if (out_nchw != 0 && out_nchw != 1) return YAT_EINVAL;
    if (upsample && ((H | W) & 1)) return YAT_EINVAL;
    const bool small = Cout <= SMALL_COUT;
    if (!small && out_nchw) return YAT_EINVAL;
    conv_epilogue e{(const bf16_t*)bias, (const bf16_t*)shortcut, (const bf16_t*)residual, (bf16_t*)y, silu, shortcut_mode,
                    shortcut_channels, 1};
    if (shortcut_mode == 1) {
        if (!shortcut || shortcut_channels <= 0 || Cout % shortcut_channels) return YAT_EINVAL;
        e.sc_rep = Cout / shortcut_channels;
    } else if (shortcut_mode == 2) {
        if (!shortcut || shortcut_channels <= 0 || ((H | W) & 1) || (4 * Cout) % shortcut_channels) return YAT_EINVAL;
        e.sc_rep = 4 * Cout / shortcut_channels;
    } else if (shortcut_mode != 0) {
        return YAT_EINVAL;
    }
    if (small && shortcut_mode) return YAT_EINVAL;
    const int Hin = upsample ? H / 2 : H, Win = upsample ? W / 2 : W;
    if (small) {
        ConvGeom g;
        if (int rc = conv_geometry(g, B, Hin, Win, H, W, Cin, Cout, upsample, x, w)) return rc;
        if (g.w_bytes > 65536) return YAT_EINVAL;
        hipLaunchKernelGGL(conv3x3_small_kernel, dim3((unsigned)(((int64_t)g.M + 255) / 256)), dim3(256), (unsigned)g.w_bytes,
                           (hipStream_t)stream, g, e, out_nchw);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    }
    return conv3x3_launch<1, 1>(B, Hin, Win, H, W, Cin, Cout, upsample, x, w, e, stream);
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
    return launch_rownorm_lpr(M, D, eps, x, w, y, RowIdentity{}, RmsnormBiasPost{(const bf16_t*)b, (const bf16_t*)residual, relu},
                              (hipStream_t)stream);
}

int yat_dcae_image_to_uint8(int64_t n, const void* x, void* out, yat_stream_t stream) {
    if (n <= 0 || n > 0x7fffffffll || !x || !out) return YAT_EINVAL;
    hipLaunchKernelGGL(image_to_uint8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       (const bf16_t*)x, (uint8_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
