// AutoencoderKL encoder kernels (diffusers AutoencoderKL.encode, the VAE encode of the PixArt-Sigma and SD3.5 feature
// extraction: train_pixart_sigma.py:61-66, train_sd35.py:63-77).  Forward only, bf16 activations, fp32 arithmetic inside
// every kernel.  Everything else the encoder needs is the decoder's (vae_kl.hip), the DC-AE convs or the GEMM family.
//
//   conv3x3_down   Downsample2D of DownEncoderBlock2D: F.pad(x, (0, 1, 0, 1)) -> 3x3 conv, stride 2, no padding, + bias.
//   kl_sample      DiagonalGaussianDistribution(moments).sample() / .mode() plus the trainers' shift and scale, NHWC
//                  moments -> NCHW latent.
//
// The conv is the kernel of dcae_conv.hpp at stride 2, pad 0 (input pixel (2 oy + ty, 2 ox + tx): the DC-AE down conv's
// without its pad-1 offset, so only the bottom row and the right column can fall outside the image); only the plain
// epilogue is here.
#include "dcae_conv.hpp"
#include <math.h>

namespace {

struct bias_store {
    const bf16_t* bias;   // [Cout] or null
    bf16_t* y;            // [B, H/2, W/2, Cout]

    __device__ __forceinline__ void operator()(const ConvGeom& g, float (&v)[4], int m, int n) const {
        if (bias) {
            float bb[4];
            unpack4(*reinterpret_cast<const u32x2*>(bias + n), bb);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bb[e];
        }
        *reinterpret_cast<u32x2*>(y + (int64_t)m * g.Cout + n) = pack4(v[0], v[1], v[2], v[3]);
    }
};

// ------------------------------------------------------------------------------------------------------------ kl_sample
// One thread per (pixel, group of 4 latent channels): the 16-B chunk of the pixel's row that holds the 4 means and the one
// that holds the 4 logvars (the same chunk when L = 4), then 4 noise loads and 4 stores, each contiguous along HW over the
// lanes.  grid: (HW / 256, L / 4, B).
__device__ __forceinline__ u32x2 half_of(const u32x4& v, int hi) { return hi ? u32x2{v[2], v[3]} : u32x2{v[0], v[1]}; }

__global__ __launch_bounds__(256) void kl_sample_kernel(int HW, int L, int ld, const bf16_t* __restrict__ moments,
                                                        const bf16_t* __restrict__ noise, int apply_shift, float shift,
                                                        float scale, bf16_t* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int c0 = 4 * blockIdx.y, b = blockIdx.z;
    const bf16_t* row = moments + ((int64_t)b * HW + pix) * ld;
    const int cm = c0, cl = L + c0;                                 // first mean / logvar column: multiples of 4
    float mean[4], lv[4];
    unpack4(half_of(*reinterpret_cast<const u32x4*>(row + (cm & ~7)), cm & 4), mean);
    unpack4(half_of(*reinterpret_cast<const u32x4*>(row + (cl & ~7)), cl & 4), lv);
    const int64_t o = ((int64_t)b * L + c0) * HW + pix;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = mean[e];
        if (noise) {
            const float l = lv[e] < -30.0f ? -30.0f : (lv[e] > 20.0f ? 20.0f : lv[e]);      // torch.clamp: NaN stays NaN
            const float sd = rbf(expf(rbf(0.5f * l)));
            x = rbf(x + rbf(sd * bf2f(noise[o + (int64_t)e * HW])));
        }
        if (apply_shift) x = rbf(x - shift);
        out[o + (int64_t)e * HW] = f2bf(x * scale);
    }
}

}  // namespace

extern "C" {

int yat_vae_conv3x3_down(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias, void* y,
                         yat_stream_t stream) {
    if (!y || ((H | W) & 1)) return YAT_EINVAL;
    return conv3x3_launch<2, 0>(B, H, W, H / 2, W / 2, Cin, Cout, 0, x, w, bias_store{(const bf16_t*)bias, (bf16_t*)y},
                                       stream);
}

int yat_vae_kl_sample(int B, int HW, int L, int ld, const void* moments, const void* noise, int apply_shift, float shift,
                      float scale, void* out, yat_stream_t stream) {
    if (B <= 0 || HW <= 0 || L <= 0 || (L & 3) || (ld & 7) || ld < 2 * (int64_t)L || !moments || !out) return YAT_EINVAL;
    if (apply_shift != 0 && apply_shift != 1) return YAT_EINVAL;
    if (((uintptr_t)moments & 15) || ((uintptr_t)noise & 1) || ((uintptr_t)out & 1)) return YAT_EINVAL;
    if (B > 65535 || L / 4 > 65535 || (int64_t)B * HW * ld > 0x7fffffffll) return YAT_EINVAL;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(L / 4), (unsigned)B);
    hipLaunchKernelGGL(kl_sample_kernel, grid, dim3(256), 0, (hipStream_t)stream, HW, L, ld, (const bf16_t*)moments,
                       (const bf16_t*)noise, apply_shift, shift, scale, (bf16_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
