// AutoencoderKL encoder kernels (diffusers AutoencoderKL.encode, the VAE encode of the PixArt-Sigma and SD3.5 feature
// extraction: train_pixart_sigma.py:61-66, train_sd35.py:63-77).  Forward only, bf16 activations, fp32 arithmetic inside
// every kernel.  Everything else the encoder needs is the decoder's (vae_kl.hip), the DC-AE convs or the GEMM family.
//
//   conv3x3_down   Downsample2D of DownEncoderBlock2D: F.pad(x, (0, 1, 0, 1)) -> 3x3 conv, stride 2, no padding, + bias.
//   kl_sample      DiagonalGaussianDistribution(moments).sample() / .mode() plus the trainers' shift and scale, NHWC
//                  moments -> NCHW latent.
//
// The conv is the implicit GEMM of dcae_conv.hpp (M = output pixels, N = Cout, K = 9 Cin); only the A-operand address math
// (input pixel (2 oy + ty, 2 ox + tx): the DC-AE down conv's without its pad-1 offset, so only the bottom row and the right
// column can fall outside the image) and the plain epilogue are here.
#include "dcae_conv.hpp"
#include <math.h>

namespace {

struct DownP {
    const bf16_t* x;      // [B, H, W, Cin]
    const bf16_t* w;      // [Cout, 9 * Cin]
    const bf16_t* bias;   // [Cout] or null
    bf16_t* y;            // [B, H/2, W/2, Cout]
    int H, W, Ho, Wo, Cin, Cout;
    int M, K, nbm, nbn;
    uint64_t x_bytes, w_bytes;
};

template <bool TAPU>
__device__ __forceinline__ void down_stage_a(const DownP& p, __amdgpu_buffer_rsrc_t rx, char* lds, int k0, int wave,
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
        const int iy = ry[j] + t3, ix = rxx[j] + (tap - 3 * t3);               // ry, rxx hold 2 oy, 2 ox: no pad offset
        const bool ok = kg < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const uint32_t voff = ok ? (uint32_t)((((int64_t)(rb[j] + iy) * p.W + ix) * p.Cin + ci) * 2) : YAT_OOB;
        lds_dma16(rx, (YAT_LDS void*)(lds + piece * 1024), voff);
    }
}

template <bool TAPU>
__global__ __launch_bounds__(256, 2) void vae_conv3x3_down_kernel(DownP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    int m0, n0;
    conv_tile_origin(p.nbm, p.nbn, m0, n0);

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

    // this lane's four A rows (output pixels): image row base, 2 oy, 2 ox, and the source chunk of each LDS slot
    int rb[4], ry[4], rxx[4], cc[4];
    const int hw = p.Ho * p.Wo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (j * 4 + wave) * 8 + (lane >> 3);
        const int m = m0 + r;
        cc[j] = swz128(r, lane & 7);
        if (m < p.M) {
            const int b = m / hw, pix = m - b * hw, oy = pix / p.Wo;
            rb[j] = b * p.H;
            ry[j] = 2 * oy;
            rxx[j] = 2 * (pix - oy * p.Wo);
        } else {
            rb[j] = 0;
            ry[j] = -4;                                  // iy = -4 + (0 .. 2) < 0 for every tap -> zeros
            rxx[j] = 0;
        }
    }

    f32x4 acc[4][4];
    conv_mainloop(smem, rw, p.Cout, p.K, n0, wave, lane, acc,
                  [&](char* lds, int k0) { down_stage_a<TAPU>(p, rx, lds, k0, wave, rb, ry, rxx, cc); });

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= p.Cout) continue;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (p.bias) {
                float bb[4];
                unpack4(*reinterpret_cast<const u32x2*>(p.bias + n), bb);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += bb[e];
            }
            *reinterpret_cast<u32x2*>(p.y + (int64_t)m * p.Cout + n) = pack4(v[0], v[1], v[2], v[3]);
        }
    }
}

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
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 7) || (Cout & 3) || !x || !w || !y) return YAT_EINVAL;
    if ((H | W) & 1) return YAT_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    const int64_t M = (int64_t)B * Ho * Wo;
    const uint64_t x_bytes = (uint64_t)B * H * W * Cin * 2, w_bytes = (uint64_t)Cout * 9 * Cin * 2;
    if (M > 0x7fffffffll || x_bytes > 0x7fffffffull || w_bytes > 0x7fffffffull) return YAT_EINVAL;
    DownP p{};
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.bias = (const bf16_t*)bias; p.y = (bf16_t*)y;
    p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin; p.Cout = Cout;
    p.M = (int)M; p.K = 9 * Cin; p.x_bytes = x_bytes; p.w_bytes = w_bytes;
    p.nbm = (int)((M + CBM - 1) / CBM);
    p.nbn = (Cout + CBN - 1) / CBN;
    if ((int64_t)p.nbm * p.nbn > 0x7fffffffll) return YAT_EINVAL;
    const dim3 grid((unsigned)(p.nbm * p.nbn));
    if (Cin % 64 == 0) hipLaunchKernelGGL((vae_conv3x3_down_kernel<true>), grid, dim3(256), CLDS, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((vae_conv3x3_down_kernel<false>), grid, dim3(256), CLDS, (hipStream_t)stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
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
