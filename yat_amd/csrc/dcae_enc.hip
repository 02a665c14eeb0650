// DC-AE encoder kernels (diffusers AutoencoderDC Encoder, the VAE encode of feature extraction: train_sana.py:78-82).
// Forward only, bf16 activations in NHWC, fp32 arithmetic inside every kernel.  Everything else the encoder needs is the
// decoder's (dcae.hip) or the GEMM / attention family.
//
//   conv3x3_down      DCDownBlock2d ("Conv" form): 3x3 conv, stride 2, pad 1, + bias, + the averaging shortcut
//                     pixel_unshuffle(x, 2).unflatten(1, (-1, g)).mean(2), g = 4 Cin / Cout, read from the conv's own input.
//   conv3x3_mean      Encoder.conv_out: 3x3 conv, stride 1, pad 1, + bias, + x.unflatten(1, (-1, Cin / Cout)).mean(2).
//   image_from_uint8  ToTensor -> Normalize(0.5, 0.5) -> bf16 of an [H, W, 3] uint8 image, padded to 8 channels.
//
// Both convs are the implicit GEMM of dcae_conv.hpp (M = output pixels, N = Cout, K = 9 Cin); only the A-operand address
// math (input pixel (S oy + ty - 1, S ox + tx - 1), S = stride) and the epilogue are here.
#include "dcae_conv.hpp"

namespace {

struct EncP {
    const bf16_t* x;      // [B, H, W, Cin]
    const bf16_t* w;      // [Cout, 9 * Cin]
    const bf16_t* bias;   // [Cout] or null
    bf16_t* y;            // [B, Ho, Wo, Cout]
    int B, H, W, Ho, Wo, Cin, Cout, g;                  // g: shortcut group size, 0 = no shortcut
    int M, K, nbm, nbn;
    uint64_t x_bytes, w_bytes;
};

template <int S, bool TAPU>
__device__ __forceinline__ void enc_stage_a(const EncP& p, __amdgpu_buffer_rsrc_t rx, char* lds, int k0, int wave,
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
        const int iy = ry[j] + t3 - 1, ix = rxx[j] + (tap - 3 * t3) - 1;      // ry, rxx already hold S * oy, S * ox
        const bool ok = kg < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const uint32_t voff = ok ? (uint32_t)((((int64_t)(rb[j] + iy) * p.W + ix) * p.Cin + ci) * 2) : YAT_OOB;
        lds_dma16(rx, (YAT_LDS void*)(lds + piece * 1024), voff);
    }
}

// epilogue of 4 consecutive output channels n..n+3 of output pixel m: + bias -> bf16; shortcut mean in fp32 -> bf16;
// sum -> bf16.
//   S = 2: output channel o averages unshuffled channels u = o g .. o g + g - 1; unshuffled channel u is input channel u / 4
//          at offset (dy, dx) = ((u % 4) / 2, u % 2) of the 2 x 2 block of input pixels under output pixel (oy, ox).
//   S = 1: output channel o averages input channels o g .. o g + g - 1 of its own pixel.
template <int S>
__device__ __forceinline__ void enc_epilogue(const EncP& p, float (&v)[4], int m, int n) {
    if (p.bias) {
        float bb[4];
        unpack4(*reinterpret_cast<const u32x2*>(p.bias + n), bb);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bb[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
    if (p.g) {
        const int hw = p.Ho * p.Wo, b = m / hw, pix = m - b * hw, oy = pix / p.Wo, ox = pix - oy * p.Wo;
        const bf16_t* s = p.x + (((int64_t)b * p.H + S * oy) * p.W + S * ox) * p.Cin;
        const float inv = 1.0f / (float)p.g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = 0.f;
            const int u0 = (n + e) * p.g;
            for (int i = 0; i < p.g; ++i) {
                const int u = u0 + i;
                if (S == 2)
                    a += bf2f(s[((int64_t)((u & 3) >> 1) * p.W + (u & 1)) * p.Cin + (u >> 2)]);
                else
                    a += bf2f(s[u]);
            }
            // g a power of two (every AutoencoderDC): a * (1 / g) is the exact fp32 quotient
            v[e] = rbf(v[e] + rbf((p.g & (p.g - 1)) ? a / (float)p.g : a * inv));
        }
    }
    *reinterpret_cast<u32x2*>(p.y + (int64_t)m * p.Cout + n) = pack4(v[0], v[1], v[2], v[3]);
}

template <int S, bool TAPU>
__global__ __launch_bounds__(256, 2) void conv3x3_enc_kernel(EncP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    int m0, n0;
    conv_tile_origin(p.nbm, p.nbn, m0, n0);

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

    // this lane's four A rows (output pixels): image row base, S * oy, S * ox, and the source chunk of each LDS slot
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
            ry[j] = S * oy;
            rxx[j] = S * (pix - oy * p.Wo);
        } else {
            rb[j] = 0;
            ry[j] = -4;                                  // every tap out of range -> zeros
            rxx[j] = 0;
        }
    }

    f32x4 acc[4][4];
    conv_mainloop(smem, rw, p.Cout, p.K, n0, wave, lane, acc,
                  [&](char* lds, int k0) { enc_stage_a<S, TAPU>(p, rx, lds, k0, wave, rb, ry, rxx, cc); });

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= p.Cout) continue;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            enc_epilogue<S>(p, v, m, n);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- image_from_uint8
// One pixel per thread: 3 bytes in, one 16-B store out.  The 256 possible values come from a table the host fills with
// torch's own ((u / 255) - 0.5) / 0.5 -> bf16, so the result is torch's for every input by construction.
__global__ __launch_bounds__(256) void image_from_uint8_kernel(int64_t npix, const uint8_t* __restrict__ x,
                                                               const bf16_t* __restrict__ table, bf16_t* __restrict__ y) {
    __shared__ bf16_t t[256];
    t[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const uint32_t r = t[x[3 * i]], g = t[x[3 * i + 1]], b = t[x[3 * i + 2]];
    *reinterpret_cast<u32x4*>(y + 8 * i) = u32x4{r | (g << 16), b, 0u, 0u};
}

int enc_conv(int S, int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias, int shortcut,
             void* y, yat_stream_t stream) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 7) || (Cout & 3) || !x || !w || !y) return YAT_EINVAL;
    if (shortcut != 0 && shortcut != 1) return YAT_EINVAL;
    if (S == 2 && ((H | W) & 1)) return YAT_EINVAL;
    const int64_t num = S == 2 ? 4ll * Cin : Cin;                       // channels the shortcut averages over, in all
    int g = 0;
    if (shortcut) {
        if (num % Cout) return YAT_EINVAL;
        g = (int)(num / Cout);
    }
    const int Ho = H / S, Wo = W / S;
    const int64_t M = (int64_t)B * Ho * Wo;
    const uint64_t x_bytes = (uint64_t)B * H * W * Cin * 2, w_bytes = (uint64_t)Cout * 9 * Cin * 2;
    if (M > 0x7fffffffll || x_bytes > 0x7fffffffull || w_bytes > 0x7fffffffull) return YAT_EINVAL;
    EncP p{};
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.bias = (const bf16_t*)bias; p.y = (bf16_t*)y;
    p.B = B; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin; p.Cout = Cout; p.g = g;
    p.M = (int)M; p.K = 9 * Cin; p.x_bytes = x_bytes; p.w_bytes = w_bytes;
    p.nbm = (int)((M + CBM - 1) / CBM);
    p.nbn = (Cout + CBN - 1) / CBN;
    if ((int64_t)p.nbm * p.nbn > 0x7fffffffll) return YAT_EINVAL;
    const dim3 grid((unsigned)(p.nbm * p.nbn));
    const bool tapu = Cin % 64 == 0;
    if (S == 2) {
        if (tapu) hipLaunchKernelGGL((conv3x3_enc_kernel<2, true>), grid, dim3(256), CLDS, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((conv3x3_enc_kernel<2, false>), grid, dim3(256), CLDS, (hipStream_t)stream, p);
    } else {
        if (tapu) hipLaunchKernelGGL((conv3x3_enc_kernel<1, true>), grid, dim3(256), CLDS, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((conv3x3_enc_kernel<1, false>), grid, dim3(256), CLDS, (hipStream_t)stream, p);
    }
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // namespace

extern "C" {

int yat_dcae_conv3x3_down(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias,
                          int shortcut, void* y, yat_stream_t stream) {
    return enc_conv(2, B, H, W, Cin, Cout, x, w, bias, shortcut, y, stream);
}

int yat_dcae_conv3x3_mean(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias,
                          int shortcut, void* y, yat_stream_t stream) {
    return enc_conv(1, B, H, W, Cin, Cout, x, w, bias, shortcut, y, stream);
}

int yat_dcae_image_from_uint8(int64_t npix, const void* x, const void* table, void* out, yat_stream_t stream) {
    if (npix <= 0 || npix > 0x0fffffffll || !x || !table || !out) return YAT_EINVAL;
    hipLaunchKernelGGL(image_from_uint8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       npix, (const uint8_t*)x, (const bf16_t*)table, (bf16_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
