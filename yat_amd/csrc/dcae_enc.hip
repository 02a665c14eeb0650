// DC-AE encoder kernels (diffusers AutoencoderDC Encoder, the VAE encode of feature extraction: train_sana.py:78-82).
// Forward only, bf16 activations in NHWC, fp32 arithmetic inside every kernel.  Everything else the encoder needs is the
// decoder's (dcae.hip) or the GEMM / attention family.
//
//   conv3x3_down      DCDownBlock2d ("Conv" form): 3x3 conv, stride 2, pad 1, + bias, + the averaging shortcut
//                     pixel_unshuffle(x, 2).unflatten(1, (-1, g)).mean(2), g = 4 Cin / Cout, read from the conv's own input.
//   conv3x3_mean      Encoder.conv_out: 3x3 conv, stride 1, pad 1, + bias, + x.unflatten(1, (-1, Cin / Cout)).mean(2).
//   image_from_uint8  ToTensor -> Normalize(0.5, 0.5) -> bf16 of an [H, W, 3] uint8 image, padded to 8 channels.
//
// Both convs are the kernel of dcae_conv.hpp at stride S = 2 / 1, pad 1; only the epilogue is here.
#include "dcae_conv.hpp"

namespace {

// epilogue of 4 consecutive output channels n..n+3 of output pixel m: + bias -> bf16; shortcut mean in fp32 -> bf16;
// sum -> bf16.
//   S = 2: output channel o averages unshuffled channels u = o g .. o g + g - 1; unshuffled channel u is input channel u / 4
//          at offset (dy, dx) = ((u % 4) / 2, u % 2) of the 2 x 2 block of input pixels under output pixel (oy, ox).
//   S = 1: output channel o averages input channels o g .. o g + g - 1 of its own pixel.
template <int S>
struct enc_epilogue {
    const bf16_t* bias;   // [Cout] or null
    bf16_t* y;            // [B, Ho, Wo, Cout]
    int g;                // shortcut group size, 0 = no shortcut

    __device__ __forceinline__ void operator()(const ConvGeom& p, float (&v)[4], int m, int n) const {
        if (bias) {
            float bb[4];
            unpack4(*reinterpret_cast<const u32x2*>(bias + n), bb);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bb[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
        if (g) {
            int b, oy, ox;
            conv_pixel(p, m, b, oy, ox);
            const bf16_t* s = p.x + (((int64_t)b * p.H + S * oy) * p.W + S * ox) * p.Cin;
            const float inv = 1.0f / (float)g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = 0.f;
                const int u0 = (n + e) * g;
                for (int i = 0; i < g; ++i) {
                    const int u = u0 + i;
                    if (S == 2)
                        a += bf2f(s[((int64_t)((u & 3) >> 1) * p.W + (u & 1)) * p.Cin + (u >> 2)]);
                    else
                        a += bf2f(s[u]);
                }
                // g a power of two (every AutoencoderDC): a * (1 / g) is the exact fp32 quotient
                v[e] = rbf(v[e] + rbf((g & (g - 1)) ? a / (float)g : a * inv));
            }
        }
        *reinterpret_cast<u32x2*>(y + (int64_t)m * p.Cout + n) = pack4(v[0], v[1], v[2], v[3]);
    }
};

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

template <int S>
int enc_conv(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias, int shortcut, void* y,
             yat_stream_t stream) {
    if (Cin <= 0 || Cout <= 0 || !y) return YAT_EINVAL;
    if (shortcut != 0 && shortcut != 1) return YAT_EINVAL;
    if (S == 2 && ((H | W) & 1)) return YAT_EINVAL;
    const int64_t num = S == 2 ? 4ll * Cin : Cin;                       // channels the shortcut averages over, in all
    int g = 0;
    if (shortcut) {
        if (num % Cout) return YAT_EINVAL;
        g = (int)(num / Cout);
    }
    return conv3x3_launch<S, 1>(B, H, W, H / S, W / S, Cin, Cout, 0, x, w,
                                       enc_epilogue<S>{(const bf16_t*)bias, (bf16_t*)y, g}, stream);
}

}  // namespace

extern "C" {

int yat_dcae_conv3x3_down(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias,
                          int shortcut, void* y, yat_stream_t stream) {
    return enc_conv<2>(B, H, W, Cin, Cout, x, w, bias, shortcut, y, stream);
}

int yat_dcae_conv3x3_mean(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias,
                          int shortcut, void* y, yat_stream_t stream) {
    return enc_conv<1>(B, H, W, Cin, Cout, x, w, bias, shortcut, y, stream);
}

int yat_dcae_image_from_uint8(int64_t npix, const void* x, const void* table, void* out, yat_stream_t stream) {
    if (npix <= 0 || npix > 0x0fffffffll || !x || !table || !out) return YAT_EINVAL;
    hipLaunchKernelGGL(image_from_uint8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       npix, (const uint8_t*)x, (const bf16_t*)table, (bf16_t*)out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
