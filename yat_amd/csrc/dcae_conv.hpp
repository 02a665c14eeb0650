// The 3x3 implicit-GEMM convolution of the VAE halves: one kernel (conv3x3_tile_kernel) and one host launcher
// (conv3x3_launch), instantiated by the DC-AE decoder (dcae.hip), the DC-AE encoder (dcae_enc.hip) and the AutoencoderKL
// encoder's Downsample2D (vae_kl_enc.hip).  M = output pixels, N = Cout, K = 9 Cin, weights [Cout, 3, 3, Cin].
//
// Geometry (template parameters): tap (ty, tx) of output pixel (oy, ox) reads input pixel (S oy + ty - P, S ox + tx - P),
// S = stride, P = padding.  TAPU: Cin % 64 == 0, a whole K-tile lies in one tap.  At stride 1 the geometry's run-time flag
// ``up`` makes the input the nearest x2 upsample of the stored image (the bounds test sees the upsampled image, the address
// its half-resolution source).
//
//   user                                   S  P  up       epilogue (a functor passed by value, called per 4 channels)
//   yat_dcae_conv3x3      (dcae.hip)       1  1  0 or 1   bias, SiLU, two repeat shortcuts, residual
//   yat_dcae_conv3x3_mean (dcae_enc.hip)   1  1  0        bias, channel-group-mean shortcut
//   yat_dcae_conv3x3_down (dcae_enc.hip)   2  1  0        bias, pixel-unshuffle group-mean shortcut
//   yat_vae_conv3x3_down  (vae_kl_enc.hip) 2  0  0        bias
//
// 128 x 128 x 64 tile, 4 waves (2 x 2), each wave 64 x 64 = 4 x 4 MFMA 16x16x32 accumulators.  Both operands move
// HBM -> LDS by LDS-DMA (16 B per lane), double-buffered, one barrier per K-tile.  The A operand (im2col rows) is never
// materialised: conv_stage_a issues, per 16-B chunk, the load of its K slice of its row's input pixel; taps outside
// the image (zero padding), rows past M and K past 9 Cin are predicated to the buffer descriptor's out-of-range offset,
// which the hardware returns as zeros.  Cin % 8 == 0, so a 16-B chunk never straddles two taps.  The K loop and with it the
// MFMA order are the same for every user.
// LDS images are lane-linear with the XOR swizzle applied to the source chunk (common.hpp swz128) and undone on the read.
#pragma once
#include "common.hpp"

constexpr int CBM = 128, CBN = 128, CBK = 64;
constexpr int CSTAGE = (CBM * CBK + CBN * CBK) * 2;  // 32 KiB
constexpr int CLDS = 2 * CSTAGE;                     // 64 KiB -> 2 workgroups / CU

struct ConvGeom {
    const bf16_t* x;      // [B, H, W, Cin], the stored input
    const bf16_t* w;      // [Cout, 9 * Cin]
    int H, W, Ho, Wo;     // stored input and output grid
    int Cin, Cout, up;    // up: the input is the nearest x2 upsample of x (stride 1 only)
    int M, K, nbm, nbn;   // M = B Ho Wo, K = 9 Cin, tiles along M and N
    uint64_t x_bytes, w_bytes;
};

// output pixel m -> image b, row oy, column ox
__device__ __forceinline__ void conv_pixel(const ConvGeom& g, int m, int& b, int& oy, int& ox) {
    const int hw = g.Ho * g.Wo;
    b = m / hw;
    const int pix = m - b * hw;
    oy = pix / g.Wo;
    ox = pix - oy * g.Wo;
}

// XCD-contiguous tile order, N fastest: the Cout / 128 tiles of one pixel band share its input rows in one L2
__device__ __forceinline__ void conv_tile_origin(int nbm, int nbn, int& m0, int& n0) {
    const int nwg = nbm * nbn;
    int id;
    {
        const int orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    const int tm = id / nbn, tn = id - tm * nbn;
    m0 = tm * CBM;
    n0 = tn * CBN;
}

// weights [Cout, K] (K = 9 Cin contiguous), rows n0 .. n0 + 127, columns k0 .. k0 + 63
__device__ __forceinline__ void conv_stage_b(int Cout, int K, __amdgpu_buffer_rsrc_t rw, char* lds, int n0, int k0, int wave,
                                             int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int piece = j * 4 + wave;
        const int r = piece * 8 + (lane >> 3);
        const int c = swz128(r, lane & 7);
        const int gn = n0 + r, gk = k0 + c * 8;
        const uint32_t voff = (gn < Cout && gk < K) ? (uint32_t)(((int64_t)gn * K + gk) * 2) : YAT_OOB;
        lds_dma16(rw, (YAT_LDS void*)(lds + piece * 1024), voff);
    }
}

__device__ __forceinline__ bf16x8 conv_frag(const char* lds, int idx0, int kk, int lane) {
    const uint32_t r = idx0 + (lane & 15);
    const uint32_t c = swz128(r, kk * 4 + (lane >> 4));
    return lds_read8(lds, r * 128 + c * 16);
}

// acc[i][j] += A-tile x B-tile over all of K.  After it lane owns, in acc[i][j][0..3], pixel
// m = m0 + wm * 64 + i * 16 + (lane & 15) and output channels n = n0 + wn * 64 + j * 16 + 4 (lane >> 4) + 0..3.
template <class StageA>
__device__ __forceinline__ void conv_mainloop(char* smem, __amdgpu_buffer_rsrc_t rw, int Cout, int K, int n0, int wave,
                                              int lane, f32x4 (&acc)[4][4], StageA&& stage_a) {
    const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nt = (K + CBK - 1) / CBK;
    stage_a(smem, 0);
    conv_stage_b(Cout, K, rw, smem + CBM * CBK * 2, n0, 0, wave, lane);

    for (int t = 0; t < nt; ++t) {
        char* cur = smem + (t & 1) * CSTAGE;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // tile t landed for every wave; every wave is done reading the other buffer
        if (t + 1 < nt) {
            char* nxt = smem + ((t + 1) & 1) * CSTAGE;
            stage_a(nxt, (t + 1) * CBK);
            conv_stage_b(Cout, K, rw, nxt + CBM * CBK * 2, n0, (t + 1) * CBK, wave, lane);
        }
        const char* la = cur;
        const char* lb = cur + CBM * CBK * 2;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = conv_frag(la, wm * 64 + i * 16, kk, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = conv_frag(lb, wn * 64 + j * 16, kk, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);  // D[n][m]
        }
    }
}

// rows m0 .. m0 + 127 of the im2col matrix, columns k0 .. k0 + 63.  rb / ry / rxx: b * H, S * oy, S * ox of the lane's row
template <int S, int P, bool TAPU>
__device__ __forceinline__ void conv_stage_a(const ConvGeom& g, __amdgpu_buffer_rsrc_t rx, char* lds, int k0, int wave,
                                             const int (&rb)[4], const int (&ry)[4], const int (&rxx)[4], const int (&cc)[4]) {
    // the image the taps see: at stride 1 (pad 1) it has the output's size, upsampled or not
    const int Hv = S == 1 ? g.Ho : g.H, Wv = S == 1 ? g.Wo : g.W;
    int tapu = 0, ciu = 0;
    if (TAPU) {                                        // Cin % 64 == 0: the whole K-tile lies in one tap
        tapu = k0 / g.Cin;
        ciu = k0 - tapu * g.Cin;
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
            tap = kg / g.Cin;
            ci = kg - tap * g.Cin;
        }
        const int t3 = tap / 3;
        int iy = ry[j] + t3 - P, ix = rxx[j] + (tap - 3 * t3) - P;
        const bool ok = kg < g.K && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
        if (S == 1 && g.up) {                          // after the bounds test: row -1 must not become row 0
            iy >>= 1;
            ix >>= 1;
        }
        const uint32_t voff = ok ? (uint32_t)((((int64_t)(rb[j] + iy) * g.W + ix) * g.Cin + ci) * 2) : YAT_OOB;
        lds_dma16(rx, (YAT_LDS void*)(lds + piece * 1024), voff);
    }
}

// epi(g, v, m, n): the epilogue of output channels n .. n + 3 (accumulators v) of output pixel m, store included
template <int S, int P, bool TAPU, class Epi>
__global__ __launch_bounds__(256, 2) void conv3x3_tile_kernel(ConvGeom g, Epi epi) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    int m0, n0;
    conv_tile_origin(g.nbm, g.nbn, m0, n0);

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(g.x, g.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.w, g.w_bytes);

    // this lane's four A rows (output pixels): image row base, S * oy, S * ox, and the source chunk of each LDS slot
    int rb[4], ry[4], rxx[4], cc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (j * 4 + wave) * 8 + (lane >> 3);
        const int m = m0 + r;
        cc[j] = swz128(r, lane & 7);
        if (m < g.M) {
            int b, oy, ox;
            conv_pixel(g, m, b, oy, ox);
            rb[j] = b * g.H;
            ry[j] = S * oy;
            rxx[j] = S * ox;
        } else {
            rb[j] = 0;
            ry[j] = -4;                                  // iy = -4 + (0 .. 2) - P < 0 for every tap -> zeros
            rxx[j] = 0;
        }
    }

    f32x4 acc[4][4];
    conv_mainloop(smem, rw, g.Cout, g.K, n0, wave, lane, acc,
                  [&](char* lds, int k0) { conv_stage_a<S, P, TAPU>(g, rx, lds, k0, wave, rb, ry, rxx, cc); });

    // lane owns pixel m = .. + (lane & 15) and output channels n = .. + 4 (lane >> 4) + 0..3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= g.Cout) continue;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            epi(g, v, m, n);
        }
    }
}

// The geometry of a conv of x [B, H, W, Cin] to an output grid Ho x Wo (everything but the tile counts), with the limits
// every kernel on it shares: 32-bit pixel index, buffer descriptors and byte offsets below 2 GiB.
inline int conv_geometry(ConvGeom& g, int B, int H, int W, int Ho, int Wo, int Cin, int Cout, int up, const void* x,
                         const void* w) {
    if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 7) || !x || !w) return YAT_EINVAL;
    const int64_t M = (int64_t)B * Ho * Wo;
    const uint64_t x_bytes = (uint64_t)B * H * W * Cin * 2, w_bytes = (uint64_t)Cout * 9 * Cin * 2;
    if (M > 0x7fffffffll || x_bytes > 0x7fffffffull || w_bytes > 0x7fffffffull) return YAT_EINVAL;
    g = ConvGeom{(const bf16_t*)x, (const bf16_t*)w, H, W, Ho, Wo, Cin, Cout, up, (int)M, 9 * Cin, 0, 0, x_bytes, w_bytes};
    return YAT_OK;
}

template <int S, int P, class Epi>
int conv3x3_launch(int B, int H, int W, int Ho, int Wo, int Cin, int Cout, int up, const void* x, const void* w,
                   const Epi& epi, yat_stream_t stream) {
    static_assert(P == 1 || S != 1, "the stride-1 bounds test assumes pad 1");
    ConvGeom g;
    if (int rc = conv_geometry(g, B, H, W, Ho, Wo, Cin, Cout, up, x, w)) return rc;
    if (Cout & 3) return YAT_EINVAL;
    g.nbm = (int)(((int64_t)g.M + CBM - 1) / CBM);
    g.nbn = (Cout + CBN - 1) / CBN;
    if ((int64_t)g.nbm * g.nbn > 0x7fffffffll) return YAT_EINVAL;
    const dim3 grid((unsigned)(g.nbm * g.nbn));
    if (Cin % 64 == 0)
        hipLaunchKernelGGL((conv3x3_tile_kernel<S, P, true, Epi>), grid, dim3(256), CLDS, (hipStream_t)stream, g, epi);
    else
        hipLaunchKernelGGL((conv3x3_tile_kernel<S, P, false, Epi>), grid, dim3(256), CLDS, (hipStream_t)stream, g, epi);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}
