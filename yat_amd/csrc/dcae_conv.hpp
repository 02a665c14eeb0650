// The 3x3 implicit-GEMM tile shared by the DC-AE decoder convs (dcae.hip) and the encoder convs (dcae_enc.hip).
//
// 128 x 128 x 64 tile, 4 waves (2 x 2), each wave 64 x 64 = 4 x 4 MFMA 16x16x32 accumulators.  Both operands move
// HBM -> LDS by LDS-DMA (16 B per lane), double-buffered, one barrier per K-tile.  The A operand (im2col rows) is never
// materialised: the kernel passes a ``stage_a(lds, k0)`` functor that issues, per 16-B chunk, the load of its K slice of
// its row's input pixel (the decoder and the encoder differ only in that address math and in the epilogue); taps outside
// the image (zero padding), rows past M and K past 9 Cin are predicated to the buffer descriptor's out-of-range offset,
// which the hardware returns as zeros.  Cin % 8 == 0, so a 16-B chunk never straddles two taps.
// LDS images are lane-linear with the XOR swizzle applied to the source chunk (common.hpp swz128) and undone on the read.
#pragma once
#include "common.hpp"

constexpr int CBM = 128, CBN = 128, CBK = 64;
constexpr int CSTAGE = (CBM * CBK + CBN * CBK) * 2;  // 32 KiB
constexpr int CLDS = 2 * CSTAGE;                     // 64 KiB -> 2 workgroups / CU

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
