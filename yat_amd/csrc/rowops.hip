// HBM-bound row kernels of the SANA block for gfx950: LayerNorm+adaLN modulate, RMSNorm, the
// modulation table, gated-residual backward and bias-gradient column sums.
//
// Common shape: one 64-lane wave owns one row (<= 4096 bf16), 16-B loads per lane, the row lives
// in registers between the statistics pass and the output pass (one HBM read, one write), fp32
// math, wave shuffles for the row reductions.  Column reductions (dshift/dscale/dgate/dbias/dw)
// are accumulated per wave in registers over a group of rows, written as fp32 partial rows to a
// caller-provided workspace and finished by one small reduce kernel -- no atomics, bit-reproducible.
#include <type_traits>
#include "common.hpp"
#include "../../include/yat_hip.h"

namespace {

constexpr int ROWS_PER_WAVE = 4;     // rows a wave walks in the backward kernels
constexpr int WAVES = 4;             // 256-thread blocks

template <int MAXV>
__device__ __forceinline__ void load_row(const bf16_t* p, int nchunk, int lane, float (&v)[MAXV][8]) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) {
            unpack8(*reinterpret_cast<const u32x4*>(p + c * 8), v[i]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        }
    }
}

// ------------------------------------------------------------------ LN + modulate forward
template <int MAXV>
__global__ __launch_bounds__(256) void ln_mod_fwd_kernel(int M, int D, int rpb, float eps, const bf16_t* x,
                                                         const bf16_t* shift, const bf16_t* scale, int mod_ld,
                                                         bf16_t* y, float* mean_out, float* rstd_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * WAVES + wave;
    if (row >= M) return;
    const int nchunk = D >> 3;
    float v[MAXV][8];
    load_row<MAXV>(x + (int64_t)row * D, nchunk, lane, v);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[i][e];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (lane + 64 * i < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { float d = v[i][e] - mean; q += d * d; }
        }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    const int b = row / rpb;
    const bf16_t* sh = shift + (int64_t)b * mod_ld;
    const bf16_t* sc = scale + (int64_t)b * mod_ld;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) {
            float a[8], g[8], o[8];
            unpack8(*reinterpret_cast<const u32x4*>(sh + c * 8), a);
            unpack8(*reinterpret_cast<const u32x4*>(sc + c * 8), g);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = rbf((v[i][e] - mean) * rstd);      // F.layer_norm output (bf16)
                o[e] = rbf(xh * rbf(1.0f + g[e])) + a[e];           // * (1 + scale) + shift
            }
            *reinterpret_cast<u32x4*>(y + (int64_t)row * D + c * 8) = pack8(o);
        }
    }
}

// ------------------------------------------------------------------ LN + modulate backward
// Two light kernels instead of one register-heavy one (the fused version held x, dy, (1+scale) and both column
// accumulators per lane: ~230 VGPRs, 1-2 waves/SIMD, 2 TB/s):
//  (a) row pass, one wave per row, two streaming sweeps (the second one hits L1/L2): dx = dres + LN'(dy * (1+scale));
//  (b) column pass (strip layout: a lane owns 8 columns and walks 32 rows, row statistics are wave-uniform scalars):
//      dshift += sum_n dy, dscale += sum_n dy * bf16(xhat).  x and dy come back from L2 / Infinity Cache.
template <int MAXV>
__global__ __launch_bounds__(256) void ln_mod_bwd_rows_kernel(int M, int D, int rpb, const bf16_t* x, const float* mean_in,
                                                              const float* rstd_in, const bf16_t* scale, int mod_ld,
                                                              const bf16_t* dy, const bf16_t* dres, bf16_t* dx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * WAVES + wave;
    if (row >= M) return;
    const int nchunk = D >> 3;
    const bf16_t* sc = scale + (int64_t)(row / rpb) * mod_ld;
    const bf16_t* xr = x + (int64_t)row * D;
    const bf16_t* gr = dy + (int64_t)row * D;
    const float mean = mean_in[row], rstd = rstd_in[row];
    // pass 1: the two row reductions (streamed, nothing kept)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) {
            float xv[8], gv[8], sv[8];
            unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), xv);
            unpack8(*reinterpret_cast<const u32x4*>(gr + c * 8), gv);
            unpack8(*reinterpret_cast<const u32x4*>(sc + c * 8), sv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (xv[e] - mean) * rstd;
                const float gg = rbf(gv[e] * rbf(1.0f + sv[e]));       // grad wrt the LN output (bf16 mul in autograd)
                s1 += gg;
                s2 += gg * xh;
            }
        }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
    // pass 2: re-read the row (L1/L2 hit) rather than holding 80 floats across the reduction -- this kernel lives on
    // occupancy.  The empty asm keeps the compiler from merging the two passes' loads.
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) {
            float xv[8], gv[8], sv[8], o[8];
            unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), xv);
            unpack8(*reinterpret_cast<const u32x4*>(gr + c * 8), gv);
            unpack8(*reinterpret_cast<const u32x4*>(sc + c * 8), sv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (xv[e] - mean) * rstd;
                const float gg = rbf(gv[e] * rbf(1.0f + sv[e]));
                o[e] = rstd * (gg - s1 - xh * s2);
            }
            if (dres) {
                float r[8];
                unpack8(*reinterpret_cast<const u32x4*>(dres + (int64_t)row * D + c * 8), r);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rbf(o[e]) + r[e];
            }
            *reinterpret_cast<u32x4*>(dx + (int64_t)row * D + c * 8) = pack8(o);
        }
    }
}

// Epilogue of the strip-layout kernels (a lane owns 8 of the workgroup's 512 columns and has summed NSET quantities over its
// wave's rows): the four waves meet in LDS and are summed in wave order, 256 threads x 2 columns, into ONE partial row per
// workgroup and set -- the follow-up reduction reads 4x less.  acc[s]: the lane's 8 sums of set s; out[s]: column 0 of set s's
// partial row, a null one is not written.  The kernels sum into one 8-float array per quantity and copy them into `acc` for
// the call: summing into a [2][8] array (or handing over pointers to the arrays) made the compiler vectorize the row loops
// another way -- ln_mod_bwd_cols_kernel went from 191 to 215 (256) VGPRs.
template <int NSET>
__device__ __forceinline__ void strip_partial_row(const float (&acc)[NSET][8], int ncols, float* const (&out)[NSET]) {
    __shared__ float red[NSET * WAVES * 512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int s = 0; s < NSET; ++s) red[(s * WAVES + wave) * 512 + lane * 8 + e] = acc[s][e];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int cl = threadIdx.x + 256 * k, c = blockIdx.x * 512 + cl;
        if (c >= ncols) continue;
#pragma unroll
        for (int s = 0; s < NSET; ++s) {
            const float* r = red + s * WAVES * 512 + cl;
            if (out[s]) out[s][c] = r[0] + r[512] + r[1024] + r[1536];
        }
    }
}

// grid = (ceil(D/512), ceil(rpb / (WAVES * LN_COL_ROWS)), B); one partial row per workgroup: ws[(b*gridDim.y + by)][2][D].
// Eight rows' loads (x, dy, mean, rstd) are issued before the first use: with one row in flight per wave the 1280 waves of
// a 8192 x 2240 gradient kept 2.6 MB in flight, a quarter of what the HBM pipe needs (3.7 TB/s measured).
constexpr int LN_COL_ROWS = 16;
__global__ __launch_bounds__(256) void ln_mod_bwd_cols_kernel(int rpb, int D, const bf16_t* x, const float* mean_in,
                                                              const float* rstd_in, const bf16_t* dy, float* ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 512 + lane * 8;
    const int b = blockIdx.z;
    const int rg = blockIdx.y * WAVES + wave;
    float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c0 < D) {
        for (int r0 = 0; r0 < LN_COL_ROWS; r0 += 8) {
            u32x4 vx[8], vg[8];
            float mean[8], rstd[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rl = rg * LN_COL_ROWS + r0 + q;
                const bool in = rl < rpb;
                const int64_t row = (int64_t)b * rpb + (in ? rl : 0);
                vx[q] = *reinterpret_cast<const u32x4*>(x + row * D + c0);
                vg[q] = in ? *reinterpret_cast<const u32x4*>(dy + row * D + c0) : u32x4{0u, 0u, 0u, 0u};
                mean[q] = mean_in[row];
                rstd[q] = rstd_in[row];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float xv[8], gv[8];
                unpack8(vx[q], xv);
                unpack8(vg[q], gv);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    a1[e] += gv[e];
                    a2[e] += gv[e] * rbf((xv[e] - mean[q]) * rstd[q]);
                }
            }
        }
    }
    float* wp = ws + ((int64_t)b * gridDim.y + blockIdx.y) * 2 * D;
    float acc[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { acc[0][e] = a1[e]; acc[1][e] = a2[e]; }
    float* const out[2] = {wp, wp + D};
    strip_partial_row<2>(acc, D, out);
}

// Partial-row reductions: a 256-thread block owns 64 columns; 4 thread rows split the G partial rows and meet in LDS
// (fixed order -> bit-reproducible).  grid.x = ceil(W / 64).
__device__ __forceinline__ float reduce_rows64(const float* ws, int G, int W, int j, bool valid) {
    __shared__ float red[4][64];
    const int part = threadIdx.x >> 6;
    float s = 0.f;
    if (valid)
        for (int g = part; g < G; g += 4) s += ws[(int64_t)g * W + j];
    red[part][threadIdx.x & 63] = s;
    __syncthreads();
    return red[0][threadIdx.x & 63] + red[1][threadIdx.x & 63] + red[2][threadIdx.x & 63] + red[3][threadIdx.x & 63];
}

// out[b*ld_out + j] += sum_g ws[(b*G + g)*W + j]   (fp32 accumulate) -- j over W columns
__global__ __launch_bounds__(256) void reduce_partials_f32_kernel(int B, int G, int W, const float* ws, float* out0,
                                                                  float* out1, int half, int ld_out) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), b = blockIdx.y;
    const float s = reduce_rows64(ws + (int64_t)b * G * W, G, W, j, j < W);
    if (threadIdx.x >= 64 || j >= W) return;
    // columns [0, half) go to out0, [half, W) to out1 (dshift / dscale live in different slots)
    if (j < half) out0[(int64_t)b * ld_out + j] += s;
    else if (out1) out1[(int64_t)b * ld_out + (j - half)] += s;
}

// bf16 output variant (bias / weight gradients), one grid row per segment: grid = (ceil(W / 64), nseg), segment s sums
// ws[s][G][W] into out0 (s = 0) or out1 (s = 1; unused with one segment): out[j] = (accumulate ? out[j] : 0) + sum_g ws[g*W + j]
__global__ __launch_bounds__(256) void reduce_partials_bf16_kernel(int G, int W, const float* ws, bf16_t* out0,
                                                                   bf16_t* out1, int accumulate) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    bf16_t* out = blockIdx.y ? out1 : out0;
    float s = reduce_rows64(ws + (int64_t)blockIdx.y * G * W, G, W, j, j < W);
    if (threadIdx.x >= 64 || j >= W) return;
    if (accumulate) s = rbf(s) + bf2f(out[j]);
    out[j] = f2bf(s);
}

// ------------------------------------------------------------------ RMSNorm over strided row segments
// The one RMSNorm kernel pair: the q/k norm of SANA-1.5 (nseg = 2 on a fused projection) and, at nseg = 1 on compact rows
// (ld = D) with no `keep`, the plain yat_rmsnorm_fwd / _bwd of the caption norm.
// One wave owns one (row, segment): segment s of row r starts at x + r * ldx + s * D and has its own weight.  The segment is
// in registers before the first store, so y may be x (in place on the q|k columns of a fused projection); `keep` (nullable)
// receives the raw values compactly, [M, nseg * D], for the backward.
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_seg_fwd_kernel(int M, int D, int nseg, float eps, const bf16_t* x, int ldx,
                                                              const bf16_t* w0, const bf16_t* w1, bf16_t* y, int ldy,
                                                              bf16_t* keep, float* rstd_out) {
    // product and sum stay two roundings: a fused multiply-add here would move rstd, and with it every y, by a bit
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t task = (int64_t)blockIdx.x * WAVES + wave;
    if (task >= (int64_t)M * nseg) return;
    const int64_t row = task / nseg;
    const int seg = (int)(task - row * nseg);
    const bf16_t* w = seg ? w1 : w0;
    const int nchunk = D >> 3;
    float v[MAXV][8];
    load_row<MAXV>(x + row * ldx + (int64_t)seg * D, nchunk, lane, v);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float sq = v[i][e] * v[i][e]; q += sq; }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0) rstd_out[task] = rstd;
    bf16_t* yr = y + row * ldy + (int64_t)seg * D;
    bf16_t* kr = keep ? keep + task * D : nullptr;          // [M, nseg * D]: (row * nseg + seg) * D
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) {
            float ww[8], o[8];
            unpack8(*reinterpret_cast<const u32x4*>(w + c * 8), ww);
            if (kr) *reinterpret_cast<u32x4*>(kr + c * 8) = pack8(v[i]);      // (bf16 -> fp32 -> bf16: the same bits)
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = rbf(v[i][e] * rstd) * ww[e];
            *reinterpret_cast<u32x4*>(yr + c * 8) = pack8(o);
        }
    }
}

// grid = (seg_bwd_blocks(M), nseg); a workgroup strides over the 16-row groups, a wave walks ROWS_PER_WAVE rows of each;
// dx may be dy (the row's dy is in registers before the first store).  The fused
// multiply-adds are written out: left to the compiler, the <.., false> instantiation (rows unrolled four times) summed
// gg * xn as a packed multiply and an add where <.., true> used a fused one, and the dx of the two differed in the last bit.  DW: the four
// waves' column sums meet in LDS in wave order and leave ONE partial row per workgroup, ws[seg][blk][D] -- at the step's
// 8192 rows one partial row per wave (2048 of them) made the follow-up reduction (18 MB per segment through 35
// workgroups, 110 us) dearer than this kernel.
constexpr int SEG_BWD_MAX_BLOCKS = 256;          // one workgroup per CU; 1024 waves x 2 rows of loads in flight
inline int seg_bwd_blocks(int M) {
    const int groups = (M + WAVES * ROWS_PER_WAVE - 1) / (WAVES * ROWS_PER_WAVE);
    return groups < SEG_BWD_MAX_BLOCKS ? groups : SEG_BWD_MAX_BLOCKS;
}
template <int MAXV, bool DW>
__global__ __launch_bounds__(256) void rmsnorm_seg_bwd_kernel(int M, int D, const bf16_t* x, int ldx, const bf16_t* w0,
                                                              const bf16_t* w1, const float* rstd_in, const bf16_t* dy,
                                                              int lddy, bf16_t* dx, int lddx, float* ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = blockIdx.y, nseg = gridDim.y;
    const bf16_t* w = seg ? w1 : w0;
    const int nchunk = D >> 3;
    float ww[MAXV][8], aw[DW ? MAXV : 1][8];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nchunk) unpack8(*reinterpret_cast<const u32x4*>(w + c * 8), ww[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) { if constexpr (DW) aw[i][e] = 0.f; if (c >= nchunk) ww[i][e] = 0.f; }
    }
    const int ngroups = (M + WAVES * ROWS_PER_WAVE - 1) / (WAVES * ROWS_PER_WAVE);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x)
    for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
        const int64_t row = (int64_t)grp * (WAVES * ROWS_PER_WAVE) + wave * ROWS_PER_WAVE + rr;
        if (row >= M) break;
        float v[MAXV][8], g[MAXV][8];
        load_row<MAXV>(x + row * ldx + (int64_t)seg * D, nchunk, lane, v);
        load_row<MAXV>(dy + row * lddy + (int64_t)seg * D, nchunk, lane, g);
        const float rstd = rstd_in[row * nseg + seg];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xn = v[i][e] * rstd;
                if constexpr (DW) aw[i][e] = __builtin_fmaf(g[i][e], rbf(xn), aw[i][e]);
                const float gg = rbf(g[i][e] * ww[i][e]);
                v[i][e] = xn; g[i][e] = gg;
                s = __builtin_fmaf(gg, xn, s);
            }
        s = wave_sum(s) / (float)D;
        bf16_t* dr = dx + row * lddx + (int64_t)seg * D;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nchunk) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rstd * __builtin_fmaf(-v[i][e], s, g[i][e]);
                *reinterpret_cast<u32x4*>(dr + c * 8) = pack8(o);
            }
        }
    }
    if constexpr (DW) {
        __shared__ float red[(WAVES - 1) * MAXV * 512];
        if (wave > 0) {
#pragma unroll
            for (int i = 0; i < MAXV; ++i)
#pragma unroll
                for (int e = 0; e < 8; e += 4)
                    *reinterpret_cast<f32x4*>(red + ((wave - 1) * MAXV + i) * 512 + lane * 8 + e) =
                        f32x4{aw[i][e], aw[i][e + 1], aw[i][e + 2], aw[i][e + 3]};
        }
        __syncthreads();
        if (wave > 0) return;
        float* wp = ws + ((int64_t)seg * gridDim.x + blockIdx.x) * D;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nchunk) {
#pragma unroll
                for (int e = 0; e < 8; e += 4) {
                    f32x4 t = f32x4{aw[i][e], aw[i][e + 1], aw[i][e + 2], aw[i][e + 3]};
#pragma unroll
                    for (int w2 = 0; w2 < WAVES - 1; ++w2)         // fixed order: wave 0 + wave 1 + wave 2 + wave 3
                        t += *reinterpret_cast<const f32x4*>(red + (w2 * MAXV + i) * 512 + lane * 8 + e);
                    *reinterpret_cast<f32x4*>(wp + c * 8 + e) = t;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ strip kernels (512 columns x 32 rows per wave)
constexpr int STRIP_ROWS = 32;            // rows per wave of the column sum
constexpr int GATE_ROWS = 16;             // ... of the gate backward (three streams per row: twice the workgroups)

// Column sum of x[rows, cols]: grid = (ceil(cols/512), ceil(rows / (WAVES * STRIP_ROWS))), partial rows ws[blockIdx.y][cols].
__global__ __launch_bounds__(256) void colsum_strip_kernel(int rows, int cols, const bf16_t* x, int ld, float* ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 512 + lane * 8;
    const int rg = blockIdx.y * WAVES + wave;                 // row group
    float acc[1][8] = {};
    if (c0 < cols) {
        // eight rows' loads in flight per lane before the first add (a wave of this kernel is alone on its SIMD more often
        // than not: 320 workgroups on 256 CUs for an 8192 x 2240 gradient); the adds keep the row order, so the sums are
        // bit-identical to the one-row-at-a-time loop
        for (int r0 = 0; r0 < STRIP_ROWS; r0 += 8) {
            u32x4 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rl = rg * STRIP_ROWS + r0 + q;
                v[q] = rl < rows ? *reinterpret_cast<const u32x4*>(x + (int64_t)rl * ld + c0) : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float a[8];
                unpack8(v[q], a);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[0][e] += a[e];
            }
        }
    }
    float* const out[1] = {ws + (int64_t)blockIdx.y * cols};
    strip_partial_row<1>(acc, cols, out);
}

// Gate backward on compact [B * rows_per_batch, cols] rows: dlin = bf16(gate * dout), partial rows of dout * lin (the gate
// gradient) in ws and, with ws2 != null, of dlin (the bias gradient of the gated Linear, for free) in ws2.
// grid = (ceil(cols/512), ceil(rpb / (WAVES * GATE_ROWS)), B); partial row (batch, row block) of ws[..][cols], ws2[..][cols].
__global__ __launch_bounds__(256) void gate_bwd_strip_kernel(int rows_per_batch, int cols, const bf16_t* dout,
                                                             const bf16_t* lin, const bf16_t* gate, int gate_ld,
                                                             bf16_t* dlin, float* ws, float* ws2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 512 + lane * 8;
    const int b = blockIdx.z;
    const int rg = blockIdx.y * WAVES + wave;                 // row group within the batch
    float dg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, db[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // dgate terms, dbias terms
    if (c0 < cols) {
        float g[8];
        unpack8(*reinterpret_cast<const u32x4*>(gate + (int64_t)b * gate_ld + c0), g);
        // the column sum's eight-rows-in-flight shape (dout and lin: 16 loads per lane before the first multiply)
        for (int r0 = 0; r0 < GATE_ROWS; r0 += 8) {
            u32x4 va[8], vl[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rl = rg * GATE_ROWS + r0 + q;
                const int64_t row = (int64_t)b * rows_per_batch + rl;
                const bool in = rl < rows_per_batch;
                va[q] = in ? *reinterpret_cast<const u32x4*>(dout + row * cols + c0) : u32x4{0u, 0u, 0u, 0u};
                vl[q] = in ? *reinterpret_cast<const u32x4*>(lin + row * cols + c0) : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rl = rg * GATE_ROWS + r0 + q;
                if (rl >= rows_per_batch) continue;
                const int64_t row = (int64_t)b * rows_per_batch + rl;
                float a[8], l[8], o[8];
                unpack8(va[q], a);
                unpack8(vl[q], l);
#pragma unroll
                for (int e = 0; e < 8; ++e) { dg[e] += rbf(a[e] * l[e]); o[e] = rbf(g[e] * a[e]); db[e] += o[e]; }
                *reinterpret_cast<u32x4*>(dlin + row * cols + c0) = pack8(o);
            }
        }
    }
    const int64_t part = (int64_t)(gridDim.y * blockIdx.z + blockIdx.y) * cols;
    float acc[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { acc[0][e] = dg[e]; acc[1][e] = db[e]; }
    float* const out[2] = {ws + part, ws2 ? ws2 + part : nullptr};
    strip_partial_row<2>(acc, cols, out);
}

// ------------------------------------------------------------------ modulation table
__global__ void modulation_fwd_kernel(int B, int S, int D, const bf16_t* table, const bf16_t* tmod, int tmod_ld,
                                      int slot_stride, bf16_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * S * D;
    if (i >= total) return;
    const int d = i % D, s = (i / D) % S, b = i / ((int64_t)D * S);
    out[i] = f2bf(bf2f(table[s * D + d]) + bf2f(tmod[(int64_t)b * tmod_ld + s * slot_stride + d]));
}

__global__ void modulation_bwd_kernel(int B, int S, int D, const float* dmod, bf16_t* dtable, int acc_table,
                                      float* dtmod, int tmod_ld, int slot_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over S*D
    if (i >= S * D) return;
    const int d = i % D, s = i / D;
    float t = 0.f;
    for (int b = 0; b < B; ++b) {
        const float g = dmod[((int64_t)b * S + s) * D + d];
        // the reference's autograd hands each consumer a bf16 gradient
        t += rbf(g);
        if (slot_stride != 0) dtmod[(int64_t)b * tmod_ld + s * slot_stride + d] += rbf(g);
    }
    if (acc_table) t = rbf(t) + bf2f(dtable[i]);
    dtable[i] = f2bf(t);
}
// slot_stride == 0 (final norm: every slot adds the same embedded_timestep): dtmod[b, d] += sum_s dmod[b,s,d]
__global__ void modulation_bwd_shared_kernel(int B, int S, int D, const float* dmod, float* dtmod, int tmod_ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over B*D
    if (i >= B * D) return;
    const int d = i % D, b = i / D;
    float t = 0.f;
    for (int s = 0; s < S; ++s) t += rbf(dmod[((int64_t)b * S + s) * D + d]);
    dtmod[(int64_t)b * tmod_ld + d] += t;
}

template <typename F>
int dispatch_maxv(int D, F&& f) {
    if (D & 7) return YAT_EINVAL;
    if (D <= 512 * 2) return f(std::integral_constant<int, 2>{});
    if (D <= 512 * 5) return f(std::integral_constant<int, 5>{});
    if (D <= 512 * 8) return f(std::integral_constant<int, 8>{});
    return YAT_EINVAL;
}

}  // namespace

extern "C" {

int yat_version(void) { return 1; }

int yat_ln_modulate_fwd(int M, int D, int rpb, float eps, const void* x, const void* shift, const void* scale,
                        int mod_ld, void* y, float* mean, float* rstd, yat_stream_t stream) {
    if (M <= 0 || rpb <= 0 || (mod_ld & 7) || !x || !shift || !scale || !y || !mean || !rstd) return YAT_EINVAL;
    return dispatch_maxv(D, [&](auto mv) {
        constexpr int MV = decltype(mv)::value;
        hipLaunchKernelGGL((ln_mod_fwd_kernel<MV>), dim3((M + WAVES - 1) / WAVES), dim3(256), 0, (hipStream_t)stream, M, D,
                           rpb, eps, (const bf16_t*)x, (const bf16_t*)shift, (const bf16_t*)scale, mod_ld, (bf16_t*)y,
                           mean, rstd);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    });
}

uint64_t yat_ln_bwd_workspace_bytes(int M, int D, int rpb) {
    if (M <= 0 || rpb <= 0) return 0;
    const uint64_t gy = (rpb + WAVES * LN_COL_ROWS - 1) / (WAVES * LN_COL_ROWS);
    return (uint64_t)(M / rpb) * gy * 2 * D * sizeof(float);
}

int yat_ln_modulate_bwd(int M, int D, int rpb, const void* x, const float* mean, const float* rstd, const void* scale,
                        int mod_ld, const void* dy, const void* dres, void* dx, float* dshift_acc, float* dscale_acc,
                        int acc_ld, void* workspace, int parts, yat_stream_t stream) {
    // (D & 7: the column pass loads 8 columns at once and, launched alone with parts = 2, has no dispatch_maxv in front of it)
    if (M <= 0 || rpb <= 0 || M % rpb || (D & 7) || (mod_ld & 7) || !x || !dy || parts < 1 || parts > 3) return YAT_EINVAL;
    if ((parts & 1) && !dx) return YAT_EINVAL;
    if ((parts & 2) && (!workspace || !dshift_acc || !dscale_acc)) return YAT_EINVAL;
    const int B = M / rpb;
    int rc = !(parts & 1) ? YAT_OK : dispatch_maxv(D, [&](auto mv) {
        constexpr int MV = decltype(mv)::value;
        hipLaunchKernelGGL((ln_mod_bwd_rows_kernel<MV>), dim3((M + WAVES - 1) / WAVES), dim3(256), 0, (hipStream_t)stream, M,
                           D, rpb, (const bf16_t*)x, mean, rstd, (const bf16_t*)scale, mod_ld, (const bf16_t*)dy,
                           (const bf16_t*)dres, (bf16_t*)dx);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    });
    if (rc || !(parts & 2)) return rc;
    const int gy = (rpb + WAVES * LN_COL_ROWS - 1) / (WAVES * LN_COL_ROWS);
    hipLaunchKernelGGL(ln_mod_bwd_cols_kernel, dim3((D + 511) / 512, gy, B), dim3(256), 0, (hipStream_t)stream, rpb, D,
                       (const bf16_t*)x, mean, rstd, (const bf16_t*)dy, (float*)workspace);
    YAT_CHECK_LAUNCH();
    const int W = 2 * D, G = gy;
    hipLaunchKernelGGL(reduce_partials_f32_kernel, dim3((W + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, B, G, W,
                       (const float*)workspace, dshift_acc, dscale_acc, D, acc_ld);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

// The one launch site of each RMSNorm kernel (and of the reduce behind the backward); the entries below check the arguments.
static int launch_rmsnorm_fwd(int M, int D, int nseg, float eps, const void* x, int ldx, const void* w0, const void* w1,
                              void* y, int ldy, void* keep, float* rstd, yat_stream_t stream) {
    const int64_t tasks = (int64_t)M * nseg;
    return dispatch_maxv(D, [&](auto mv) {
        constexpr int MV = decltype(mv)::value;
        hipLaunchKernelGGL((rmsnorm_seg_fwd_kernel<MV>), dim3((unsigned)((tasks + WAVES - 1) / WAVES)), dim3(256), 0,
                           (hipStream_t)stream, M, D, nseg, eps, (const bf16_t*)x, ldx, (const bf16_t*)w0, (const bf16_t*)w1,
                           (bf16_t*)y, ldy, (bf16_t*)keep, rstd);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    });
}

// dw0 null: dx only (no workspace, no reduce)
static int launch_rmsnorm_bwd(int M, int D, int nseg, const void* x, int ldx, const void* w0, const void* w1,
                              const float* rstd, const void* dy, int lddy, void* dx, int lddx, void* dw0, void* dw1,
                              int accumulate_dw, void* workspace, yat_stream_t stream) {
    const bool want_dw = dw0 != nullptr;
    const int nblk = seg_bwd_blocks(M);
    int rc = dispatch_maxv(D, [&](auto mv) {
        constexpr int MV = decltype(mv)::value;
        hipLaunchKernelGGL((want_dw ? rmsnorm_seg_bwd_kernel<MV, true> : rmsnorm_seg_bwd_kernel<MV, false>), dim3(nblk, nseg),
                           dim3(256), 0, (hipStream_t)stream, M, D, (const bf16_t*)x, ldx, (const bf16_t*)w0, (const bf16_t*)w1,
                           rstd, (const bf16_t*)dy, lddy, (bf16_t*)dx, lddx, (float*)workspace);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    });
    if (rc || !want_dw) return rc;
    hipLaunchKernelGGL(reduce_partials_bf16_kernel, dim3((D + 63) / 64, nseg), dim3(256), 0, (hipStream_t)stream, nblk, D,
                       (const float*)workspace, (bf16_t*)dw0, (bf16_t*)dw1, accumulate_dw);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

// yat_rmsnorm_fwd / _bwd: the one-segment, compact-row case (nseg = 1, every leading dimension D, no raw copy) of the
// segment kernels -- same arithmetic, same workspace.
int yat_rmsnorm_fwd(int M, int D, float eps, const void* x, const void* w, void* y, float* rstd, yat_stream_t stream) {
    if (M <= 0 || !x || !w || !y || !rstd) return YAT_EINVAL;
    return launch_rmsnorm_fwd(M, D, 1, eps, x, D, w, nullptr, y, D, nullptr, rstd, stream);
}

uint64_t yat_rmsnorm_bwd_workspace_bytes(int M, int D) {
    return (uint64_t)seg_bwd_blocks(M) * D * sizeof(float);                     // one partial row per workgroup
}

int yat_rmsnorm_bwd(int M, int D, const void* x, const void* w, const float* rstd, const void* dy, void* dx,
                    void* dw, int accumulate_dw, void* workspace, yat_stream_t stream) {
    if (M <= 0 || !x || !w || !rstd || !dy || !dx || !dw || !workspace) return YAT_EINVAL;
    return launch_rmsnorm_bwd(M, D, 1, x, D, w, nullptr, rstd, dy, D, dx, D, dw, nullptr, accumulate_dw, workspace, stream);
}

static bool seg_args_bad(int M, int D, int nseg, int ld) {
    return M <= 0 || D <= 0 || (D & 7) || nseg < 1 || nseg > 2 || (ld & 7) || (int64_t)ld < (int64_t)nseg * D;
}

int yat_rmsnorm_seg_fwd(int M, int D, int nseg, float eps, const void* x, int ldx, const void* w0, const void* w1, void* y,
                        int ldy, void* keep, float* rstd, yat_stream_t stream) {
    if (seg_args_bad(M, D, nseg, ldx) || seg_args_bad(M, D, nseg, ldy) || !x || !w0 || (nseg == 2 && !w1) || !y || !rstd)
        return YAT_EINVAL;
    return launch_rmsnorm_fwd(M, D, nseg, eps, x, ldx, w0, w1, y, ldy, keep, rstd, stream);
}

uint64_t yat_rmsnorm_seg_bwd_workspace_bytes(int M, int D, int nseg) {
    if (M <= 0 || D <= 0 || nseg < 1) return 0;
    return (uint64_t)nseg * seg_bwd_blocks(M) * D * sizeof(float);              // one partial row per workgroup and segment
}

int yat_rmsnorm_seg_bwd(int M, int D, int nseg, const void* x, int ldx, const void* w0, const void* w1, const float* rstd,
                        const void* dy, int lddy, void* dx, int lddx, void* dw0, void* dw1, int accumulate_dw,
                        void* workspace, yat_stream_t stream) {
    if (seg_args_bad(M, D, nseg, ldx) || seg_args_bad(M, D, nseg, lddy) || seg_args_bad(M, D, nseg, lddx) || !x || !w0 ||
        (nseg == 2 && !w1) || !rstd || !dy || !dx)
        return YAT_EINVAL;
    const bool want_dw = dw0 != nullptr;                      // a frozen base under adapters passes no dw at all
    if (nseg == 2 && want_dw != (dw1 != nullptr)) return YAT_EINVAL;
    if (want_dw && !workspace) return YAT_EINVAL;
    return launch_rmsnorm_bwd(M, D, nseg, x, ldx, w0, w1, rstd, dy, lddy, dx, lddx, dw0, dw1, accumulate_dw, workspace, stream);
}

uint64_t yat_colsum_workspace_bytes(int rows, int cols) {
    const int gy = (rows + WAVES * STRIP_ROWS - 1) / (WAVES * STRIP_ROWS);
    return (uint64_t)gy * cols * sizeof(float);
}

int yat_colsum_bf16(int rows, int cols, const void* x, int ld, void* out, int accumulate, void* workspace,
                    yat_stream_t stream) {
    if (rows <= 0 || cols <= 0 || (cols & 7) || (ld & 7) || !x || !out || !workspace) return YAT_EINVAL;
    const int gy = (rows + WAVES * STRIP_ROWS - 1) / (WAVES * STRIP_ROWS);
    hipLaunchKernelGGL(colsum_strip_kernel, dim3((cols + 511) / 512, gy), dim3(256), 0, (hipStream_t)stream, rows, cols,
                       (const bf16_t*)x, ld, (float*)workspace);
    YAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(reduce_partials_bf16_kernel, dim3((cols + 63) / 64), dim3(256), 0, (hipStream_t)stream, gy, cols,
                       (const float*)workspace, (bf16_t*)out, (bf16_t*)nullptr, accumulate);      // one segment: no out1
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

uint64_t yat_gate_bwd_workspace_bytes(int M, int D, int rpb) {
    if (M <= 0 || rpb <= 0) return 0;
    const uint64_t gy = (rpb + WAVES * GATE_ROWS - 1) / (WAVES * GATE_ROWS);
    return 2 * (uint64_t)(M / rpb) * gy * D * sizeof(float);        // gate partials + bias-gradient partials
}

int yat_gate_bwd(int M, int D, int rpb, const void* dout, const void* lin, const void* gate, int gate_ld, void* dlin,
                 float* dgate_acc, int acc_ld, void* dbias, int accumulate_bias, void* workspace, yat_stream_t stream) {
    if (M <= 0 || rpb <= 0 || M % rpb || (D & 7) || (gate_ld & 7) || !dout || !lin || !gate || !dlin || !dgate_acc ||
        !workspace)
        return YAT_EINVAL;
    const int B = M / rpb;
    const int gy = (rpb + WAVES * GATE_ROWS - 1) / (WAVES * GATE_ROWS);
    float* ws2 = dbias ? (float*)workspace + (int64_t)B * gy * D : nullptr;
    hipLaunchKernelGGL(gate_bwd_strip_kernel, dim3((D + 511) / 512, gy, B), dim3(256), 0, (hipStream_t)stream, rpb, D,
                       (const bf16_t*)dout, (const bf16_t*)lin, (const bf16_t*)gate, gate_ld, (bf16_t*)dlin,
                       (float*)workspace, ws2);
    YAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(reduce_partials_f32_kernel, dim3((D + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, B, gy, D,
                       (const float*)workspace, dgate_acc, (float*)nullptr, D, acc_ld);
    YAT_CHECK_LAUNCH();
    if (dbias) {                                              // bias gradient of the gated Linear = column sum of dlin
        hipLaunchKernelGGL(reduce_partials_bf16_kernel, dim3((D + 63) / 64), dim3(256), 0, (hipStream_t)stream, B * gy, D,
                           (const float*)ws2, (bf16_t*)dbias, (bf16_t*)nullptr, accumulate_bias);
        YAT_CHECK_LAUNCH();
    }
    return YAT_OK;
}

int yat_modulation_fwd(int B, int S, int D, const void* table, const void* tmod, int tmod_ld, int slot_stride,
                       void* mod_out, yat_stream_t stream) {
    if (B <= 0 || S <= 0 || D <= 0 || !table || !tmod || !mod_out) return YAT_EINVAL;
    const int64_t total = (int64_t)B * S * D;
    hipLaunchKernelGGL(modulation_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B,
                       S, D, (const bf16_t*)table, (const bf16_t*)tmod, tmod_ld, slot_stride, (bf16_t*)mod_out);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_modulation_bwd(int B, int S, int D, const float* dmod, void* dtable, int accumulate_table, float* dtmod_acc,
                       int tmod_ld, int slot_stride, yat_stream_t stream) {
    if (B <= 0 || S <= 0 || D <= 0 || !dmod || !dtable || !dtmod_acc) return YAT_EINVAL;
    hipLaunchKernelGGL(modulation_bwd_kernel, dim3((S * D + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, S, D, dmod,
                       (bf16_t*)dtable, accumulate_table, dtmod_acc, tmod_ld, slot_stride);
    YAT_CHECK_LAUNCH();
    if (slot_stride == 0) {
        hipLaunchKernelGGL(modulation_bwd_shared_kernel, dim3((B * D + 255) / 256), dim3(256), 0, (hipStream_t)stream, B,
                           S, D, dmod, dtmod_acc, tmod_ld);
        YAT_CHECK_LAUNCH();
    }
    return YAT_OK;
}

}  // extern "C"
