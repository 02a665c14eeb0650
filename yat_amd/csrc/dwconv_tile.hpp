// LDS-tiled kernels of the GLU depthwise convolution (w <= 64, channel counts that are multiples of 8) and their launch
// geometry; included once, by dwconv_glu.hip, which adds the direct kernels for every other shape and the C ABI.
//
// The kernels issue no per-lane guarded global loads: a workgroup stages a whole (R+2)-row x w-column x TCH-channel tile
// with LDS-DMA (16 B/lane, no VGPRs, zero fill at the image border from the buffer range check) and computes from LDS.
//   tile[half][(R+2) rows][WP = w+1 columns][TCH ch]: column 0 of a row is the zero left halo AND (being the element after
//   column w of the previous row) the zero right halo, so no second halo column is stored.  WP is odd for even w:
//   consecutive rows start 64 B (mod 256 B) apart and the four runs one ds_read_b64 serves per cycle hit disjoint banks.
//   TILE_PAD pixels after each half absorb the over-read of a partial last column segment.
// A thread owns 4 channels of one run = SEG output columns of one row; the column walk is fully unrolled with three
// statically rotated accumulators (no register shuffling), every tap is applied exactly once.
//
// Everything is a template on the tile configuration:
//   TCH = channels per half per tile.  64 makes every pixel slice a full 128-byte line (the 64-byte slices of TCH = 32
//         cost the forward 25-35 % on every bucket);
//   WPS = workgroups per CU the LDS budget and __launch_bounds__ are sized for: trades occupancy for taller bands (less
//         halo re-read), which wins on wide rows.
// Only the instantiations a launcher names exist: forward / pass 1 at <32, 3>, <64, 3>, <64, 2>, the streaming forward at
// <64, 3>, pass 2 at <32, z in LDS> and <64, z from global>.
#pragma once
#include "common.hpp"

namespace {

#ifndef YAT_DW_SEG
#define YAT_DW_SEG 8
#endif
constexpr int SEG = YAT_DW_SEG;      // output columns per thread
constexpr int PK = 11;               // partial values per channel: 9 taps, conv bias, column sum of dz
constexpr int TILE_PAD = 9;

template <int TCH>
struct Tile {
    static constexpr int NCG = TCH / 4;     // 4-channel groups (threads) across a tile pixel
    static constexpr int PPP = TCH / 8;     // 16-byte pieces per tile pixel
    static constexpr int GPX = 64 / PPP;    // pixels one DMA wave instruction moves
    static constexpr int NS = 256 / NCG;    // run slots of a 256-thread workgroup
};
constexpr int lds_budget(int WPS) { return 159744 / WPS; }      // dynamic LDS of one of WPS workgroups on a CU

// pixel slots of `rows` tile rows (+ the shared zero slot and the pad), a multiple of 16 = one DMA instruction
__host__ __device__ inline int tile_slots(int rows, int WP) { return (rows * WP + 1 + TILE_PAD + 15) & ~15; }

// Work-unit order for a 1-D grid: workgroups are dealt round-robin to the 8 XCDs (each with a private L2), so unit
// u = xcd * ceil(total/8) + slot gives every XCD one contiguous run of units.  With (segment, row) fastest inside a
// (channel chunk, image) the three-row halo a unit re-reads was fetched by its neighbour on the SAME L2 moments before.
__device__ __forceinline__ int xcd_unit(int total) {
    const int per = (total + 7) >> 3;
    return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}
inline unsigned grid8(int64_t total) { return (unsigned)(((total + 7) / 8) * 8); }

// bands per workgroup: as many as still leave `min_wgs` workgroups (taps are loaded and the tile cleared once per workgroup)
inline int bands_per_wg(int nbands, int64_t wgs_per_band_group, int min_wgs) {
    int bpb = nbands;
    while (bpb > 1 && (nbands + bpb - 1) / bpb * wgs_per_band_group < min_wgs) --bpb;
    return bpb;
}

// 9 taps of 4 consecutive channels = 36 contiguous bf16 (8-byte aligned since the channel index is a multiple of 4):
// nine 8-byte loads issued together, then regrouped as channel pairs per tap
__device__ __forceinline__ void load_taps(const bf16_t* wdw, int c, f32x2 (&wv)[9][2]) {
    u32x2 raw[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) raw[k] = *reinterpret_cast<const u32x2*>(wdw + (int64_t)c * 9 + k * 4);
    float flat[36];
#pragma unroll
    for (int k = 0; k < 9; ++k) unpack4(raw[k], flat + 4 * k);      // flat[e*9 + t]
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) wv[t][pr] = f32x2{flat[(2 * pr) * 9 + t], flat[(2 * pr + 1) * 9 + t]};
    // opaque to the optimizer (after ALL loads): otherwise it keeps the packed words and re-unpacks each weight in the run loop
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) asm volatile("" : "+v"(wv[t][pr]));
}

// Stage `nrows` image rows (first one ii0; rows outside [0,h) become zeros) of TCH channels starting at element `chan`
// of a [B,h,w,C2] array into tile slots slot0 + r*WP + 1 + j.  One wave instruction moves GPX consecutive pixels x TCH * 2 B:
// the lane pattern (pixel lane / PPP, 16-byte piece lane % PPP) never changes, only the scalar offset does, so staging costs
// a few SALU instructions per KiB instead of per-lane index arithmetic.  Slot 0 of every row (the shared zero halo) and the
// pad are never written here; the whole tile is cleared once per workgroup.
template <int TCH>
__device__ __forceinline__ void stage_rows(const __amdgpu_buffer_rsrc_t rs, unsigned char* tile, int slot0, int nrows,
                                           int ii0, int b, int h, int w, int WP, int C2, int chan, bool lane_ch_ok,
                                           int wave_s, int nwaves, int lane) {
    constexpr int PPP = Tile<TCH>::PPP, GPX = Tile<TCH>::GPX;
    const int ngroups = (w + GPX - 1) / GPX;
    const uint32_t vlane = (uint32_t)(lane / PPP) * (uint32_t)C2 * 2u + (uint32_t)(lane % PPP) * 16u;
    int k = 0;
    for (int r = 0; r < nrows; ++r) {
        const int ii = ii0 + r;
        const bool row_ok = ii >= 0 && ii < h;
        for (int g = 0; g < ngroups; ++g, ++k) {
            if ((k & (nwaves - 1)) != wave_s) continue;                   // wave-uniform: rows x groups dealt round-robin
            const int jj0 = g * GPX;
            const uint32_t soff = row_ok ? (uint32_t)(((((int64_t)b * h + ii) * w + jj0) * C2 + chan) * 2) : 0u;
            if ((lane / PPP) < w - jj0)                                   // partial last group: EXEC-masked lanes write nothing
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (YAT_LDS void*)(tile + (slot0 + r * WP + 1 + jj0) * (TCH * 2)),
                                                         16, row_ok && lane_ch_ok ? vlane : YAT_OOB, soff, 0, 0);
        }
    }
}
__device__ __forceinline__ void clear_tile(unsigned char* tile, int bytes) {
    for (int o = threadIdx.x * 16; o < bytes; o += blockDim.x * 16) *reinterpret_cast<u32x4*>(tile + o) = u32x4{0u, 0u, 0u, 0u};
}

// The forward column walk of one run: NS output columns from j0 of image row i, 4 channels of either half.
//   prow[r]: this thread's bytes of tile column j0 (= input column j0 - 1) of image row i - 1 + r, `a` half; the `g` half lies
//   goff bytes behind.  The caller supplies the row pointers because a band's rows are contiguous and a ring's are not, and
//   row_live (false: every store of the run carries an out-of-range offset).
// MODE 0: forward (two u stores, then y).  MODE 1: backward pass 1 (reads dy, stores du for both halves).
// Both forward kernels are bit-identical because they share this: taps in dj = 2..0 order into A[o % 3] / G[o % 3], u rounded
// to bf16 before the GLU.  All global traffic goes through range-checked buffer instructions: a guarded plain store makes
// the optimizer sink each output's FMAs into its branch, which keeps three unpacked input columns live (299 VGPRs).
template <int NS, int TCH, int MODE>
__device__ __forceinline__ void dwglu_fwd_walk(const unsigned char* const (&prow)[3], int goff, bool row_live, int j0, int w,
                                               int64_t pix0, int Hc, int ca, const f32x2 (&wa)[9][2], const f32x2 (&wg)[9][2],
                                               const f32x2 (&ba)[2], const f32x2 (&bg2)[2], const __amdgpu_buffer_rsrc_t rout,
                                               const __amdgpu_buffer_rsrc_t ru, const __amdgpu_buffer_rsrc_t rdy) {
    const int C2 = 2 * Hc;
    u32x2 dyv[3];                                           // dy of output o is fetched at step o, used at step o + 2
    f32x2 A[3][2], G[3][2];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) { A[m][pr] = ba[pr]; G[m][pr] = bg2[pr]; }
    u32x2 nxt[6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        nxt[2 * r] = *reinterpret_cast<const u32x2*>(prow[r]);
        nxt[2 * r + 1] = *reinterpret_cast<const u32x2*>(prow[r] + goff);
    }
#pragma unroll
    for (int t = 0; t < NS + 2; ++t) {                      // input column j0 - 1 + t  (tile column j0 + t)
        u32x2 cur[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) cur[m] = nxt[m];
        if (MODE == 1 && t < NS)
            dyv[t % 3] = __builtin_amdgcn_raw_buffer_load_b64(
                rdy, j0 + t < w ? (uint32_t)(((pix0 + t) * Hc + ca) * 2) : YAT_OOB, 0, 0);
        if (t + 1 < NS + 2) {                               // next column's LDS reads fly under this column's FMAs
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                nxt[2 * r] = *reinterpret_cast<const u32x2*>(prow[r] + (t + 1) * TCH * 2);
                nxt[2 * r + 1] = *reinterpret_cast<const u32x2*>(prow[r] + goff + (t + 1) * TCH * 2);
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            f32x2 za[2], zg[2];
            unpack22(cur[2 * r], za);
            unpack22(cur[2 * r + 1], zg);
#pragma unroll
            for (int dj = 2; dj >= 0; --dj) {               // output o = t - dj takes tap column dj
                const int o = t - dj;
                if (o < 0 || o >= NS) continue;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    A[o % 3][pr] += wa[r * 3 + dj][pr] * za[pr];
                    G[o % 3][pr] += wg[r * 3 + dj][pr] * zg[pr];
                }
            }
        }
        const int o = t - 2;                                // output column j0 + o has now seen all three input columns
        if (o >= 0) {
            float ua[4], ug[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { ua[e] = rbf(A[o % 3][e >> 1][e & 1]); ug[e] = rbf(G[o % 3][e >> 1][e & 1]); }
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) { A[o % 3][pr] = ba[pr]; G[o % 3][pr] = bg2[pr]; }
            const bool live = row_live && j0 + o < w;
            if (MODE == 0) {
                // keep u for the backward (the GLU backward then runs in the dy GEMM's epilogue): written once, read again a
                // whole forward + half a backward later -> non-temporal (common.hpp YAT_AUX_NT).  Branch-free: without u_out
                // the descriptor has zero records and the range check drops the stores.
                const uint32_t uo = live ? (uint32_t)(((pix0 + o) * C2 + ca) * 2) : YAT_OOB;
                __builtin_amdgcn_raw_buffer_store_b64(pack4(ua[0], ua[1], ua[2], ua[3]), ru, uo, 0, YAT_AUX_NT);
                __builtin_amdgcn_raw_buffer_store_b64(pack4(ug[0], ug[1], ug[2], ug[3]), ru,
                                                      live ? uo + (uint32_t)Hc * 2 : YAT_OOB, 0, YAT_AUX_NT);
                __builtin_amdgcn_raw_buffer_store_b64(
                    pack4(ua[0] * rbf(silu_f(ug[0])), ua[1] * rbf(silu_f(ug[1])), ua[2] * rbf(silu_f(ug[2])),
                          ua[3] * rbf(silu_f(ug[3]))),
                    rout, live ? (uint32_t)(((pix0 + o) * Hc + ca) * 2) : YAT_OOB, 0, 0);
            } else {
                float d[4], da[4], dg[4];
                unpack4(dyv[o % 3], d);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    da[e] = d[e] * rbf(silu_f(ug[e]));                 // d u_a
                    dg[e] = rbf(d[e] * ua[e]) * dsilu_f(ug[e]);        // d u_g
                }
                const uint32_t off = live ? (uint32_t)(((pix0 + o) * C2 + ca) * 2) : YAT_OOB;
                __builtin_amdgcn_raw_buffer_store_b64(pack4(da[0], da[1], da[2], da[3]), rout, off, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(pack4(dg[0], dg[1], dg[2], dg[3]), rout,
                                                      live ? off + (uint32_t)Hc * 2 : YAT_OOB, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);                  // keep the unrolled columns from hoisting all their reads
    }
}

// Band kernel.  MODE 0: forward (writes y, and u when u_out is given).  MODE 1: backward pass 1 (reads dy, writes du).
// s_bytes = bytes of the [B,h,w,2Hc] arrays (s, du, u_out); dy / y are half that.  A workgroup owns `bpb` consecutive bands
// of R rows of one (image, TCH-channel chunk): taps are loaded and the tile cleared once.
template <int MODE, int TCH, int WPS>
__global__ __launch_bounds__(256, WPS) void dwglu_tile_kernel(int h, int w, int Hc, int B, int R, int rmagic, int nbands,
                                                              int bpb, int nchunk, const bf16_t* s, uint64_t s_bytes,
                                                              const bf16_t* wdw, const bf16_t* bdw, const bf16_t* dy,
                                                              bf16_t* out, bf16_t* u_out) {
    constexpr int NCG = Tile<TCH>::NCG, PPP = Tile<TCH>::PPP;
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
    const int ngrp = (nbands + bpb - 1) / bpb;
    const int total = ngrp * nchunk * B;
    int u = xcd_unit(total);
    if (u >= total) return;
    const int bg = u % ngrp; u /= ngrp;
    const int cx = u % nchunk, b = u / nchunk;
    const int ch0 = cx * TCH;
    const int WP = w + 1, PHp = tile_slots(R + 2, WP), C2 = 2 * Hc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, nslots = blockDim.x / NCG;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    clear_tile(tile, 2 * PHp * TCH * 2);
    const int cg = lane & (NCG - 1);
    const int ca = ch0 + cg * 4;
    const bool chan_ok = ca < Hc;
    // taps and biases as channel pairs, explicit 2-vectors: every multiply-add of the walk is one v_pk_fma_f32 with a fixed
    // register pairing (left to the SLP vectorizer, taps get paired across different weights and the weight set is kept twice)
    f32x2 wa[9][2], wg[9][2], ba[2], bg2[2];
    {
        const int cs = chan_ok ? ca : 0;
        load_taps(wdw, cs, wa);
        load_taps(wdw, Hc + cs, wg);
        unpack22(*reinterpret_cast<const u32x2*>(bdw + cs), ba);
        unpack22(*reinterpret_cast<const u32x2*>(bdw + Hc + cs), bg2);
    }
    const int nseg = (w + SEG - 1) / SEG, nruns = R * nseg;
    const int slot = threadIdx.x / NCG;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(s, s_bytes);
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(out, MODE == 0 ? s_bytes / 2 : s_bytes);
    const __amdgpu_buffer_rsrc_t rdy = make_rsrc(MODE == 1 ? dy : s, s_bytes / 2);
    const __amdgpu_buffer_rsrc_t ru = make_rsrc(u_out ? u_out : out, u_out ? s_bytes : 0);      // forward only, optional
    const bool lane_ch_ok = ch0 + (lane % PPP) * 8 < Hc;

    for (int rb = bg * bpb; rb < min(nbands, (bg + 1) * bpb); ++rb) {
        const int i0 = rb * R;
        __syncthreads();                                    // tile cleared / previous band fully consumed
        stage_rows<TCH>(rs, tile, 0, R + 2, i0 - 1, b, h, w, WP, C2, ch0, lane_ch_ok, wave_s, nwaves, lane);
        stage_rows<TCH>(rs, tile, PHp, R + 2, i0 - 1, b, h, w, WP, C2, Hc + ch0, lane_ch_ok, wave_s, nwaves, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        for (int run = slot; run < nruns; run += nslots) {
            const int seg = (run * rmagic) >> 16, row = run - seg * R;      // rows fastest: neighbouring runs, other bank group
            const int i = i0 + row;
            if (i >= h || !chan_ok) continue;
            const int j0 = seg * SEG;
            const unsigned char* pa = tile + ((row * WP + j0) * TCH + cg * 4) * 2;       // row `row` of the tile = image row i-1
            const unsigned char* const prow[3] = {pa, pa + WP * TCH * 2, pa + 2 * WP * TCH * 2};
            const int64_t pix0 = ((int64_t)b * h + i) * w + j0;
            dwglu_fwd_walk<SEG, TCH, MODE>(prow, PHp * TCH * 2, true, j0, w, pix0, Hc, ca, wa, wg, ba, bg2, rout, ru, rdy);
        }
    }
}

// rows per band: the largest R whose tile leaves room for WPS workgroups per CU, weighted by how well R * nseg runs
// fill the run slots and by the (R+2)/R halo re-read
template <int TCH, int WPS>
inline int pick_band_rows(int h, int w, size_t* lds_bytes) {
    const int nseg = (w + SEG - 1) / SEG, ns = Tile<TCH>::NS;
    int best = 0;
    double best_score = 0;
    for (int R = 2; R <= 16 && R <= ((h + 1) & ~1); ++R) {
        const size_t bytes = (size_t)2 * tile_slots(R + 2, w + 1) * TCH * 2;
        if (bytes > (size_t)lds_budget(WPS)) break;
        const int nruns = R * nseg, passes = (nruns + ns - 1) / ns;
        const int nb = (h + R - 1) / R;
        const double score = (double)nruns / (passes * ns) * R / (R + 2) * h / (nb * R);
        if (score > best_score) { best_score = score; best = R; *lds_bytes = bytes; }
    }
    return best;
}

// -> 0 when launched, -1 when the shape is not this kernel's (the caller goes on to the next variant / the direct kernels)
template <int MODE, int TCH, int WPS>
int launch_tile(int B, int h, int w, int Hc, const bf16_t* s, const bf16_t* wdw, const bf16_t* bdw, const bf16_t* dy,
                bf16_t* out, bf16_t* u_out, hipStream_t stream) {
    size_t lds = 0;
    const int R = pick_band_rows<TCH, WPS>(h, w, &lds);
    const uint64_t s_bytes = (uint64_t)B * h * w * 2 * Hc * 2;
    if (!R || (Hc & 7) || s_bytes > 0x7fffffffull) return -1;
    const int nbands = (h + R - 1) / R, nchunk = (Hc + TCH - 1) / TCH;
    const int bpb = bands_per_wg(nbands, (int64_t)nchunk * B, 3 * 256 * WPS);      // >= 3 rounds of resident workgroups
    const int ngrp = (nbands + bpb - 1) / bpb;
    static bool attr_set = false;      // idempotent: tiles above 64 KiB of dynamic LDS (two workgroups per CU) need the opt-in
    if (!attr_set && lds > 65536) {
        if (hipFuncSetAttribute((const void*)dwglu_tile_kernel<MODE, TCH, WPS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds_budget(WPS)) != hipSuccess)
            return -1;
        attr_set = true;
    }
    hipLaunchKernelGGL((dwglu_tile_kernel<MODE, TCH, WPS>), dim3(grid8((int64_t)ngrp * nchunk * B)), dim3(256), lds, stream,
                       h, w, Hc, B, R, (65536 + R - 1) / R, nbands, bpb, nchunk, s, s_bytes, wdw, bdw, dy, out, u_out);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Streaming forward.  The band kernel above alternates "stage a band, wait" with "compute the band": its memory pipe idles
// while it computes and its VALUs idle while it stages (measured 130 us = ~80 us of traffic + ~50 us of VALU, i.e. the sum),
// and every band re-reads its two halo rows.  Here a workgroup walks DOWN an (image, TCH-channel chunk) column of rows in
// steps of R rows over a ring of 2R+2 tile rows: while step k computes from rows i0-1 .. i0+R, the LDS-DMA of the next R
// rows lands in the ring slots step k-1 has released -- one barrier per step, no halo re-read inside the walk, and reads,
// VALU work and the u / y stores of one workgroup overlap.
//   ring slot of image row ii = (ii + 1) mod (2R+2); tile row q occupies pixel slots [q*WP, q*WP + WP), slot 0 = the shared
//   zero halo (never written by the DMA), one extra cleared slot after the last row.
// Every thread runs exactly one run per step (R * nseg <= 256 / NCG, guaranteed by the launcher) and issues all 3*SSEG
// stores whether live or not (dead ones carry an out-of-range offset): so the per-wave count of vector-memory operations
// younger than the prefetch is a constant and `s_waitcnt vmcnt(3*SSEG)` waits for the prefetch without draining the stores
// (yat_amd/build.py check_dwconv_stream_asm holds the compiler to that count).
template <int SSEG, int TCH, int WPS>
__global__ __launch_bounds__(256, WPS) void dwglu_stream_kernel(int h, int w, int Hc, int B, int R, int rmagic, int rpg,
                                                                int ngrp, int nchunk, const bf16_t* s, uint64_t s_bytes,
                                                                const bf16_t* wdw, const bf16_t* bdw, bf16_t* out,
                                                                bf16_t* u_out) {
    constexpr int NCG = Tile<TCH>::NCG, PPP = Tile<TCH>::PPP, GPX = Tile<TCH>::GPX;
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
    const int total = ngrp * nchunk * B;
    int u = xcd_unit(total);
    if (u >= total) return;
    const int bg = u % ngrp; u /= ngrp;
    const int cx = u % nchunk, b = u / nchunk;
    const int ch0 = cx * TCH;
    const int WP = w + 1, RING = 2 * R + 2, C2 = 2 * Hc;
    const int PHp = tile_slots(RING, WP);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    clear_tile(tile, 2 * PHp * TCH * 2);
    const int cg = lane & (NCG - 1);
    const int ca = ch0 + cg * 4;
    const bool chan_ok = ca < Hc;
    f32x2 wa[9][2], wg[9][2], ba[2], bg2[2];
    {
        const int cs = chan_ok ? ca : 0;
        load_taps(wdw, cs, wa);
        load_taps(wdw, Hc + cs, wg);
        unpack22(*reinterpret_cast<const u32x2*>(bdw + cs), ba);
        unpack22(*reinterpret_cast<const u32x2*>(bdw + Hc + cs), bg2);
    }
    const int nseg = (w + SSEG - 1) / SSEG, nruns = R * nseg;
    const int slot = threadIdx.x / NCG;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(s, s_bytes);
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(out, s_bytes / 2);
    const __amdgpu_buffer_rsrc_t ru = make_rsrc(u_out ? u_out : out, u_out ? s_bytes : 0);
    const bool lane_ch_ok = ch0 + (lane % PPP) * 8 < Hc;
    const int ngroups = (w + GPX - 1) / GPX;
    const uint32_t vlane = (uint32_t)(lane / PPP) * (uint32_t)C2 * 2u + (uint32_t)(lane % PPP) * 16u;

    // rows [ii0, ii0 + nrows) of both halves -> their ring slots; (row, half, pixel group) dealt round-robin to the waves
    auto stage = [&](int ii0, int nrows) {
        int kk = 0;
        for (int r = 0; r < nrows; ++r) {
            const int ii = ii0 + r;
            const bool row_ok = ii >= 0 && ii < h;
            const int q = (ii + 1) % RING;
            for (int half = 0; half < 2; ++half)
                for (int g = 0; g < ngroups; ++g, ++kk) {
                    if ((kk & 3) != wave_s) continue;
                    const int jj0 = g * GPX;
                    const uint32_t soff =
                        row_ok ? (uint32_t)(((((int64_t)b * h + ii) * w + jj0) * C2 + half * Hc + ch0) * 2) : 0u;
                    if ((lane / PPP) < w - jj0)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(
                            rs, (YAT_LDS void*)(tile + (half * PHp + q * WP + 1 + jj0) * (TCH * 2)), 16,
                            row_ok && lane_ch_ok ? vlane : YAT_OOB, soff, 0, 0);
                }
        }
    };

    const int r_lo = bg * rpg, r_hi = min(h, r_lo + rpg);
    const int nsteps = (r_hi - r_lo + R - 1) / R;
    // this thread's run: the same (segment, row-in-step) at every step
    const bool run_ok = slot < nruns && chan_ok;
    const int run = slot < nruns ? slot : 0;
    const int seg = (run * rmagic) >> 16, row = run - seg * R;
    const int j0 = seg * SSEG;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the clear has landed before the DMA writes the tile
    __builtin_amdgcn_s_barrier();
    stage(r_lo - 1, R + 2);

    for (int st = 0; st < nsteps; ++st) {
        const int i0 = r_lo + st * R;
        if (st == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * SSEG) : "memory");
        __builtin_amdgcn_s_barrier();                        // rows of step st visible; step st-1 has released its oldest R rows
        if (st + 1 < nsteps) stage(i0 + R + 1, R);
        const int i = i0 + row;
        const bool row_live = run_ok && i < r_hi;
        const unsigned char* prow[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) prow[r] = tile + ((((i + r) % RING) * WP + j0) * TCH + cg * 4) * 2;   // image row i-1+r
        const int64_t pix0 = ((int64_t)b * h + i) * w + j0;
        dwglu_fwd_walk<SSEG, TCH, 0>(prow, PHp * TCH * 2, row_live, j0, w, pix0, Hc, ca, wa, wg, ba, bg2, rout, ru, rout);
    }
}

// -> 0 when launched.  Applicable when one step's runs fill the run slots (R * nseg close to 256 / NCG) and the ring of
// 2R+2 rows leaves WPS workgroups per CU.
template <int TCH, int WPS>
int launch_stream(int B, int h, int w, int Hc, const bf16_t* s, const bf16_t* wdw, const bf16_t* bdw, bf16_t* out,
                  bf16_t* u_out, hipStream_t stream) {
    constexpr int SSEG = 4;
    static const int rpg_tune = YAT_TUNE_INT("YAT_DW_STREAM_ROWS", 0);   // force the rows one workgroup walks
    const int nseg = (w + SSEG - 1) / SSEG, ns = Tile<TCH>::NS;
    const int R = ns / nseg;
    const uint64_t s_bytes = (uint64_t)B * h * w * 2 * Hc * 2;
    if (R < 1 || R > 8 || R * nseg * 8 < ns * 7 || (Hc & 7) || s_bytes > 0x7fffffffull) return -1;
    const size_t lds = (size_t)2 * tile_slots(2 * R + 2, w + 1) * TCH * 2;
    if (lds > (size_t)lds_budget(WPS)) return -1;
    // rows one workgroup walks: the whole image height when that still gives ~0.8 of the 768 resident workgroups (one round,
    // no halo re-read at all: 32 x 32, B = 8: 704 workgroups, 118.7 us against 122 - 123 us for 8- or 16-row walks), else
    // shorter walks until the grid does
    const int nchunk = (Hc + TCH - 1) / TCH;
    int rpg = ((h + R - 1) / R) * R;
    if (rpg_tune > 0) rpg = min(rpg, ((rpg_tune + R - 1) / R) * R);
    else
        while (rpg > R && (int64_t)((h + rpg - 1) / rpg) * nchunk * B < 600) rpg -= R;
    const int ngrp = (h + rpg - 1) / rpg;
    hipLaunchKernelGGL((dwglu_stream_kernel<SSEG, TCH, WPS>), dim3(grid8((int64_t)ngrp * nchunk * B)), dim3(256), lds, stream,
                       h, w, Hc, B, R, (65536 + R - 1) / R, rpg, ngrp, nchunk, s, s_bytes, wdw, bdw, out, u_out);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Backward pass 2 (same staging scheme; all 2*Hc channels are independent here, TCH per workgroup):
//   du tile: rows i0-1 .. i0+R (zero outside the image), with the shared zero column;
//   dz[i,j] = SiLU'(z[i,j]) * bf16( sum_taps W[tap] du[i-di, j-dj] );  dW[tap] += s[i,j] * du[i-di, j-dj];  db += du[i,j]
// s = bf16(z sigmoid(z)) is what the conv_inverted GEMM stored (gemm_common.hpp: silu_f on the rounded z, rounded again by
// the store).  Since round 5 it is recomputed here, bit for bit, from the z this pass reads anyway -- the sigmoid is kept for
// the SiLU' of the same column two iterations on -- so s is not read at all: a quarter of the pass's bytes (181 -> 163 us
// at 32 x 32, 239 -> 175 at 16 x 64; profiles/r05_o_*).
// z is needed at the output position only, and comes from either of two places:
//   Z_IN_LDS (TCH = 32): rows i0 .. i0+R-1 staged behind the du tile;
//   otherwise (TCH = 64): straight from global, 8 bytes per lane, 16 lanes = one whole 128-byte pixel slice, all SEG columns
//   of the run in flight before the column walk -- only du is tiled, which is what makes 64 channels per tile fit.
// The thread's dW/db registers are summed over the run slots through the (then free) tile memory: one partial row
// per workgroup, ws[(b*ngrp + band group)][2Hc*PK].
// (two workgroups per CU; sized for three -- 53 KB tiles, which the band form's 166 registers would allow -- it is 5 .. 8 %
// slower: shorter bands re-read more halo; profiles/r05_q_*)
template <int TCH, bool Z_IN_LDS>
__global__ __launch_bounds__(256, 2) void dwglu_bwd2_kernel(int h, int w, int Hc, int B, int R, int rmagic, int nbands,
                                                            int bpb, int nchunk, const bf16_t* z, const bf16_t* du,
                                                            uint64_t bytes, const bf16_t* wdw, bf16_t* dz, float* ws) {
    constexpr int NCG = Tile<TCH>::NCG, PPP = Tile<TCH>::PPP;
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
    const int ngrp = (nbands + bpb - 1) / bpb;
    const int total = ngrp * nchunk * B;
    int u = xcd_unit(total);
    if (u >= total) return;
    const int bg = u % ngrp; u /= ngrp;
    const int cx = u % nchunk, b = u / nchunk;
    const int ch0 = cx * TCH, C2 = 2 * Hc;
    const int WP = w + 1;
    const int PHd = tile_slots(R + 2, WP), PHc = Z_IN_LDS ? tile_slots(R, WP) : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, nslots = blockDim.x / NCG;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    clear_tile(tile, (PHd + PHc) * TCH * 2);
    const int cg = lane & (NCG - 1);
    const int c0 = ch0 + cg * 4;
    const bool chan_ok = c0 < C2;
    // channel pairs as explicit 2-vectors, as in the forward
    f32x2 wt[9][2], dW[9][2], db[2], dzs[2];                 // dzs: column sum of dz = bias gradient of conv_inverted
    {
        const int cs = chan_ok ? c0 : 0;
        load_taps(wdw, cs, wt);
#pragma unroll
        for (int t = 0; t < 9; ++t) dW[t][0] = dW[t][1] = f32x2{0.f, 0.f};
        db[0] = db[1] = dzs[0] = dzs[1] = f32x2{0.f, 0.f};
    }
    const int nseg = (w + SEG - 1) / SEG, nruns = R * nseg;
    const int slot = threadIdx.x / NCG;
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(du, bytes), rz = make_rsrc(z, bytes);
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(dz, bytes);
    const bool lane_ch_ok = ch0 + (lane % PPP) * 8 < C2;

    for (int rb = bg * bpb; rb < min(nbands, (bg + 1) * bpb); ++rb) {
        const int i0 = rb * R;
        __syncthreads();
        stage_rows<TCH>(rd, tile, 0, R + 2, i0 - 1, b, h, w, WP, C2, ch0, lane_ch_ok, wave_s, nwaves, lane);
        if constexpr (Z_IN_LDS) stage_rows<TCH>(rz, tile, PHd, R, i0, b, h, w, WP, C2, ch0, lane_ch_ok, wave_s, nwaves, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        for (int run = slot; run < nruns; run += nslots) {
            const int seg = (run * rmagic) >> 16, row = run - seg * R;
            const int i = i0 + row;
            if (i >= h || !chan_ok) continue;
            const int j0 = seg * SEG;
            const unsigned char* pd = tile + ((row * WP + j0) * TCH + cg * 4) * 2;                 // du rows row .. row+2
            const unsigned char* pz = tile + ((PHd + row * WP + j0 + 1) * TCH + cg * 4) * 2;       // z at output column j0
            const int64_t pix0 = ((int64_t)b * h + i) * w + j0;
            u32x2 zv[SEG];                                  // global z: columns past the image read 0
            if constexpr (!Z_IN_LDS) {
#pragma unroll
                for (int t = 0; t < SEG; ++t) {
                    const uint32_t off = j0 + t < w ? (uint32_t)(((pix0 + t) * C2 + c0) * 2) : YAT_OOB;
                    zv[t] = __builtin_amdgcn_raw_buffer_load_b64(rz, off, 0, 0);
                }
            }
            f32x2 acc[3][2], S[3][2], SG[3][2], ZC[3][2];
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[m][0] = acc[m][1] = f32x2{0.f, 0.f};
            u32x2 nxt[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) nxt[r] = *reinterpret_cast<const u32x2*>(pd + (r * WP) * TCH * 2);
#pragma unroll
            for (int t = 0; t < SEG + 2; ++t) {             // du column j0 - 1 + t
                u32x2 cur[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) cur[r] = nxt[r];
                if (t + 1 < SEG + 2) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) nxt[r] = *reinterpret_cast<const u32x2*>(pd + (r * WP + t + 1) * TCH * 2);
                }
                if (t < SEG) {                              // s of output column t (zero past the image: it must not count)
                    if constexpr (Z_IN_LDS) unpack22(*reinterpret_cast<const u32x2*>(pz + t * TCH * 2), ZC[t % 3]);
                    else unpack22(zv[t], ZC[t % 3]);
                    // past the image the LDS tile wraps to real data; a global z reads as 0 there and s = 0 * sigmoid(0) = 0
                    const bool in_img = !Z_IN_LDS || j0 + t < w;
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const float zz = ZC[t % 3][pr][e], sg = sigmoid_f(zz);
                            SG[t % 3][pr][e] = sg;
                            S[t % 3][pr][e] = in_img ? rbf(zz * sg) : 0.f;
                        }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    f32x2 d[2];
                    unpack22(cur[r], d);
                    const int tr = (2 - r) * 3;             // du row i + r - 1 -> tap row 2 - r
#pragma unroll
                    for (int tc = 0; tc < 3; ++tc) {        // output o = t + tc - 2 takes tap column tc
                        const int o = t + tc - 2;
                        if (o < 0 || o >= SEG) continue;
#pragma unroll
                        for (int pr = 0; pr < 2; ++pr) {
                            acc[o % 3][pr] += wt[tr + tc][pr] * d[pr];
                            dW[tr + tc][pr] += S[o % 3][pr] * d[pr];
                        }
                    }
                    if (r == 1 && t >= 1 && t <= SEG) {     // du[i, j0 + t - 1]: the bias gradient; past the image edge the
                        const float m = j0 + t - 1 < w ? 1.f : 0.f;                  // tile wraps to real data: mask it
                        db[0] += m * d[0];
                        db[1] += m * d[1];
                    }
                }
                const int o = t - 2;
                if (o >= 0) {
                    float ds[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) ds[e] = dsilu_from_sigmoid(ZC[o % 3][e >> 1][e & 1], SG[o % 3][e >> 1][e & 1]);
                    const f32x2 a0 = acc[o % 3][0], a1 = acc[o % 3][1];
                    const u32x2 v = pack4(rbf(a0[0]) * ds[0], rbf(a0[1]) * ds[1], rbf(a1[0]) * ds[2], rbf(a1[1]) * ds[3]);
                    acc[o % 3][0] = acc[o % 3][1] = f32x2{0.f, 0.f};
                    const bool live = j0 + o < w;
                    f32x2 vz[2];
                    unpack22(live ? v : u32x2{0u, 0u}, vz);     // the rounded values, as a later column sum over dz would see them
                    dzs[0] += vz[0];
                    dzs[1] += vz[1];
                    __builtin_amdgcn_raw_buffer_store_b64(v, rout, live ? (uint32_t)(((pix0 + o) * C2 + c0) * 2) : YAT_OOB, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // ---- sum the run slots through LDS: red[slot][cg*4*PK + e*PK + k]; one partial row per workgroup
    __syncthreads();
    float* red = reinterpret_cast<float*>(tile);
    {
        float* mine = red + slot * (NCG * 4 * PK) + cg * 4 * PK;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int t = 0; t < 9; ++t) mine[e * PK + t] = dW[t][e >> 1][e & 1];
            mine[e * PK + 9] = db[e >> 1][e & 1];
            mine[e * PK + 10] = dzs[e >> 1][e & 1];
        }
    }
    __syncthreads();
    float* wp = ws + ((int64_t)b * ngrp + bg) * C2 * PK + (int64_t)ch0 * PK;
    const int nvalid = min(TCH, C2 - ch0) * PK;
    for (int idx = threadIdx.x; idx < nvalid; idx += blockDim.x) {
        float t = 0.f;
        for (int sl = 0; sl < nslots; ++sl) t += red[sl * (NCG * 4 * PK) + idx];
        wp[idx] = t;
    }
}

// rows per band of pass 2, two workgroups per CU: the du tile with its halo, the z tile behind it when z is staged, and
// never less than the slot reduction needs.  The global-z form may use the whole half of a CU's LDS.
template <int TCH, bool Z_IN_LDS>
inline int pick_band_rows_bwd2(int h, int w, size_t* lds_bytes) {
    constexpr int NCG = Tile<TCH>::NCG, ns = Tile<TCH>::NS;
    constexpr size_t cap = Z_IN_LDS ? 65536 : lds_budget(2);
    const int nseg = (w + SEG - 1) / SEG, WP = w + 1;
    int best = 0;
    double best_score = 0;
    for (int R = 4; R <= 16 && R <= ((h + 1) & ~1); ++R) {     // >= 4 rows: the partial rows fit the workspace
        size_t bytes = (size_t)(tile_slots(R + 2, WP) + (Z_IN_LDS ? tile_slots(R, WP) : 0)) * TCH * 2;
        if (bytes < ns * NCG * 4 * PK * sizeof(float)) bytes = ns * NCG * 4 * PK * sizeof(float);
        if (bytes > cap) break;
        const int nruns = R * nseg, passes = (nruns + ns - 1) / ns;
        const int nb = (h + R - 1) / R;
        // du is a third of the traffic: its halo re-read weighs a third
        const double score = (double)nruns / (passes * ns) * (3.0 * R / (3.0 * R + 2.0)) * h / (nb * R);
        if (score > best_score) { best_score = score; best = R; *lds_bytes = bytes; }
    }
    return best;
}

// -> number of partial rows written to ws (0: not applicable, the caller uses another kernel)
template <int TCH, bool Z_IN_LDS>
int launch_bwd2(int B, int h, int w, int Hc, const bf16_t* z, const bf16_t* du, const bf16_t* wdw, bf16_t* dz, float* ws,
                hipStream_t stream) {
    const int C2 = 2 * Hc;
    size_t lds = 0;
    const uint64_t bytes = (uint64_t)B * h * w * C2 * 2;
    const int R = (w <= 64 && !(C2 & 7) && bytes <= 0x7fffffffull) ? pick_band_rows_bwd2<TCH, Z_IN_LDS>(h, w, &lds) : 0;
    if (!R) return 0;
    static bool attr_set = false;
    if (!attr_set && lds > 65536) {
        if (hipFuncSetAttribute((const void*)dwglu_bwd2_kernel<TCH, Z_IN_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds_budget(2)) != hipSuccess)
            return 0;
        attr_set = true;
    }
    const int nbands = (h + R - 1) / R, nchunk = (C2 + TCH - 1) / TCH;
    const int bpb = bands_per_wg(nbands, (int64_t)nchunk * B, 4 * 512);
    const int ngrp = (nbands + bpb - 1) / bpb;      // B * ngrp <= B * ceil(h / 4): the partial rows fit the direct path's workspace
    hipLaunchKernelGGL((dwglu_bwd2_kernel<TCH, Z_IN_LDS>), dim3(grid8((int64_t)ngrp * nchunk * B)), dim3(256), lds, stream, h,
                       w, Hc, B, R, (65536 + R - 1) / R, nbands, bpb, nchunk, z, du, bytes, wdw, dz, ws);
    return B * ngrp;
}

}  // namespace
