// Image ingest kernels: Pillow's antialiased bilinear resize of a packed uint8 RGB image, bit for bit
// (img.resize((tw, th), Image.BILINEAR) == ImagingResample with the triangle filter), written into a slot of the
// [B, th, tw, 3] uint8 batch that the VAE encoders' encode_uint8 reads.
//
// Pillow's 8-bit resample is integer arithmetic over per-axis tables: output index i reads n_i source samples from xmin_i
// on, out = clamp((2^21 + sum_x in[xmin_i + x] * k_i[x]) >> 22, 0, 255), horizontal pass first, its result rounded to uint8
// before the vertical pass reads it.  The tables are computed in doubles on the host (yat_amd/image.py resample_tables) and
// arrive as one packed int32 block
//     [ hbounds: tw x (xmin, n) | hk: tw x ksize_h | vbounds: th x (ymin, n) | vk: th x ksize_v ]
// where an axis whose size does not change has ksize 0 and no entries (the kernels then use the identity tap k = 2^22, for
// which the pass returns its input).  The kernels do integer work only; 32-bit accumulators suffice (sum k ~ 2^22, a pixel
// <= 255: below 2^30 + 2^21).
//
//   plan 1  resize_tile_kernel: a workgroup owns a 16-row x 64-pixel output tile.  It runs the horizontal pass of the source
//           rows its 16 output rows read (ymin of its first row .. ymin + n of its last) into LDS as uint8 [rows][192],
//           then the vertical pass out of LDS.  One thread per byte column (pixel, channel) of the tile in both passes, so
//           the lanes of a wave touch consecutive bytes of a source row, of LDS and of dst.
//   plan 2  when 16 output rows read more source rows than the LDS image holds (TILE_ROWS; vertical reductions beyond ~9x):
//           hpass_kernel over all H rows into the caller's [H, tw, 3] workspace, then vpass_kernel into dst.
//
// Ragged ends: rows of 3-byte pixels are not dword aligned and neither src nor a dst slot has slack around it, so EVERY
// access to src, the workspace and dst is a single-byte load / store of an element whose index was bounded first -- there is
// no wide access to round down or up at a row's or the image's end, and no lane of a partial tile touches memory.  The
// tables are device data the library cannot inspect, so the kernels clamp what they read from them (xmin to [0, in - 1], n
// to [0, min(ksize, in - xmin)], LDS rows to the image held): a wrong table gives wrong pixels, never an access outside
// src[0 .. H*W*3), the workspace, or dst[0 .. th*tw*3).
#include "common.hpp"

#include <math.h>

namespace {

constexpr int PREC = 22;              // Pillow's PRECISION_BITS
constexpr int TILE_H = 16;            // output rows per workgroup
constexpr int TILE_W = 64;            // output pixels per tile row
constexpr int PITCH = TILE_W * 3;     // bytes per LDS row = threads per workgroup
constexpr int TILE_ROWS = 170;        // source rows the LDS image holds: 170 * 192 B = 31.9 KiB, 5 workgroups per CU

struct Taps {
    const int* bounds;   // [out][2] or null (identity)
    const int* kk;       // [out][ksize]
    int ksize;
    int in_size;
};

// (first source index, tap count) of output index i, clamped to the source
__device__ __forceinline__ void tap_range(const Taps& t, int i, int& first, int& n) {
    if (t.ksize == 0) {
        first = i;
        n = 1;
        return;
    }
    first = min(max(t.bounds[2 * i], 0), t.in_size - 1);
    n = min(max(t.bounds[2 * i + 1], 0), min(t.ksize, t.in_size - first));
}
__device__ __forceinline__ int tap_k(const Taps& t, int i, int x) { return t.ksize == 0 ? (1 << PREC) : t.kk[(size_t)i * t.ksize + x]; }
__device__ __forceinline__ uint8_t clip8(int acc) { return (uint8_t)min(max(acc >> PREC, 0), 255); }

__global__ __launch_bounds__(PITCH) void resize_tile_kernel(int W, int th, int tw, Taps ht, Taps vt,
                                                            const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
    __shared__ uint8_t rows[TILE_ROWS * PITCH];
    const int tiles_x = (tw + TILE_W - 1) / TILE_W;
    const int ty0 = (blockIdx.x / tiles_x) * TILE_H, tx0 = (blockIdx.x % tiles_x) * TILE_W;
    const int ny = min(TILE_H, th - ty0);
    const int e = threadIdx.x, col = tx0 + e / 3, c = e - 3 * (e / 3);
    // source rows of this tile (uniform): bounds are monotonic, but take the maximum anyway
    int row0, nrows = 0;
    {
        int f, n;
        tap_range(vt, ty0, row0, n);
        for (int y = 0; y < ny; ++y) {
            tap_range(vt, ty0 + y, f, n);
            nrows = max(nrows, f + n - row0);
        }
        nrows = min(nrows, TILE_ROWS);
    }
    if (col < tw) {
        int x0, nx;
        tap_range(ht, col, x0, nx);
        const uint8_t* s = src + (size_t)row0 * W * 3 + x0 * 3 + c;
        // four source rows per walk of the taps: one coefficient load feeds four independent byte loads (a row past the
        // tile's last is read as that last row again and not stored)
        for (int r = 0; r < nrows; r += 4) {
            const uint8_t* p[4];
            int acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[j] = s + (size_t)min(r + j, nrows - 1) * W * 3;
                acc[j] = 1 << (PREC - 1);
            }
            for (int x = 0; x < nx; ++x) {
                const int k = tap_k(ht, col, x);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += (int)p[j][3 * x] * k;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r + j < nrows) rows[(r + j) * PITCH + e] = clip8(acc[j]);
        }
    }
    __syncthreads();
    if (col >= tw) return;
    for (int y = 0; y < ny; ++y) {
        int f, n;
        tap_range(vt, ty0 + y, f, n);
        int acc = 1 << (PREC - 1);
        for (int x = 0; x < n; ++x) {
            const unsigned r = (unsigned)(f + x - row0);
            if (r < (unsigned)nrows) acc += (int)rows[r * PITCH + e] * tap_k(vt, ty0 + y, x);
        }
        dst[((size_t)(ty0 + y) * tw + col) * 3 + c] = clip8(acc);
    }
}

// plan 2, launch 1: ws[r][col][c] for every source row r; one thread per output byte
__global__ __launch_bounds__(256) void hpass_kernel(int H, int W, int tw, Taps ht, const uint8_t* __restrict__ src,
                                                    uint8_t* __restrict__ ws) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)H * tw * 3) return;
    const int r = i / (tw * 3), e = i - r * (tw * 3), col = e / 3, c = e - 3 * col;
    int x0, nx;
    tap_range(ht, col, x0, nx);
    const uint8_t* s = src + (size_t)r * W * 3 + x0 * 3 + c;
    int acc = 1 << (PREC - 1);
    for (int x = 0; x < nx; ++x) acc += (int)s[3 * x] * tap_k(ht, col, x);
    ws[i] = clip8(acc);
}

// plan 2, launch 2: dst[y][e] from ws [H][tw * 3]
__global__ __launch_bounds__(256) void vpass_kernel(int th, int tw, Taps vt, const uint8_t* __restrict__ ws,
                                                    uint8_t* __restrict__ dst) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)th * tw * 3) return;
    const int y = i / (tw * 3), e = i - y * (tw * 3);
    int f, n;
    tap_range(vt, y, f, n);
    const uint8_t* s = ws + (size_t)f * tw * 3 + e;
    int acc = 1 << (PREC - 1);
    for (int x = 0; x < n; ++x) acc += (int)s[(size_t)x * tw * 3] * tap_k(vt, y, x);
    dst[i] = clip8(acc);
}

// Pillow's ksize of an axis; 0 for an axis that is skipped
int axis_ksize(int in_size, int out_size) {
    if (in_size == out_size) return 0;
    const double scale = (double)in_size / (double)out_size;
    return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

bool sizes_ok(int H, int W, int th, int tw) {
    if (H <= 0 || W <= 0 || th <= 0 || tw <= 0) return false;
    return (int64_t)H * W * 3 < (1ll << 31) && (int64_t)th * tw * 3 < (1ll << 31);
}

// Source rows that TILE_H consecutive output rows can read: (TILE_H - 1) scale + 2 support + 1 at the most, since
// ymin >= c - support - 0.5 and ymin + n <= c + support + 0.5; rounded up.
int64_t tile_rows_bound(int H, int th) {
    const int t = th < TILE_H ? th : TILE_H;
    if (H == th) return t;
    return (int64_t)ceil((double)t * (double)H / (double)th) + axis_ksize(H, th);
}

}  // namespace

extern "C" {

int yat_image_resize_plan(int H, int W, int th, int tw) {
    if (!sizes_ok(H, W, th, tw)) return YAT_EINVAL;
    if (tile_rows_bound(H, th) <= TILE_ROWS) return 1;
    return (int64_t)H * tw * 3 < (1ll << 31) ? 2 : YAT_EINVAL;
}

uint64_t yat_image_resize_workspace_bytes(int H, int W, int th, int tw) {
    return yat_image_resize_plan(H, W, th, tw) == 2 ? (uint64_t)H * tw * 3 : 0;
}

int yat_image_resize_u8(int H, int W, int th, int tw, int ksize_h, int ksize_v, const void* src, const void* tables,
                        void* dst, void* workspace, yat_stream_t stream) {
    const int plan = yat_image_resize_plan(H, W, th, tw);
    if (plan < 0 || !src || !dst || src == dst) return YAT_EINVAL;
    if (ksize_h != axis_ksize(W, tw) || ksize_v != axis_ksize(H, th)) return YAT_EINVAL;
    if ((ksize_h || ksize_v) && !tables) return YAT_EINVAL;
    if (plan == 2 && !workspace) return YAT_EINVAL;
    const int* t = (const int*)tables;
    Taps ht{nullptr, nullptr, 0, W}, vt{nullptr, nullptr, 0, H};
    if (ksize_h) {
        ht = Taps{t, t + 2 * (int64_t)tw, ksize_h, W};
        t += (2 + (int64_t)ksize_h) * tw;
    }
    if (ksize_v) vt = Taps{t, t + 2 * (int64_t)th, ksize_v, H};
    const uint8_t* s = (const uint8_t*)src;
    uint8_t* d = (uint8_t*)dst;
    if (plan == 1) {
        const int64_t tiles = (int64_t)((tw + TILE_W - 1) / TILE_W) * ((th + TILE_H - 1) / TILE_H);
        hipLaunchKernelGGL(resize_tile_kernel, dim3((unsigned)tiles), dim3(PITCH), 0, (hipStream_t)stream, W, th, tw, ht, vt, s, d);
        YAT_CHECK_LAUNCH();
        return YAT_OK;
    }
    uint8_t* ws = (uint8_t*)workspace;
    hipLaunchKernelGGL(hpass_kernel, dim3((unsigned)(((int64_t)H * tw * 3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       H, W, tw, ht, s, ws);
    YAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(vpass_kernel, dim3((unsigned)(((int64_t)th * tw * 3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       th, tw, vt, (const uint8_t*)ws, d);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
