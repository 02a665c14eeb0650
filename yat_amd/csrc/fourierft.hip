// FourierFT adapters (``lora_algo: fourierft``) for gfx950: the sparse half of the sparse-spectrum inverse DFT and of its adjoint.
//
// [RECALL peft/tuners/fourierft/layer.py -- parity unpinned]  For a target Linear / 1x1 Conv with weight [out, in], n real
// coefficients c_l at fixed positions (u_l, v_l) of an otherwise empty [out, in] spectrum:
//   delta_w[j, k] = s * sum_l c_l * cos(2 pi (u_l j / out + v_l k / in))          (= ifft2(dense_spectrum, norm).real * scaling)
// The transform is separable.  With rows = the SHORT dimension and cols = the long one (out > in works on the transpose: the
// positions are then grouped by v and the roles of u and v are exchanged by the caller), cos(a + b) = cos a cos b - sin a sin b:
//   yat_fourier_expand   : Y[u, k] = bf16(sum_{e in row u} s c_e cos phi),  Y[rows + u, k] = bf16(sum_e s c_e sin phi),
//                          phi = 2 pi ((v_e k) mod cols) / cols -- the long dimension, sparse: only the populated (u, v) cost;
//   an ordinary GEMM     : delta_w = B [rows, 2 rows] Y,  B[j, u] = cos 2 pi (u j) / rows,  B[j, rows + u] = -sin .. -- the short
//                          dimension, dense, on the matrix cores;
//   the adjoint GEMM     : Z [2 rows, cols] = B^T d_delta_w;
//   yat_fourier_contract : dc[perm[e]] = bf16(s * sum_k (Z[u_e, k] cos phi + Z[rows + u_e, k] sin phi)).
// The positions come as a CSR over the spectrum's rows (row_ptr [rows + 1], col = v per entry, perm = the coefficient's place
// in the spectrum vector).  cos / sin come from a host-built table T[m] = (cos, sin)(2 pi m / cols), fp32 pairs: the device
// never evaluates a trigonometric function, and a phase is an integer below cols.  Both kernels keep the table in LDS when it
// fits (8 cols bytes <= 128 KiB of the CU's 160) and read it from global memory (L2) otherwise; sums are fp32 in a fixed order.
#include "common.hpp"
#include "../../include/yat_hip.h"

namespace {

constexpr int kMaxDim = 46340;           // (v * k) stays below 2^31 for v, k < 46341
constexpr int kLdsTableCols = 16384;     // the table's 8 bytes per entry: 128 KiB
constexpr int ET = 256;                  // entries staged per tile of the expand kernel: (v, s c) = 2 KiB

// (a * b) mod d for 0 <= a, b < d <= 46340 without an integer division: the quotient from a float reciprocal is off by at most
// one (a * b < 2^31 and the quotient < 2^16 carry a relative error below 2^-21), corrected in both directions.
__device__ __forceinline__ int mulmod(int a, int b, int d, float inv_d) {
    const int p = a * b;
    int r = p - (int)((float)p * inv_d) * d;
    if (r < 0) r += d;
    if (r >= d) r -= d;
    return r;
}

// The table in LDS (or the global one); `fill` = this workgroup has entries and copies it, 8-byte loads along the table.
template <bool LDS_TABLE>
__device__ __forceinline__ const f32x2* stage_table(char* lds, const f32x2* table, int cols, bool fill) {
    if constexpr (LDS_TABLE) {
        f32x2* t = reinterpret_cast<f32x2*>(lds);
        if (fill)
            for (int i = threadIdx.x; i < cols; i += blockDim.x) t[i] = table[i];
        return t;
    } else {
        return table;
    }
}

// grid (ceil(cols / 8 / block), rows): a workgroup owns one spectrum row u and a run of 16-byte chunks of its two output rows,
// a thread one chunk (8 consecutive k).  The row's entries pass through LDS a tile at a time; per entry a thread finds its first
// phase with one mulmod and walks on by v with a conditional subtract.  A row without entries writes zeros (no memset).
template <bool LDS_TABLE>
__global__ __launch_bounds__(1024) void fourier_expand_kernel(int rows, int cols, int n, const int* row_ptr, const int* col,
                                                              const int* perm, const bf16_t* spec, float s, const f32x2* table,
                                                              bf16_t* Y, int ldy) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* ev = reinterpret_cast<int*>(smem);
    float* ec = reinterpret_cast<float*>(smem + ET * 4);
    const int u = blockIdx.y;
    int e0 = row_ptr[u], e1 = row_ptr[u + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > n ? n : e1;                                      // (a broken CSR reads nothing outside the n entries)
    const f32x2* tab = stage_table<LDS_TABLE>(smem + ET * 8, table, cols, e1 > e0);
    const int k0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
    const bool live = k0 < cols;
    const float inv = 1.0f / (float)cols;
    float ac[8], sn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ac[j] = sn[j] = 0.f;
    for (int t0 = e0; t0 < e1; t0 += ET) {
        const int nt = e1 - t0 < ET ? e1 - t0 : ET;
        __syncthreads();                                       // the previous tile is consumed
        for (int i = threadIdx.x; i < nt; i += blockDim.x) {
            const int v = col[t0 + i], q = perm[t0 + i];
            const bool ok = (unsigned)v < (unsigned)cols && (unsigned)q < (unsigned)n;
            ev[i] = ok ? v : 0;
            ec[i] = ok ? s * bf2f(spec[q]) : 0.f;
        }
        __syncthreads();                                       // (the first one also covers the table)
        if (live) {
            for (int i = 0; i < nt; ++i) {
                const int v = ev[i];
                const float c = ec[i];
                int p = mulmod(v, k0, cols, inv);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f32x2 w = tab[p];
                    ac[j] += c * w[0];
                    sn[j] += c * w[1];
                    p += v;
                    if (p >= cols) p -= cols;
                }
            }
        }
    }
    if (live) {
        *reinterpret_cast<u32x4*>(Y + (int64_t)u * ldy + k0) = pack8(ac);
        *reinterpret_cast<u32x4*>(Y + (int64_t)(rows + u) * ldy + k0) = pack8(sn);
    }
}

// grid (rows): a workgroup owns one spectrum row u (and leaves at once when the row is empty), a wave one entry of it at a time.
// A lane reads 16-byte chunks of Z's two rows (the same two rows for every entry of the workgroup: L2), sums its products in
// fp32, and the lanes are reduced by wave_sum.
template <bool LDS_TABLE>
__global__ __launch_bounds__(1024) void fourier_contract_kernel(int rows, int cols, int n, const int* row_ptr, const int* col,
                                                                const int* perm, const bf16_t* Z, int ldz, float s,
                                                                const f32x2* table, bf16_t* dc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int u = blockIdx.x;
    int e0 = row_ptr[u], e1 = row_ptr[u + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > n ? n : e1;
    if (e1 <= e0) return;                                      // (uniform: before the only barrier)
    const f32x2* tab = stage_table<LDS_TABLE>(smem, table, cols, true);
    if (LDS_TABLE) __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const bf16_t* zc = Z + (int64_t)u * ldz;
    const bf16_t* zs = Z + (int64_t)(rows + u) * ldz;
    const float inv = 1.0f / (float)cols;
    const int chunks = cols >> 3;
    for (int e = e0 + wave; e < e1; e += nw) {
        const int v = col[e], q = perm[e];
        if ((unsigned)v >= (unsigned)cols || (unsigned)q >= (unsigned)n) continue;      // (wave-uniform)
        float acc = 0.f;
        for (int ch = lane; ch < chunks; ch += 64) {
            const int k0 = ch * 8;
            float a[8], b[8];
            unpack8(*reinterpret_cast<const u32x4*>(zc + k0), a);
            unpack8(*reinterpret_cast<const u32x4*>(zs + k0), b);
            int p = mulmod(v, k0, cols, inv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x2 w = tab[p];
                acc += a[j] * w[0];
                acc += b[j] * w[1];
                p += v;
                if (p >= cols) p -= cols;
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) dc[q] = f2bf(s * acc);
    }
}

// Launch with the dynamic LDS the kernel needs; more than 64 KiB takes the attribute, set once per kernel.
template <auto Kernel, class... Args>
int launch_lds(dim3 grid, int block, int lds, hipStream_t st, Args... args) {
    static bool attr_set = false;
    if (lds > 65536 && !attr_set) {
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * kLdsTableCols + ET * 8) !=
            hipSuccess)
            return YAT_EINVAL;
        attr_set = true;
    }
    hipLaunchKernelGGL(Kernel, grid, dim3(block), lds, st, args...);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

bool fourier_args_ok(int rows, int cols, int n, const void* row_ptr, const void* col, const void* perm, const void* table,
                     int ld) {
    return rows >= 1 && rows <= kMaxDim && cols >= 8 && cols <= kMaxDim && !(cols & 7) && n >= 1 && ld >= cols && !(ld & 7) &&
           row_ptr && col && perm && table;
}

}  // namespace

extern "C" {

int yat_fourier_expand(int rows, int cols, int n, const int* row_ptr, const int* col, const int* perm, const void* spectrum,
                       float s, const void* table, void* Y, int ldy, yat_stream_t stream) {
    if (!fourier_args_ok(rows, cols, n, row_ptr, col, perm, table, ldy) || !spectrum || !Y) return YAT_EINVAL;
    const int chunks = cols >> 3;
    const int block = chunks >= 1024 ? 1024 : (chunks + 63) / 64 * 64;
    const dim3 grid((chunks + block - 1) / block, rows);
    hipStream_t st = (hipStream_t)stream;
    const f32x2* tab = (const f32x2*)table;
    if (cols <= kLdsTableCols)
        return launch_lds<fourier_expand_kernel<true>>(grid, block, ET * 8 + 8 * cols, st, rows, cols, n, row_ptr, col, perm,
                                                       (const bf16_t*)spectrum, s, tab, (bf16_t*)Y, ldy);
    return launch_lds<fourier_expand_kernel<false>>(grid, block, ET * 8, st, rows, cols, n, row_ptr, col, perm,
                                                    (const bf16_t*)spectrum, s, tab, (bf16_t*)Y, ldy);
}

int yat_fourier_contract(int rows, int cols, int n, const int* row_ptr, const int* col, const int* perm, const void* Z, int ldz,
                         float s, const void* table, void* dc, yat_stream_t stream) {
    if (!fourier_args_ok(rows, cols, n, row_ptr, col, perm, table, ldz) || !Z || !dc) return YAT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const f32x2* tab = (const f32x2*)table;
    if (cols <= kLdsTableCols)                                 // 16 waves share the staged table
        return launch_lds<fourier_contract_kernel<true>>(dim3(rows), 1024, 8 * cols, st, rows, cols, n, row_ptr, col, perm,
                                                         (const bf16_t*)Z, ldz, s, tab, (bf16_t*)dc);
    return launch_lds<fourier_contract_kernel<false>>(dim3(rows), 256, 0, st, rows, cols, n, row_ptr, col, perm, (const bf16_t*)Z,
                                                      ldz, s, tab, (bf16_t*)dc);
}

}  // extern "C"
