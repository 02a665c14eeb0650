// bf16 MFMA GEMM family for gfx950 with fused epilogues.
//
//   C[M,N] = epilogue( A_op[M,K] * B_op[K,N] ),   fp32 accumulate, bf16 in/out
//
// Three operand layouts cover forward, dgrad and wgrad of every Linear / 1x1-conv in the SANA
// block (reference call sites: utils/patch_sana_attention_layers.py:94-113 via diffusers
// Attention/GLUMBConv; autograd backward at common/trainer.py:344):
//   NT  (a_t=0,b_t=0)  A[M,K] k-contiguous, B[N,K] k-contiguous   y  = x W^T
//   NN  (a_t=0,b_t=1)  A[M,K] k-contiguous, B[K,N] n-contiguous   dx = dy W
//   TN  (a_t=1,b_t=1)  A[K,M] m-contiguous, B[K,N] n-contiguous   dW = dy^T x
//
// Design (MI355X-first): 128x128x64 tile, 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32
// accumulators.  Operand tiles are moved HBM->LDS by LDS-DMA (buffer_load ... lds, 16 B/lane,
// hardware range check supplies the zero padding of ragged M/N/K tails), double-buffered, one
// barrier per K-tile.  LDS images are lane-linear (DMA constraint) with the bank-conflict
// swizzle applied to the *source* address and undone on the read:
//   k-contiguous operand: [128 rows][64 k] 128-B rows, ds_read_b128, chunk ^= (row>>1)&7
//   k-strided operand   : [64 k][128 cols] 256-B rows, ds_read_b64_tr_b16 (hardware
//                         transpose), 32-B block ^= (k&3)|((k>>3)&1)<<2
// MFMA operands are swapped (D = B_frag x A_frag) so a lane owns 4 consecutive n of one row m:
// the epilogue loads/stores 8 B per lane.  Workgroups are remapped so each XCD (private L2)
// works on a contiguous band of tiles.
#include <math.h>
#include "common.hpp"
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include "gemm_common.hpp"
#include "../../include/yat_hip.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int STAGE_BYTES = (BM * BK + BN * BK) * 2;  // 32 KiB
constexpr int LDS_BYTES = 2 * STAGE_BYTES;            // 64 KiB -> 2 workgroups / CU


__device__ __forceinline__ uint32_t trswz(uint32_t krow) { return ((krow & 3) | (((krow >> 3) & 1) << 2)) << 1; }

// stage one operand tile (16 KiB) into LDS: 4 LDS-DMA instructions per wave
template <bool KSTRIDED>
__device__ __forceinline__ void stage_tile(__amdgpu_buffer_rsrc_t rsrc, char* lds, int ld, int idx0, int idx_max,
                                           int k0, int K, int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int piece = j * 4 + wave;  // 1-KiB piece index 0..15
        uint32_t voff;
        if (!KSTRIDED) {
            const int r = piece * 8 + (lane >> 3);           // tile row (m or n index)
            const int c = swz128(r, lane & 7);               // source chunk for this LDS slot
            const int gi = idx0 + r, gk = k0 + c * 8;
            voff = (gi < idx_max && gk < K) ? (uint32_t)(((int64_t)gi * ld + gk) * 2) : YAT_OOB;
        } else {
            const int r = piece * 4 + (lane >> 4);           // tile k-row
            const int c = (lane & 15) ^ trswz(r);            // source chunk (8 cols)
            const int gk = k0 + r, gi = idx0 + c * 8;
            voff = (gk < K && gi < idx_max) ? (uint32_t)(((int64_t)gk * ld + gi) * 2) : YAT_OOB;
        }
        lds_dma16(rsrc, (YAT_LDS void*)(lds + piece * 1024), voff);
    }
}

// fragment for 16 consecutive output indices starting at idx0 (tile-local), k-substep kk (32 wide)
template <bool KSTRIDED>
__device__ __forceinline__ bf16x8 load_frag(const char* lds, int idx0, int kk, int lane) {
    if (!KSTRIDED) {
        const uint32_t r = idx0 + (lane & 15);
        const uint32_t c = swz128(r, kk * 4 + (lane >> 4));
        return lds_read8(lds, r * 128 + c * 16);
    } else {
        const uint32_t g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
        const uint32_t col = idx0 + 4 * p;
        const uint32_t r0 = kk * 32 + 8 * g + q, r1 = r0 + 4;
        const uint32_t c0 = (col >> 3) ^ trswz(r0), c1 = (col >> 3) ^ trswz(r1);
        bf16x4 lo = lds_read_tr4(lds, r0 * 256 + c0 * 16 + (p & 1) * 8);
        bf16x4 hi = lds_read_tr4(lds, r1 * 256 + c1 * 16 + (p & 1) * 8);
        return cat4(lo, hi);
    }
}

template <bool A_T, bool B_T, bool PRE = false>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(GemmP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // XCD-aware remap (bijective): blocks b and b+8 share an XCD -> give each XCD a contiguous band
    const int nwg = p.nbm * p.nbn;
    int id;
    {
        const int orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    // grouped ordering: 8 M-tiles x all N-tiles per group keeps A/B panels L2-resident
    const int GROUP = 8;
    const int per_group = GROUP * p.nbn;
    const int gid = id / per_group, first_m = gid * GROUP;
    const int gsz = min(p.nbm - first_m, GROUP);
    const int tm = first_m + (id % per_group) % gsz;
    const int tn = (id % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.A, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.B, p.b_bytes);

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nt = (p.K + BK - 1) / BK;
    stage_tile<A_T>(ra, smem, p.lda, m0, p.M, 0, p.K, wave, lane);
    stage_tile<B_T>(rb, smem + BM * BK * 2, p.ldb, n0, p.N, 0, p.K, wave, lane);

    for (int t = 0; t < nt; ++t) {
        char* cur = smem + (t & 1) * STAGE_BYTES;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // tile t landed for every wave; every wave is done reading the other buffer
        if (t + 1 < nt) {
            char* nxt = smem + ((t + 1) & 1) * STAGE_BYTES;
            stage_tile<A_T>(ra, nxt, p.lda, m0, p.M, (t + 1) * BK, p.K, wave, lane);
            stage_tile<B_T>(rb, nxt + BM * BK * 2, p.ldb, n0, p.N, (t + 1) * BK, p.K, wave, lane);
        }
        const char* la = cur;
        const char* lb = cur + BM * BK * 2;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = load_frag<A_T>(la, wm * 64 + i * 16, kk, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = load_frag<B_T>(lb, wn * 64 + j * 16, kk, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);  // D[n][m]
        }
    }

    // ---- epilogue: lane owns row m = ..+(lane&15), cols n = ..+4*(lane>>4) + 0..3 ----
    const int rpb = p.rows_per_batch > 0 ? p.rows_per_batch : p.M;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
        const int b = m / rpb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= p.N) continue;
            gemm_epilogue_store<PRE>(p, acc[i][j], m, n, b);
        }
    }
}

}  // namespace

// first published layout of yat_gemm_epilogue: struct_size .. rows_per_batch
static constexpr uint32_t YAT_GEMM_EPILOGUE_V1_BYTES = offsetof(yat_gemm_epilogue, glu_u);
static_assert(YAT_GEMM_EPILOGUE_V1_BYTES == 64 && sizeof(yat_gemm_epilogue) % 8 == 0, "yat_gemm_epilogue layout");

// argument checks + descriptor + epilogue class, shared by the single and the grouped entry points.  Which layout, tile and
// split a class exists in is not checked here: GEMM_RULES (gemm_policy.hpp).
static int fill_gemm_p(int a_t, int b_t, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                       int ldc, const yat_gemm_epilogue* ep, GemmP& p, GemmEpi& epi) {
    epi = EPI_PLAIN;
    if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return YAT_EINVAL;
    if ((N & 3) || (lda & 7) || (ldb & 7) || (ldc & 3)) return YAT_EINVAL;
    if (!a_t && (K & 7)) return YAT_EINVAL;            // 16-B chunks along k
    if (a_t && (M & 7)) return YAT_EINVAL;             // 16-B chunks along m
    if (b_t && (N & 7)) return YAT_EINVAL;
    if (!b_t && (K & 7)) return YAT_EINVAL;
    if (lda < (a_t ? M : K) || ldb < (b_t ? N : K) || ldc < N) return YAT_EINVAL;   // a leading dimension covers its row
    p = GemmP{};
    p.A = (const bf16_t*)A; p.B = (const bf16_t*)B; p.C = (bf16_t*)C;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    yat_gemm_epilogue e_{};
    if (ep) {
        // versioned struct: copy exactly what the caller owns, zero-fill options it does not know (never read past it)
        const uint32_t sz = ep->struct_size;
        if (sz < YAT_GEMM_EPILOGUE_V1_BYTES || sz > sizeof(e_) || (sz & 7)) return YAT_EINVAL;
        memcpy(&e_, ep, sz);
        ep = &e_;
        p.bias = (const bf16_t*)ep->bias; p.gate = (const bf16_t*)ep->gate; p.res = (const bf16_t*)ep->residual;
        p.aux = (bf16_t*)ep->aux_out; p.ldr = ep->ld_residual ? ep->ld_residual : ldc;
        p.ldaux = ep->ld_aux ? ep->ld_aux : ldc; p.gate_ld = ep->ld_gate; p.rows_per_batch = ep->rows_per_batch;
        p.act = ep->activation;
        if (p.act < 0 || p.act > 2) return YAT_EINVAL;
        if ((ep->ld_residual && ep->ld_residual < N) || (ep->ld_aux && ep->ld_aux < N)) return YAT_EINVAL;   // (0: ldc)
        if (p.gate && (p.gate_ld & 3)) return YAT_EINVAL;
        p.pre_add = (const bf16_t*)ep->pre_add; p.ld_pre = ep->ld_pre_add;
        if (p.pre_add && ((p.ld_pre & 3) || p.ld_pre < N)) return YAT_EINVAL;
        p.glu_u = (const bf16_t*)ep->glu_u; p.ld_glu = ep->ld_glu_u;
        if (p.glu_u && (p.bias || p.gate || p.res || p.aux || p.act || (p.ld_glu & 3) || p.ld_glu < 2 * N || ldc < 2 * N))
            return YAT_EINVAL;
        p.dact_z = (const bf16_t*)ep->dact_z; p.ld_z = ep->ld_dact_z;
        if (p.dact_z && (p.bias || p.gate || p.res || p.aux || !p.act || (p.ld_z & 3) || p.ld_z < N)) return YAT_EINVAL;
        p.rowsum = (bf16_t*)ep->a_rowsum_out; p.rowsum_acc = ep->a_rowsum_accumulate;
        if (p.rowsum && (p.bias || p.gate || p.aux || p.act)) return YAT_EINVAL;      // plain (or accumulating) epilogue
        p.A2 = (const bf16_t*)ep->a2; p.B2 = (const bf16_t*)ep->b2; p.K2 = ep->k2; p.a2_group = ep->a2_group_n;
        // the class: at most one of the options that have a kernel instantiation of their own
        const bool pair2 = p.A2 || p.B2;
        if ((p.glu_u != nullptr) + (p.pre_add != nullptr) + (p.dact_z != nullptr) + (p.rowsum != nullptr) + pair2 > 1) return YAT_EINVAL;
        epi = p.glu_u ? EPI_GLU_BWD : p.pre_add ? EPI_PRE_ADD : p.dact_z ? EPI_ACT_BWD : p.rowsum ? EPI_ROWSUM : pair2 ? EPI_PAIR2 : EPI_PLAIN;
        if (epi == EPI_PAIR2) {                                  // second operand pair (K2, a2_group: gemm_plan)
            if (!p.A2 || !p.B2 || p.K2 <= 0 || p.a2_group < 0) return YAT_EINVAL;
            const int blocks = p.a2_group > 0 ? (N + p.a2_group - 1) / p.a2_group : 1;
            if ((int64_t)blocks * p.K2 > lda || p.K2 > ldb) return YAT_EINVAL;     // the rows of A2 / B2 have A's / B's stride
            p.a2_bytes = ((uint64_t)(M - 1) * lda + (uint64_t)blocks * p.K2) * 2;
            p.b2_bytes = ((uint64_t)(N - 1) * ldb + (uint64_t)p.K2) * 2;
            if (p.a2_bytes > 0x7fffffffull || p.b2_bytes > 0x7fffffffull) return YAT_EINVAL;
        }
    }
    p.a_bytes = (uint64_t)(a_t ? K : M) * lda * 2;
    p.b_bytes = (uint64_t)(b_t ? K : N) * ldb * 2;
    if (p.a_bytes > 0x7fffffffull || p.b_bytes > 0x7fffffffull) return YAT_EINVAL;
    p.ksplit = 1;
    return YAT_OK;
}

extern "C" uint64_t yat_gemm_epilogue_size(void) { return sizeof(yat_gemm_epilogue); }

int yat_gemm256_grouped_launch(int a_t, int b_t, int ngroups, const GemmP* probs, hipStream_t stream);

extern "C" int yat_gemm_grouped_bf16(int a_t, int b_t, int count, const yat_gemm_problem* problems, yat_stream_t stream) {
    if (count < 1 || count > 8 || !problems) return YAT_EINVAL;
    GemmP ps[8];
    for (int i = 0; i < count; ++i) {
        const yat_gemm_problem& q = problems[i];
        GemmEpi epi;
        const int rc = fill_gemm_p(a_t, b_t, q.M, q.N, q.K, q.A, q.lda, q.B, q.ldb, q.C, q.ldc, q.epilogue, ps[i], epi);
        if (rc) return rc;
        if (!GEMM_RULES[epi].grouped || !(GEMM_RULES[epi].layouts & gemm_layout_bit(a_t != 0, b_t != 0))) return YAT_EINVAL;
    }
    return yat_gemm256_grouped_launch(a_t, b_t, count, ps, (hipStream_t)stream);
}

extern "C" int yat_gemm_bf16_ex(int a_t, int b_t, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                                void* C, int ldc, const yat_gemm_epilogue* ep, int variant, void* workspace,
                                uint64_t workspace_bytes, yat_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // decode the policy word -> check the arguments -> plan (gemm_policy.hpp: pure, the library holds no policy state) -> launch
    GemmWord word;
    GemmP p;
    GemmEpi epi;
    if (int rc = decode_gemm_word(variant, word)) return rc;
    if (int rc = fill_gemm_p(a_t, b_t, M, N, K, A, lda, B, ldb, C, ldc, ep, p, epi)) return rc;
    const bool wide_ok = !(N & 7) && !(ldc & 7) && !(p.res && (p.ldr & 7)) && !(p.aux && (p.ldaux & 7)) &&
                         !(p.gate && (p.gate_ld & 7)) && !(p.glu_u && (p.ld_glu & 7)) && !(p.pre_add && (p.ld_pre & 7));
    const GemmQuery query{a_t != 0, b_t != 0, M, N, K, p.K2, epi, wide_ok, p.a2_group, workspace != nullptr, workspace_bytes};
    GemmPlan plan;
    if (int rc = gemm_plan(query, word, plan)) return rc;
    if (plan.tile != 1) {
        p.ksplit = plan.ksplit;
        p.partial = (float*)workspace;
        p.group = plan.group;
        const int rc = yat_gemm256_launch(a_t, b_t, plan.tile, epi, p, stream);
        if (rc || plan.ksplit == 1) return rc;
        return yat_gemm_splitk_reduce(p, stream);
    }
    p.nbm = (M + BM - 1) / BM; p.nbn = (N + BN - 1) / BN;
    using Kernel = void (*)(GemmP);
    static const Kernel kernels[5] = {gemm_bf16_kernel<false, false>, gemm_bf16_kernel<false, true>, gemm_bf16_kernel<true, false>,
                                      gemm_bf16_kernel<true, true>, gemm_bf16_kernel<false, false, true>};
    static bool attr_set = false;   // idempotent one-time launch attribute (64 KiB dynamic LDS)
    if (!attr_set) {
        for (Kernel k : kernels) {
            const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
            if (e != hipSuccess) return (int)e;          // a HIP error (e.g. no device), not an argument error
        }
        attr_set = true;
    }
    hipLaunchKernelGGL(kernels[epi == EPI_PRE_ADD ? 4 : 2 * (a_t != 0) + (b_t != 0)], dim3(p.nbm * p.nbn), dim3(256), LDS_BYTES, stream, p);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

extern "C" int yat_gemm_bf16(int a_t, int b_t, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                             void* C, int ldc, const yat_gemm_epilogue* ep, yat_stream_t stream) {
    return yat_gemm_bf16_ex(a_t, b_t, M, N, K, A, lda, B, ldb, C, ldc, ep, 0, nullptr, 0, stream);
}
