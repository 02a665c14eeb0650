// The optimizer of the step loop over ONE flat parameter buffer, for gfx950:
//   global gradient-norm clip (torch.nn.utils.clip_grad_norm_, common/trainer.py:347)
//   + AdamW (torch.optim.AdamW, common/trainer.py:246-248,348) + zero_grad (:356) + optional EMA (:350-351).
// The norm: per-chunk sums of squares, then one workgroup that applies torch's clip arithmetic -- over SEGMENTS (whole tensors,
//   yat_gradnorm_clip) and over PIECES (tensors cut at the eighths of their data-parallel bucket, yat_gradnorm_pieces_*: what
//   FlatAdamW calls, and what a sharded step can split over ranks); both forms share the chunk sum and the clip tail.
// The bf16 step (adamw_kernel, yat_adamw_step): all state bf16, 14 B / parameter of algorithmic traffic (read p, g, m, v;
//   write p, m, v) + 2 B for the gradient clear.  The arithmetic follows torch's single-tensor op sequence on bf16 tensors:
//   every torch op computes in fp32 and rounds its result to bf16, so the kernel rounds at the same points.
// Two opt-in steps that answer the stall of sub-ulp updates: fp32 master weights (adamw_master_kernel, 28 B / parameter) and
//   stochastic rounding of an all-bf16 state (adamw_sr_kernel, 14 B / parameter, Philox bits made in registers).
// The three steps are HBM-bound streams of 16-byte accesses with one launch shape: 8 parameters per lane and iteration, a
//   grid-stride loop over a grid capped at STEP_MAX_BLOCKS.
#include "common.hpp"
#include "../../include/yat_hip.h"
#include <math.h>
#include <initializer_list>

namespace {

constexpr int64_t NORM_CHUNK = 1 << 18;  // elements per gradnorm workgroup

// sum over the 256 lanes of a workgroup, the four wave sums added in wave order
__device__ __forceinline__ float block_sum(float s) {
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// one workgroup's sum of squares of g[c0, c1): 16-byte vector body (chunk starts are 16-B aligned) + scalar tail
__device__ __forceinline__ float chunk_sumsq(const bf16_t* g, int64_t c0, int64_t c1) {
    float s = 0.f;
    const int64_t nvec = (c1 - c0) >> 3;
    for (int64_t i = threadIdx.x; i < nvec; i += 256) {
        float v[8];
        unpack8(*reinterpret_cast<const u32x4*>(g + c0 + i * 8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e] * v[e];
    }
    for (int64_t i = c0 + (nvec << 3) + threadIdx.x; i < c1; i += 256) { const float v = bf2f(g[i]); s += v * v; }
    return block_sum(s);
}

// the end of both finish kernels: acc = this lane's sum of squared per-tensor norms -> total norm and clip coefficient,
// torch's clip_grad_norm_ arithmetic on bf16 gradients (every intermediate is a bf16 tensor)
__device__ __forceinline__ void clip_tail(float acc, float max_norm, float* norm_out, float* clip_coef) {
    const float sum = block_sum(acc);
    if (threadIdx.x == 0) {
        const float total = rbf(sqrtf(sum));
        float coef = rbf(max_norm / rbf(total + 1e-6f));
        coef = coef > 1.0f ? 1.0f : coef;   // torch.clamp(max=1.0) keeps a NaN (fminf would give 1)
        norm_out[0] = total;
        clip_coef[0] = coef;
    }
}

// grid = (maxchunks, nseg): sum of squares of one chunk of one parameter tensor
__global__ __launch_bounds__(256) void gradnorm_partial_kernel(const bf16_t* g, const int64_t* seg_start, int maxchunks,
                                                               float* partial) {
    const int seg = blockIdx.y, ck = blockIdx.x;
    const int64_t s0 = seg_start[seg], s1 = seg_start[seg + 1];
    const int64_t c0 = s0 + (int64_t)ck * NORM_CHUNK;
    if (c0 >= s1) return;
    const int64_t c1 = (c0 + NORM_CHUNK < s1) ? c0 + NORM_CHUNK : s1;
    const float s = chunk_sumsq(g, c0, c1);
    if (threadIdx.x == 0) partial[(int64_t)seg * maxchunks + ck] = s;
}

__global__ __launch_bounds__(256) void gradnorm_final_kernel(int nseg, const int64_t* seg_start, int maxchunks,
                                                             const float* partial, float max_norm, float* norm_out,
                                                             float* clip_coef) {
    float acc = 0.f;
    for (int seg = threadIdx.x; seg < nseg; seg += 256) {
        const int64_t len = seg_start[seg + 1] - seg_start[seg];
        const int nck = (int)((len + NORM_CHUNK - 1) / NORM_CHUNK);
        float s = 0.f;
        for (int c = 0; c < nck; ++c) s += partial[(int64_t)seg * maxchunks + c];
        const float nb = rbf(sqrtf(s));   // per-tensor norm comes back as a bf16 tensor
        acc += nb * nb;
    }
    clip_tail(acc, max_norm, norm_out, clip_coef);
}

// ---- the same norm over PIECES (round 6): a piece is a tensor, or the part of a tensor inside one eighth of its
// data-parallel bucket; partial sums live compactly at chunk_base[piece] + chunk.  A tensor's sum of squares is the sum over its
// pieces, in order, of the sum over each piece's chunks, in order -- the same numbers whoever computed each piece, which is
// what lets N ranks each sum only the pieces they hold reduced gradients for (``owned``), add the arrays up (every slot has
// exactly one non-zero contributor) and arrive at the clip coefficient of the one-rank run BIT FOR BIT.
__global__ __launch_bounds__(256) void gradnorm_pieces_partial_kernel(const bf16_t* g, const int64_t* piece_start,
                                                                      const int* chunk_base, const unsigned char* owned,
                                                                      float* partial) {
    const int pc = blockIdx.y, ck = blockIdx.x;
    const int nck = chunk_base[pc + 1] - chunk_base[pc];
    if (ck >= nck) return;
    float* dst = partial + chunk_base[pc] + ck;
    if (owned && !owned[pc]) {
        if (threadIdx.x == 0) *dst = 0.f;
        return;
    }
    const int64_t s1 = piece_start[pc + 1];
    const int64_t c0 = piece_start[pc] + (int64_t)ck * NORM_CHUNK;
    const int64_t c1 = (c0 + NORM_CHUNK < s1) ? c0 + NORM_CHUNK : s1;
    const float s = chunk_sumsq(g, c0, c1);
    if (threadIdx.x == 0) *dst = s;
}

__global__ __launch_bounds__(256) void gradnorm_pieces_final_kernel(int ntensor, const int* tensor_first_piece,
                                                                    const int* chunk_base, const float* partial,
                                                                    float max_norm, float* norm_out, float* clip_coef) {
    float acc = 0.f;
    for (int t = threadIdx.x; t < ntensor; t += 256) {
        float s = 0.f;
        for (int pc = tensor_first_piece[t]; pc < tensor_first_piece[t + 1]; ++pc) {
            float sp = 0.f;
            for (int c = chunk_base[pc]; c < chunk_base[pc + 1]; ++c) sp += partial[c];
            s += sp;
        }
        const float nb = rbf(sqrtf(s));   // per-tensor norm comes back as a bf16 tensor
        acc += nb * nb;
    }
    clip_tail(acc, max_norm, norm_out, clip_coef);
}

struct AdamP {
    float wd_mul, w1, beta2, om_b2, bc2_sqrt, eps, neg_step_size, ema_omd;
    int use_wd, zero_grad;
};

// one parameter's update: torch's single-tensor AdamW op sequence with a bf16 rounding after every op
__device__ __forceinline__ void adamw_elem(float& pr, float g, float& mr_, float& vr_, float coef, bool clip, const AdamP& a) {
    const float gr = clip ? rbf(g * coef) : g;                      // grads.mul_(clip_coef_clamped)
    if (a.use_wd) pr = rbf(pr * a.wd_mul);                          // param.mul_(1 - lr*wd)
    const float mr = rbf(mr_ + a.w1 * (gr - mr_));                  // exp_avg.lerp_(grad, 1-beta1)
    float vr = rbf(vr_ * a.beta2);                                  // exp_avg_sq.mul_(beta2)
    vr = rbf(vr + a.om_b2 * gr * gr);                               //   .addcmul_(grad, grad, value=1-beta2)
    float den = rbf(sqrtf(vr));                                     // exp_avg_sq.sqrt()
    den = rbf(den / a.bc2_sqrt);                                    //   / bias_correction2_sqrt
    den = rbf(den + a.eps);                                         //   .add_(eps)
    pr = rbf(pr + a.neg_step_size * mr / den);                      // param.addcdiv_(exp_avg, denom, -step_size)
    mr_ = mr;
    vr_ = vr;
}

constexpr int STEP_MAX_BLOCKS = 8192;        // x 256 lanes x 8 parameters = 2^24 parameters per grid pass (yat_amd/optim.py MASTER_GRID_PASS)

// U = 1 vector of 8 parameters per thread and iteration, every load of the iteration issued before the first use (4 or 5
// independent 16-byte loads in flight per lane), grid capped at STEP_MAX_BLOCKS.  The state streams through once per step, so
// its accesses are non-temporal: measured alone the plain and the non-temporal form (and U = 2) are equal; in the step the
// non-temporal form is 0.3 ms shorter -- 22 GB of state do not sweep the Infinity Cache of what the forward that runs beside
// this kernel re-reads.  A 48-VGPR form of it (a few persistent workgroups that share a CU with two resident GEMM waves,
// for an update that runs under the next forward) was measured and rejected in round 3.
// The load block and the arithmetic block stay loops over the (one) vector: written straight-line the compiler resolves the
// optional shadow load before it unrolls and emits a loop that, with a shadow, waits for all five loads before the first
// parameter's arithmetic (4 instructions more) instead of this one, which starts on g, v, m, p as they arrive.
__global__ __launch_bounds__(256) void adamw_kernel(int64_t nvec, bf16_t* p, bf16_t* g, bf16_t* m, bf16_t* v,
                                                    const float* clip_coef, bf16_t* ema, AdamP a) {
    constexpr int U = 1;
    const float coef = clip_coef ? clip_coef[0] : 1.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        u32x4 rp[U], rg[U], rm[U], rv[U], rs[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            rp[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + i * 8));
            rg[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + i * 8));
            rm[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(m + i * 8));
            rv[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(v + i * 8));
            if (ema) rs[q] = *reinterpret_cast<const u32x4*>(ema + i * 8);
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            float pp[8], gg[8], mm[8], vv[8], ss[8];
            unpack8(rp[q], pp);
            unpack8(rg[q], gg);
            unpack8(rm[q], mm);
            unpack8(rv[q], vv);
            if (ema) unpack8(rs[q], ss);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                adamw_elem(pp[e], gg[e], mm[e], vv[e], coef, clip_coef != nullptr, a);
                if (ema) {                                                  // s.sub_(one_minus_decay * (s - p))
                    const float d = rbf(ss[e] - pp[e]);
                    ss[e] = rbf(ss[e] - rbf(a.ema_omd * d));
                }
            }
            __builtin_nontemporal_store(pack8(pp), reinterpret_cast<u32x4*>(p + i * 8));
            __builtin_nontemporal_store(pack8(mm), reinterpret_cast<u32x4*>(m + i * 8));
            __builtin_nontemporal_store(pack8(vv), reinterpret_cast<u32x4*>(v + i * 8));
            if (ema) *reinterpret_cast<u32x4*>(ema + i * 8) = pack8(ss);
            if (a.zero_grad) *reinterpret_cast<u32x4*>(g + i * 8) = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

// ---- mixed-precision step: fp32 master weights, fp32 moments, fp32 EMA shadow; bf16 gradients in, bf16 working copy out.
// torch's single-tensor AdamW op sequence on fp32 tensors, i.e. the sequence of adamw_elem WITHOUT the bf16 roundings: a
// parameter of magnitude 0.02 has a bf16 ulp of 6e-5, an update at the recipes' learning rates is ~1e-5, so the all-bf16 step
// above leaves most weights where they are; the master copy takes every update and the working copy is its rounding.
// Where torch's CPU kernels fuse a product into a sum (lerp_, and addcmul_ once the compiler contracts it) an fma stands.
__device__ __forceinline__ void adamw_master_elem(float& pw, float g, float& m, float& v, float coef, bool clip, const AdamP& a) {
    const float gr = clip ? g * coef : g;                           // grads.mul_(clip_coef_clamped): exact, g has 8 bits
    if (a.use_wd) pw = pw * a.wd_mul;                               // param.mul_(1 - lr*wd)
    m = __builtin_fmaf(a.w1, gr - m, m);                            // exp_avg.lerp_(grad, 1-beta1)
    v = v * a.beta2;                                                // exp_avg_sq.mul_(beta2)
    v = __builtin_fmaf(a.om_b2 * gr, gr, v);                        //   .addcmul_(grad, grad, value=1-beta2)
    const float den = sqrtf(v) / a.bc2_sqrt + a.eps;                // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    pw = pw + a.neg_step_size * m / den;                            // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ void load8f(const float* src, float* o) {
    const f32x4 lo = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
    const f32x4 hi = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src) + 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
}
__device__ __forceinline__ void store8f(float* dst, const float* f) {
    __builtin_nontemporal_store(f32x4{f[0], f[1], f[2], f[3]}, reinterpret_cast<f32x4*>(dst));
    __builtin_nontemporal_store(f32x4{f[4], f[5], f[6], f[7]}, reinterpret_cast<f32x4*>(dst) + 1);
}

// 8 parameters per thread and iteration, 16 bytes per access: 2 loads each of master, m, v (and the shadow) + 1 of the
// gradients, all issued before the first use (7 or 9 independent loads in flight per lane); 28 B / parameter, 36 with EMA.
// The fp32 state (19 - 26 GB at SANA-1.6B) streams through once per step: non-temporal, for the reason given at adamw_kernel.
__global__ __launch_bounds__(256) void adamw_master_kernel(int64_t nvec, bf16_t* p, float* w, bf16_t* g, float* m, float* v,
                                                           const float* clip_coef, float* ema, AdamP a) {
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        float ww[8], gg[8], mm[8], vv[8], ss[8];
        load8f(w + i * 8, ww);
        load8f(m + i * 8, mm);
        load8f(v + i * 8, vv);
        const u32x4 rg = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + i * 8));
        if (ema) load8f(ema + i * 8, ss);
        unpack8(rg, gg);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            adamw_master_elem(ww[e], gg[e], mm[e], vv[e], coef, clip, a);
            if (ema) ss[e] = ss[e] - a.ema_omd * (ss[e] - ww[e]);      // s.sub_(one_minus_decay * (s - p))
        }
        store8f(w + i * 8, ww);
        store8f(m + i * 8, mm);
        store8f(v + i * 8, vv);
        if (ema) store8f(ema + i * 8, ss);
        __builtin_nontemporal_store(pack8(ww), reinterpret_cast<u32x4*>(p + i * 8));   // the working copy: bf16(master), RNE, NaN kept
        if (a.zero_grad) *reinterpret_cast<u32x4*>(g + i * 8) = u32x4{0u, 0u, 0u, 0u};
    }
}

// ---- stochastic-rounding step: ALL state bf16 (p, g, m, v, shadow), the update computed in fp32 from it (adamw_master_elem's
// sequence on the unpacked values) and every stored value rounded up or down at random, so that E[stored] = computed: a
// sub-ulp update, the 1e-3 decay of v and of the shadow accumulate in expectation where round-to-nearest drops them.
// 14 B / parameter (18 with the shadow) like adamw_kernel, no extra state; the random bits are made in registers.
//   sr_bf16(x, r), r a 16-bit random: finite x -> the top 16 bits of (bits(x) + r), a 32-bit add then truncation, i.e. away
//   from zero with probability (low 16 bits of x) / 65536, a bf16-representable x unchanged for every r; NaN and +-Inf take
//   the round-to-nearest conversion of pack8 (the add must not touch them: a NaN payload + r can carry into the sign).
//   bits: Philox4x32 (multipliers D2511F53 / CD9E8D57, Weyl key increments 9E3779B9 / BB67AE85), one call per PAIR of
//   consecutive parameters: pair j = (elem_offset + i) >> 1, key = (seed lo, seed hi), counter = (j lo, j hi, rng_step lo,
//   rng_step hi); the even parameter takes the words (w0, w1), the odd one (w2, w3); of a parameter's words (wa, wb):
//   p <- wa & 0xFFFF, exp_avg <- wa >> 16, exp_avg_sq <- wb & 0xFFFF, shadow <- wb >> 16.
// The bits depend on (seed, rng_step, global index, field) only: not on the grid, not on how the buffer is sliced into calls
// (buckets, ranges, rank shards), not on which rank runs the call.
constexpr int SR_PHILOX_ROUNDS = 10;         // tests/sr_adamw_ref.py PHILOX_ROUNDS restates this; the two must agree

__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t* w) {
#pragma unroll
    for (int r = 0; r < SR_PHILOX_ROUNDS; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;    // v_mad_u64_u32: high and low at once
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ uint32_t sr_bf16(float x, uint32_t r) {          // r < 65536; the bf16 in the low half
    const uint32_t u = __float_as_uint(x);
    return (u & 0x7f800000u) != 0x7f800000u ? (u + r) >> 16 : (uint32_t)f2bf(x);
}

// adamw_kernel's shape: 8 parameters per lane and iteration, the four (five) 16-byte loads issued before the first use,
// non-temporal, grid capped at STEP_MAX_BLOCKS with a grid-stride loop; four Philox calls per 8-parameter vector.
__global__ __launch_bounds__(256) void adamw_sr_kernel(int64_t nvec, bf16_t* p, bf16_t* g, bf16_t* m, bf16_t* v,
                                                       const float* clip_coef, bf16_t* ema, AdamP a, uint32_t seed_lo,
                                                       uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi, int64_t pair0) {
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const u32x4 rp = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + i * 8));
        const u32x4 rg = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + i * 8));
        const u32x4 rm = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(m + i * 8));
        const u32x4 rv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(v + i * 8));
        u32x4 rs = u32x4{0u, 0u, 0u, 0u};
        if (ema) rs = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ema + i * 8));
        const uint64_t j0 = (uint64_t)(pair0 + i * 4);         // elem_offset % 8 == 0: the vector's four pairs are j0 .. j0 + 3
        float pp[8], gg[8], mm[8], vv[8], ss[8];
        unpack8(rp, pp);
        unpack8(rg, gg);
        unpack8(rm, mm);
        unpack8(rv, vv);
        unpack8(rs, ss);
        u32x4 op, om, ov, os;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t w[4];
            philox4x32((uint32_t)j0 | q, (uint32_t)(j0 >> 32), step_lo, step_hi, seed_lo, seed_hi, w);
            uint32_t hp[2], hm[2], hv[2], hs[2] = {0u, 0u};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int e = 2 * q + h;
                const uint32_t wa = w[2 * h], wb = w[2 * h + 1];
                adamw_master_elem(pp[e], gg[e], mm[e], vv[e], coef, clip, a);
                hp[h] = sr_bf16(pp[e], wa & 0xffffu);
                hm[h] = sr_bf16(mm[e], wa >> 16);
                hv[h] = sr_bf16(vv[e], wb & 0xffffu);
                if (ema) {                                      // the EMA of the weights the model uses: the bf16 just stored
                    const float ps = __uint_as_float(hp[h] << 16);
                    hs[h] = sr_bf16(ss[e] - a.ema_omd * (ss[e] - ps), wb >> 16);
                }
            }
            op[q] = hp[0] | (hp[1] << 16);
            om[q] = hm[0] | (hm[1] << 16);
            ov[q] = hv[0] | (hv[1] << 16);
            os[q] = hs[0] | (hs[1] << 16);
        }
        __builtin_nontemporal_store(op, reinterpret_cast<u32x4*>(p + i * 8));
        __builtin_nontemporal_store(om, reinterpret_cast<u32x4*>(m + i * 8));
        __builtin_nontemporal_store(ov, reinterpret_cast<u32x4*>(v + i * 8));
        if (ema) __builtin_nontemporal_store(os, reinterpret_cast<u32x4*>(ema + i * 8));
        if (a.zero_grad) *reinterpret_cast<u32x4*>(g + i * 8) = u32x4{0u, 0u, 0u, 0u};
    }
}

}  // namespace

extern "C" {

static int norm_maxchunks(int64_t n) { return (int)((n + NORM_CHUNK - 1) / NORM_CHUNK); }

uint64_t yat_gradnorm_workspace_bytes(int64_t n, int nseg) {
    return (uint64_t)nseg * norm_maxchunks(n) * sizeof(float);
}

int yat_gradnorm_clip(int64_t n, const void* grad, int nseg, const int64_t* seg_start, float max_norm, float* norm_out,
                      float* clip_coef, void* workspace, yat_stream_t stream) {
    if (n <= 0 || nseg <= 0 || nseg > 65535 || !grad || !seg_start || !norm_out || !clip_coef || !workspace)
        return YAT_EINVAL;
    const int mc = norm_maxchunks(n);
    hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(mc, nseg), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)grad,
                       seg_start, mc, (float*)workspace);
    YAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(gradnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nseg, seg_start, mc,
                       (const float*)workspace, max_norm, norm_out, clip_coef);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_gradnorm_pieces_partial(const void* grad, int npiece, const int64_t* piece_start, const int* chunk_base,
                                int max_piece_chunks, const unsigned char* owned, float* partial, yat_stream_t stream) {
    if (!grad || npiece <= 0 || npiece > 65535 || !piece_start || !chunk_base || max_piece_chunks <= 0 || !partial)
        return YAT_EINVAL;
    hipLaunchKernelGGL(gradnorm_pieces_partial_kernel, dim3(max_piece_chunks, npiece), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)grad, piece_start, chunk_base, owned, partial);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_gradnorm_pieces_finish(int ntensor, const int* tensor_first_piece, const int* chunk_base, const float* partial,
                               float max_norm, float* norm_out, float* clip_coef, yat_stream_t stream) {
    if (ntensor <= 0 || !tensor_first_piece || !chunk_base || !partial || !norm_out || !clip_coef) return YAT_EINVAL;
    hipLaunchKernelGGL(gradnorm_pieces_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ntensor, tensor_first_piece,
                       chunk_base, partial, max_norm, norm_out, clip_coef);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

// scalar prep in double exactly as torch's python does, then narrowed to the kernels' opmath (float)
static AdamP adam_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, int step, int zero_grad,
                          double ema_decay) {
    const double dlr = lr, db1 = beta1, db2 = beta2;
    AdamP a;
    a.use_wd = weight_decay != 0.0;
    a.wd_mul = (float)(1.0 - dlr * weight_decay);
    a.w1 = (float)(1.0 - db1);
    a.beta2 = (float)db2;
    a.om_b2 = (float)(1.0 - db2);
    const double bc1 = 1.0 - pow(db1, (double)step), bc2 = 1.0 - pow(db2, (double)step);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.neg_step_size = (float)(-(dlr / bc1));
    a.eps = (float)eps;
    a.ema_omd = (float)(1.0 - ema_decay);
    a.zero_grad = zero_grad;
    return a;
}

// what the three step entry points share: the argument check (before any launch), the scalars and the capped grid
struct StepLaunch {
    AdamP a;
    int64_t nvec;
    unsigned blocks;
};
static bool step_launch(StepLaunch& L, int64_t n, std::initializer_list<const void*> required, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int step, int zero_grad, double ema_decay) {
    if (n <= 0 || (n & 7) || step < 1) return false;
    for (const void* buf : required)
        if (!buf) return false;
    L.a = adam_scalars(lr, beta1, beta2, eps, weight_decay, step, zero_grad, ema_decay);
    L.nvec = n >> 3;
    const int64_t nb = (L.nvec + 255) / 256;
    L.blocks = (unsigned)(nb > STEP_MAX_BLOCKS ? STEP_MAX_BLOCKS : nb);
    return true;
}

int yat_adamw_step(int64_t n, void* param, void* grad, void* exp_avg, void* exp_avg_sq, const float* clip_coef, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int step, int zero_grad, void* ema_shadow,
                   double ema_decay, yat_stream_t stream) {
    StepLaunch L;
    if (!step_launch(L, n, {param, grad, exp_avg, exp_avg_sq}, lr, beta1, beta2, eps, weight_decay, step, zero_grad, ema_decay))
        return YAT_EINVAL;
    hipLaunchKernelGGL(adamw_kernel, dim3(L.blocks), dim3(256), 0, (hipStream_t)stream, L.nvec, (bf16_t*)param, (bf16_t*)grad,
                       (bf16_t*)exp_avg, (bf16_t*)exp_avg_sq, clip_coef, (bf16_t*)ema_shadow, L.a);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_adamw_master_step(int64_t n, void* param_bf16, float* master, void* grad_bf16, float* exp_avg, float* exp_avg_sq,
                          const float* clip_coef, double lr, double beta1, double beta2, double eps, double weight_decay,
                          int step, int zero_grad, float* ema_shadow, double ema_decay, yat_stream_t stream) {
    StepLaunch L;
    if (!step_launch(L, n, {param_bf16, master, grad_bf16, exp_avg, exp_avg_sq}, lr, beta1, beta2, eps, weight_decay, step,
                     zero_grad, ema_decay))
        return YAT_EINVAL;
    hipLaunchKernelGGL(adamw_master_kernel, dim3(L.blocks), dim3(256), 0, (hipStream_t)stream, L.nvec, (bf16_t*)param_bf16,
                       master, (bf16_t*)grad_bf16, exp_avg, exp_avg_sq, clip_coef, ema_shadow, L.a);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

int yat_adamw_sr_step(int64_t n, void* param, void* grad, void* exp_avg, void* exp_avg_sq, const float* clip_coef, double lr,
                      double beta1, double beta2, double eps, double weight_decay, int step, int zero_grad, void* ema_shadow,
                      double ema_decay, uint64_t seed, int64_t rng_step, int64_t elem_offset, yat_stream_t stream) {
    StepLaunch L;
    if (elem_offset < 0 || (elem_offset & 7) || rng_step < 0 ||
        !step_launch(L, n, {param, grad, exp_avg, exp_avg_sq}, lr, beta1, beta2, eps, weight_decay, step, zero_grad, ema_decay))
        return YAT_EINVAL;
    hipLaunchKernelGGL(adamw_sr_kernel, dim3(L.blocks), dim3(256), 0, (hipStream_t)stream, L.nvec, (bf16_t*)param,
                       (bf16_t*)grad, (bf16_t*)exp_avg, (bf16_t*)exp_avg_sq, clip_coef, (bf16_t*)ema_shadow, L.a, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)rng_step, (uint32_t)((uint64_t)rng_step >> 32), elem_offset >> 1);
    YAT_CHECK_LAUNCH();
    return YAT_OK;
}

}  // extern "C"
