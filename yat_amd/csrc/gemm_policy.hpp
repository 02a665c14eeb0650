// Host-side policy of the bf16 GEMM family: which kernel (128 x 128, 256 x 256 or 256 x 320 tile), which K split and which
// tile order a call of yat_gemm_bf16_ex gets, and which combinations of epilogue class, layout, tile and split exist at all.
// Pure functions of their arguments: no HIP, no environment, no statics, no state from call to call -- the same query
// always gets the same plan (a training step's fp32 summation order does not depend on what ran before it), and a plain
// host compiler can build and test this file alone (tests/gemm_policy_probe.cpp, tests/test_gemm_policy_cpu.py).
#ifndef YAT_GEMM_POLICY_HPP      // (a guard, not #pragma once: the file also compiles as a translation unit of its own)
#define YAT_GEMM_POLICY_HPP
#include <cmath>
#include <cstdint>

#ifndef YAT_OK               // include/yat_hip.h, token for token (this header stands alone)
#define YAT_OK 0
#define YAT_EINVAL (-1)
#endif

// The policy word of yat_gemm_bf16_ex (include/yat_hip.h): tile + 100 * ksplit + 10000 * streams + 1000000 * group.
struct GemmWord {
    int tile;      // 0 = the policy picks, 1 = 128 x 128, 4 = 256 x 256, 5 = 256 x 320
    int ksplit;    // 1..32; > 1 forces that split (a word field of 0 reads as 1: the policy decides)
    int streams;   // 1..8 independent GEMM streams the caller keeps in flight (a word field of 0 reads as 1)
    int group;     // 0 = the policy's tile order, 1..64 = 256-row tiles per row group (tuning)
};

inline int decode_gemm_word(int word, GemmWord& w) {
    if (word < 0) return YAT_EINVAL;
    w.group = word / 1000000; word %= 1000000;
    w.streams = word >= 10000 ? word / 10000 : 1; word %= 10000;
    w.ksplit = word >= 100 ? word / 100 : 1;
    w.tile = word % 100;
    if (w.group > 64 || w.streams > 8 || w.ksplit > 32) return YAT_EINVAL;
    if (w.tile != 0 && w.tile != 1 && w.tile != 4 && w.tile != 5) return YAT_EINVAL;
    return YAT_OK;
}

// Epilogue class of a call = the EPI template argument of gemm256_kernel (gemm256.hip).  A call has exactly one.
enum GemmEpi : int {
    EPI_PLAIN = 0,      // bias / aux / activation / gate / residual
    EPI_GLU_BWD = 1,    // yat_gemm_epilogue.glu_u
    EPI_PRE_ADD = 2,    // .pre_add (+ the plain options)
    EPI_ACT_BWD = 3,    // .dact_z
    EPI_ROWSUM = 4,     // .a_rowsum_out (+ residual)
    EPI_PAIR2 = 5,      // .a2 / .b2 (+ the plain options)
    EPI_COUNT = 6
};

// layouts as a bit set, bit = 2 * a_t + b_t (bit 2, x^T W^T, has no name: only the plain class has it)
constexpr unsigned LAY_FWD = 1u << 0, LAY_DGRAD = 1u << 1, LAY_WGRAD = 1u << 3, LAY_ALL = 15u;
constexpr unsigned gemm_layout_bit(bool a_t, bool b_t) { return 1u << (2 * (int)a_t + (int)b_t); }

// What exists per class.  Every "only / excludes" rule of the family is a cell of this table; fill_gemm_p (gemm.hip) checks
// arguments, yat_gemm256_launch (gemm256.hip) dispatches, neither restates a rule.
struct GemmRule {
    unsigned layouts;   // instantiated layouts
    bool k128;          // the 128 x 128 kernel has this epilogue
    bool split_k;       // K may be split (the split-K reduce pass applies the plain epilogue only)
    bool tile4, tile5;  // 256 x 256 / 256 x 320 tile instantiated
    bool need_wide;     // needs 16-byte epilogue accesses (GemmQuery::wide_ok)
    bool grouped;       // yat_gemm_grouped_bf16's kernel has this epilogue
};
constexpr GemmRule GEMM_RULES[EPI_COUNT] = {
    /* EPI_PLAIN   */ {LAY_ALL,   true,  true,  true, true,  false, true},
    /* EPI_GLU_BWD */ {LAY_DGRAD, false, false, true, true,  true, false},
    /* EPI_PRE_ADD */ {LAY_FWD,   true,  false, true, true,  false, false},
    /* EPI_ACT_BWD */ {LAY_DGRAD, false, false, true, true,  false, false},
    // bias gradient fused into the weight gradient: the 320-wide tile has no registers for the extra accumulators
    /* EPI_ROWSUM  */ {LAY_WGRAD, false, false, true, false, false, true},
    /* EPI_PAIR2   */ {LAY_FWD,   false, false, true, true,  true, false},
};

struct GemmQuery {
    bool a_t, b_t;
    int M, N, K;
    int K2;                     // EPI_PAIR2: columns of the second operand pair (the K loop runs over K + K2), else 0
    GemmEpi epi;
    bool wide_ok;               // N and every leading dimension the epilogue touches are multiples of 8
    int a2_group;               // EPI_PAIR2: yat_gemm_epilogue.a2_group_n, else 0
    bool has_workspace;
    uint64_t workspace_bytes;
};

struct GemmPlan {
    int tile;      // 1, 4 or 5
    int ksplit;    // 1 with tile 1
    int group;     // GemmP::group of the 256-row kernels; 0 with tile 1
};

// Tile-shape policy.  Modelled per-CU rates (TFLOP/s per CU, measured on MI355X): the 128x128 kernel
// runs 2 workgroups per CU, the 256-row kernels one.  Cost = rounds of workgroups x work per round.
inline double est_time_128(int M, int N, int K) {
    const double tiles = (double)((M + 127) / 128) * ((N + 127) / 128);
    const double rounds = std::ceil(tiles / 512.0);
    // per-round fixed cost: the kernel alone runs 32768 x 2240 x 320 in 85 us (9 rounds of 6.2 us of MFMA work) and
    // 32768 x 11200 x 320 in 401 us (44 rounds) -- ~3 us a round that the rate does not cover, and what made the policy
    // keep short-K products on this kernel that the 256 x 320 tile runs 7..16 % faster (profiles/r04_k_*)
    const double fixed = 3e-6;
    return rounds * (2.0 * (2.0 * 128 * 128 * (double)K) / 3.4e12 + fixed);
}
// ``streams``: the caller's per-call hint (policy word of yat_gemm_bf16_ex): independent GEMM streams sharing the chip
inline double est_time_256(int M, int N, int K, int BNv, int ksplit, int streams) {
    const double tiles = (double)((M + 255) / 256) * ((N + BNv - 1) / BNv) * ksplit;
    // A GEMM of the training step seldom has the chip to itself (weight gradients on the side stream beside the dgrad chain, two
    // forward chains), and a whole-round model then picks wrongly: it splits K (slab traffic + a reduce kernel) or takes the
    // narrower tile to fill a last round that the neighbouring stream would have filled anyway.  The host says how many
    // independent GEMM streams it keeps in flight (per call, in the policy word of yat_gemm_bf16_ex).  One: whole rounds, the choice that is fastest
    // for the launch alone.  More: the launch is charged its CU-time (tiles / 256 rounds) but at least 0.375 of the chip, so K
    // is still split until ~96 workgroups exist (a 25-tile K = 32768 weight gradient left unsplit is cheap in CU-time and
    // 0.75 ms long: the side stream becomes the critical path).  Measured in the step on one box, every bench
    // (git history: scripts/gpu_policy_sweep.sh; today scripts/gpu_ab.sh): whole rounds -> this: SANA 88.3 -> 86.0 ms, PixArt 235 -> 232, LoKr B=32 354 -> 352;
    // floor 0.25 loses PixArt (260), no floor loses LoKr (431) and PixArt (315); planning for a 128-CU share with whole
    // rounds of THAT (the obvious model) keeps half the gain (87.4).
    const double rounds = streams <= 1 ? std::ceil(tiles / 256.0)               // alone on the chip: whole rounds
                                       : std::fmax(tiles / 256.0, 0.375);       // sharing it: CU-time, but spread over >= 96 CUs
    double t = rounds * ((2.0 * 256 * BNv * (double)K / ksplit) / 5.0e12 + 8e-6);   // + per-workgroup fixed cost
    if (ksplit > 1) t += (ksplit + 0.5) * (double)M * N * 4.0 / 4.0e12 + 3e-6;      // slab write + reduce pass
    return t;
}

inline int gemm_plan(const GemmQuery& q, const GemmWord& w, GemmPlan& plan) {
    if (q.epi < 0 || q.epi >= EPI_COUNT) return YAT_EINVAL;
    const GemmRule& rule = GEMM_RULES[q.epi];
    const int M = q.M, N = q.N, K = q.K;
    if (!(rule.layouts & gemm_layout_bit(q.a_t, q.b_t)) || (rule.need_wide && !q.wide_ok)) return YAT_EINVAL;
    if (q.epi == EPI_PAIR2 && (q.K2 <= 0 || q.K2 % 64 || q.a2_group < 0)) return YAT_EINVAL;      // whole K-tiles of K2
    // second operand pair with one block of A2 per a2_group columns of C: a column tile must not straddle two blocks
    const bool pair_blocks = q.epi == EPI_PAIR2 && q.a2_group != 0;
    const bool ok4 = rule.tile4 && !(pair_blocks && q.a2_group % 256), ok5 = rule.tile5 && !(pair_blocks && q.a2_group % 320);
    const bool split_ok = rule.split_k && q.has_workspace && q.wide_ok;
    const auto fits = [&](int s) { return (uint64_t)s * M * N * 4 <= q.workspace_bytes; };
    int tile = w.tile, ksplit = w.ksplit;
    if (tile == 0 && !rule.k128) {
        // 256-row-only class, whole K per workgroup: the wider tile where the model says it is faster
        if (!ok4 && !ok5) return YAT_EINVAL;
        const int Kt = q.epi == EPI_PAIR2 ? K + q.K2 : K;
        tile = !ok4 ? 5 : !ok5 ? 4 : est_time_256(M, N, Kt, 320, 1, w.streams) < est_time_256(M, N, Kt, 256, 1, w.streams) ? 5 : 4;
    } else if (tile == 0) {
        tile = 1;
        // (N >= 256: one 256/320-wide column tile is fine when K is long enough to split -- the [out, in_m*r] weight
        //  gradients of the factored LoKr path are 2240 x 320 x 32768: 9 tiles, split 28 ways)
        const bool big = M >= 1024 && (N >= 512 || (N >= 256 && K >= 2048)) && K >= 256;
        // Skinny outputs with a long reduction -- the embedders' M = B rows (time_embed.linear dgrad: 8 x 2240 x 13440), the
        // patch-embedding / output-head weight gradients (32 channels x 2240 x 8192 tokens): on the 128 x 128 kernel they are
        // 18 workgroups walking 128..210 k-tiles each (150..250 us with the chip idle, at the head of the forward and the tail
        // of the backward); split along K on the 256-row kernel (mostly zero-filled tile, but the launch is bound by reading
        // the weight) they are ~7 tiles x 16..26 slices.  Only with a split: unsplit, the small kernel is the better one.
        const bool skinny = !big && K >= 2048 && M >= 8 && N >= 32;
        if (big || skinny) {
            double best = est_time_128(M, N, K);
            for (int v = 4; v <= 5; ++v)
                for (int s = skinny ? 2 : 1; s <= 32; ++s) {
                    // any factor, not only powers of two: what matters is tiles x s against the 256 CUs (75 tiles x 3 = 225
                    // fills one round; x 2 leaves 106 CUs idle, x 4 spills into a second round)
                    if (s > 1 && (!split_ok || !fits(s) || K / s < 512)) continue;
                    const double t = est_time_256(M, N, K, v == 4 ? 256 : 320, s, w.streams);
                    if (t < best) { best = t; tile = v; ksplit = s; }
                }
        }
    }
    if (tile == 1 ? !rule.k128 : tile == 4 ? !ok4 : !ok5) return YAT_EINVAL;
    if (ksplit > 1 && (tile == 1 || !split_ok || !fits(ksplit))) return YAT_EINVAL;      // (a forced split the pick did not replace)
    plan.tile = tile;
    plan.ksplit = ksplit;
    // Tile order: 4 rows of 256-row tiles share their B panels inside one XCD's contiguous run.  Swept per shape
    // (scripts/gemm_group_sweep.py, profiles/r03_d_gemm_group_sweep.txt): the L2-miss traffic moves by up to 2.7 x with the
    // group size (profiles/r03_d_gemm_traffic_vs_tile_order.txt) and the time by < 1 % -- the re-reads are served by the
    // Infinity Cache -- except the long-K input gradient (8192 x 2240 x 11200: 7 MB B panels), 3 - 6 % faster with 8.
    plan.group = tile == 1 ? 0 : w.group ? w.group : (!q.a_t && q.b_t && K >= 8192) ? 8 : 0;
    return YAT_OK;
}

#endif  // YAT_GEMM_POLICY_HPP
