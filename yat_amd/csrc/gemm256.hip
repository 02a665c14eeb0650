// gemm256: 256 x (256|320) x 64 tile bf16 MFMA GEMM for gfx950 with two staggered wave groups.
//
// Why a second kernel: the 128x128 kernel (gemm.hip) needs ~150 GB/s of L2->LDS traffic per CU at
// full MFMA rate (38 TB/s chip-wide, above the ~34 TB/s aggregate L2 bandwidth); a 256-wide tile
// halves the bytes per flop.  A 256x256 tile fills the LDS of a CU (2 x 64..72 KiB), so there is
// one workgroup per CU and nothing from a neighbouring workgroup to hide its barriers; the overlap
// has to come from inside the workgroup:
//
//   8 waves = 2 groups (g = wave>>2, rows [128g,128g+128)) x 4 column slices.  Waves w and w+4 land
//   on the same SIMD.  Every K-tile is split into two 32-deep sub-steps, each a LOAD segment (12+
//   ds_reads of the fragments and nothing else) followed by a COMPUTE segment (32..40 MFMA 16x16x32 on
//   registers only, with the wave's LDS-DMA pieces issued between them), separated by raw s_barriers.
//   Group 1 executes one extra barrier before its loop (group 0 one after), so on each SIMD one wave
//   computes while the other loads: the matrix pipe sees back-to-back MFMA segments.
//
// LDS-DMA protocol.  The only ordering for a DMA'd piece is the issuing wave's vmcnt + a barrier the reader has passed.  The
// n-th barrier of every wave is one rendezvous.
//   Numbering.  u = 2 t + kk numbers the 32-deep sub-steps (K-tile t, half kk).  Tile t lives in stage t & 1; the k-rows
//           0..31 / 32..63 of an image are contiguous, so the halves form a four-slot ring in the two stages and half u + 4
//           takes the place of half u.  Group 0's LOAD(u) ends with rendezvous 2u+1, its COMPUTE(u) with 2u+2; group 1's with
//           2u+2 / 2u+3.  Hence half u is last read before rendezvous 2u+2, and half v is first read after rendezvous 2v.
//   Issue.  Every wave fetches a share of every half, as one BATCH of pieces per COMPUTE segment (one piece every GAP MFMAs;
//           with the issue in a LOAD segment that segment outlasts the partner's COMPUTE segment and the matrix pipe idles):
//           group 0 issues its share of half u+3 in COMPUTE(u)  -- after 2u+1 > 2(u-1)+2: the slot's half u-1 has been read;
//           group 1 issues its share of half u+4 in COMPUTE(u)  -- after 2u+2: half u has been read.
//   Waits.  Counted: group 0 waits for its share of half u+3 at the end of COMPUTE(u+2) (before 2u+6, the first read of it)
//           with its two younger batches still in flight, s_waitcnt vmcnt(n(u+1) + n(u+2)) = the pieces of one K-tile; group 1
//           waits for its share of half u+4 at the end of LOAD(u+3) (before 2u+8), again past two younger batches.  The counts
//           hold only while a loop iteration issues exactly the pieces the source counts and no other vector-memory
//           operation: yat_amd/build.py (check_gemm256_deep_asm) checks that on the compiler's assembly at every build.  The
//           prologue fetches tile 0 in full and then issues the batches a running loop would have issued before iteration 0,
//           so the same counts hold from the first iteration; the last iterations (a batch of the window is missing or
//           belongs to the ragged last K-tile, whose pieces take the per-lane CHECKED form) wait with vmcnt(0).
//   k-contiguous A (forward and input-gradient layouts).  A 128-B row of this image carries both halves of a row of A, so
//           it cannot be refilled per half -- but rows [128g, 128g+128) are read by group g alone: group g issues its own 128
//           rows of tile t+2 in COMPUTE(t, kk = 1), first in the batch, right after its own last read of tile t, and waits for
//           them before the rendezvous that precedes its LOAD(t+2, kk = 0).  A k-strided A (weight gradient, `tn`) is
//           fetched per half like B.
//   k-contiguous B (forward layouts).  Both groups read every column of B, so there is no such private part; its LDS image is
//           HALF-MAJOR instead ([half][column][4 chunks of 16 B], see B_KH in the kernel body): piece for piece the shape of
//           the k-strided image, fetched per half by the same batches under the same counts.
// A piece has 4..6 segments (1.0..1.5 K-tiles) to land.
//
// Predecessor.  Until round 4 (k-strided B) / round 5 (every layout) the K loop was a two-stage ring of whole tiles: group 0
// issued tile t+1 in COMPUTE(t, 0), group 1 tile t+2 in COMPUTE(t, 1) (forward layouts: every wave tile t+1 in LOAD(t, 0)), all
// waits vmcnt(0) before rendezvous 4t+4.  A piece then had 2..4 segments to land: enough for the Infinity Cache, short for HBM
// under load -- operands from HBM cost the same launches +10..+25 % at the sustained clock (scripts/gemm_sustained_probe.py).
// This schedule fills the same LDS bytes with the same pieces and keeps the fragment reads and the MFMA order, so it was
// bit-identical to the two-stage build over 113 cases (profiles/r04_c_gemm_hash_deep_equals_two_stage.txt,
// profiles/r05_a_gemm_hash_kh_deep_equals_r04.txt) and took the cold / hot gap from 15..24 % to 2..6 % and the step from 79.6
// to 77.4 ms (profiles/r04_a_*, r04_b_gemm_deep_in_step_ab.txt; forward layouts: r05_a_gemm_kh_deep_step_ab.txt).  What its
// switches had decided for the forward layouts before that: all DMA in compute segments + 4..6 % on the shapes alone but 2.4 ms
// slower in the step; the pieces behind the fragment reads of LOAD(t, 0) + 3..4 % alone, 84.4 -> 84.6 ms in the step.  The
// two-stage loop, its build switches (DMA placement, early rendezvous, ablations) and its s_memtime stamps
// (profiles/r02_h_gemm_ablation.txt, r02_k_gemm_stamps.txt, r02_n_gemm_stamps.txt, r02_t_gemm_energy_ablation.txt) can last be
// read at commit 4a098f80e878c3dca5c41c4d5967b747e19b3a55; that this file compiles to the same instructions without them is
// recorded in profiles/gemm256_one_schedule_a_asm_identity.txt.
//
// Operand layouts, swizzles, swapped-operand MFMA and epilogue are those of gemm.hip.
#include "common.hpp"
#include "gemm_common.hpp"
#include <type_traits>

namespace {

constexpr int BM = 256, BK = 64;

template <int NT> struct Geo {
    static constexpr int BN = 64 * NT;                 // 4 column slices x NT tiles of 16
    static constexpr int A_BYTES = BM * BK * 2;        // 32 KiB
    static constexpr int B_BYTES = BN * BK * 2;        // 32 / 40 KiB
    static constexpr int STAGE = A_BYTES + B_BYTES;
    static constexpr int LDS = 2 * STAGE;              // 128 / 144 KiB
};

// Swizzle of the k-strided image (XOR on the 16-B chunk index of k-row `krow`; bit 0 untouched so a 32-B block of
// ds_read_b64_tr_b16 stays together).  The 8 rows one 32-lane half reads ({0..3, 8..11} + 4n) must land on 8 distinct
// 32-B blocks of the 256-B bank row:
//  * row stride = 0 mod 256 B (256 columns): every row starts on the same bank -> XOR 3 bits (closed over 16 chunks);
//  * row stride = 128 mod 256 B (320 columns, 40 chunks per row): odd rows are already offset by 128 B, so XOR only
//    2 bits (closed over groups of 8 chunks -- a 4-bit XOR would leave the 40-chunk row).
template <int COLS>
__device__ __forceinline__ uint32_t trswz2(uint32_t krow) {
    if ((COLS * 2) % 256 == 0) return ((krow & 3) | (((krow >> 3) & 1) << 2)) << 1;
    return (((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 1;
}

// loop-invariant part of one DMA piece (1 KiB of an LDS image): byte offset of this lane's 16-B chunk at k-tile 0 (or OOB).
template <bool KSTRIDED, int ROWS_OR_COLS>
__device__ __forceinline__ uint32_t make_piece(int piece, int lane, int ld, int idx0, int idx_max) {
    if (!KSTRIDED) {
        const int r = piece * 8 + (lane >> 3);
        const int c = swz128(r, lane & 7);
        const int gi = idx0 + r;
        return gi < idx_max ? (uint32_t)(((int64_t)gi * ld + c * 8) * 2) : YAT_OOB;
    } else {
        constexpr int ROWB = ROWS_OR_COLS * 2;                 // bytes per k-row of the LDS image
        const uint32_t o = piece * 1024 + lane * 16;
        const uint32_t r = o / ROWB, slot = (o % ROWB) >> 4;
        const uint32_t c = slot ^ trswz2<ROWS_OR_COLS>(r);
        const int gi = idx0 + c * 8;
        return gi < idx_max ? (uint32_t)(((int64_t)r * ld + gi) * 2) : YAT_OOB;   // k-rows past K: buffer range check
    }
}

// fragment of the k-contiguous A image (128-B rows, swz128): rows idx0 .. idx0 + 15, 32-deep half kk
__device__ __forceinline__ bf16x8 frag256(const char* lds, int idx0, int kk, int lane) {
    const uint32_t r = idx0 + (lane & 15);
    const uint32_t c = swz128(r, kk * 4 + (lane >> 4));
    return lds_read8(lds, r * 128 + c * 16);
}

// The k-strided fragment addresses, arranged so a LOAD segment computes almost nothing.  A lane reads rows r0 = 32 kk + 8 g + q
// and r0 + 4; trswz2 is the same for r0, r0 + 4 and r0 + 32 (it looks at bits 0, 1 and 3 of the row only), so ONE address per
// 16-column fragment serves both rows and both sub-steps through the instruction's immediate offset.
//  * 256-column image (operand A always; B of the 256 x 256 tile): the chunk index of fragment f is (first/8 + 2 f + p/2) ^ swz
//    with `first` a multiple of 64 columns, so bits 1..3 of first/8 are free and the XOR lands on 2 f alone:
//    address(f) = address(0) ^ (f << 5) -- one per-lane base, one v_xor per fragment.
//  * 320-column image (B of the 256 x 320 tile): first = 80 wc is not aligned like that; one per-lane address per fragment.
template <int COLS>
__device__ __forceinline__ uint32_t tr_lane_addr(uint32_t col0, int lane) {
    const uint32_t g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const uint32_t r0 = 8 * g + q;
    const uint32_t c = ((col0 + 4 * p) >> 3) ^ trswz2<COLS>(r0);
    return r0 * (COLS * 2) + c * 16 + (p & 1) * 8;
}
// The transposing read is issued as inline assembly on purpose.  Through the builtin the compiler cannot tell that the read
// does not alias a pending LDS-DMA write and puts an `s_waitcnt vmcnt(0)` in front of the first transposing read of EVERY load
// segment: the wave then waits for the tile it has only just started fetching -- the prefetch distance of the whole design
// collapses to zero for the k-strided layouts (stamps: that load segment 840..900 ticks instead of 410..490).  The ordering
// a DMA'd tile needs is in the protocol already (the issuing wave's own vmcnt wait + the rendezvous before the first read);
// the reads' own completion is the explicit `s_waitcnt lgkmcnt(0)` that ends every load segment, before any MFMA uses them.
template <int OFF>
__device__ __forceinline__ bf16x4 lds_read_tr4_asm(uint32_t lds_addr) {
    bf16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_addr), "i"(OFF));
    return v;
}
template <int COLS>
__device__ __forceinline__ bf16x8 frag_tr(uint32_t lds_addr, int kk) {
    constexpr int R4 = 4 * COLS * 2, K1 = 32 * COLS * 2;
    if (kk == 0) return cat4(lds_read_tr4_asm<0>(lds_addr), lds_read_tr4_asm<R4>(lds_addr));
    return cat4(lds_read_tr4_asm<K1>(lds_addr), lds_read_tr4_asm<K1 + R4>(lds_addr));
}

#define YAT_PHASE_BARRIER()                  \
    do {                                     \
        __builtin_amdgcn_sched_barrier(0);   \
        __builtin_amdgcn_s_barrier();        \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)

// workgroups are dealt round-robin to the 8 XCDs: give every XCD one contiguous run of `nwg` work items
__device__ __forceinline__ int xcd_contiguous(int nwg) {
    const int orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// One workgroup's whole job: `id` = work item inside problem p (tile x K slice, before the row-group swizzle).
// EPI: the epilogue class, a GemmEpi (gemm_policy.hpp): plain | GLU backward | plain + pre_add | activation backward |
// plain + row sums of A (wgrad + bias gradient) | plain, second operand pair behind K (forward layout)
template <bool A_T, bool B_T, int NT, int EPI = EPI_PLAIN>
__device__ __forceinline__ void gemm256_body(const GemmP p, int id) {
    using G = Geo<NT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave >> 2, wc = wave & 3;

    const int ksl = id % p.ksplit;             // K slice of this workgroup (slices of one tile are neighbours -> same XCD)
    id /= p.ksplit;
    const int GROUP = p.group > 0 ? p.group : 4;
    const int per_group = GROUP * p.nbn;
    const int gid = id / per_group, first_m = gid * GROUP;
    const int gsz = min(p.nbm - first_m, GROUP);
    const int tm = first_m + (id % per_group) % gsz;
    const int tn = (id % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * G::BN;

    const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.A, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.B, p.b_bytes);
    // EPI 5, the second operand pair (C = epilogue(A B^T + A2 B2^T): a PEFT adapter's factored term T P^T folded into the base
    // Linear): A2 / B2 have the row strides of A / B, so the K2 / 64 k-tiles behind the last tile of K are the same per-lane
    // offsets against two other buffer resources -- nothing else in the loop knows.  Column tiles of one A2 block: a2_group.
    const int a2_col = (EPI == EPI_PAIR2 && p.a2_group > 0) ? (n0 / p.a2_group) * p.K2 : 0;
    const __amdgpu_buffer_rsrc_t ra2 = make_rsrc(EPI == EPI_PAIR2 ? p.A2 + a2_col : p.A, EPI == EPI_PAIR2 ? p.a2_bytes - (uint64_t)a2_col * 2 : 0);
    const __amdgpu_buffer_rsrc_t rb2 = make_rsrc(EPI == EPI_PAIR2 ? p.B2 : p.B, EPI == EPI_PAIR2 ? p.b2_bytes : 0);

    const uint32_t a_kstep = A_T ? (uint32_t)(BK * p.lda * 2) : (uint32_t)(BK * 2);
    const uint32_t b_kstep = B_T ? (uint32_t)(BK * p.ldb * 2) : (uint32_t)(BK * 2);
    const int nt_main = (p.K + BK - 1) / BK;
    const int nt_all = nt_main + (EPI == EPI_PAIR2 ? p.K2 / BK : 0);
    const int kt0 = (int)(((int64_t)nt_all * ksl) / p.ksplit);                 // this slice: k-tiles [kt0, kt0 + nt)
    const int nt = (int)(((int64_t)nt_all * (ksl + 1)) / p.ksplit) - kt0;
    const bool ragged = (p.K & (BK - 1)) != 0;

    // A DMA piece costs the issuing wave its instruction AND whatever computes its operands.  The k-tile advance therefore
    // rides in the instruction's scalar offset (one s_mul per segment, no VALU per piece) and the per-lane offsets stay the
    // loop-invariant registers of make_piece.  The scalar offset is not part of the buffer range check, so the two cases that
    // lean on per-lane checks -- the ragged last k-tile (row-mode chunks past K, k-strided rows past K) -- take the CHECKED
    // form (per-lane add + compare) instead; which form a segment uses is one uniform branch per segment, not per piece.
    // (K rotation -- workgroups that share a B panel starting their loops at different depths, so that only one of them at
    // a time waits for a line's HBM miss -- was built and measured in round 5: the cold / hot gap of the forward GEMMs fell
    // from 9 .. 19 % to 3 .. 13 %, but giving up the lockstep L2 sharing cost more than that: hot + 10 %, step 76.5 -> 80.4 ms.
    // profiles/r05_b_gemm_k_rotation_rejected_*.)
    auto ktile = [&](int tl) { return kt0 + tl; };                              // iteration tl of this slice -> global K-tile
    auto is_tail = [&](int tl) { return ragged && ktile(tl) == nt_main - 1; };
    // leading k-tiles of this slice that are all full ones: up to the ragged tile of K if the slice holds it (it is the slice's
    // last tile unless a second operand pair follows it)
    const int tail_at = ragged ? nt_main - 1 - kt0 : nt;
    const int nfull = (tail_at >= 0 && tail_at < nt) ? tail_at : nt;

    f32x4 acc[8][NT];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    bf16x8 af[8], bfr[NT];
    // EPI 4: the bias gradient of the Linear whose weight gradient this is = row sums of A (= dy^T) over K, from one extra MFMA
    // per A fragment against a fragment of ones -- in the waves that own column slice 0 of the FIRST column tile only (every
    // column tile sees the same A panel).  All 16 result columns of such a tile are equal; column 0 is stored.
    const bool rs_wave = EPI == EPI_ROWSUM && p.rowsum != nullptr && tn == 0 && wc == 0;
    f32x4 racc[EPI == EPI_ROWSUM ? 8 : 1];
    if (EPI == EPI_ROWSUM) {
#pragma unroll
        for (int i = 0; i < 8; ++i) racc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // per-lane LDS addresses of the k-strided fragments (tr_lane_addr above): one for A, one (256-column) or NT for B
    const uint32_t lds0 = (uint32_t)(uintptr_t)(YAT_LDS char*)smem;
    uint32_t a_tr[1] = {0}, b_tr[NT == 4 ? 1 : NT] = {0};
    if (A_T) a_tr[0] = tr_lane_addr<BM>(0, lane);
    if (B_T && NT == 4) b_tr[0] = tr_lane_addr<G::BN>(wc * 64, lane);
    else if (B_T) {
#pragma unroll
        for (int j = 0; j < NT; ++j) b_tr[j] = tr_lane_addr<G::BN>(wc * 16 * NT + j * 16, lane);
    }
    // A COMPUTE segment issues one DMA piece every GAP MFMAs from its start: the matrix pipe keeps draining queued MFMAs
    // while the wave issues a DMA, so the LOAD segments carry only the fragment reads and stay shorter than the partner's
    // COMPUTE segment.  (2 or 4: no measurable difference once the transposing reads stopped waiting for the DMA, see frag_tr.)
    constexpr int GAP = 2;

    // B image of a k-contiguous B operand (the forward GEMMs: B = W[N, K]).  A row image like A's would keep both 32-deep
    // halves of a column in one 128-B row, so no half could be refilled before the other has been read.  Here the image is
    // HALF-MAJOR: [half h][column n][4 chunks of 16 B] -- 64-B rows, half h at h * 64 * BN bytes -- which makes it piece for
    // piece the shape of the k-strided image (1 KiB = 16 columns of one half; BN / 16 pieces per half), so the loop, its
    // batches and its counted waits are the same for both B layouts.  Chunk c of column n sits at slot
    // c ^ kh_perm((n >> 2) & 3): the 16 lanes one ds_read_b128 services together (MI355X_MICROARCH.md, LDS) read columns
    // {0..3, 12..15} of one chunk and {4..11} of its neighbour and land on 16 distinct 16-B slots of the 256-B bank row.
    constexpr bool B_KH = !B_T;
    auto kh_perm = [](uint32_t x) { return (0x78u >> (2 * x)) & 3u; };          // 0, 2, 3, 1
    const uint32_t kh_lane = ((uint32_t)(lane & 15) * 64) + ((((uint32_t)lane >> 4) ^ kh_perm((lane & 15) >> 2)) << 4);

    // the fragment reads of sub-step kk of the tile in stage t & 1 (the LDS traffic of a LOAD segment)
    auto load_frags = [&](auto grp_c, int t, int kk) {
        constexpr int GRP = decltype(grp_c)::value;
        const char* cur = smem + (t & 1) * G::STAGE;
        const uint32_t st = lds0 + (t & 1) * G::STAGE;
        if (A_T) {
            const uint32_t a0 = a_tr[0] + st + GRP * 256;            // group's rows = columns 128 GRP.. of the image
#pragma unroll
            for (int i = 0; i < 8; ++i) af[i] = frag_tr<BM>(a0 ^ (i << 5), kk);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) af[i] = frag256(cur, GRP * 128 + i * 16, kk, lane);
        }
        if (B_T && NT == 4) {
            const uint32_t b0 = b_tr[0] + st + G::A_BYTES;
#pragma unroll
            for (int j = 0; j < NT; ++j) bfr[j] = frag_tr<G::BN>(b0 ^ (j << 5), kk);
        } else if (B_T) {
#pragma unroll
            for (int j = 0; j < NT; ++j) bfr[j] = frag_tr<G::BN>(b_tr[j] + st + G::A_BYTES, kk);
        } else {                                                     // (B_KH: the half-major image)
            const char* b0 = cur + G::A_BYTES + kk * (G::B_BYTES / 2) + wc * (16 * NT * 64) + kh_lane;
#pragma unroll
            for (int j = 0; j < NT; ++j) bfr[j] = lds_read8(b0, j * 1024);
        }
    };

    // The K loop of one wave group (GRP a constant: which batches a segment carries and what its waits count is decided at
    // compile time).  The loop body exists as a FAST form -- every batch of the wait window was issued in full and none of its
    // tiles is the ragged one, so its pieces are unconditional scalar-offset DMAs and its waits are counted -- plus the general
    // form (per-piece tile checks, vmcnt(0)) for the last iterations.  Both groups execute the same number of barriers per
    // iteration in either form.
    auto k_loop = [&](auto grp_c) {
        constexpr int GRP = decltype(grp_c)::value;
        constexpr int NB = (NT == 5 && GRP == 1) ? 3 : 2;    // B pieces per half and wave (320 columns: 20 = 4 x 2 + 4 x 3)
        constexpr int NAH = A_T ? 2 : 0;                      // k-strided A: pieces per half and wave
        constexpr int NAO = A_T ? 0 : 4;                      // k-contiguous A: pieces of the group's own 128 rows per tile and wave
        // ---- this wave's pieces.  A piece index fixes both the 1 KiB of the LDS image it fills and (make_piece) the global
        // bytes that belong there, so any assignment of pieces to waves fills the same image.  The pieces of one wave are
        // chosen a whole number of swizzle periods apart (16 or 32 k-rows of a k-strided image, 32 rows of a k-contiguous
        // one): their per-lane offsets then differ by a wave-uniform number of rows, so ONE per-lane offset per operand (two
        // for the odd piece of group 1 in the 320-column image) serves them all and the row delta rides, with the K-tile
        // advance, in the instruction's scalar offset -- 2..3 address registers instead of one per piece (9).
        //   k-strided 256-column image (A; B of the 256-wide tile): piece = wave + 8 i + 16 h   -> k-row delta 16 i + 32 h
        //   k-strided 320-column image: 20 pieces per half = classes {q, q + 10}; group 0 wave wc: class wc; group 1 wave wc:
        //                               class 4 + wc and one piece of classes 8 / 9 (8, 18, 9, 19)       -> deltas 16 i + 32 h
        //   k-contiguous A, own rows:   piece = 16 GRP + wc + 4 j                                       -> own offsets (below)
        const int pa0 = A_T ? wave : 16 * GRP + wc;
        const int pb0 = NT == 4 ? wave : (GRP ? 4 + wc : wc);
        const int pbx = 8 + (wc >> 1) + 10 * (wc & 1);                     // (320 columns, group 1: 8, 18, 9, 19)
        const uint32_t va0 = make_piece<A_T, BM>(pa0, lane, p.lda, m0, p.M);
        // (k-contiguous A: the pieces of a wave are 32 ROWS of M apart, and a scalar-offset delta is outside the buffer range
        // check -- past the last row of a ragged M it would read beyond the operand.  They keep their own per-lane offsets,
        // each with make_piece's row check.)
        uint32_t vao[A_T ? 1 : 4];
        if (!A_T) {
#pragma unroll
            for (int j = 0; j < 4; ++j) vao[j] = j == 0 ? va0 : make_piece<false, BM>(pa0 + 4 * j, lane, p.lda, m0, p.M);
        }
        const uint32_t vb0 = B_KH ? 0 : make_piece<true, G::BN>(pb0, lane, p.ldb, n0, p.N);
        const uint32_t vbx = (NB == 3 && !B_KH) ? make_piece<true, G::BN>(pbx, lane, p.ldb, n0, p.N) : 0;
        // half-major k-contiguous B image (B_KH): piece q of half h = the 64-B half rows of columns 16 q .. 16 q + 15.  The
        // pieces of a wave are 128 or 160 COLUMNS of N apart, and a scalar-offset delta is outside the buffer range check (past
        // the last column of a ragged N it would read beyond the operand): each keeps its own per-lane offset with its own column
        // check; only the half (+ 64 B inside a valid row) and the K-tile advance ride in the scalar offset.
        constexpr int PH = G::BN / 16;                                                      // pieces per half
        const uint32_t kchunk_b = ((uint32_t)lane & 3) ^ kh_perm(((uint32_t)lane >> 4) & 3);  // source chunk of a B_KH lane
        auto kh_q = [&](int i) { return NT == 4 ? pb0 + 8 * i : (i < 2 ? pb0 + 10 * i : pbx); };
        uint32_t vbk[B_KH ? NB : 1];
        if (B_KH) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int col = n0 + 16 * kh_q(i) + (lane >> 2);
                vbk[i] = col < p.N ? (uint32_t)(((int64_t)col * p.ldb + kchunk_b * 8) * 2) : YAT_OOB;
            }
        }
        const uint32_t a_row = (uint32_t)p.lda * 2, b_row = (uint32_t)p.ldb * 2;           // bytes per k-row (k-strided)
        const uint32_t kchunk_a = swz128((uint32_t)pa0 * 8 + (lane >> 3), lane & 7);       // (k-contiguous A: the same for all 4)

        // one piece: operand / image piece / source offset (per-lane + uniform) / target tile (local index tl)
        auto dma = [&](auto checked, bool is_a, int pi, uint32_t voff, uint32_t delta, int tl, int kh_half = 0) {
            constexpr bool CHECKED = decltype(checked)::value;
            const int tg = ktile(tl);
            const bool second = EPI == EPI_PAIR2 && tg >= nt_main;                  // uniform: a tile of the second operand pair
            const int t = second ? tg - nt_main : tg;
            YAT_LDS void* dst = (YAT_LDS void*)(smem + (tl & 1) * G::STAGE + (is_a ? 0 : G::A_BYTES) + pi * 1024);
            const uint32_t soff = (uint32_t)t * (is_a ? a_kstep : b_kstep) + delta;
            if (CHECKED) {                                                  // (only the ragged tile of K: never `second`)
                uint32_t v = voff + soff;
                if (is_a && !A_T && kchunk_a >= ((uint32_t)(p.K - t * BK) >> 3)) v = YAT_OOB;
                if (!is_a && B_KH && kchunk_b + 4 * kh_half >= ((uint32_t)(p.K - t * BK) >> 3)) v = YAT_OOB;
                lds_dma16(is_a ? ra : rb, dst, v);
            } else if (second) {
                lds_dma16s(is_a ? ra2 : rb2, dst, voff, soff);
            } else {
                lds_dma16s(is_a ? ra : rb, dst, voff, soff);
            }
        };
        // piece i of half h of the k-strided images / own-row piece j of the k-contiguous A image
        auto dma_ah = [&](auto checked, int h, int i, int tl) {
            dma(checked, true, pa0 + 8 * i + 16 * h, va0, (uint32_t)(16 * i + 32 * h) * a_row, tl);
        };
        auto dma_ao = [&](auto checked, int j, int tl) { dma(checked, true, pa0 + 4 * j, vao[A_T ? 0 : j], 0u, tl); };
        auto dma_bh = [&](auto checked, int h, int i, int tl) {
            if (B_KH) dma(checked, false, kh_q(i) + PH * h, vbk[B_KH ? i : 0], 64u * h, tl, h);
            else if (NT == 4) dma(checked, false, pb0 + 8 * i + 16 * h, vb0, (uint32_t)(16 * i + 32 * h) * b_row, tl);
            else if (i < 2) dma(checked, false, pb0 + 10 * i + 20 * h, vb0, (uint32_t)(16 * i + 32 * h) * b_row, tl);
            else dma(checked, false, pbx + 20 * h, vbx, (uint32_t)(32 * h) * b_row, tl);
        };
        // batch(u), u = 2 t + kk: piece j of [own A rows of tile t + 2 (kk = 1, k-contiguous A)] [A half] [B half] where the
        // half is u + 3 + GRP: tile t + (c >> 1), half c & 1 with c = kk + 3 + GRP
        auto batch_count = [](int kk) constexpr { return (NAO && kk == 1 ? NAO : 0) + NAH + NB; };
        auto batch_piece = [&](auto kk_c, auto fast_c, int t, int j) {
            constexpr int KK = decltype(kk_c)::value;
            constexpr bool FAST = decltype(fast_c)::value;
            constexpr int C = KK + 3 + GRP, HV = C & 1, NOWN = (NAO && KK == 1) ? NAO : 0;
            const bool own = j < NOWN;
            const int tl = own ? t + 2 : t + (C >> 1);
            auto go = [&](auto checked) {
                if (own) dma_ao(checked, j, tl);
                else if (j < NOWN + NAH) dma_ah(checked, HV, j - NOWN, tl);
                else dma_bh(checked, HV, j - NOWN - NAH, tl);
            };
            if (FAST) go(std::false_type{});
            else if (tl < nt) {
                if (is_tail(tl)) go(std::true_type{});
                else go(std::false_type{});
            }
        };
        // counted waits (FAST iterations: every batch of the window was issued in full; otherwise vmcnt(0))
        constexpr int PER_TILE = NAO + 2 * NAH + 2 * NB;                   // pieces per wave and K-tile = two consecutive batches
        auto wait_g0 = [&](auto fast_c) {                                  // end of COMPUTE(u): batch(u - 2) landed
            if (decltype(fast_c)::value) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_TILE) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        auto wait_g1 = [&](auto kk_c, auto fast_c) {                       // end of LOAD(u): batch(u - 3) landed, and the own
            constexpr int KK = decltype(kk_c)::value;                      // A rows of batch(u - 2) when u is odd
            constexpr int N = NAO ? (KK == 1 ? 2 * NB : 2 * NB + NAO) : PER_TILE;
            if (decltype(fast_c)::value) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        auto compute = [&](auto kk_c, auto fast_c, int t) {
            constexpr int KK = decltype(kk_c)::value;
            constexpr int NP = batch_count(KK);
            static_assert((8 * NT) / GAP >= NP, "not enough MFMA slots for the DMA pieces of a batch");
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);   // D[n][m]
                    const int idx = i * NT + j;
                    if (idx % GAP == GAP - 1 && idx / GAP < NP) {
                        __builtin_amdgcn_sched_barrier(0);
                        batch_piece(kk_c, fast_c, t, idx / GAP);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (EPI == EPI_ROWSUM && idx == 8 * NT - 1 && rs_wave) {
                        bf16x8 ones;
#pragma unroll
                        for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
#pragma unroll
                        for (int q = 0; q < 8; ++q) racc[q] = mfma16(ones, af[q], racc[q]);
                    }
                    if (idx == 8 * NT - 1) {
                        // (the counted wait is an asm the scheduler may hoist over the register-only MFMAs -- it did, to right
                        // behind the segment's last piece, giving up a segment of landing time: pinned behind them)
                        if (GRP == 0) {
                            __builtin_amdgcn_sched_barrier(0);
                            wait_g0(fast_c);
                        }
                        YAT_PHASE_BARRIER();
                    }
                }
            }
            __builtin_amdgcn_s_setprio(0);
        };
        auto iteration = [&](auto fast_c, int t) {
            // ---- sub-step 0
            load_frags(grp_c, t, 0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (GRP == 1) wait_g1(std::integral_constant<int, 0>{}, fast_c);
            YAT_PHASE_BARRIER();
            compute(std::integral_constant<int, 0>{}, fast_c, t);
            // ---- sub-step 1
            load_frags(grp_c, t, 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (GRP == 1) wait_g1(std::integral_constant<int, 1>{}, fast_c);
            YAT_PHASE_BARRIER();
            compute(std::integral_constant<int, 1>{}, fast_c, t);
        };

        // prologue: tile 0 in full (every wave its own pieces), then the batches a running loop would have issued for tile 1:
        // group 0 batch(-1); group 1 batch(-2) and batch(-1) -- the counted waits of the first iterations count on them
        {
            auto all_of_tile0 = [&](auto checked) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (A_T) dma_ah(checked, j >> 1, j & 1, 0);
                    else dma_ao(checked, j, 0);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < NB; ++i) dma_bh(checked, h, i, 0);
            };
            if (is_tail(0)) all_of_tile0(std::true_type{});
            else all_of_tile0(std::false_type{});
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        YAT_PHASE_BARRIER();                       // rendezvous 0: tile 0 visible to everyone
        if (GRP == 1) {
#pragma unroll
            for (int j = 0; j < batch_count(0); ++j) batch_piece(std::integral_constant<int, 0>{}, std::false_type{}, -1, j);
        }
#pragma unroll
        for (int j = 0; j < batch_count(1); ++j) batch_piece(std::integral_constant<int, 1>{}, std::false_type{}, -1, j);
        if (GRP == 1) YAT_PHASE_BARRIER();         // stagger: group 1 runs one segment behind group 0

        const int nfast = max(0, nfull - 2);
        int t = 0;
        for (; t < nfast; ++t) iteration(std::true_type{}, t);
        for (; t < nt; ++t) iteration(std::false_type{}, t);
    };
    if (grp == 0) k_loop(std::integral_constant<int, 0>{});
    else k_loop(std::integral_constant<int, 1>{});
    if (grp == 0) YAT_PHASE_BARRIER();         // pair group 1's last barrier

    if (EPI == EPI_ROWSUM && rs_wave && p.ksplit == 1 && (lane >> 4) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + grp * 128 + i * 16 + lane;
            if (m < p.M) {
                float v = racc[i][0];
                if (p.rowsum_acc) v = rbf(v) + bf2f(p.rowsum[m]);
                p.rowsum[m] = f2bf(v);
            }
        }
    }
    // ---- epilogue.  The MFMA layout gives a lane 4 columns of 16 different rows (8-B accesses in 32-B runs).  When
    // everything is 16-B aligned the accumulators go through the (now free) LDS instead: each wave transposes 32 rows
    // at a time in a private padded fp32 slab and reads back 8 consecutive columns per lane, so bias / gate / residual
    // loads and C / aux stores are 16 B per lane over whole 128..160-B row segments.
    const int rpb = p.rows_per_batch > 0 ? p.rows_per_batch : p.M;
    const bool wide = !(p.N & 7) && !(p.ldc & 7) && !(p.res && (p.ldr & 7)) && !(p.aux && (p.ldaux & 7)) &&
                      !(p.gate && (p.gate_ld & 7)) && !(p.glu_u && (p.ld_glu & 7)) && !(p.pre_add && (p.ld_pre & 7)) &&
                      !(p.dact_z && (p.ld_z & 7));
    const bool split = p.ksplit > 1;           // host guarantees `wide` alignment when splitting
    // (Round 5 built the 8-column units by a LANE EXCHANGE instead -- v_permlane16_swap of two neighbouring result tiles leaves
    // every lane with 8 consecutive columns of one row, no LDS slab, no lgkmcnt waits; bit-identical -- and it was 3 .. 10 %
    // SLOWER per launch (step 76.5 -> 79.7 ms): a store instruction then covers 16 rows x 64 B instead of 6.4 rows x 160 B.
    // The epilogue is bound by the row segments its stores touch, not by the LDS round trip.  profiles/r05_g_*.)
    if (wide || split) {
        constexpr int WCOLS = 16 * NT;             // columns per wave
        constexpr int LDW = WCOLS + 4;             // padded fp32 row (conflict-free ds_write_b128)
        constexpr int CPR = WCOLS / 8;             // 8-column chunks per row
        float* slab = reinterpret_cast<float*>(smem) + wave * (32 * LDW);
        const int g4 = lane >> 4, li = lane & 15;
        // The epilogue's own global INPUTS (residual, pre_add, GLU u, activation input z) are loaded one pass of 32 rows
        // ahead of their use, into the registers the pass before has just emptied: read where they are consumed, each of the
        // four passes of a tile paid an HBM round trip behind its slab round trip (the gated-residual and GLU-backward GEMMs
        // ran 714 .. 990 TFLOP/s in the step).  Same loads, same arithmetic, same stores: bit-identical.
        constexpr int UPL = (32 * CPR + 63) / 64;          // 8-column units per lane and pass
        const bool pre_on = !split && (EPI == EPI_GLU_BWD || EPI == EPI_ACT_BWD || EPI == EPI_PRE_ADD || p.res != nullptr);
        // one input stream (residual | z): a whole pass ahead, double-buffered; two streams (GLU u_a + u_g, residual + pre_add):
        // the registers do not hold two passes of both -- loaded at the top of their own pass, before its slab round trip
        constexpr bool AHEAD = EPI != EPI_GLU_BWD && EPI != EPI_PRE_ADD;
        EpiIn ein[AHEAD ? 2 : 1][UPL];
        auto unit = [&](int pass, int k, int& row, int& ch, int& m, int& n) {
            const int u = lane + 64 * k;
            row = u / CPR;
            ch = u % CPR;
            m = m0 + grp * 128 + pass * 32 + row;
            n = n0 + wc * WCOLS + ch * 8;
            return u < 32 * CPR && m < p.M && n < p.N;
        };
        auto prefetch = [&](int pass, EpiIn (&in)[UPL]) {
#pragma unroll
            for (int k = 0; k < UPL; ++k) {
                int row, ch, m, n;
                if (!unit(pass, k, row, ch, m, n)) continue;
                if (EPI == EPI_GLU_BWD) {
                    const bf16_t* up = p.glu_u + (int64_t)m * p.ld_glu + n;
                    in[k].a = *reinterpret_cast<const u32x4*>(up);
                    in[k].b = *reinterpret_cast<const u32x4*>(up + p.N);
                } else if (EPI == EPI_ACT_BWD) {
                    in[k].a = *reinterpret_cast<const u32x4*>(p.dact_z + (int64_t)m * p.ld_z + n);
                } else {
                    if (p.res) in[k].a = *reinterpret_cast<const u32x4*>(p.res + (int64_t)m * p.ldr + n);
                    if (EPI == EPI_PRE_ADD) in[k].b = *reinterpret_cast<const u32x4*>(p.pre_add + (int64_t)m * p.ld_pre + n);
                }
            }
        };
        if (pre_on && AHEAD) prefetch(0, ein[0]);
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            if (pre_on && !AHEAD) prefetch(pass, ein[0]);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    *reinterpret_cast<f32x4*>(slab + (ii * 16 + li) * LDW + j * 16 + 4 * g4) = acc[pass * 2 + ii][j];
            if (pre_on && AHEAD && pass + 1 < 4) prefetch(pass + 1, ein[(pass + 1) & 1]);       // (into the registers this pass freed)
            // wave-private slab: the wave's own LDS writes are ordered before its reads by lgkmcnt; no barrier needed
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < UPL; ++k) {
                int row, ch, m, n;
                if (unit(pass, k, row, ch, m, n)) {
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(slab + row * LDW + ch * 8);
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(slab + row * LDW + ch * 8 + 4);
                    if (split) {               // fp32 partial slab [ksl][m][n]; epilogue runs in the reduce kernel
                        float* dst = p.partial + ((int64_t)ksl * p.M + m) * p.N + n;
                        *reinterpret_cast<f32x4*>(dst) = lo;
                        *reinterpret_cast<f32x4*>(dst + 4) = hi;
                    } else {
                        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        const EpiIn* pin = pre_on ? &ein[AHEAD ? (pass & 1) : 0][k] : nullptr;
                        if (EPI == EPI_GLU_BWD) glu_bwd_store<8>(p, v, m, n, pin);
                        else if (EPI == EPI_ACT_BWD) act_bwd_store<8>(p, v, m, n, pin);
                        else gemm_epilogue_store8<EPI == EPI_PRE_ADD, A_T && B_T>(p, v, m, n, m / rpb, pin);     // (weight-gradient layout: non-temporal result)
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads retired before the next pass overwrites the slab
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + grp * 128 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
        const int b = m / rpb;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + wc * 16 * NT + j * 16 + 4 * (lane >> 4);
            if (n >= p.N) continue;
            if (EPI == EPI_GLU_BWD || EPI == EPI_ACT_BWD) {
                const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                if (EPI == EPI_GLU_BWD) glu_bwd_store<4>(p, v, m, n);
                else act_bwd_store<4>(p, v, m, n);
            } else {
                gemm_epilogue_store<EPI == EPI_PRE_ADD>(p, acc[i][j], m, n, b);
            }
        }
    }
}

// One tile per workgroup.  Measured in round 5 and not kept (profiles/r05_d_*): a PERSISTENT form (256 workgroups walking the
// tile list, same tile -> XCD assignment, bit-identical) is 1.7 .. 2.3 % faster alone on launches of five and more rounds,
// 4.6 % slower on two-round ones and 0.5 % slower in the step, where its grid holds every CU against the other stream; the
// K sweep it came with puts the fixed cost of a tile round at 6.6 us against 1.75 us per K-tile -- the time is in the loop,
// not between tiles.  Delaying the first round's workgroups so that the epilogues leave lockstep changes nothing (the
// epilogue is not HBM-bound: cold outputs cost nothing).
template <bool A_T, bool B_T, int NT, int EPI = EPI_PLAIN>
__global__ __launch_bounds__(512, 1) void gemm256_kernel(GemmP p) {
    gemm256_body<A_T, B_T, NT, EPI>(p, xcd_contiguous(p.nbm * p.nbn * p.ksplit));
}

// Grouped launch: up to YAT_MAX_GROUP independent problems of one layout in ONE grid (problem g owns work items
// [first[g], first[g+1])).  A transformer block's seven weight-gradient GEMMs launched one by one leave 5..45 % of the
// CUs idle in their last round (81..396 tiles on 256 CUs) or pay for split-K slabs; together they are ~1240 full-K
// tiles = 4.85 rounds.  The descriptors travel in the kernel argument segment (no device allocation, no copy).
constexpr int YAT_MAX_GROUP = 8;
struct GroupedP {
    int ngroups;
    int first[YAT_MAX_GROUP + 1];
    GemmP g[YAT_MAX_GROUP];
};

template <bool A_T, bool B_T, int NT>
__global__ __launch_bounds__(512, 1) void gemm256_grouped_kernel(GroupedP gp) {
    const int id = xcd_contiguous(gp.first[gp.ngroups]);
    int g = 0;
    while (g + 1 < gp.ngroups && id >= gp.first[g + 1]) ++g;
    // the weight-gradient layout carries the row sums of A (bias gradients) for the problems that ask for them
    gemm256_body<A_T, B_T, NT, (A_T && B_T && NT == 4) ? EPI_ROWSUM : EPI_PLAIN>(gp.g[g], id - gp.first[g]);
}

template <bool A_T, bool B_T, int NT>
int launch256_grouped(int ngroups, const GemmP* probs, hipStream_t stream) {
    using G = Geo<NT>;
    if (ngroups < 1 || ngroups > YAT_MAX_GROUP) return YAT_EINVAL;
    GroupedP gp{};
    gp.ngroups = ngroups;
    for (int i = 0; i < ngroups; ++i) {
        GemmP q = probs[i];
        q.nbm = (q.M + BM - 1) / BM;
        q.nbn = (q.N + G::BN - 1) / G::BN;
        q.ksplit = 1;
        q.partial = nullptr;
        gp.g[i] = q;
        gp.first[i + 1] = gp.first[i] + q.nbm * q.nbn;
    }
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)gemm256_grouped_kernel<A_T, B_T, NT>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS) != hipSuccess)
            return YAT_EINVAL;
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm256_grouped_kernel<A_T, B_T, NT>), dim3(gp.first[ngroups]), dim3(512), G::LDS, stream, gp);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? YAT_OK : (int)e;
}

// (gemm1w -- the same 256 x 256 x 64 tile with ONE wave per SIMD and the K loop software-pipelined inside each wave, tile
// variant 6 -- was measured in round 2, never won a shape and is gone; profiles/LOG_r01_r03.md section 9.)

template <bool A_T, bool B_T, int NT, int EPI = EPI_PLAIN>
int launch256(const GemmP& p0, hipStream_t stream) {
    using G = Geo<NT>;
    GemmP p = p0;
    p.nbm = (p.M + BM - 1) / BM;
    p.nbn = (p.N + G::BN - 1) / G::BN;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)gemm256_kernel<A_T, B_T, NT, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                G::LDS) != hipSuccess)
            return YAT_EINVAL;
        attr_set = true;
    }
    if (p.ksplit < 1) p.ksplit = 1;
    hipLaunchKernelGGL((gemm256_kernel<A_T, B_T, NT, EPI>), dim3(p.nbm * p.nbn * p.ksplit), dim3(512), G::LDS, stream, p);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? YAT_OK : (int)e;
}

}  // namespace

// out[m, n..n+7] = epilogue( sum_s partial[s][m][n..] ): one thread per 8 columns, 16-B accesses
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmP p) {
    const int64_t nchunk = (int64_t)p.M * (p.N >> 3);
    const int rpb = p.rows_per_batch > 0 ? p.rows_per_batch : p.M;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nchunk; u += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(u / (p.N >> 3)), n = (int)(u % (p.N >> 3)) * 8;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int s = 0; s < p.ksplit; ++s) {
            const float* src = p.partial + ((int64_t)s * p.M + m) * p.N + n;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
            v[0] += lo[0]; v[1] += lo[1]; v[2] += lo[2]; v[3] += lo[3];
            v[4] += hi[0]; v[5] += hi[1]; v[6] += hi[2]; v[7] += hi[3];
        }
        gemm_epilogue_store8(p, v, m, n, m / rpb);
    }
}

int yat_gemm_splitk_reduce(const GemmP& p, hipStream_t stream) {
    const int64_t nchunk = (int64_t)p.M * (p.N >> 3);
    int64_t nb = (nchunk + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, stream, p);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? YAT_OK : (int)e;
}

// grouped launch, 256 x 256 tiles (the one geometry whose tile counts add up well for the weight-gradient set)
int yat_gemm256_grouped_launch(int a_t, int b_t, int ngroups, const GemmP* probs, hipStream_t stream) {
#define YAT_CASE(AT, BT) \
    if (a_t == AT && b_t == BT) return launch256_grouped<AT, BT, 4>(ngroups, probs, stream);
    YAT_CASE(false, false)
    YAT_CASE(false, true)
    YAT_CASE(true, true)
    YAT_CASE(true, false)
#undef YAT_CASE
    return YAT_EINVAL;
}

// variant: 4 -> BN=256, 5 -> BN=320.  (A 256 x 192 tile -- no ragged column tile at N = 1152 / 3456 / 4608 -- was
// instantiated and measured at the PixArt shapes: never faster than the policy's pick, 5-25 % slower than BN=320; removed.)
// Plain dispatch on (layout, tile, class); which combinations exist is GEMM_RULES (gemm_policy.hpp), which gemm_plan has applied.
int yat_gemm256_launch(int a_t, int b_t, int tile, GemmEpi epi, const GemmP& p, hipStream_t stream) {
#define YAT_CASE(AT, BT, EPI)                            \
    if ((a_t != 0) == AT && (b_t != 0) == BT && epi == EPI)  \
        return tile == 5 ? launch256<AT, BT, 5, EPI>(p, stream) : launch256<AT, BT, 4, EPI>(p, stream);
    YAT_CASE(false, false, EPI_PLAIN)
    YAT_CASE(false, true, EPI_PLAIN)
    YAT_CASE(true, true, EPI_PLAIN)
    YAT_CASE(true, false, EPI_PLAIN)
    YAT_CASE(false, true, EPI_GLU_BWD)
    YAT_CASE(false, false, EPI_PRE_ADD)
    YAT_CASE(false, true, EPI_ACT_BWD)
    YAT_CASE(false, false, EPI_PAIR2)
#undef YAT_CASE
    if (a_t && b_t && epi == EPI_ROWSUM && tile == 4) return launch256<true, true, 4, EPI_ROWSUM>(p, stream);
    return YAT_EINVAL;
}
