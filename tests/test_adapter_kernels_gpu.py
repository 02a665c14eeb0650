"""The adapter kernels of csrc/lokr.hip (LoKr, plain LoRA at every padded rank, LoHa, DoRA) at every grid wrap, ragged edge,
dispatch class and row stride -- GPU, kernel level, through yat_amd.ops.

The method: operands are SMALL INTEGERS stored as bf16.  Every product is then exact, and every fp32 partial sum is exact as
long as the sum of the absolute products stays below 2^24 -- in any order, on MFMA or VALU, over any split into chunks, waves
and workgroups.  What is left are the roundings each kernel's header comment spells out, so the reference is fp64 arithmetic
with those same roundings (``bf()`` below, at the same places) and every comparison is ``torch.equal``: a dropped, repeated
or misplaced tile changes bits, where a relative L2 norm over 10^5 rows does not move.  Each test asserts the exact-sum
condition on its own reference before it looks at the device.  (Where a scale of 0.5 makes the terms multiples of 1/2 or 1/4
the limit is 2^23 or 2^22: the condition is "every partial sum fits 24 bits at the terms' common granularity".)

The two weight-gradient kernels also run a CENSUS: a[row, q] = [q == (row // N) % R], x[row, n] = [n == row % N], so that every
row adds exactly 1 to exactly one output and out[q, n] counts the rows of its cell (<= 256: exact in bf16).

Outputs and the padding columns of strided views are pre-filled with a sentinel (7.0, or NaN where the kernel overwrites);
every test asserts that everything outside the target view keeps the sentinel's bits.

The only bounds that are not equalities are DoRA's n, s (the criteria of test_dora_row_kernels_match_torch) and dmag (one
bf16 step of exact_sum / n: the quotient is rounded once to fp32 and once to bf16)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
I16 = torch.int16
DEV = "cuda"
NAN = float("nan")
YAT_EINVAL = -1


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi):
    """Integers of [lo, hi] as bf16 (|value| <= 256: exact)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(BF)


def bf(t64):
    """One rounding to bf16 of an fp64 value that fp32 holds exactly (the tests assert that it does)."""
    return t64.float().to(BF)


def f32(scale):
    """A Python-float scale as the fp32 scalar the kernels receive."""
    return torch.tensor(scale, dtype=torch.float32)


def keeps(t, sentinel):
    """Every element of ``t`` still has the sentinel's bits (the sentinel made as the buffer was: torch.full on t's device)."""
    t = t.contiguous()
    return torch.equal(t.view(I16), torch.full_like(t, sentinel).view(I16))


def only_view_changed(buf, before, rs, cs):
    """``buf`` has the bits of ``before`` (its clone from before the call) everywhere outside buf[rs, cs]."""
    b = before.clone()
    b[rs, cs] = buf[rs, cs]
    return torch.equal(b.view(I16), buf.view(I16))


# ------------------------------------------------------------------------------------- 1. yat_lokr_rows, forward
def _rows_fwd(ops, g, rows, N, R, wb=None):
    wb = ints(g, (R, N), -2, 2) if wb is None else wb
    x = ints(g, (rows, N), -3, 3)
    assert (x.abs().double() @ wb.abs().double().T).max() < 2 ** 24
    want = bf(x.double() @ wb.double().T)                     # t1 = bf16(sum_n x wb): the kernel's one rounding
    buf = torch.full((rows + 2, R), NAN, dtype=BF, device=DEV)           # a guard row on either side of the result
    ops.lokr_rows_fwd(x.to(DEV), wb.to(DEV), buf[1:rows + 1])
    got = buf.cpu()
    assert torch.equal(got[1:rows + 1], want), (rows, N, R)
    assert keeps(buf[0], NAN) and keeps(buf[rows + 1], NAN), (rows, N, R)


def test_rows_fwd_every_class():
    """lokr_rows_fwd_kernel<KS>, KS = ceil(N / 32): N on both sides of every class boundary (32 | 40, 64 | 72, 96 | 104) and at
    8 and 128, R = 8 (lane groups g >= 2 store nothing) and 16; rows = 1, 15, 16, 17 (one tile, ragged / full / one row into
    the second), 63, 65 (the four tiles of one wave step, ragged / one row into the next wave) and 1029 (= 4 workgroup steps
    of 256 rows + 5: five workgroups, the last with one ragged tile)."""
    from yat_amd import ops
    g = gen(1)
    for R in (8, 16):
        for N in (8, 32, 40, 64, 72, 96, 104, 128):
            wb = ints(g, (R, N), -2, 2)
            for rows in (1, 15, 16, 17, 63, 65, 1029):
                _rows_fwd(ops, g, rows, N, R, wb)


def test_rows_fwd_grid_wrap():
    """grid = ceil(ceil(rows / 16) / 16) capped at 8192, 256 rows per workgroup step: 2,097,425 = 8192 * 256 + 256 + 17 rows are
    131,090 tiles = 8194 steps, so workgroups 0 and 1 make a second pass and the very last tile has one row."""
    from yat_amd import ops
    _rows_fwd(ops, gen(2), 8192 * 256 + 256 + 17, 8, 8)


def test_rows_fwd_flat_into_a_slab():
    """yat_lokr_rows_fwd_flat at R = 16, N = 80 (KS = 3), in_m = 7 (row -> (m, j) by a division that is no shift), M = 301:
    T1 as [M, in_m R] = 112 columns of a 160-wide slab, equal to the contiguous result reshaped, which equals the reference."""
    from yat_amd import ops
    M, im, N, R, ld, c0 = 301, 7, 80, 16, 160, 24
    g = gen(3)
    x, wb = ints(g, (M * im, N), -3, 3), ints(g, (R, N), -2, 2)
    assert (x.abs().double() @ wb.abs().double().T).max() < 2 ** 24
    want = bf(x.double() @ wb.double().T)
    t1 = ops.lokr_rows_fwd(x.to(DEV), wb.to(DEV), torch.full((M * im, R), NAN, dtype=BF, device=DEV))
    slab = torch.full((M, ld), 7.0, dtype=BF, device=DEV)
    before = slab.clone()
    ops.lokr_rows_fwd_flat(x.to(DEV), wb.to(DEV), slab[:, c0:c0 + im * R], im)
    assert torch.equal(t1.cpu(), want)
    assert torch.equal(slab[:, c0:c0 + im * R], t1.view(M, im * R))
    assert only_view_changed(slab, before, slice(None), slice(c0, c0 + im * R))


# ------------------------------------------------------------------------------------ 2. yat_lokr_rows, backward
def _rows_bwd(ops, g, rows, N, R):
    h, wb, dx0 = ints(g, (rows, R), -3, 3), ints(g, (R, N), -2, 2), ints(g, (rows, N), -3, 3)
    assert (h.abs().double() @ wb.abs().double()).max() + 3 < 2 ** 24
    want = bf(bf(h.double() @ wb.double()).double() + dx0.double())      # bf16(bf16(h wb) + dx0)
    buf = torch.full((rows + 2, N), 7.0, dtype=BF, device=DEV)
    buf[1:rows + 1].copy_(dx0)
    ops.lokr_rows_bwd(h.to(DEV), wb.to(DEV), buf[1:rows + 1])
    got = buf.cpu()
    assert torch.equal(got[1:rows + 1], want), (rows, N, R)
    assert keeps(buf[0], 7.0) and keeps(buf[rows + 1], 7.0), (rows, N, R)


def test_rows_bwd_every_class():
    """lokr_rows_bwd_kernel<R>: one thread per 16-byte chunk, N / 8 = 1, 7, 10, 15, 16 chunks per row (row = chunk / cpr by a
    division, a workgroup's 256 chunks end inside a row unless cpr divides 256), R = 8 and 16; rows = 1, 3 (a fraction of
    one workgroup) and 257 (several workgroups, the last partly idle)."""
    from yat_amd import ops
    g = gen(4)
    for R in (8, 16):
        for N in (8, 56, 80, 120, 128):
            for rows in (1, 3, 257):
                _rows_bwd(ops, g, rows, N, R)


def test_rows_bwd_grid_wrap():
    """grid capped at 8192 workgroups of 256 chunks = 2,097,152 chunks per pass: 131,075 rows of N = 128 (16 chunks each) are
    2,097,200 chunks, so the first 48 threads of workgroup 0 make a second pass over the last three rows."""
    from yat_amd import ops
    _rows_bwd(ops, gen(5), 131075, 128, 16)


# ----------------------------------------------------------------------------------------------- 3 / 4. yat_rank_expand
def _rank_expand(ops, rows, R, N, ld):
    g = gen(rows + R + N)
    h, w, io0 = ints(g, (rows, R), -3, 3), ints(g, (R, N), -2, 2), ints(g, (rows, N), -3, 3)
    assert (h.abs().double() @ w.abs().double()).max() + 3 < 2 ** 24
    prod = bf(h.double() @ w.double())                        # bf16(sum): the first rounding of both forms
    hd, wd = h.to(DEV), w.to(DEV)
    for residual, scale in ((0, 1.0), (0, 0.5), (0, 2.0 / 3.0), (1, 1.0)):
        buf = torch.full((rows + 1, ld), 7.0 if residual else NAN, dtype=BF, device=DEV)    # + a guard row
        if residual:
            buf[:rows, :N].copy_(io0)
            want = (prod.float() + io0.float()).to(BF)        # bf16(bf16(sum) + io)
        else:
            want = (prod.float() * f32(scale)).to(BF)         # bf16(bf16(sum) * scale)
        before = buf.clone()
        ops.rank_expand(hd, wd, buf[:rows, :N], scale=scale, residual=bool(residual))
        assert torch.equal(buf[:rows, :N].cpu(), want), (residual, scale)
        assert only_view_changed(buf, before, slice(0, rows), slice(0, N)), (residual, scale)


@pytest.mark.parametrize("rows,R,N,ld", [
    (8201, 8, 8, 16),        # 1 block of 512 columns: grid x = min(2048 / 1 + 1, ceil(8201 / 4) = 2051) = 2049 -> wraps; one live lane
    (8201, 16, 520, 528),    # 2 blocks, the second 8 columns wide: grid x = min(1025, 2051) -> every workgroup wraps
    (4105, 8, 1544, 1544),   # 4 blocks (3 x 512 + 8): grid x = min(2048 / 4 + 1 = 513, ceil(4105 / 4) = 1027) -> wraps
    (5, 8, 504, 504), (5, 16, 504, 512),     # one column short of a full wave of lanes; 2 workgroups, the second with one row
    (5, 8, 512, 520), (5, 16, 512, 512),     # exactly one full block
])
def test_rank_expand_stream(rows, R, N, ld):
    """lokr_wide_rows_kernel<8 / 16>: io = bf16(bf16(h w) * scale) at scale 1, 1/2, 2/3 and io = bf16(bf16(h w) + io), four rows
    per workgroup step under a capped grid; columns N .. ld and the guard row keep their bits."""
    from yat_amd import ops
    _rank_expand(ops, rows, R, N, ld)


@pytest.mark.parametrize("rows,R,N,ld", [
    (32805, 32, 72, 80),     # 1 block of 256 columns: grid x = min(2049, ceil(32805 / 16) = 2051 tiles) -> wraps, last tile 5 rows;
                             # wave 1 owns columns 64 .. 71 only: its lane group 0 stores `lo` without `hi`
    (16421, 64, 264, 264),   # 2 blocks (256 + 8): grid x = min(1025, 1027 tiles) -> wraps, last tile 5 rows
    (10947, 128, 520, 528),  # 3 blocks (256 + 256 + 8): grid x = min(2048 / 3 + 1 = 683, 685 tiles) -> wraps, last tile 3 rows
])
def test_rank_expand_mfma_grid_wrap(rows, R, N, ld):
    """lora_expand_mfma_kernel<32 / 64 / 128>: the same two forms with the sum on the matrix cores, 16-row tiles under a capped
    grid, ragged last tile, partial last column block."""
    from yat_amd import ops
    _rank_expand(ops, rows, R, N, ld)


# -------------------------------------------------------------------------------------------- 5 / 6. yat_lokr_small_wgrad
def _census(rows, R, N):
    row = torch.arange(rows)
    a, x = torch.zeros(rows, R, dtype=BF), torch.zeros(rows, N, dtype=BF)
    a[row, (row // N) % R] = 1
    x[row, row % N] = 1
    return a, x


def _small_wgrad(ops, rows, R, N, r_out, ldx, ldo):
    """The integer data at accumulate off / on x scale 1, 2/3 and the census at accumulate off / on; x = xw[:, 8:8 + N] of a
    NaN-padded [rows, ldx] matrix and out = ow[1:1 + r_out, c0:c0 + N] of a sentinel-filled one (c0 = 8 where ldo leaves room)."""
    g = gen(rows + R + N)
    xc0 = 8 if ldx >= N + 8 else 0
    oc0 = 8 if ldo >= N + 8 else 0
    out0 = ints(g, (r_out, N), -3, 3)
    ws = torch.empty(int(ops._lib().yat_lokr_small_wgrad_workspace_bytes(rows, R, N)), dtype=torch.uint8, device=DEV)
    cen_a, cen_x = _census(rows, R, N)
    count = cen_a.double().T @ cen_x.double()
    assert count.sum() == rows and count.max() <= 256 - 3      # every row lands in exactly one cell; counts (+ out0) exact in bf16
    print(f"[census] rows={rows} R={R} N={N}: largest cell {int(count.max())}")
    for name, a, x, scales in (("ints", ints(g, (rows, R), -2, 2), ints(g, (rows, N), -3, 3), (1.0, 2.0 / 3.0)),
                               ("census", cen_a, cen_x, (1.0,))):
        assert (a.abs().double().T @ x.abs().double()).max() < 2 ** 24
        total = (a.double().T @ x.double())[:r_out]
        xw = torch.full((rows, ldx), NAN, dtype=BF, device=DEV)
        xw[:, xc0:xc0 + N].copy_(x)
        ad = a.to(DEV)
        for scale in scales:
            new = (total.float() * f32(scale)).to(BF)          # bf16(scale * sum): the sum is exact in fp32
            for acc in (False, True):
                want = (new.float() + out0.float()).to(BF) if acc else new       # out + bf16(scale * sum), rounded
                outs = []
                for _ in range(2):
                    ow = torch.full((r_out + 2, ldo), 7.0 if acc else NAN, dtype=BF, device=DEV)
                    if acc:
                        ow[1:1 + r_out, oc0:oc0 + N].copy_(out0)
                    before = ow.clone()
                    ops.lokr_small_wgrad(ad, xw[:, xc0:xc0 + N], ow[1:1 + r_out, oc0:oc0 + N], ws, accumulate=acc, scale=scale)
                    assert torch.equal(ow[1:1 + r_out, oc0:oc0 + N].cpu(), want), (name, scale, acc)
                    assert only_view_changed(ow, before, slice(1, 1 + r_out), slice(oc0, oc0 + N)), (name, scale, acc)
                    outs.append(ow)
                assert torch.equal(outs[0].view(I16), outs[1].view(I16)), (name, scale, acc)     # two calls, equal bits


@pytest.mark.parametrize("rows,R,N,r_out,ldx,ldo", [
    # 2 column blocks (128 + 8): G = min(257 chunks of 256 rows, max(32, 512 / 2)) = 256 -> workgroup 0 takes chunk 256 as well,
    # and that wrapped chunk is the ragged one (65636 = 256 * 256 + 100)
    (65636, 8, 136, 8, 136, 136),
    # 18 column blocks (17 x 128 + 64): G = min(34 chunks, max(32, 512 / 18 = 28)) = 32 -> workgroups 0, 1 wrap (8492 = 33 * 256 + 44);
    # r_out < R, x a column block of a 2304-wide matrix, out a column block with ldo = 2248
    (8492, 16, 2240, 12, 2304, 2248),
])
def test_small_wgrad_stream_grid_wrap(rows, R, N, r_out, ldx, ldo):
    """lokr_small_wgrad_kernel (R = 8 / 16, 256-row chunks, the four waves split the k-steps) + the final sum: exact sums and
    exact counts with more chunks than workgroups, at several column blocks."""
    from yat_amd import ops
    _small_wgrad(ops, rows, R, N, r_out, ldx, ldo)


@pytest.mark.parametrize("rows,R,N,r_out,ldx,ldo", [
    # 1 column block: G = min(258 chunks of 128 rows, max(4, 256 / 1)) = 256 -> workgroups 0, 1 wrap; last chunk 37 rows
    # (32933 = 257 * 128 + 37: two full 16-row groups and one of 5)
    (32933, 32, 56, 32, 56, 56),
    # 3 column blocks (128 + 128 + 72): G = min(87, max(4, 256 / 3 = 85)) = 85 -> workgroups 0, 1 wrap; last chunk 5 rows; r_out < R
    (11013, 64, 328, 48, 328, 336),
    # 10 column blocks (9 x 128 + 8): G = min(27, max(4, 256 / 10 = 25)) = 25 -> workgroups 0, 1 wrap; last chunk 3 rows; strided x
    (3331, 128, 1160, 128, 1184, 1160),
])
def test_small_wgrad_mfma_grid_wrap(rows, R, N, r_out, ldx, ldo):
    """lora_wgrad_mfma_kernel<32 / 64 / 128> (128-row chunks, the four waves split the accumulator block) + the final sum: the
    same two data sets with more chunks than workgroups and a ragged last chunk."""
    from yat_amd import ops
    _small_wgrad(ops, rows, R, N, r_out, ldx, ldo)


# ---------------------------------------------------------------------------------------------- 7. yat_lora_scatter_b
@pytest.mark.parametrize("R", [8, 32, 128])
def test_lora_scatter_b(R):
    """lora_scatter_b_kernel<R>: dst[n, :R] = bf16(scale * src[q, n]) for three targets in one launch -- out = 8 (two of the three
    256-row workgroups of its table entry idle), 257 (one live thread in the second), 520 = max_out; in = R (the R columns are
    the whole row), R + 8, 2 R; offsets are multiples of 8 elements with gaps.  Columns R .. in of every target row, the gaps
    and both ends of dst keep the sentinel."""
    from yat_amd import ops
    g = gen(R)
    shapes = [(8, R), (257, R + 8), (520, 2 * R)]
    table, s_off, d_off = [], 8, 16
    for out, inn in shapes:
        table.append([s_off, d_off, out, inn])
        s_off += R * out + 8 * (1 + out % 3)                  # (R * out is a multiple of 8)
        d_off += out * inn + 8 * (2 + out % 5)
    src = ints(g, (s_off,), -64, 64)
    tab = torch.tensor(table, dtype=torch.int64, device=DEV)
    for scale in (0.5, 2.0 / 3.0):
        want = torch.full((d_off,), 7.0, dtype=BF)
        for so, do, out, inn in table:
            bt = src[so:so + R * out].view(R, out)            # lora_B^T [R, out]
            want[do:do + out * inn].view(out, inn)[:, :R] = (bt.float().T * f32(scale)).to(BF)
        dst = torch.full((d_off,), 7.0, dtype=BF, device=DEV)
        ops.lora_scatter_b(tab, len(table), max(o for o, _ in shapes), R, scale, src.to(DEV), dst)
        assert torch.equal(dst.cpu(), want), scale            # 7.0 has one bit pattern: the sentinel's bits everywhere else


# --------------------------------------------------------------------------------- 8. yat_lokr_delta / yat_lokr_project
@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("out_dim,in_dim", [(448, 96), (2240, 2240)])
@pytest.mark.parametrize("r", [4, 16])
def test_lokr_delta_and_project(r, out_dim, in_dim, scale):
    """delta = bf16(bf16(w1 (x) w2) * scale) with w2 = bf16(w2_a w2_b), and its autograd from d_delta: dR = bf16(dd * scale),
    d_w1 = bf16(sum dR w2), d_w2 = bf16(sum dR w1), d_w2_a = bf16(d_w2 w2_b^T), d_w2_b = bf16(w2_a^T d_w2) -- op by op, all four
    results bit for bit.  delta and d_delta are the middle third of a 3 in-wide matrix (ld = 3 in).  The scales are powers of
    two, so dR is exact; at 0.5 every term is a multiple of 1/2, hence the 2^23."""
    from yat_amd import ops
    from yat_amd.lokr import factorization
    (out_l, out_k), (in_m, in_n) = factorization(out_dim), factorization(in_dim)
    g = gen(r + out_dim + in_dim)
    w1, wa, wb = ints(g, (out_l, in_m), -2, 2), ints(g, (out_k, r), -2, 2), ints(g, (r, in_n), -2, 2)
    dd = ints(g, (out_dim, in_dim), -2, 2)
    lim = 2 ** 23
    assert (wa.abs().double() @ wb.abs().double()).max() < lim
    w2 = bf(wa.double() @ wb.double())
    delta_ref = bf(torch.kron(w1.double(), w2.double()))      # a product of an integer <= 2 and a bf16 value: exact in fp32
    if scale != 1.0:
        delta_ref = bf(delta_ref.double() * scale)
    dR = bf(dd.double() * scale)
    blk = dR.double().view(out_l, out_k, in_m, in_n)
    assert torch.einsum("ikjn,kn->ij", blk.abs(), w2.double().abs()).max() < lim
    dw1_ref = bf(torch.einsum("ikjn,kn->ij", blk, w2.double()))
    assert torch.einsum("ikjn,ij->kn", blk.abs(), w1.double().abs()).max() < lim
    dw2 = bf(torch.einsum("ikjn,ij->kn", blk, w1.double()))
    assert (dw2.abs().double() @ wb.abs().double().T).max() < lim and (wa.abs().double().T @ dw2.abs().double()).max() < lim
    dwa_ref, dwb_ref = bf(dw2.double() @ wb.double().T), bf(wa.double().T @ dw2.double())

    mid = slice(in_dim, 2 * in_dim)
    w1d, wad, wbd = w1.to(DEV), wa.to(DEV), wb.to(DEV)
    big = torch.full((out_dim, 3 * in_dim), NAN, dtype=BF, device=DEV)
    before = big.clone()
    ops.lokr_delta(w1d, wad, wbd, scale, big[:, mid])
    assert torch.equal(big[:, mid].cpu(), delta_ref)
    assert only_view_changed(big, before, slice(None), mid)
    big[:, mid].copy_(dd)                                     # d_delta between NaN thirds: a read outside the view poisons a sum
    g1, ga, gb = (torch.full((t.shape[0] + 2, t.shape[1]), NAN, dtype=BF, device=DEV) for t in (w1, wa, wb))   # guard rows
    ws = torch.empty(int(ops._lib().yat_lokr_project_workspace_bytes(out_l, out_k, in_n)), dtype=torch.uint8, device=DEV)
    ops.lokr_project(w1d, wad, wbd, scale, big[:, mid], g1[1:-1], ga[1:-1], gb[1:-1], ws)
    for got, want, nm in ((g1, dw1_ref, "d_w1"), (ga, dwa_ref, "d_w2_a"), (gb, dwb_ref, "d_w2_b")):
        assert torch.equal(got[1:-1].cpu(), want), nm
        assert keeps(got[0], NAN) and keeps(got[-1], NAN), nm


def test_lokr_project_rejects_a_w2_tile_beyond_its_lds():
    """The d_w2 tile is staged in LDS as out_k * in_n fp32 <= 64 KiB: 128 x 136 = 17408 > 16384 elements is YAT_EINVAL."""
    from yat_amd import ops
    out_l, out_k, in_m, in_n, r = 2, 128, 2, 136, 4
    z = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)
    w1, wa, wb, dd = z(out_l, in_m), z(out_k, r), z(r, in_n), z(out_l * out_k, in_m * in_n)
    ws = torch.empty(int(ops._lib().yat_lokr_project_workspace_bytes(out_l, out_k, in_n)), dtype=torch.uint8, device=DEV)
    rc = ops._lib().yat_lokr_project(out_l, out_k, in_m, in_n, r, ops._p(w1), ops._p(wa), ops._p(wb), 1.0, ops._p(dd), in_m * in_n,
                                     ops._p(z(out_l, in_m)), ops._p(z(out_k, r)), ops._p(z(r, in_n)), ops._p(ws), ops._stream())
    assert rc == YAT_EINVAL


# ----------------------------------------------------------------------------- 9. yat_hadamard_scale / yat_hadamard_bwd
def _hadamard(ops, rows, cols, lds, offs, scales, seed):
    """out = bf16(bf16(a b) * scale); g = bf16(dd * scale), t1 = bf16(g a2), t2 = bf16(g a1): bit-exact against torch's CPU bf16
    arithmetic (each op rounds once), as in test_hadamard_kernels_bit_exact.  Operand / result k is the column block
    [offs[k], offs[k] + cols) of a [rows + 1, lds[k]] matrix: inputs NaN-padded, results in NaN-filled matrices."""
    g = gen(seed)
    names = ("a", "b", "dd", "out", "t1", "t2")
    cs = {n: slice(o, o + cols) for n, o in zip(names, offs)}
    m = {n: torch.full((rows + 1, ld), NAN, dtype=BF, device=DEV) for n, ld in zip(names, lds)}
    cpu = {}
    for n in ("a", "b", "dd"):
        cpu[n] = torch.randn(rows, cols, generator=g).to(BF)
        m[n][:rows, cs[n]].copy_(cpu[n])
    v = {n: m[n][:rows, cs[n]] for n in names}
    for scale in scales:
        sc = torch.tensor(scale)
        for n in ("out", "t1", "t2"):
            m[n].fill_(NAN)
        before = {n: m[n].clone() for n in ("out", "t1", "t2")} if rows < 1000 else None
        ops.hadamard_scale(v["a"], v["b"], scale, v["out"])
        ops.hadamard_bwd(v["dd"], v["a"], v["b"], scale, v["t1"], v["t2"])
        ref = (cpu["a"] * cpu["b"]) * sc
        assert ref.dtype == BF and torch.equal(v["out"].cpu(), ref), scale
        gsc = cpu["dd"] * sc
        assert torch.equal(v["t1"].cpu(), gsc * cpu["b"]) and torch.equal(v["t2"].cpu(), gsc * cpu["a"]), scale
        for n in ("out", "t1", "t2"):
            if before is not None:
                assert only_view_changed(m[n], before[n], slice(0, rows), cs[n]), (n, scale)
            else:                                             # (the large case: contiguous, the guard row is all there is outside)
                assert keeps(m[n][rows], NAN), (n, scale)


@pytest.mark.parametrize("rows,cols", [(5, 8), (33, 72)])
def test_hadamard_every_stride_differs(rows, cols):
    """hadamard_scale_kernel / hadamard_bwd_kernel at 5 x 8 (one chunk per row: five live threads) and 33 x 72 (9 chunks per row,
    297 chunks: two workgroups, the second ragged), every operand and result a column block of a differently padded matrix, so
    that all of lda / ldb / ldo and ldd / ld1 / ld2 / ldt1 / ldt2 differ."""
    from yat_amd import ops
    lds = [cols + 8 * k for k in (1, 3, 2, 5, 4, 6)]
    offs = [8, 0, 16, 24, 8, 40]
    _hadamard(ops, rows, cols, lds, offs, (1.0, 0.5, 2.0 / 3.0), rows)


def test_hadamard_grid_wrap():
    """grid capped at 8192 workgroups of 256 chunks: 4100 x 4096 is 2,099,200 chunks against 2,097,152 per pass, so the first
    eight workgroups make a second pass over the last four rows (34 MB per tensor, six tensors)."""
    from yat_amd import ops
    _hadamard(ops, 4100, 4096, [4096] * 6, [0] * 6, (2.0 / 3.0,), 9)


# --------------------------------------------------------------------------------- 10. yat_dora_delta / yat_dora_bwd
@pytest.mark.parametrize("cols", [8, 2048, 2056, 2240, 5600])
def test_dora_row_loops(cols):
    """dora_delta_kernel / dora_bwd_kernel, one workgroup per row, 256 threads x 8 columns per pass of the row loops: cols / 8 =
    1 (one live thread), 256 (one pass, exactly full), 257 and 280 (two passes), 700 (three).  W, lw, dd, delta and t1 are column blocks of
    wider matrices (inputs NaN-padded, results NaN-filled).  Integer W, lw, dd and scaling 0.5: u = W + lw / 2 is exact, and
    so are sum u^2 (multiples of 1/4: below 2^22) and sum dd u (multiples of 1/2: below 2^23) in any order.
    n, s: the criteria of test_dora_row_kernels_match_torch (one bf16 step on n, two on s).  Given the device's own s and n:
    delta = bf16(s u - W) and t1 = bf16(bf16(s / 2) dd) bit for bit (s u is exact in fp32, so a fused multiply-add and a separate
    one round alike); dmag within one bf16 step of exact_sum / n."""
    from yat_amd import ops
    rows, scaling = 3, 0.5
    g = gen(cols)
    W, lw, dd = ints(g, (rows, cols), -3, 3), ints(g, (rows, cols), -4, 4), ints(g, (rows, cols), -3, 3)
    W[:, 0], lw[:, 0] = 3, 0                                  # no all-zero row at cols = 8
    mag = (torch.rand(rows, generator=g) * 20 + 5).to(BF)
    u = W + torch.tensor(scaling) * lw                        # bf16 op by op; exact here
    assert torch.equal(u.double(), W.double() + 0.5 * lw.double())
    assert (u.double() ** 2).sum(1).max() < 2 ** 22 and (dd.double().abs() * u.double().abs()).sum(1).max() < 2 ** 23
    n = torch.linalg.norm(u.float(), dim=1).to(BF)
    s = mag / n

    def block(t, ld, c0, fill=NAN):                           # t as the column block [c0, c0 + cols) of a [rows + 1, ld] matrix
        m = torch.full((rows + 1, ld), fill, dtype=BF, device=DEV)
        if t is not None:
            m[:rows, c0:c0 + cols].copy_(t)
        return m, m[:rows, c0:c0 + cols], slice(c0, c0 + cols)
    (_, Wv, _), (_, lwv, _), (_, ddv, _) = block(W, cols + 8, 8), block(lw, cols + 24, 0), block(dd, cols + 16, 16)
    (dm, deltav, dcs), (tm, t1v, tcs) = block(None, cols + 32, 24), block(None, cols + 40, 8)
    dbefore, tbefore = dm.clone(), tm.clone()
    sn = torch.full((2, rows + 2), NAN, dtype=torch.float32, device=DEV)          # s, n: fp32 [rows] between guards
    s_buf, n_buf = sn[0, 1:rows + 1], sn[1, 1:rows + 1]
    dmag_m = torch.full((rows + 2,), NAN, dtype=BF, device=DEV)
    ops.dora_delta(Wv, lwv, mag.to(DEV), scaling, deltav, s_buf, n_buf)
    ops.dora_bwd(ddv, Wv, lwv, scaling, s_buf, n_buf, t1v, dmag_m[1:rows + 1])
    sd, nd = s_buf.cpu(), n_buf.cpu()
    assert ((nd - n.float()).abs() <= 2.0 ** -7 * n.float()).all()
    assert ((sd - s.float()).abs() <= 2.0 ** -6 * s.float()).all()
    assert torch.equal(sn[:, [0, rows + 1]].view(torch.int32), torch.full_like(sn[:, [0, rows + 1]], NAN).view(torch.int32))
    d2 = sd[:, None] * (W.float() + scaling * lw.float()) - W.float()
    assert torch.equal(deltav.cpu(), d2.to(BF))
    assert only_view_changed(dm, dbefore, slice(0, rows), dcs)
    sc = (sd * scaling).to(BF)
    assert torch.equal(t1v.cpu(), (sc[:, None].float() * dd.float()).to(BF))
    assert only_view_changed(tm, tbefore, slice(0, rows), tcs)
    q = (dd.double() * u.double()).sum(1) / nd.double()
    dmag = dmag_m.cpu()
    print(f"[parity] dora cols={cols}: dmag / (exact_sum / n) - 1 = {((dmag[1:-1].double() - q) / q.abs().clamp_min(1e-30)).tolist()}")
    assert ((dmag[1:-1].double() - q).abs() <= 2.0 ** -7 * q.abs()).all()
    assert keeps(dmag_m[:1], NAN) and keeps(dmag_m[-1:], NAN)
