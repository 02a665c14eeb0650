"""The GLU depthwise convolution (csrc/dwconv_glu.hip, csrc/dwconv_tile.hpp) held to exact sums: the case table, a replica of
the launchers' arithmetic, the input builder, the fp64 model, the checker and a plain-torch executor with planted errors.
Shared by test_dwconv_ref_cpu.py (no GPU, no yat_amd) and test_dwconv_gpu.py.

Why exact.  The kernels' arithmetic is fp32 multiply-adds over bf16 data.  build() draws inputs for which every sum any kernel
forms is a sum of integers whose absolute values total less than 2^24, so it is exact in fp32 in any order, and every stored
bf16 is an integer of at most 8 significant bits or one round-to-nearest-even of an exact integer.  The comparison is therefore
torch.equal (after + 0.0, so that -0 equals +0): a dropped tap, halo row, column or channel changes the answer.
  s (forward, pass 1)  integers in [-2, 2]
  wdw[c]               a random permutation of {-4, -3, -2, -1, 1, 2, 3, 4, 5}: nine distinct taps, sum |w| = 25, |conv| <= 50
  bdw, `a` half        integers in [-8, 8];  so |ua| <= 58
  bdw, `g` half        per channel G_LIVE = +96 or G_DEAD = -180: ug in [46, 146] (sigmoid exactly 1: SiLU(ug) = ug, SiLU' = 1)
                       or in [-230, -130] (sigmoid exactly 0: SiLU = +-0, SiLU' = +-0)
  z (pass 2)           per element an integer in Z_LIVE = [32, 47] (s = z, SiLU' = 1) or Z_DEAD = [-128, -105] (s = SiLU' = +-0)
  dy                   {-1, 0, 1};  du of the du= entry: integers in [-2, 2];  previous contents for accumulate: [-8, 8]
Both conditions are asserted, not assumed: model() returns the largest sum of |terms| of every reduced output (bounds, < 2^24),
and the GPU file asserts that the library's own SiLU returns exactly z / +-0 on the four ranges above.

plan(B, h, w, Hc) mirrors launch_stream, pick_band_rows, bands_per_wg, launch_tile, launch_tile_best, pick_band_rows_bwd2,
launch_bwd2 and the gs_shape rule of yat_dwconv_glu_bwd line for line (product build: every YAT_TUNE_INT is its default).
"""
import types

import torch

BF = torch.bfloat16
SEG, SSEG, PK, TILE_PAD, ROWS = 8, 4, 11, 9, 4
GUARD_BITS = 0x4B4B               # bf16 13303808: finite, and twice what any output of a new case can hold (6.6e6)
G_LIVE, G_DEAD = 96, -180
Z_LIVE, Z_DEAD = (32, 47), (-128, -105)
EXACT_LIMIT = 2 ** 24


# ------------------------------------------------------------------------------------------------ the launch plan
def tile_slots(rows, WP):
    return (rows * WP + 1 + TILE_PAD + 15) & ~15


def lds_budget(WPS):
    return 159744 // WPS


def bands_per_wg(nbands, wgs_per_band_group, min_wgs):
    bpb = nbands
    while bpb > 1 and (nbands + bpb - 1) // bpb * wgs_per_band_group < min_wgs:
        bpb -= 1
    return bpb


def pick_band_rows(TCH, WPS, h, w):
    nseg, ns = (w + SEG - 1) // SEG, 256 // (TCH // 4)
    best, best_score, lds = 0, 0.0, 0
    R = 2
    while R <= 16 and R <= ((h + 1) & ~1):
        nbytes = 2 * tile_slots(R + 2, w + 1) * TCH * 2
        if nbytes > lds_budget(WPS):
            break
        nruns = R * nseg
        passes = (nruns + ns - 1) // ns
        nb = (h + R - 1) // R
        score = nruns / (passes * ns) * R / (R + 2) * h / (nb * R)
        if score > best_score:
            best_score, best, lds = score, R, nbytes
        R += 1
    return best, lds


def pick_band_rows_bwd2(TCH, z_in_lds, h, w):
    NCG = TCH // 4
    ns = 256 // NCG
    cap = 65536 if z_in_lds else lds_budget(2)
    nseg, WP = (w + SEG - 1) // SEG, w + 1
    best, best_score, lds = 0, 0.0, 0
    R = 4
    while R <= 16 and R <= ((h + 1) & ~1):
        nbytes = (tile_slots(R + 2, WP) + (tile_slots(R, WP) if z_in_lds else 0)) * TCH * 2
        nbytes = max(nbytes, ns * NCG * 4 * PK * 4)
        if nbytes > cap:
            break
        nruns = R * nseg
        passes = (nruns + ns - 1) // ns
        nb = (h + R - 1) // R
        score = nruns / (passes * ns) * (3.0 * R / (3.0 * R + 2.0)) * h / (nb * R)
        if score > best_score:
            best_score, best, lds = score, R, nbytes
        R += 1
    return best, lds


def _bands(kernel, TCH, R, h, channels, B, min_wgs, lds):
    nbands, nchunk = (h + R - 1) // R, (channels + TCH - 1) // TCH
    bpb = bands_per_wg(nbands, nchunk * B, min_wgs)
    return dict(kernel=kernel, TCH=TCH, R=R, nbands=nbands, bpb=bpb, ngrp=(nbands + bpb - 1) // bpb, nchunk=nchunk,
                last_band_rows=h - (nbands - 1) * R, tail=channels % TCH, lds=lds)


def launch_tile(TCH, WPS, B, h, w, Hc):
    R, lds = pick_band_rows(TCH, WPS, h, w)
    if not R or (Hc & 7) or B * h * w * 2 * Hc * 2 > 0x7fffffff:
        return None
    return _bands(f"tile{TCH}x{WPS}", TCH, R, h, Hc, B, 3 * 256 * WPS, lds)


def launch_stream(B, h, w, Hc, TCH=64, WPS=3):
    nseg, ns = (w + SSEG - 1) // SSEG, 256 // (TCH // 4)
    R = ns // nseg
    if R < 1 or R > 8 or R * nseg * 8 < ns * 7 or (Hc & 7) or B * h * w * 2 * Hc * 2 > 0x7fffffff:
        return None
    lds = 2 * tile_slots(2 * R + 2, w + 1) * TCH * 2
    if lds > lds_budget(WPS):
        return None
    nchunk = (Hc + TCH - 1) // TCH
    rpg = ((h + R - 1) // R) * R
    while rpg > R and (h + rpg - 1) // rpg * nchunk * B < 600:
        rpg -= R
    ngrp = (h + rpg - 1) // rpg
    rows = [min(h, (g + 1) * rpg) - g * rpg for g in range(ngrp)]
    return dict(kernel="stream", TCH=TCH, R=R, rpg=rpg, ngrp=ngrp, nchunk=nchunk, nseg=nseg, idle=ns - R * nseg,
                steps=tuple((r + R - 1) // R for r in rows), ragged=tuple(r % R != 0 for r in rows), tail=Hc % TCH, lds=lds)


def launch_bwd2(TCH, z_in_lds, B, h, w, Hc):
    C2 = 2 * Hc
    ok = w <= 64 and not (C2 & 7) and B * h * w * C2 * 2 <= 0x7fffffff
    R, lds = pick_band_rows_bwd2(TCH, z_in_lds, h, w) if ok else (0, 0)
    if not R:
        return None
    return _bands("bwd2_lds32" if z_in_lds else "bwd2_gz64", TCH, R, h, C2, B, 4 * 512, lds)


def plan(B, h, w, Hc):
    """-> {"fwd", "pass1", "pass2"}: the kernel each entry point launches for the shape, and its geometry"""
    fwd = p1 = None
    if w <= 64:
        fwd = launch_stream(B, h, w, Hc)
        if fwd is None and w > 48:
            fwd = launch_tile(64, 2, B, h, w, Hc)
        if fwd is None:
            fwd = launch_tile(64, 3, B, h, w, Hc)
        if fwd is None:
            fwd = launch_tile(32, 3, B, h, w, Hc)
        p1 = launch_tile(32, 3, B, h, w, Hc)
    direct = dict(kernel="direct", nx=(Hc // 4 + 255) // 256, nseg=(w + SEG - 1) // SEG, tail=Hc % 8)
    fwd, p1 = fwd or dict(direct), p1 or dict(direct)
    p2 = None
    if (24 < w <= 32) or w < 16:
        p2 = launch_bwd2(64, False, B, h, w, Hc)
    if p2 is None and B * h * w * 2 * Hc * 2 <= 0x7fffffff:
        p2 = launch_bwd2(32, True, B, h, w, Hc)
    if p2 is None:
        p2 = dict(kernel="direct", nrg=(h + ROWS - 1) // ROWS, nsb=(w + 4 * SEG - 1) // (4 * SEG),
                  nx2=(2 * Hc // 4 + 63) // 64, last_group_rows=h - ((h + ROWS - 1) // ROWS - 1) * ROWS)
    return dict(fwd=fwd, pass1=p1, pass2=p2)


# ------------------------------------------------------------------------------------------------ the case table
class Case(types.SimpleNamespace):
    @property
    def name(self):
        return f"{self.B}x{self.h}x{self.w}x{self.Hc}"

    @property
    def dims(self):
        return self.B, self.h, self.w, self.Hc


def _c(B, h, w, Hc, group, **want):
    return Case(B=B, h=h, w=w, Hc=Hc, group=group, want=want)


def _st(R, rpg, steps, idle, tail):
    return dict(kernel="stream", R=R, rpg=rpg, ngrp=len(steps), steps=steps, idle=idle, tail=tail)


def _bd(kernel, R, nbands, bpb, ngrp, last=1):
    return dict(kernel=kernel, R=R, nbands=nbands, bpb=bpb, ngrp=ngrp, last_band_rows=last)


# what test_dwconv_glu_fwd_bwd of test_kernels_gpu.py runs (its last two shapes, 40 MB and 59 MB with up to 2754 pixels,
# are not taken into the exact table: see OLD_LARGE)
OLD_SMALL = [(2, 4, 4, 16), (2, 5, 9, 40), (1, 16, 64, 160), (2, 33, 3, 8), (2, 32, 32, 72), (1, 3, 70, 8), (1, 6, 5, 12),
             (1, 7, 20, 40), (2, 9, 16, 64), (1, 10, 8, 24), (3, 31, 30, 136)]
OLD_LARGE = [(9, 34, 4, 8192), (8, 9, 50, 4096)]

TABLE = [
    # the streaming forward walks three steps in each of three groups that start mid-image; the last group is one step shorter
    # and ends on a ragged step; nchunk * B = 200
    _c(2, 15, 32, 6400, "stream3", fwd=_st(2, 6, (3, 3, 2), 0, 0)),
    _c(2, 15, 27, 6392, "stream3", fwd=_st(2, 6, (3, 3, 2), 2, 56)),
    _c(2, 22, 20, 6400, "stream3", fwd=_st(3, 9, (3, 3, 2), 1, 0)),
    _c(2, 22, 17, 6392, "stream3", fwd=_st(3, 9, (3, 3, 2), 1, 56)),
    _c(2, 29, 13, 6400, "stream3", fwd=_st(4, 12, (3, 3, 2), 0, 0)),
    _c(2, 36, 9, 6392, "stream3", fwd=_st(5, 15, (3, 3, 2), 1, 56)),
    _c(2, 57, 5, 6400, "stream3", fwd=_st(8, 24, (3, 3, 2), 0, 0)),
    # one group walks the whole image (nchunk * B = 600): zero halos at both ends, a ragged last step
    _c(3, 7, 20, 12800, "stream1", fwd=_st(3, 9, (3,), 1, 0)),
    _c(3, 11, 12, 12800, "stream1", fwd=_st(5, 15, (3,), 1, 0)),
    _c(3, 7, 32, 12800, "stream1", fwd=_st(2, 8, (4,), 0, 0)),                      # the ring index wraps twice
    # band kernels: bpb >= 2, at least two groups per image, a one-row last band, nbands % bpb != 0
    _c(2, 33, 3, 18432, "band", pass1=_bd("tile32x3", 16, 3, 2, 2), pass2=_bd("bwd2_gz64", 16, 3, 2, 2)),
    _c(1, 21, 20, 16384, "band", pass2=_bd("bwd2_lds32", 10, 3, 2, 2)),
    _c(3, 65, 3, 16384, "band", fwd=_bd("tile64x3", 16, 5, 2, 3), pass1=_bd("tile32x3", 16, 5, 4, 2),
       pass2=_bd("bwd2_gz64", 16, 5, 4, 2)),
    _c(3, 5, 49, 16384, "band", fwd=_bd("tile64x2", 2, 3, 2, 2)),
    # direct kernels: w > 64 and Hc % 8 != 0, nx = 2 with the channel tail in the second 256-group block; pass 2 with a ragged
    # last row group (6 = 4 + 2) and a ragged last 32-column block
    _c(2, 6, 70, 1028, "direct", fwd=dict(kernel="direct", nx=2, nseg=9, tail=4), pass1=dict(kernel="direct", nx=2),
       pass2=dict(kernel="direct", nrg=2, nsb=3, last_group_rows=2)),
] + [_c(*s, "old") for s in OLD_SMALL]

STREAM_MULTI = [c for c in TABLE if c.group in ("stream3", "stream1")]


def reduced_channels(Hc):
    """a channel count of at most 128 with the same Hc % 64 (and so the same Hc % 8 and channel tail) for the CPU executor"""
    if Hc <= 128:
        return Hc
    return 64 + Hc % 64 if Hc % 64 else 128


# ------------------------------------------------------------------------------------------------ inputs
def build(dims, device="cpu", seed=0):
    """-> namespace of bf16 tensors for dims = (B, h, w, Hc), drawn from a seeded generator on `device`"""
    B, h, w, Hc = dims
    M, C2 = B * h * w, 2 * Hc
    g = torch.Generator(device=device).manual_seed(1000 * seed + 7 * h + w)

    def ri(lo, hi, *shape):                                   # integers in [lo, hi]
        return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()

    taps = torch.tensor([-4., -3., -2., -1., 1., 2., 3., 4., 5.], device=device)
    wdw = taps[torch.rand(C2, 9, generator=g, device=device).argsort(1)]
    bg = torch.where(torch.randperm(Hc, generator=g, device=device) % 2 == 0, float(G_LIVE), float(G_DEAD))   # half of each
    z = torch.where(ri(0, 1, M, C2) > 0, ri(*Z_LIVE, M, C2), ri(*Z_DEAD, M, C2))
    t = dict(s=ri(-2, 2, M, C2), z=z, wdw=wdw, bdw=torch.cat([ri(-8, 8, Hc), bg]), dy=ri(-1, 1, M, Hc), du=ri(-2, 2, M, C2),
             prev_dw=ri(-8, 8, C2, 9), prev_db=ri(-8, 8, C2), prev_dzs=ri(-8, 8, C2))
    return types.SimpleNamespace(**{k: v.to(BF) for k, v in t.items()})


# ------------------------------------------------------------------------------------------------ the fp64 model
def rb(x):
    return x.to(BF).to(torch.float64)


def step_sigmoid(x):
    """what sigmoid_f returns on the live and dead ranges: exactly 1 or exactly 0"""
    return (x > 0).to(x.dtype)


def _pad(x, B, h, w):
    """[M, C] -> [B, h + 2, w + 2, C] in fp64 with a zero border"""
    p = torch.zeros(B, h + 2, w + 2, x.shape[-1], dtype=torch.float64, device=x.device)
    p[:, 1:h + 1, 1:w + 1] = x.view(B, h, w, -1).double()
    return p


def model_fwd(dims, s, wdw, bdw, sigmoid=step_sigmoid):
    """u = bf16(conv3x3(s) + b), y = bf16(ua * bf16(SiLU(ug))): nine shifted slices of the zero-padded image times the tap.
    -> u, y (fp64 holding bf16 values), y before its rounding, the largest sum of |terms| of one u"""
    B, h, w, Hc = dims
    sp, wt = _pad(s, B, h, w), wdw.double()
    u = bdw.double().expand(B, h, w, -1).clone()
    mag = bdw.double().abs().expand(B, h, w, -1).clone()
    for a in range(3):
        for b_ in range(3):
            term = sp[:, a:a + h, b_:b_ + w] * wt[:, a * 3 + b_]
            u += term
            mag += term.abs()
    u = rb(u.reshape(B * h * w, 2 * Hc))
    ua, ug = u[:, :Hc], u[:, Hc:]
    y_exact = ua * rb(ug * sigmoid(ug))
    return u, rb(y_exact), y_exact, mag.max().item()


def model_pass1(u, dy, Hc, sigmoid=step_sigmoid):
    """du_a = bf16(dy * bf16(SiLU(ug))), du_g = bf16(bf16(dy * ua) * SiLU'(ug))"""
    ua, ug, d = u[:, :Hc], u[:, Hc:], dy.double()
    sg = sigmoid(ug)
    return rb(torch.cat([d * rb(ug * sg), rb(d * ua) * (sg * (1.0 + ug * (1.0 - sg)))], 1))


def model_pass2(dims, z, du, wdw, sigmoid=step_sigmoid):
    """dz = bf16(SiLU'(z) * bf16(sum_taps W[tap] du[i - di, j - dj])); the three reductions before their rounding:
    dW[tap] = sum s[i, j] du[i - di, j - dj] with s = bf16(z sigmoid(z)), db = sum du, dz_colsum = sum dz (the stored values).
    -> dz, sums {dw, db, dzs}, dz before its last rounding, bounds {name: largest sum of |terms| over the output's elements}"""
    B, h, w, _ = dims
    dp, wt, zz = _pad(du, B, h, w), wdw.double(), z.double().view(B, h, w, -1)
    sg = sigmoid(zz)
    s = rb(zz * sg)
    acc, mag = torch.zeros_like(zz), torch.zeros_like(zz)
    dw, dw_mag = [], []
    for a in range(3):
        for b_ in range(3):
            sl = dp[:, 2 - a:2 - a + h, 2 - b_:2 - b_ + w]      # du[i + 1 - a, j + 1 - b_]
            acc += sl * wt[:, a * 3 + b_]
            mag += (sl * wt[:, a * 3 + b_]).abs()
            dw.append((s * sl).sum((0, 1, 2)))
            dw_mag.append((s * sl).abs().sum((0, 1, 2)))
    dz_exact = rb(acc) * (sg * (1.0 + zz * (1.0 - sg)))
    dz = rb(dz_exact)
    dud = du.double()
    sums = dict(dw=torch.stack(dw, 1), db=dud.sum(0), dzs=dz.sum((0, 1, 2)))
    bounds = dict(dz=mag.max().item(), dw=torch.stack(dw_mag, 1).max().item(), db=dud.abs().sum(0).max().item(),
                  dzs=dz.abs().sum((0, 1, 2)).max().item())
    return dz.reshape(B * h * w, -1), sums, dz_exact.reshape(B * h * w, -1), bounds


def model_reduce(total, prev=None):
    """dwconv_reduce_kernel / reduce_partials_bf16_kernel: bf16(sum), or bf16(bf16(sum) + previous) with accumulate"""
    return rb(total) if prev is None else rb(rb(total) + prev.double())


def model(dims, inp):
    """everything the GPU file compares, for one built case"""
    Hc = dims[3]
    m = types.SimpleNamespace()
    m.u, m.y, m.y_exact, u_mag = model_fwd(dims, inp.s, inp.wdw, inp.bdw)
    m.du1 = model_pass1(m.u, inp.dy, Hc)
    m.dz1, m.sums1, m.dz1_exact, b1 = model_pass2(dims, inp.z, m.du1, inp.wdw)
    m.dz2, m.sums2, m.dz2_exact, b2 = model_pass2(dims, inp.z, inp.du, inp.wdw)
    m.bounds = dict(u=u_mag, **{k + "_dy": v for k, v in b1.items()}, **{k + "_du": v for k, v in b2.items()})
    prev = dict(dw=inp.prev_dw, db=inp.prev_db, dzs=inp.prev_dzs)
    m.dw1, m.db1 = model_reduce(m.sums1["dw"]), model_reduce(m.sums1["db"])
    m.plain = {k: model_reduce(v) for k, v in m.sums2.items()}
    m.accum = {k: model_reduce(v, prev[k]) for k, v in m.sums2.items()}
    return m


# ------------------------------------------------------------------------------------------------ windows and the checker
class Win:
    """an output as a window inside a larger buffer: at least `guard` elements of GUARD_BITS on both sides (rounded up to
    256 bytes, the alignment of an allocation of its own); the window starts as GUARD_BITS too, or as `prev`"""

    def __init__(self, shape, guard, device, prev=None):
        n = 1
        for d in shape:
            n *= d
        g = -(-guard // 128) * 128
        self.buf = torch.full((2 * g + n,), GUARD_BITS, dtype=torch.int16, device=device).view(BF)
        self.off, self.n, self.shape = g, n, tuple(shape)
        if prev is not None:
            self.view.copy_(prev)

    @property
    def view(self):
        return self.buf[self.off:self.off + self.n].view(self.shape)

    def guards_intact(self):
        bits = self.buf.view(torch.int16)
        return bool((bits[:self.off] == GUARD_BITS).all()) and bool((bits[self.off + self.n:] == GUARD_BITS).all())


def windows(dims, device, names=("y", "u", "dz", "dw", "db", "dzs"), prev=None):
    """the named outputs as guarded windows; the guard is one image row of 2 Hc channels"""
    B, h, w, Hc = dims
    M, C2 = B * h * w, 2 * Hc
    prev = prev or {}
    shapes = dict(y=(M, Hc), u=(M, C2), dz=(M, C2), dw=(C2, 9), db=(C2,), dzs=(C2,))
    return {k: Win(shapes[k], w * C2, device, prev.get(k)) for k in names}


def first_diff(got, want, dims, cols):
    """(b, i, j, c) of the first element that differs, for an [M, cols] output; the flat index otherwise"""
    bad = ((got + 0.0) != (want + 0.0)).reshape(-1).nonzero()
    k = int(bad[0])
    if got.dim() == 2 and got.shape[0] == dims[0] * dims[1] * dims[2]:
        pix, c = divmod(k, cols)
        b, r = divmod(pix, dims[1] * dims[2])
        return (b, *divmod(r, dims[2]), c)
    return k


def check(dims, name, got, want):
    """-> list of failures: the window `got` (a Win or a tensor) equals the model bit for bit up to the sign of zero, and the
    guards around it are untouched"""
    fails = []
    v = got.view if isinstance(got, Win) else got
    a, b = v.double() + 0.0, want.double().reshape(v.shape) + 0.0
    if not torch.equal(a, b):
        n = int((a != b).sum())
        at = first_diff(a, b, dims, v.shape[-1])
        fails.append(f"{name}: {n} of {a.numel()} elements differ from the model, first at {at}: "
                     f"{a.reshape(-1)[(a != b).reshape(-1)][0].item()} for {b.reshape(-1)[(a != b).reshape(-1)][0].item()}")
    if isinstance(got, Win) and not got.guards_intact():
        fails.append(f"{name}: guard overwritten")
    return fails


# ------------------------------------------------------------------------------------------------ the CPU executor
# Plain torch in fp32, addressing memory the way the kernels do: (image, channel chunk, band group) workgroups, bands staged
# into a tile with zero rows outside the image, the streaming forward's ring of 2R + 2 rows with its prefetch one step ahead,
# SEG- / SSEG-column runs, fp32 partial rows summed by the reduce kernel.  `fault` plants one error.
FAULTS = ("halo_bottom_zero", "ring_slot_stale", "below_image_stale", "skip_ragged_step", "drop_left_col", "swap_taps",
          "skip_channel_tail", "g_bias_from_a", "dw_miss_last_band", "accumulate_overwrites", "store_past_end")
# the calls a fault can change: f = forward, 1 = backward with dy (pass 1 + pass 2), 2 = backward through du=, a = accumulate
FAULT_CALLS = dict(halo_bottom_zero="f12", ring_slot_stale="f", below_image_stale="f", skip_ragged_step="f", drop_left_col="f12",
                   swap_taps="f12", skip_channel_tail="f12", g_bias_from_a="f1", dw_miss_last_band="2", accumulate_overwrites="a",
                   store_past_end="f2")


def _r32(x):
    return x.to(BF).float()


def _sig(x):
    return (x > 0).float()


def _dsilu(x):
    sg = _sig(x)
    return sg * (1.0 + x * (1.0 - sg))


def _taps(wdw, fault):
    wt = wdw.float()
    return wt[:, [1, 0, 2, 3, 4, 5, 6, 7, 8]] if fault == "swap_taps" else wt


def _fwd_run(rows, wt, bias, j0, n, dead_first):
    """u of output columns [j0, j0 + n) from three tile rows [w + 2, C] (a zero column on either side)"""
    acc = bias.expand(n, -1).clone()
    for r in range(3):
        x = rows[r][j0:j0 + n + 2]                            # input columns j0 - 1 .. j0 + n
        if dead_first:
            x = x.clone()
            x[0] = 0
        for dj in range(3):
            acc += wt[:, r * 3 + dj] * x[dj:dj + n]
    return acc


def _fwd_store(mode, acc, na, pix, Hc, ca, dy, out, u_out):
    """the GLU (forward) or its backward (pass 1) of one run, stored at pixels [pix, pix + n)"""
    n = acc.shape[0]
    ua, ug = _r32(acc[:, :na]), _r32(acc[:, na:])
    silu = _r32(ug * _sig(ug))
    if mode == 0:
        if u_out is not None:
            u_out[pix:pix + n, ca] = ua.to(BF)
            u_out[pix:pix + n, Hc + ca] = ug.to(BF)
        out[pix:pix + n, ca] = (ua * silu).to(BF)
    else:
        d = dy[pix:pix + n, ca].float()
        out[pix:pix + n, ca] = (d * silu).to(BF)
        out[pix:pix + n, Hc + ca] = (_r32(d * ua) * _dsilu(ug)).to(BF)


def _stage_row(dst, src, b, ii, h, idx):
    """one tile row: image row ii of channels idx, zeros when the row lies outside the image"""
    dst.zero_()
    if 0 <= ii < h:
        dst[1:-1] = src[b, ii][:, idx]


def _exec_fwd(mode, geo, dims, s, wdw, bdw, dy, out, u_out, fault):
    """forward (mode 0) or pass 1 (mode 1) with the kernel plan() names; out / u_out are [M, .] views"""
    B, h, w, Hc = dims
    C2 = 2 * Hc
    s4, wt, bias = s.float().view(B, h, w, C2), _taps(wdw, fault), bdw.float()
    kernel = geo["kernel"]
    if kernel == "direct":                                    # one thread per (image, row, SEG columns, 4 channels)
        chunks, seg_w = [torch.arange(Hc)], SEG
    else:
        TCH = geo["TCH"]
        chunks = [torch.arange(c0, min(Hc, c0 + TCH)) for c0 in range(0, Hc, TCH)]
        seg_w = SSEG if kernel == "stream" else SEG
    R = geo.get("R", 1)
    for b in range(B):
        for ca in chunks:
            if fault == "skip_channel_tail" and kernel != "direct" and len(ca) < geo["TCH"]:
                continue
            na, idx = len(ca), torch.cat([ca, Hc + ca])
            wsel = wt[idx]
            bsel = torch.cat([bias[ca], bias[ca] if fault == "g_bias_from_a" else bias[Hc + ca]])

            def run_row(i, rows):
                for j0 in range(0, w, seg_w):
                    n = min(seg_w, w - j0)
                    acc = _fwd_run(rows, wsel, bsel, j0, n, fault == "drop_left_col" and j0 > 0)
                    _fwd_store(mode, acc, na, (b * h + i) * w + j0, Hc, ca, dy, out, u_out)

            if kernel == "direct":
                tile = torch.zeros(3, w + 2, 2 * na)
                for i in range(h):
                    for r in range(3):
                        _stage_row(tile[r], s4, b, i - 1 + r, h, idx)
                    run_row(i, tile)
            elif kernel == "stream":
                RING, rpg = 2 * R + 2, geo["rpg"]
                for bg in range(geo["ngrp"]):
                    ring = torch.zeros(RING, w + 2, 2 * na)      # cleared once per workgroup
                    r_lo, r_hi = bg * rpg, min(h, bg * rpg + rpg)

                    def stage(ii0, nrows, prefetch_of):
                        for r in range(nrows):
                            ii = ii0 + r
                            if fault == "ring_slot_stale" and prefetch_of >= 1 and r == 0:
                                continue
                            if fault == "below_image_stale" and prefetch_of >= 0 and ii >= h:
                                continue
                            _stage_row(ring[(ii + 1) % RING], s4, b, ii, h, idx)
                            if fault == "halo_bottom_zero" and ii == r_hi and ii < h:
                                ring[(ii + 1) % RING].zero_()

                    nsteps = (r_hi - r_lo) // R if fault == "skip_ragged_step" else (r_hi - r_lo + R - 1) // R
                    stage(r_lo - 1, R + 2, -1)
                    for st in range(nsteps):
                        i0 = r_lo + st * R
                        if st + 1 < nsteps:
                            stage(i0 + R + 1, R, st)
                        for row in range(R):
                            i = i0 + row
                            if i < r_hi:
                                run_row(i, [ring[(i + r) % RING] for r in range(3)])
            else:
                nbands, bpb = geo["nbands"], geo["bpb"]
                tile = torch.zeros(R + 2, w + 2, 2 * na)
                for bg in range(geo["ngrp"]):
                    for band in range(bg * bpb, min(nbands, (bg + 1) * bpb)):
                        i0 = band * R
                        for r in range(R + 2):
                            _stage_row(tile[r], s4, b, i0 - 1 + r, h, idx)
                        if fault == "halo_bottom_zero" and band != nbands - 1:
                            tile[R + 1].zero_()
                        for row in range(R):
                            if i0 + row < h:
                                run_row(i0 + row, tile[row:row + 3])


def _exec_pass2(geo, dims, z, du, wdw, dz, fault):
    """-> fp32 partial rows [P, 2Hc, PK] (PK = 9 taps, bias, column sum of dz; the direct kernel leaves the last at 0)"""
    B, h, w, Hc = dims
    C2 = 2 * Hc
    z4, d4, wt = z.float().view(B, h, w, C2), du.float().view(B, h, w, C2), _taps(wdw, fault)
    direct = geo["kernel"] == "direct"
    if direct:
        R, nbands, bpb, ngrp = ROWS, geo["nrg"], 1, geo["nrg"]
        chunks = [torch.arange(C2)]
    else:
        R, nbands, bpb, ngrp, TCH = geo["R"], geo["nbands"], geo["bpb"], geo["ngrp"], geo["TCH"]
        chunks = [torch.arange(c0, min(C2, c0 + TCH)) for c0 in range(0, C2, TCH)]
    ws = torch.zeros(B * ngrp, C2, PK)
    for b in range(B):
        for idx in chunks:
            if fault == "skip_channel_tail" and not direct and len(idx) < TCH:
                continue
            wsel = wt[idx]
            tile = torch.zeros(R + 2, w + 2, len(idx))
            for bg in range(ngrp):
                part = torch.zeros(len(idx), PK)
                for band in range(bg * bpb, min(nbands, (bg + 1) * bpb)):
                    i0 = band * R
                    for r in range(R + 2):
                        _stage_row(tile[r], d4, b, i0 - 1 + r, h, idx)
                    if fault == "halo_bottom_zero" and band != nbands - 1:
                        tile[R + 1].zero_()
                    for row in range(R):
                        i = i0 + row
                        if i >= h:
                            continue
                        zrow = z4[b, i][:, idx]
                        for j0 in range(0, w, SEG):
                            n = min(SEG, w - j0)
                            zz = zrow[j0:j0 + n]
                            S = _r32(zz * _sig(zz))
                            acc = torch.zeros(n, len(idx))
                            for r in range(3):
                                x = tile[row + r][j0:j0 + n + 2]          # du columns j0 - 1 .. j0 + n of image row i + r - 1
                                if fault == "drop_left_col" and j0 > 0:
                                    x = x.clone()
                                    x[0] = 0
                                for tc in range(3):
                                    t, sl = (2 - r) * 3 + tc, x[2 - tc:2 - tc + n]
                                    acc += wsel[:, t] * sl
                                    if not (fault == "dw_miss_last_band" and band == nbands - 1):
                                        part[:, t] += (S * sl).sum(0)
                            part[:, 9] += tile[row + 1][j0 + 1:j0 + 1 + n].sum(0)
                            v = (_r32(acc) * _dsilu(zz)).to(BF)
                            pix = (b * h + i) * w + j0
                            dz[pix:pix + n, idx] = v
                            if not direct:
                                part[:, 10] += v.float().sum(0)
                ws[b * ngrp + bg, idx] = part
    return ws


def _reduce(ws, dw, db, dzs, accumulate, fault):
    total = ws.sum(0)                                         # [C2, PK]
    add = accumulate and fault != "accumulate_overwrites"
    for dst, val in ((dw, total[:, :9]), (db, total[:, 9]), (dzs, total[:, 10])):
        if dst is not None:
            dst.copy_((_r32(val) + dst.float() if add else val).to(BF))


def _past_end(win, last_pixel):
    """the planted store one pixel past the image end: the last pixel's values again, behind the window"""
    cols = win.shape[-1]
    win.buf[win.off + win.n:win.off + win.n + cols] = last_pixel


def cpu_fwd(geo, dims, inp, y, u_out=None, fault=None):
    """what ops.dwconv_glu_fwd does; y, u_out are Win"""
    _exec_fwd(0, geo["fwd"], dims, inp.s, inp.wdw, inp.bdw, None, y.view, None if u_out is None else u_out.view, fault)
    if fault == "store_past_end":
        _past_end(y, y.view[-1])


def cpu_bwd(geo, dims, inp, dz, dw, db, du_ws, accumulate=False, dzs=None, du=None, fault=None):
    """what ops.dwconv_glu_bwd does; dz, dw, db, dzs are Win, du_ws the [M, 2Hc] head of the workspace"""
    if du is None:
        _exec_fwd(1, geo["pass1"], dims, inp.s, inp.wdw, inp.bdw, inp.dy, du_ws, None, fault)
        du = du_ws
    ws = _exec_pass2(geo["pass2"], dims, inp.z, du, inp.wdw, dz.view, fault)
    tiled = geo["pass2"]["kernel"] != "direct"
    _reduce(ws, dw.view, db.view, dzs.view if dzs is not None and tiled else None, accumulate, fault)
    if dzs is not None and not tiled:                         # the direct path: a column sum over the stored dz
        col = torch.zeros(1, dz.shape[1], PK)
        col[0, :, 10] = dz.view.float().sum(0)
        _reduce(col, None, None, dzs.view, accumulate, fault)
    if fault == "store_past_end":
        _past_end(dz, dz.view[-1])
