"""Plain references, exact inputs and case lists for the VAE kernels: the shared 3x3 implicit-GEMM conv (csrc/dcae_conv.hpp
with its four entry points in dcae.hip, dcae_enc.hip and vae_kl_enc.hip, and the direct kernel for Cout <= 4),
yat_vae_groupnorm (vae_kl.hip) and yat_dcae_msla_aggregate (dcae.hip).  No GPU code is imported here:
test_vae_kernels_ref_cpu.py proves on the CPU what test_vae_kernels_exact_gpu.py relies on, and the GPU file compares the
kernels with what this file computes -- never with another run of a kernel.

The expectations are computed the plain way (``*_expect``): torch.nn.functional.conv2d / interpolate / pixel_shuffle /
pixel_unshuffle / group_norm in fp64 on the CPU, with one bf16 rounding at each point include/yat_hip.h states.  Inputs are
chosen so that the expected bits need neither device arithmetic nor an order:
  * conv: x dense in {-1, 0, 1}, w = +-1 at one seeded position of every 16-byte chunk (8 channels) of every tap of every
    output channel: every product and partial sum is a small integer, every chunk of K matters to every output;
  * one g = 3 case (``thirds``) has zero weights and group sums of 24 significant bits chosen so that the fp32 quotient
    a / 3 and the product a * (1 / 3) round to different bf16 numbers (small sums cannot tell the two apart);
  * SiLU sees the saturated integers of glue_ref.saturated only ([32, 255] and [-255, -128]: exactly x or -0), moved there
    by a per-channel bias of +128 / -192;
  * the rounding-chain cases (``chain``) put the value before each epilogue rounding on or next to a tie between two bf16
    numbers (bias 254 / 256 / 258; the encoder and KL chains also widen x to [-200, 200] so that the conv sum and the group
    mean are no bf16 numbers): dropping or adding one rounding moves stored bits;
  * GroupNorm (eps = 0): per (image, group) a population of deviations +-a and +-7a in the ratio 15 : 15 : 1 : 1, filled up
    with pairs +-2a and, for an odd count, one block (3a, -3a, a, -a, 0): mean exact, variance exactly 4 a^2, rstd = 1 / (2a),
    xhat a multiple of 1/2.  The group's first value K is its minimum, so every shifted partial sum is positive.  Two
    cases (``tie``) put every output on a tie between two bf16 numbers (odd w, b >= 129): the bits then move with the last
    bit of a statistic, which a one-pixel slab out of 131 073 pixels would otherwise not reach;
  * MSLA: x in [-2, 2], depthwise weights in {-1, 0, 1}, pointwise weights +-1 at four positions of each row.
The ``*_exec`` functions are plain numpy executors that walk tiles, chunks and slabs as the kernels do and can carry one
planted error (FAULTS); the ``*_classes`` functions derive from a case alone which dispatch classes it reaches.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as Fn

from tests.glue_ref import CANARY, F32, _rbf_np, as_i16, bf_bits, fold  # noqa: F401  (re-exported for the two test files)

BF = torch.bfloat16
LEAD, TAIL = 16, 24                  # canary elements before (a multiple of 8: 16-byte alignment stays) and behind an output
WS_CANARY = 0x7FC12345               # fp32 NaN bits the GroupNorm workspace starts as
BM, BN, BK = 128, 128, 64            # the conv tile
GN_SLAB = 512


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def rb64(t):
    """fp64 tensor -> rounded to bf16 (through fp32, which holds every value here exactly), back in fp64"""
    return t.float().to(BF).double()


def out_buffer(n):
    """the int16 bits of an output buffer before the launch: LEAD + n + TAIL canaries"""
    return torch.full((LEAD + n + TAIL,), CANARY, dtype=torch.int16)


def want_buffer(bits):
    """expected bits of the whole buffer: canaries around ``bits`` (int16, any shape), -0 folded"""
    w = out_buffer(bits.numel())
    w[LEAD:LEAD + bits.numel()] = fold(bits.reshape(-1))
    return w


def mismatches(what, got, want):
    """whole-buffer comparison on bits (int16 CPU tensors), -0 folded -> [] or one line that names the first bad index and
    both bit patterns"""
    got, want = fold(got.reshape(-1)), want.reshape(-1)
    if got.shape != want.shape:
        return [f"{what}: {got.numel()} elements, expected {want.numel()}"]
    if torch.equal(got, want):
        return []
    bad = (got != want).nonzero().reshape(-1)
    i = int(bad[0])
    where = "before the output" if i < LEAD else ("behind the output" if i >= want.numel() - TAIL else f"element {i - LEAD}")
    return [f"{what}: {bad.numel()} elements differ, first at {where}: bits {got[i].item() & 0xffff:#06x}, "
            f"expected {want[i].item() & 0xffff:#06x}"]


def to_bits(v):
    """fp64 tensor of values fp32 holds exactly -> bf16 bits (int16)"""
    return bf_bits(v.float().to(BF))


# ------------------------------------------------------------------------------------------------ conv: cases
KINDS = ("dec", "mean", "down", "kl")                     # (S, P): dec and mean (1, 1), down (2, 1), kl (2, 0)
STRIDE = dict(dec=1, mean=1, down=2, kl=2, direct=1)


def _c(name, kind, B, Ho, Wo, Cin, Cout, **kw):
    d = dict(name=name, kind=kind, B=B, Ho=Ho, Wo=Wo, Cin=Cin, Cout=Cout, up=0, bias=None, silu=0, sc_mode=0, sc_rep=0,
             sc_own=0, res=0, nchw=0, shortcut=0, chain=0, thirds=0)
    d.update(kw)
    return d


# the tile geometry every entry point shares (B, Ho, Wo on the output side, Cin, Cout)
GEOM = [
    ("m35", 1, 5, 7, 8, 8),           # M < 128, one workgroup, odd x odd, K = 72: the second K tile is 7/8 past K
    ("m128", 1, 8, 16, 24, 124),      # M = 128, Cout 124
    ("m257", 1, 1, 257, 40, 260),     # M = 2 * 128 + 1, three N tiles: 9 workgroups; an output row of height 1
    ("wg8", 3, 9, 15, 72, 132),       # 4 x 2 = 8 workgroups, tiles straddle the three images, a second N tile of 4 columns
    ("wg11", 2, 2, 323, 64, 128),     # 11 workgroups, output height 2, one K tile per tap
    ("wg15", 1, 3, 171, 128, 260),    # 5 x 3 = 15 workgroups, M = 4 * 128 + 1, height 3, two K tiles per tap
    ("k1024", 1, 2, 3, 1024, 8),      # sixteen K tiles per tap
    ("w1", 2, 7, 1, 8, 8),            # output width 1
    ("one", 1, 1, 1, 8, 8),           # one output pixel: a 2 x 2 input at stride 2
    ("w2", 1, 5, 2, 24, 8),           # output width 2
    ("w3", 1, 3, 3, 40, 8),           # 3 x 3
]
_DEC_EPI = dict(m35={}, m128=dict(bias="small"), m257=dict(bias="sat", silu=1), wg8=dict(bias="small", sc_mode=1, sc_rep=1, sc_own=1),
                wg11=dict(sc_mode=1, sc_rep=32, sc_own=1), wg15=dict(bias="small", res=1), k1024=dict(bias="small"),
                w1=dict(res=1), one=dict(bias="small"), w2=dict(bias="sat", silu=1, res=1), w3=dict(sc_mode=1, sc_rep=2, sc_own=1))
_ENC_SC = {"down": {"m35": 1, "w1": 1, "one": 1, "wg11": 1}, "mean": {"m35": 1, "w1": 1, "one": 1}}      # g in {1, 2, 4} there


def _conv_cases():
    cs = []
    for kind in KINDS:
        for tag, B, Ho, Wo, Cin, Cout in GEOM:
            kw = {}
            if kind == "dec":
                kw = dict(_DEC_EPI[tag])
            elif kind in _ENC_SC:
                kw = dict(shortcut=_ENC_SC[kind].get(tag, 0), bias=None if tag in ("m35", "wg15") else "small")
            else:
                kw = dict(bias=None if tag in ("m35", "wg15") else "small")
            cs.append(_c(f"{kind}-{tag}", kind, B, Ho, Wo, Cin, Cout, **kw))
    # decoder: upsample and the pixel-shuffle shortcut
    cs += [
        _c("dec-up1x1", "dec", 1, 2, 2, 8, 8, up=1, sc_mode=2, sc_rep=4),                      # 1 x 1 stored input, shortcut = x
        _c("dec-up-sc2r1", "dec", 2, 6, 10, 24, 16, up=1, bias="small", sc_mode=2, sc_rep=1, sc_own=1),
        _c("dec-sc2r2", "dec", 1, 4, 6, 8, 8, sc_mode=2, sc_rep=2, sc_own=1),
        _c("dec-up-odd", "dec", 1, 6, 14, 40, 8, up=1),                                         # 3 x 7 stored
        _c("dec-all-sc2", "dec", 2, 6, 10, 24, 24, up=1, bias="sat", silu=1, sc_mode=2, sc_rep=4, res=1),
        _c("dec-all-sc1", "dec", 2, 5, 7, 128, 132, bias="sat", silu=1, sc_mode=1, sc_rep=2, sc_own=1, res=1),
    ]
    # encoder shortcut group sizes (g = 4 Cin / Cout at stride 2, Cin / Cout at stride 1), 3 included
    for g, cin, cout in ((1, 8, 32), (2, 8, 16), (4, 16, 16), (8, 16, 8), (3, 24, 32)):
        cs.append(_c(f"down-g{g}", "down", 2, 3, 5, cin, cout, bias="small", shortcut=1))
    for g, cin, cout in ((1, 8, 8), (2, 16, 8), (4, 32, 8), (8, 64, 8), (3, 24, 8)):
        cs.append(_c(f"mean-g{g}", "mean", 2, 3, 5, cin, cout, bias="small", shortcut=1))
    # g = 3 with sums of 24 significant bits, zero weights: a / 3 and a * (1 / 3) round to different bf16 numbers
    cs.append(_c("mean-thirds", "mean", 1, 2, 3, 24, 8, shortcut=1, thirds=1))
    # rounding chains
    cs += [
        _c("dec-chain", "dec", 2, 4, 6, 24, 24, up=1, bias="chain", silu=1, sc_mode=2, sc_rep=4, sc_own=0, res=1, chain=1),
        _c("dec-chain-sc1", "dec", 1, 5, 7, 8, 8, bias="chain", sc_mode=1, sc_rep=1, sc_own=1, res=1, chain=1),
        _c("down-chain", "down", 2, 3, 5, 16, 8, bias="chain", shortcut=1, chain=1),
        _c("mean-chain", "mean", 2, 3, 5, 64, 8, bias="chain", shortcut=1, chain=1),
        _c("kl-chain", "kl", 2, 3, 5, 8, 8, bias="chain", chain=1),
    ]
    # the direct kernel (Cout <= 4): 256 output pixels per workgroup
    cs += [
        _c("direct-c1", "direct", 1, 15, 17, 8, 1),                                             # M = 255, NHWC, no bias
        _c("direct-c2", "direct", 2, 8, 16, 8, 2, bias="small", nchw=1),                        # M = 256, two images in NCHW
        _c("direct-c3", "direct", 1, 1, 257, 128, 3, bias="small", nchw=1),                     # M = 257; 3456 weights: two passes
        _c("direct-c4", "direct", 2, 6, 10, 16, 4, up=1, bias="sat", silu=1, res=1),
        _c("direct-c3-all", "direct", 2, 6, 10, 24, 3, up=1, bias="sat", silu=1, res=1, nchw=1),
    ]
    return cs


CONV_CASES = _conv_cases()
CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)


def conv_dims(c):
    """-> (S, P, stored input H, W, shortcut group size g or 0)"""
    S = STRIDE[c["kind"]]
    P = 0 if c["kind"] == "kl" else 1
    H, W = (c["Ho"] // 2, c["Wo"] // 2) if c["up"] else (c["Ho"] * S, c["Wo"] * S)
    g = 0
    if c["shortcut"]:
        num = 4 * c["Cin"] if S == 2 else c["Cin"]
        assert num % c["Cout"] == 0
        g = num // c["Cout"]
    return S, P, H, W, g


def conv_sc_channels(c):
    return {0: 0, 1: c["Cout"] // max(c["sc_rep"], 1), 2: 4 * c["Cout"] // max(c["sc_rep"], 1)}[c["sc_mode"]]


def thirds_triples():
    """(m1 2^16, m2 2^8, m3) whose exact sum A lies one below three times a tie between two bf16 numbers: the fp32 quotient
    A / 3 rounds below the tie and A * fl(1 / 3) onto it, so the two give different bf16 means"""
    out = []
    for k in range(40, 250):
        A = 3 * (2 * k + 1) * 16384 - 1
        m1, rem = divmod(A, 65536)
        if m1 <= 255:
            a = F32(A)
            if _rbf_np(np.array([a / F32(3)], dtype=F32))[0] != _rbf_np(np.array([a * (F32(1) / F32(3))], dtype=F32))[0]:
                out.append((m1 * 65536, (rem >> 8) * 256, rem & 255))
    return np.array(out, dtype=np.int64)


def conv_inputs(c):
    """int64 numpy operands: x [B, H, W, Cin], w [Cout, 3, 3, Cin], bias [Cout] | None, sc (the shortcut source, NHWC; x
    itself unless sc_own) | None, res [B, Ho, Wo, Cout] | None"""
    r = _rng(c["name"])
    S, P, H, W, g = conv_dims(c)
    B, Cin, Cout = c["B"], c["Cin"], c["Cout"]
    wide = c["chain"] and c["kind"] != "dec"
    x = r.integers(-200, 201, (B, H, W, Cin)) if wide else r.integers(-1, 2, (B, H, W, Cin))
    w = np.zeros((Cout, 3, 3, Cin // 8, 8), dtype=np.int64)
    pos = r.integers(0, 8, (Cout, 3, 3, Cin // 8))
    sign = r.integers(0, 2, (Cout, 3, 3, Cin // 8)) * 2 - 1
    np.put_along_axis(w, pos[..., None], sign[..., None], axis=-1)
    w = w.reshape(Cout, 3, 3, Cin)
    if c["thirds"]:
        t = thirds_triples()
        n = B * H * W * Cout
        x = t[np.arange(n) % len(t)]
        x = np.stack([np.roll(x[i], i // len(t) % 3) for i in range(n)]).reshape(B, H, W, Cin)      # every order of the three summands
        w = np.zeros_like(w)
    bias = {None: None, "small": r.integers(-8, 9, Cout), "sat": np.where(r.integers(0, 2, Cout) == 1, 128, -192),
            "chain": np.array([254, 256, 258])[r.integers(0, 3, Cout)]}[c["bias"]]
    sc = None
    if c["sc_mode"]:
        sch = conv_sc_channels(c)
        hs, ws = (c["Ho"], c["Wo"]) if c["sc_mode"] == 1 else (c["Ho"] // 2, c["Wo"] // 2)
        if c["sc_own"]:
            sc = np.array([-1, 1, 2])[r.integers(0, 3, (B, hs, ws, sch))] if c["chain"] else r.integers(-8, 9, (B, hs, ws, sch))
        else:
            assert x.shape == (B, hs, ws, sch), (c["name"], x.shape, (B, hs, ws, sch))
            sc = x
    res = None
    if c["res"]:
        shape = (B, c["Ho"], c["Wo"], Cout)
        res = np.array([-1, 1, 3])[r.integers(0, 3, shape)] if c["chain"] else r.integers(-8, 9, shape)
    return dict(x=x, w=w, bias=bias, sc=sc, res=res)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


ROUNDINGS = dict(dec=("bias", "silu", "sc", "res"), direct=("bias", "silu", "res"), mean=("bias", "mean", "sum"),
                 down=("bias", "mean", "sum"), kl=("bias",))


def conv_expect(c, inp, skip=None, extra=None):
    """the plain reference -> (values as stored, fp64: [B, Ho, Wo, Cout], or [B, Cout, Ho, Wo] with nchw; stages: the fp64
    value before each rounding, by name).  ``skip`` leaves one named rounding out, ``extra`` = "conv" rounds the conv sum
    before the bias is added (neither happens in the library: the chain cases must notice both)."""
    S, P, H, W, g = conv_dims(c)
    stages = {}

    def r(name, v):
        stages[name] = v
        return v if skip == name else rb64(v)

    x = _nchw(inp["x"])
    xi = Fn.interpolate(x, scale_factor=2, mode="nearest") if c["up"] else x
    wt = torch.from_numpy(inp["w"]).double().permute(0, 3, 1, 2)
    conv = Fn.conv2d(Fn.pad(xi, (0, 1, 0, 1)), wt, stride=2) if c["kind"] == "kl" else Fn.conv2d(xi, wt, stride=S, padding=1)
    stages["conv"] = conv
    if extra == "conv":
        conv = rb64(conv)
    v = conv if inp["bias"] is None else conv + torch.from_numpy(inp["bias"]).double().view(1, -1, 1, 1)
    v = r("bias", v)
    if c["kind"] in ("dec", "direct"):
        if c["silu"]:
            v = r("silu", Fn.silu(v))
        if c["sc_mode"] == 1:
            v = r("sc", v + _nchw(inp["sc"]).repeat_interleave(c["sc_rep"], dim=1))
        elif c["sc_mode"] == 2:
            v = r("sc", v + Fn.pixel_shuffle(_nchw(inp["sc"]).repeat_interleave(c["sc_rep"], dim=1), 2))
        if c["res"]:
            v = r("res", v + _nchw(inp["res"]))
    elif g:
        u = Fn.pixel_unshuffle(x, 2) if S == 2 else x
        s = r("mean", u.unflatten(1, (-1, g)).mean(dim=2))
        v = r("sum", v + s)
    v = rb64(v)                                           # the store is bf16 whatever was skipped
    return (v if c["nchw"] else v.permute(0, 2, 3, 1)).contiguous(), stages


def conv_classes(c):
    """what the case reaches, from the case alone: the launch arithmetic of conv3x3_launch / conv_tile_origin restated"""
    k, B, Cin, Cout = c["kind"], c["B"], c["Cin"], c["Cout"]
    S, P, H, W, g = conv_dims(c)
    hw = c["Ho"] * c["Wo"]
    M = B * hw
    out = set()
    if k == "direct":
        out |= {f"direct/Cout:{Cout}", "direct/nchw" if c["nchw"] else "direct/nhwc"}
        out |= {f"direct/M:{M}"} if M in (255, 256, 257) else set()
        out |= {f"direct/{n}" for n in ("up", "silu", "res") if c[n]}
        if B >= 2 and c["nchw"]:
            out.add("direct/nchw:B2")
        if Cout * 9 * Cin > 2048:
            out.add("direct/stage:2")
        return out
    nbm, nbn = -(-M // BM), -(-Cout // BN)
    nwg = nbm * nbn
    out.add(f"{k}/M:<128" if M < BM else f"{k}/M:=128" if M == BM else f"{k}/M:128k+1" if M % BM == 1 else f"{k}/M:other")
    if any((b * hw) % BM for b in range(1, B)):
        out.add(f"{k}/M:straddle")
    out.add(f"{k}/Cout:{Cout}")
    out.add(f"{k}/wg:<8" if nwg < 8 else f"{k}/wg:=8" if nwg == 8 else f"{k}/wg:8q+{nwg % 8}")
    out.add(f"{k}/Cin:{Cin}")
    if Cin % 64 == 0:
        out.add(f"{k}/tapu:{Cin // 64}")
    if S == 1 and not c["up"]:
        out |= {f"{k}/grid:{n}" for n in (1, 2, 3) if n in (c["Ho"], c["Wo"])}
    if S == 2 and (H, W) == (2, 2):
        out.add(f"{k}/grid:2x2in")
    if c["up"] and (H, W) == (1, 1):
        out.add("dec/grid:up1x1")
    if c["Ho"] % 2 and c["Wo"] % 2 and c["Ho"] > 1 and c["Wo"] > 1:
        out.add(f"{k}/grid:odd")
    if c["chain"]:
        out.add(f"{k}/chain")
    if c["thirds"]:
        out.add(f"{k}/g:3:quotient")
    if k == "dec":
        out.add("dec/bias:1" if c["bias"] else "dec/bias:0")
        out |= {f"dec/{n}" for n in ("silu", "res", "up") if c[n]}
        if c["sc_mode"]:
            out.add(f"dec/sc{c['sc_mode']}:rep{c['sc_rep']}")
            if c["sc_own"]:
                out.add(f"dec/sc{c['sc_mode']}:own")
            if c["bias"] and c["silu"] and c["res"]:
                out.add(f"dec/all:sc{c['sc_mode']}")
    elif k == "kl":
        out.add("kl/bias:1" if c["bias"] else "kl/bias:0")
    else:
        out.add(f"{k}/g:{g}" if g else f"{k}/g:off")
    return out


def conv_required():
    req = set()
    for k in KINDS:
        req |= {f"{k}/M:{m}" for m in ("<128", "=128", "128k+1", "straddle")}
        req |= {f"{k}/Cout:{n}" for n in (8, 124, 128, 132, 260)}
        req |= {f"{k}/wg:{n}" for n in ("<8", "=8", "8q+1", "8q+3", "8q+7")}
        req |= {f"{k}/Cin:{n}" for n in (8, 24, 40, 72, 64, 128, 1024)} | {f"{k}/tapu:{n}" for n in (1, 2, 16)}
        req |= {f"{k}/grid:odd", f"{k}/chain"}
        req |= {f"{k}/grid:{n}" for n in (1, 2, 3)} if STRIDE[k] == 1 else {f"{k}/grid:2x2in"}
    req |= {"dec/grid:up1x1", "dec/bias:0", "dec/bias:1", "dec/silu", "dec/res", "dec/up", "dec/sc2:own", "dec/all:sc1",
            "dec/all:sc2", "kl/bias:0", "kl/bias:1"}
    req |= {f"dec/sc1:rep{n}" for n in (1, 2, 32)} | {f"dec/sc2:rep{n}" for n in (1, 2, 4)}
    req |= {f"{k}/g:{g}" for k in ("down", "mean") for g in ("off", 1, 2, 3, 4, 8)} | {"mean/g:3:quotient"}
    req |= {f"direct/Cout:{n}" for n in (1, 2, 3, 4)} | {f"direct/M:{n}" for n in (255, 256, 257)}
    req |= {"direct/nchw", "direct/nhwc", "direct/up", "direct/silu", "direct/res", "direct/nchw:B2", "direct/stage:2"}
    return req


def reached(cases, classes):
    """class -> names of the cases that reach it"""
    m = {}
    for c in cases:
        for k in classes(c):
            m.setdefault(k, []).append(c["name"])
    return m


# ------------------------------------------------------------------------------------------------ conv: numpy executor
FAULTS = ("drop_chunk", "tail_quad", "sc_index", "skip_round", "inv_quotient", "drop_slab", "neighbour_stat", "missing_tap")


def silu_f32(v):
    """the library's fp32 formula x * 1 / (1 + exp(-x)) in numpy float32"""
    with np.errstate(all="ignore"):
        return (v * (F32(1.0) / (F32(1.0) + np.exp(-v).astype(F32)))).astype(F32)


def conv_int_sums(c, inp, fault=None):
    """im2col rows gathered tap by tap, the product summed 16-byte chunk by chunk in int64 -> ([M, Cout] sums, the largest
    sum of |products| of one output: the bound of every partial sum in any order)"""
    S, P, H, W, g = conv_dims(c)
    B, Cin, Cout, Ho, Wo = c["B"], c["Cin"], c["Cout"], c["Ho"], c["Wo"]
    x, M, K = inp["x"], B * Ho * Wo, 9 * Cin
    m = np.arange(M)
    b, pix = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = pix // Wo, pix % Wo
    Hv, Wv = (Ho, Wo) if S == 1 else (H, W)
    A = np.zeros((M, K), dtype=np.int64)
    for tap in range(9):
        iy, ix = S * oy + tap // 3 - P, S * ox + tap % 3 - P
        ok = (iy >= 0) & (iy < Hv) & (ix >= 0) & (ix < Wv)
        if c["up"]:
            iy, ix = iy >> 1, ix >> 1
        A[ok, tap * Cin:(tap + 1) * Cin] = x[b[ok], iy[ok], ix[ok]]
    wm = inp["w"].reshape(Cout, K)
    acc = np.zeros((M, Cout), dtype=np.int64)
    dropped = 4 * (Cin // 8) + Cin // 8 - 1              # the last chunk of the centre tap
    for ch in range(K // 8):
        if fault == "drop_chunk" and ch == dropped:
            continue
        acc += A[:, ch * 8:ch * 8 + 8] @ wm[:, ch * 8:ch * 8 + 8].T
    if fault == "tail_quad" and Cout >= 8:
        acc[:, Cout - 4:] = acc[:, Cout - 8:Cout - 4].copy()
    return acc, int((np.abs(A) @ np.abs(wm).T).max())


def conv_exec(c, inp, fault=None):
    """the sums of conv_int_sums, then the epilogue with the kernels' own index arithmetic in numpy float32 -> bf16 bits
    (int16 tensor) in the stored layout"""
    S, P, H, W, g = conv_dims(c)
    B, Cin, Cout, Ho, Wo = c["B"], c["Cin"], c["Cout"], c["Ho"], c["Wo"]
    x, M = inp["x"], B * Ho * Wo
    m = np.arange(M)
    b, pix = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = pix // Wo, pix % Wo
    acc, _ = conv_int_sums(c, inp, fault)
    v = acc.astype(F32)
    if inp["bias"] is not None:
        v = v + inp["bias"].astype(F32)[None]
    if fault != "skip_round":
        v = _rbf_np(v)
    n = np.arange(Cout)
    if c["kind"] in ("dec", "direct"):
        if c["silu"]:
            v = _rbf_np(silu_f32(v))
        if c["sc_mode"]:
            sch = conv_sc_channels(c)
            off = 1 if fault == "sc_index" else 0
            if c["sc_mode"] == 1:
                idx = np.minimum((n[None] + off) // c["sc_rep"], sch - 1) + np.zeros((M, 1), dtype=np.int64)
                src = inp["sc"].reshape(M, sch)
                rows = m
            else:
                sub = 2 * (oy & 1) + (ox & 1)
                idx = np.minimum((4 * n[None] + sub[:, None] + off) // c["sc_rep"], sch - 1)
                src = inp["sc"].reshape(-1, sch)
                rows = (b * (Ho >> 1) + (oy >> 1)) * (Wo >> 1) + (ox >> 1)
            v = _rbf_np(v + src[rows[:, None], idx].astype(F32))
        if c["res"]:
            v = _rbf_np(v + inp["res"].reshape(M, Cout).astype(F32))
    elif g:
        a = np.zeros((M, Cout), dtype=F32)
        for i in range(g):
            u = n * g + i
            if S == 2:
                a += x[b[:, None], (2 * oy)[:, None] + ((u & 3) >> 1)[None], (2 * ox)[:, None] + (u & 1)[None], (u >> 2)[None]].astype(F32)
            else:
                a += x[b[:, None], oy[:, None], ox[:, None], u[None]].astype(F32)
        q = a * (F32(1) / F32(g)) if fault == "inv_quotient" else a / F32(g)
        v = _rbf_np(v + _rbf_np(q.astype(F32)))
    y = torch.from_numpy(_rbf_np(v).astype(F32)).to(BF).view(B, Ho, Wo, Cout)
    return bf_bits(y.permute(0, 3, 1, 2).contiguous() if c["nchw"] else y)


# ------------------------------------------------------------------------------------------------ groupnorm
def _g(name, B, HW, C, G, K, a, silu, inplace, tie=0):
    return dict(name=name, B=B, HW=HW, C=C, G=G, K=K, a=a, silu=silu, inplace=inplace, tie=tie)


GN_CASES = [
    _g("hw131073-c8", 1, 131073, 8, 8, -20, 1, 0, 0, tie=1),       # 257 slabs, the last of one pixel; one chunk per pixel; C / G = 1
    _g("hw512-c24", 2, 512, 24, 8, 300, 2, 1, 1),           # 85 rows in flight, one idle thread; a chunk spans 3 groups unevenly
    _g("hw511-c96", 3, 511, 96, 12, -300, 2, 0, 1),         # C / 8 = 12 (21 rows, 4 idle threads), C / G = 8, B = 3
    _g("hw513-c128", 2, 513, 128, 8, -20, 1, 1, 0, tie=1),         # two slabs, the second of one pixel; C / G = 16
    _g("hw16-c2048", 2, 16, 2048, 1024, 300, 2, 0, 0),      # one row in flight; 1024 groups: four passes of the g += 256 loop
    _g("hw64-c24", 2, 64, 24, 8, -20, 1, 0, 0),             # HW below the 85 rows in flight
    _g("hw1-c128", 2, 1, 128, 4, 40, 1, 1, 1),              # one pixel: the group is its 32 channels
]
GN_SECOND = _g("hw64-c24-second", 2, 64, 24, 8, 300, 2, 1, 0)      # the second call on the workspace of hw64-c24
GN_BY_NAME = {c["name"]: c for c in GN_CASES + [GN_SECOND]}


def gn_devs(N, a):
    """the population of N deviations: mean 0 and mean square 4 a^2 exactly; the first is the minimum"""
    n32, rem = divmod(N, 32)
    if rem % 2 and rem < 5:
        n32, rem = n32 - 1, rem + 32
    assert n32 >= 0 and N not in (1, 3), N
    d = [a] * (15 * n32) + [-a] * (15 * n32) + [7 * a] * n32 + [-7 * a] * n32
    if rem % 2:
        d += [3 * a, -3 * a, a, -a, 0]
        rem -= 5
    d += [2 * a, -2 * a] * (rem // 2)
    d = np.array(d, dtype=np.int64)
    assert len(d) == N and d.sum() == 0 and (d * d).sum() == 4 * a * a * N
    return d


def gn_inputs(c):
    """x [B, HW, C], w, b [C] (int64 numpy) and the exact statistics K, mean [B, G]"""
    r = _rng("gn-" + c["name"])
    B, HW, C, G, a = c["B"], c["HW"], c["C"], c["G"], c["a"]
    cg = C // G
    x = np.zeros((B, HW, G, cg), dtype=np.int64)
    Ks, means = np.zeros((B, G), dtype=np.int64), np.zeros((B, G), dtype=np.int64)
    base = gn_devs(HW * cg, a)
    lo = int(base.argmin())
    base[[0, lo]] = base[[lo, 0]]
    for bi in range(B):
        perm = np.argsort(r.random((G, HW * cg - 1)), axis=1) + 1
        for gi in range(G):
            k = c["K"] + 2 * a * ((3 * bi + 5 * gi) % 7)
            d = np.concatenate([base[:1], base[perm[gi]]])
            Ks[bi, gi], means[bi, gi] = k, k - base[0]
            x[bi, :, gi, :] = (k - base[0] + d).reshape(HW, cg)
    if c["tie"]:            # odd w, b at 129 and above (bf16 steps of 1): xhat w + b = b +- w / 2, b +- 7 w / 2 are all ties
        w = np.array([-3, -1, 1, 3])[r.integers(0, 4, C)]
        b = np.where(r.integers(0, 2, C) == 1, 140, -192) if c["silu"] else r.integers(140, 201, C)
    else:
        w = np.array([-4, -2, 2, 4])[r.integers(0, 4, C)] if c["silu"] else np.array([-3, -2, 1, 2, 3, 4])[r.integers(0, 6, C)]
        b = np.where(r.integers(0, 2, C) == 1, 128, -192) if c["silu"] else r.integers(-8, 9, C)
    return dict(x=x.reshape(B, HW, C), w=w, b=b, K=Ks, mean=means)


def gn_expect(c, inp):
    """nn.GroupNorm(G, C, eps = 0) in fp64, one bf16 rounding, then SiLU and another -> ([B, HW, C] fp64, pre-activation).
    The exact result is a multiple of 1/2 (xhat is one, w and b are integers); torch's fp64 result is off it by some 1e-14,
    which would make an exact 0 a tiny bf16 number, so it is taken to the nearest multiple of 1/4 before the rounding
    (test_vae_kernels_ref_cpu.py holds it to the closed form in integers)."""
    x = torch.from_numpy(inp["x"]).double().permute(0, 2, 1)                       # [B, C, HW]
    y = Fn.group_norm(x, c["G"], torch.from_numpy(inp["w"]).double(), torch.from_numpy(inp["b"]).double(), eps=0.0)
    assert (y - torch.round(y * 4) / 4).abs().max() < 1e-9
    y = rb64((torch.round(y * 4) / 4).permute(0, 2, 1).contiguous())
    return (rb64(Fn.silu(y)) if c["silu"] else y), y


def gn_rows(C):
    return 256 // (C // 8)


def gn_classes(c):
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    nch, cg, rows, nslab = C // 8, C // G, gn_rows(C), -(-HW // GN_SLAB)
    out = {f"C/8:{nch}", f"C/G:{cg}" if cg < 16 else "C/G:>=16", f"silu:{c['silu']}", "inplace" if c["inplace"] else "separate"}
    if rows * nch < 256:
        out.add("idle-threads")
    if rows == 1:
        out.add("rows:1")
    if 8 % cg and cg % 8:
        out.add("chunk-spans-groups-unevenly")
    if G > 256:
        out.add("G>256")
    out.add("HW:1" if HW == 1 else f"HW:{HW}" if HW in (511, 512, 513) else "HW:>131072" if HW > 256 * GN_SLAB else
            "HW:<rows" if HW < rows else "HW:other")
    if HW < rows:
        out.add("HW:<rows")
    if nslab > 256:
        out.add("slabs:>256")
    if HW % GN_SLAB == 1 and HW > 1:
        out.add("last-slab:1")
    if B >= 3:
        out.add("B:3")
    if abs(c["K"]) >= 256:
        out.add("K:large")
    if c["tie"]:
        out.add("ties")
    return out


GN_REQUIRED = ({f"C/8:{n}" for n in (1, 3, 12, 16, 256)} | {f"C/G:{n}" for n in (1, 2, 3, 8, ">=16")} |
               {f"HW:{n}" for n in (1, "<rows", 511, 512, 513, ">131072")} |
               {"G>256", "B:3", "inplace", "separate", "silu:0", "silu:1", "idle-threads", "rows:1", "slabs:>256",
                "last-slab:1", "chunk-spans-groups-unevenly", "K:large", "ties"})


def gn_workspace_floats(B, HW, G):
    """[B, nslab, G, 2] partials padded to 16 bytes, then [B, G, 4] statistics (include/yat_hip.h)"""
    return ((B * -(-HW // GN_SLAB) * G * 2 + 3) & ~3) + B * G * 4


def gn_exec(c, inp, fault=None):
    """slab partials of shifted sums, the finish and the apply pass in numpy float32 -> bf16 bits [B, HW, C]"""
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    cg, nslab = C // G, -(-HW // GN_SLAB)
    x = inp["x"].astype(F32).reshape(B, HW, G, cg)
    k = x[:, 0, :, 0]                                                               # [B, G]
    d = x - k[:, None, :, None]
    part = np.zeros((B, nslab, G, 2), dtype=F32)
    for s in range(nslab):
        ds = d[:, s * GN_SLAB:(s + 1) * GN_SLAB]
        part[:, s, :, 0] = ds.sum(axis=(1, 3), dtype=F32)
        part[:, s, :, 1] = (ds * ds).sum(axis=(1, 3), dtype=F32)
    if fault == "drop_slab":
        part = part[:, :max(nslab - 1, 1)] if nslab > 1 else part * F32(0.5)
    tot = part.sum(axis=1, dtype=F32)
    n = F32(HW) * F32(cg)
    m1 = (tot[..., 0] / n).astype(F32)
    var = np.maximum((tot[..., 1] / n).astype(F32) - m1 * m1, F32(0))
    with np.errstate(all="ignore"):
        rstd = (F32(1.0) / np.sqrt(var).astype(F32)).astype(F32)
    if fault == "neighbour_stat":
        k, m1, rstd = np.roll(k, 1, axis=0), np.roll(m1, 1, axis=0), np.roll(rstd, 1, axis=0)
    xh = ((x - k[:, None, :, None]) - m1[:, None, :, None]) * rstd[:, None, :, None]
    y = _rbf_np((xh.reshape(B, HW, C).astype(np.float64) * inp["w"] + inp["b"]).astype(F32))
    if c["silu"]:
        y = _rbf_np(silu_f32(y))
    return bf_bits(torch.from_numpy(y.astype(F32)).to(BF))


# ------------------------------------------------------------------------------------------------ msla_aggregate
MSLA_CASES = [dict(name=f"b{B}-h{H}-w{W}-c{C3}", B=B, H=H, W=W, C3=C3) for B, H, W, C3 in
              ((1, 1, 1, 32), (1, 2, 2, 32), (2, 3, 3, 96), (1, 5, 63, 32), (1, 1, 64, 32), (1, 2, 65, 96), (2, 3, 130, 32))]
MSLA_TAP_CASE = dict(name="taps", B=2, H=5, W=66, C3=32)


def msla_inputs(c):
    """x [B, H, W, C3] in [-2, 2], w_dw [C3, 25] in {-1, 0, 1}, w_pw [C3, 32]: +-1 at four positions of each row"""
    r = _rng("msla-" + c["name"])
    B, H, W, C3 = c["B"], c["H"], c["W"], c["C3"]
    x = r.integers(-2, 3, (B, H, W, C3))
    wdw = r.integers(-1, 2, (C3, 25))
    wpw = np.zeros((C3, 32), dtype=np.int64)
    for o in range(C3):
        wpw[o, r.choice(32, 4, replace=False)] = r.integers(0, 2, 4) * 2 - 1
    return dict(x=x, wdw=wdw, wpw=wpw)


def msla_expect(c, inp):
    """depthwise 5 x 5 (pad 2) -> bf16 -> grouped 1 x 1 (32 -> 32) -> bf16, fp64 -> ([B, H, W, C3], the depthwise stage)"""
    C3 = c["C3"]
    x = _nchw(inp["x"])
    t = Fn.conv2d(x, torch.from_numpy(inp["wdw"]).double().view(C3, 1, 5, 5), padding=2, groups=C3)
    y = Fn.conv2d(rb64(t), torch.from_numpy(inp["wpw"]).double().view(C3, 32, 1, 1), groups=C3 // 32)
    return rb64(y).permute(0, 2, 3, 1).contiguous(), t


def msla_classes(c):
    out = {f"W:{c['W']}", f"H:{c['H']}", f"C3:{c['C3']}", f"segments:{-(-c['W'] // 64)}"}
    if c["B"] >= 2:
        out.add("B:2")
    return out


MSLA_REQUIRED = ({f"W:{n}" for n in (1, 2, 3, 63, 64, 65, 130)} | {f"H:{n}" for n in (1, 2, 3, 5)} |
                 {"C3:32", "C3:96", "B:2", "segments:1", "segments:2", "segments:3"})


def msla_exec(c, inp, fault=None):
    """tap by tap with the bounds tests of the kernel, then the grouped product, in numpy -> bf16 bits [B, H, W, C3]"""
    B, H, W, C3 = c["B"], c["H"], c["W"], c["C3"]
    x = inp["x"]
    t = np.zeros((B, H, W, C3), dtype=np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            tap = (dy + 2) * 5 + dx + 2
            if fault == "missing_tap" and tap == 12:
                continue
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                t[:, y0:y1, x0:x1] += inp["wdw"][:, tap] * x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    tr = _rbf_np(t.astype(F32)).astype(np.float64).reshape(B, H, W, C3 // 32, 32)
    y = np.einsum("bhwgi,goi->bhwgo", tr, inp["wpw"].reshape(C3 // 32, 32, 32).astype(np.float64)).reshape(B, H, W, C3)
    return bf_bits(torch.from_numpy(_rbf_np(y.astype(F32)).astype(F32)).to(BF))


def msla_tap_inputs(c, tap):
    """one depthwise tap of weight 1 on every channel, identity pointwise map; x distinct small integers"""
    B, H, W, C3 = c["B"], c["H"], c["W"], c["C3"]
    i = np.arange(B * H * W * C3, dtype=np.int64).reshape(B, H, W, C3)
    x = (i * 7 + i // C3) % 251 - 125
    wdw = np.zeros((C3, 25), dtype=np.int64)
    wdw[:, tap] = 1
    return dict(x=x, wdw=wdw, wpw=np.tile(np.eye(32, dtype=np.int64), (C3 // 32, 1)))


def msla_tap_expect(c, inp, tap):
    """the input pixel the tap reads, (y + tap / 5 - 2, x + tap % 5 - 2), or zero outside: a plain shift (int64 numpy)"""
    dy, dx = tap // 5 - 2, tap % 5 - 2
    x = inp["x"]
    p = np.pad(x, ((0, 0), (2, 2), (2, 2), (0, 0)))
    return p[:, 2 + dy:2 + dy + c["H"], 2 + dx:2 + dx + c["W"]]


def ints_bf(a):
    """integers a bf16 number holds exactly -> bf16 tensor (asserted by the round trip)"""
    t = torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))
    assert torch.equal(t.to(BF).float(), t), "an input is no bf16 number"
    return t.to(BF)
