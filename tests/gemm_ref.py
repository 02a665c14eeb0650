"""Case table, CPU model and checker of the GEMM family (csrc/gemm.hip, csrc/gemm256.hip, csrc/gemm_common.hpp) for
test_gemm_layout_cpu.py and test_gemm_layout_gpu.py, written apart from yat_amd (it does not import yat_amd).  Everything here
runs on the CPU.

    Case, Place          one launch: layout, M, N, K, the `variant` word, the placement of every operand in a larger buffer and
                         the epilogue members in use
    TABLE                the cases; GROUPED the problems of the grouped entry point
    classes(case)        what a case reaches, derived from the case alone: the wide / narrow predicate of gemm256.hip, tiles per
                         path, ragged flags, the leading dimensions that are 4 (mod 8)
    build(case, seed)    (bufs, twin): every operand as a view into a larger buffer -- inputs NaN outside the view, outputs the
                         sentinel everywhere -- and the same values in exact-shape tensors
    views(case, bufs)    the operand views of a set of buffers (also after the buffers moved to another device)
    model(case, v, own)  the expected windows in fp32, with the rounding points include/yat_hip.h and gemm_common.hpp state
    check(case, before, after, twin_out)    guard, inputs intact, same bits as the contiguous twin: a list of failure strings
    cpu_execute(case, v, fault)             a plain-torch executor that addresses memory the way the kernels do (base pointer,
                                            leading dimension); `fault` plants one error (FAULTS) for test_gemm_layout_cpu.py

Layouts (yat_hip.h): A is [M, K] (a_t = 0) or [K, M]; B is [N, K] (b_t = 0) or [K, N].  NT = (0, 0), NN = (0, 1), TN = (1, 1),
TT = (1, 0).  A *placement* puts an [rows, cols] operand at rows [top, top + rows), columns [col, col + cols) of a
[top + rows + bottom, ld] buffer, so ld is its leading dimension.

Epilogue, one fp32 value per element: +bias -> (pre_add: round to bf16, + pre_add) -> round to bf16 where aux_out, an activation
or a residual follows -> aux_out copy -> activation -> bf16(gate[m / rows_per_batch] * .) -> +residual -> round to bf16.
glu_u, dact_z and a_rowsum_out are forms of their own (model()).
"""
import dataclasses
import math
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F

BF = torch.bfloat16
SENTINEL = 0x7FA5                 # a signalling bf16 NaN: arithmetic quiets it (0x7FE5), so only a copy reproduces these bits
LAYOUTS = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1), "TT": (1, 0)}
TILE = {1: (128, 128), 4: (256, 256), 5: (256, 320)}            # rows x columns per workgroup of each tile variant
OUTPUTS = ("c", "aux", "rowsum")
MAX_DIM, SPLIT_K = 700, 1096


@dataclasses.dataclass(frozen=True)
class Place:
    top: int
    bottom: int
    col: int
    ld: int


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str                      # shape class: wide | narrow_n | narrow_ld | rank
    placement: str                  # plain | a | b | c | abc | mid
    epi: str                        # epilogue class (EPIS)
    a_t: int
    b_t: int
    M: int
    N: int
    K: int
    path: int                       # the `variant` word: 1, 4, 5, 204, 305 or 0
    a: Place
    b: Place
    c: Place
    bias: Optional[Tuple[int, int]] = None            # (offset, tail) inside a longer vector
    aux: Optional[Place] = None
    res: Union[None, Place, str] = None               # a placement of its own, or "out": C is the residual (accumulate)
    gate: Optional[Tuple[int, int, int]] = None       # (ld_gate, rows_per_batch, column offset); ld_gate 0: one row for all
    act: str = "none"
    pre: Optional[Place] = None
    dact: Optional[Place] = None
    glu: Optional[Place] = None
    rowsum: Optional[str] = None                      # "plain" | "acc"
    member: Optional[str] = None                      # narrow_ld: the one leading dimension that is 4 (mod 8)

    @property
    def layout(self):
        return {v: k for k, v in LAYOUTS.items()}[(self.a_t, self.b_t)]

    @property
    def tile(self):
        return self.path % 100

    @property
    def cw(self):
        return 2 * self.N if self.glu else self.N     # columns of C


def shapes(case):
    """name -> (rows, cols, Place) of every 2-D operand in use"""
    M, N, K = case.M, case.N, case.K
    s = {"a": ((K, M) if case.a_t else (M, K)) + (case.a,), "b": ((K, N) if case.b_t else (N, K)) + (case.b,),
         "c": (M, case.cw, case.c)}
    for name, cols in (("aux", N), ("pre", N), ("dact", N), ("glu", 2 * N)):
        if getattr(case, name) is not None:
            s[name] = (M, cols, getattr(case, name))
    if isinstance(case.res, Place):
        s["res"] = (M, N, case.res)
    if case.gate is not None and case.gate[0] > 0:
        s["gate"] = (gate_rows(case), N, Place(1, 1, case.gate[2], case.gate[0]))
    return s


def gate_rows(case):
    rpb = case.gate[1] if case.gate[1] > 0 else case.M
    return (case.M + rpb - 1) // rpb


def wide(case, ld=None):
    """the `wide` predicate of gemm256_body (16-byte epilogue), from the leading dimensions `ld` (default: the case's own)"""
    ld = ld or lds(case)
    return not (case.N % 8 or ld["c"] % 8 or (case.res is not None and ld["res"] % 8) or (case.aux and ld["aux"] % 8)
                or (case.gate and ld["gate"] % 8) or (case.glu and ld["glu"] % 8) or (case.pre and ld["pre"] % 8)
                or (case.dact and ld["dact"] % 8))


def lds(case):
    d = {k: p.ld for k, (_, _, p) in shapes(case).items()}
    if case.res == "out":
        d["res"] = d["c"]
    if case.gate is not None:
        d["gate"] = case.gate[0]
    return d


def classes(case):
    tm, tn = TILE.get(case.tile, TILE[1])
    return {
        "group": case.group, "placement": case.placement, "epi": case.epi, "layout": case.layout, "path": case.path,
        "wide": wide(case),
        "tiles": {v: (-(-case.M // r), -(-case.N // c)) for v, (r, c) in TILE.items()},
        "ragged_m": case.M % tm != 0, "ragged_n": case.N % tn != 0, "ragged_k": case.K % 64 != 0,
        "n_mod8_is_4": case.N % 8 == 4,
        "ld4": tuple(sorted(k for k, v in lds(case).items() if v % 8 == 4)),
    }


# ------------------------------------------------------------------------------------------------ the table
EPIS = ("none", "bias", "aux", "res", "acc", "gate6", "gate0", "silu", "gelu", "pre", "dact_silu", "dact_gelu", "glu",
        "rowsum", "rowsum_acc", "chain")
PAD = 24                                              # a strided operand's leading dimension exceeds its width by this


def _places(kind, a_t, b_t, M, N, K, cw, c_col=8, c_pad=PAD):
    aw, bw = (M if a_t else K), (N if b_t else K)
    pa, pb, pc = Place(0, 0, 0, aw), Place(0, 0, 0, bw), Place(0, 0, 0, cw)
    if kind in ("a", "abc"):
        pa = Place(1, 1, 8, aw + PAD)
    if kind in ("b", "abc"):
        pb = Place(1, 1, 16, bw + PAD)
    if kind in ("c", "abc"):
        pc = Place(2, 2, c_col, cw + c_pad)
    if kind == "mid":                                 # the middle of three adjacent windows (c_col: where the first begins)
        first = c_col if c_col % 8 else 0
        pc = Place(1, 1, first + cw, first + 3 * cw)
    return pa, pb, pc


def _case(group, placement, epi, layout, M, N, K, path, member=None):
    a_t, b_t = LAYOUTS[layout]
    narrow = group in ("narrow_n", "narrow_ld")
    off = 4 if narrow else 8                          # column offset of C / aux / residual / bias: 8 bytes where the 8-byte
    cw = 2 * N if epi == "glu" else N                 # epilogue runs, 16 where the 16-byte one may
    pad = lambda name, p: p - 4 if member == name else p
    pa, pb, pc = _places(placement, a_t, b_t, M, N, K, cw, c_col=off, c_pad=pad("c", PAD))
    if member == "c" and placement not in ("c", "abc", "mid"):
        pc = Place(2, 2, off, cw + PAD - 4)
    kw = {}
    chain = epi == "chain"
    if chain or epi == "bias":
        kw["bias"] = (off, 5)
    if chain or epi in ("aux", "silu", "gelu"):
        kw["aux"] = Place(1, 1, off, N + pad("aux", 40))
    if chain or epi == "res":
        kw["res"] = Place(1, 2, off, N + pad("res", 56))
    if epi == "acc":
        kw["res"] = "out"
    if chain or epi == "gate6":
        kw["gate"] = (N + 20 if member == "gate" else 6 * N, 88, 0 if member == "gate" or narrow else 8)
    if epi == "gate0":
        kw["gate"] = (0, 0, 0)
    if chain or epi in ("silu", "dact_silu"):
        kw["act"] = "silu"
    if epi in ("gelu", "dact_gelu"):
        kw["act"] = "gelu_tanh"
    if epi == "pre" or member == "pre":
        kw["pre"] = Place(1, 1, off, N + pad("pre", 72))
    if epi in ("dact_silu", "dact_gelu"):
        kw["dact"] = Place(1, 1, off, N + pad("dact", 40))
    if epi == "glu":
        kw["glu"] = Place(1, 1, 8, 2 * N + 40)
    if epi in ("rowsum", "rowsum_acc"):
        kw["rowsum"] = "acc" if epi == "rowsum_acc" else "plain"
        if epi == "rowsum_acc":
            kw["res"] = "out"                         # gradient accumulation: dW += and db += in one launch
    name = f"{group}-{placement}-{epi}{'-' + member if member else ''}-{layout}-{M}x{N}x{K}-v{path}"
    return Case(name, group, placement, epi, a_t, b_t, M, N, K, path, pa, pb, pc, member=member, **kw)


def _table():
    t = []
    W = (264, 328, 72)
    # ---- shapes, wide: two row tiles of 256 (8 ragged rows) / three of 128; two column tiles at 256 and 320, three at 128
    for layout in LAYOUTS:
        for path in (1, 4, 5):
            t.append(_case("wide", "plain", "none", layout, *W, path))
    for path in (204, 305):
        for layout in ("TN", "NT"):
            t.append(_case("wide", "plain", "none", layout, 264, 328, SPLIT_K, path))
    # ---- shapes, narrow by N (N % 8 == 4: b_t = 0 only)
    for N in (332, 12, 4):
        for layout in ("NT", "TT"):
            for path in (1, 4, 5):
                t.append(_case("narrow_n", "plain", "none", layout, 264, N, 72, path))
    # ---- narrow by stride: one leading dimension 4 (mod 8), every other one a multiple of 8
    for path in (4, 5):
        for layout in LAYOUTS:
            for member in ("c", "aux", "res", "gate"):
                t.append(_case("narrow_ld", "c", "chain", layout, *W, path, member=member))
        t.append(_case("narrow_ld", "c", "chain", "NT", *W, path, member="pre"))
        t.append(_case("narrow_ld", "c", "dact_silu", "NN", *W, path, member="dact"))
    # ---- adapter ranks and single rows: the policy's own pick and the 128 x 128 kernel
    ranks = [("NT", 264, 8, 72), ("NT", 264, 16, 8), ("NT", 264, 72, 8), ("NN", 264, 72, 8), ("TN", 8, 72, 264),
             ("TN", 16, 328, 264), ("NT", 1, 72, 72), ("NT", 7, 72, 72), ("NN", 1, 72, 72), ("NN", 7, 72, 72)]
    for path in (0, 1):
        for layout, M, N, K in ranks:
            t.append(_case("rank", "plain", "none", layout, M, N, K, path))
    # ---- placements, for every shape class
    kinds = ("a", "b", "c", "abc", "mid")
    lay4 = tuple(LAYOUTS)
    for i, kind in enumerate(kinds):
        for j, path in enumerate((1, 4, 5)):
            t.append(_case("wide", kind, "none", lay4[(i + j) % 4], *W, path))
            t.append(_case("narrow_n", kind, "none", ("NT", "TT")[(i + j) % 2], 264, (332, 12, 4)[(i + j) % 3], 72, path))
        for j, path in enumerate((4, 5)):
            t.append(_case("narrow_ld", kind, "chain", lay4[(i + j) % 4], *W, path, member="c"))
        for j, path in enumerate((0, 1)):
            layout, M, N, K = ranks[(2 * i + j) % len(ranks)]
            t.append(_case("rank", kind, "none", layout, M, N, K, path))
    t.append(_case("wide", "abc", "none", "NT", 264, 328, SPLIT_K, 204))
    t.append(_case("wide", "abc", "none", "TN", 264, 328, SPLIT_K, 305))
    # ---- epilogues on strided operands
    for path in (1, 4, 5):
        for epi in ("bias", "aux", "res", "gate6", "gate0", "silu", "gelu", "pre", "chain"):
            t.append(_case("wide", "abc", epi, "NT", *W, path))
        for layout in ("TN", "NN"):
            t.append(_case("wide", "abc", "acc", layout, *W, path))
        for i, N in enumerate((332, 12, 4)):
            t.append(_case("narrow_n", "abc", "chain", ("NT", "TT")[(i + path) % 2], 264, N, 72, path))
    for path in (4, 5):
        for epi in ("dact_silu", "dact_gelu", "glu"):
            t.append(_case("wide", "abc", epi, "NN", *W, path))
    for path in (0, 4):
        for epi in ("rowsum", "rowsum_acc"):
            t.append(_case("wide", "a", epi, "TN", *W, path))
    for path in (204, 305):
        for layout in ("NT", "TN"):
            t.append(_case("wide", "abc", "chain", layout, 264, 328, SPLIT_K, path))
    return tuple({c.name: c for c in t}.values())      # (a placement case that a shape class already holds counts once)


TABLE = _table()

# the grouped entry point (ops.wgrad_grouped): (tokens, N, K) of three weight gradients dW = dy^T x; dy and x are column slices
# of wider buffers, each out is the first N rows of a taller buffer, the bias gradient sits in a longer vector
GROUPED = ((264, 328, 72), (264, 72, 328), (136, 264, 520))


# ------------------------------------------------------------------------------------------------ buffers
def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16).view(BF)


def bits(t):
    return t.contiguous().view(torch.int16)


def build(case, seed=0):
    """(bufs, twin): name -> full buffer, name -> contiguous exact-shape tensor with the same values"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    bufs, twin = {}, {}
    scale = {"b": case.K ** -0.5, "a": case.K ** -0.5 if case.rowsum else 1.0}

    def window(name, rows, cols):
        live = name in ("a", "b", "pre", "dact", "glu", "res", "gate") or (name == "c" and case.res == "out")
        return (torch.randn(rows, cols, generator=g) * scale.get(name, 1.0)).to(BF) if live else _sentinel(rows, cols)

    for name, (rows, cols, p) in shapes(case).items():
        w = window(name, rows, cols)
        full = _sentinel(p.top + rows + p.bottom, p.ld) if name in OUTPUTS else \
            torch.full((p.top + rows + p.bottom, p.ld), float("nan"), dtype=BF)
        full[p.top:p.top + rows, p.col:p.col + cols] = w
        bufs[name], twin[name] = full, w.clone()
    if case.bias is not None:
        off, tail = case.bias
        w = torch.randn(case.N, generator=g).to(BF)
        bufs["bias"] = torch.full((off + case.N + tail,), float("nan"), dtype=BF)
        bufs["bias"][off:off + case.N] = w
        twin["bias"] = w.clone()
    if case.gate is not None and case.gate[0] == 0:
        w = torch.randn(case.N, generator=g).to(BF)
        bufs["gate"] = torch.full((8 + case.N + 3,), float("nan"), dtype=BF)
        bufs["gate"][8:8 + case.N] = w
        twin["gate"] = w.clone()
    if case.rowsum is not None:
        w = torch.randn(case.M, generator=g).to(BF) if case.rowsum == "acc" else _sentinel(case.M)
        bufs["rowsum"] = _sentinel(3 + case.M + 5)
        bufs["rowsum"][3:3 + case.M] = w
        twin["rowsum"] = w.clone()
    _match_signs(case, twin, g)
    for name, t in views(case, bufs).items():
        t.copy_(twin["c" if name == "res" and case.res == "out" else name])
    return bufs, twin


def _match_signs(case, twin, g):
    """Every addend that follows a rounding (pre_add, residual, the accumulated C and a_rowsum) gets the sign of the value it is
    added to.  A sum accumulated in another order may round that value to the neighbouring bf16 number, one ulp of ITS
    magnitude; were the addend free to cancel it, that ulp could be many ulps of the result, which close() measures
    against.  With equal signs the result is the larger one.  Magnitudes stay random, so a wrong row or column still shows."""
    if case.pre is None and case.res is None and case.rowsum != "acc":
        return
    a, b = twin["a"].double(), twin["b"].double()
    acc = ((a.T if case.a_t else a) @ (b if case.b_t else b.T)).float()
    w = {k: t.float() for k, t in twin.items() if k not in ("a", "b", "c", "aux", "rowsum")}

    def like(t):
        return (torch.randn(t.shape, generator=g).abs() * torch.where(t < 0, -1.0, 1.0)).to(BF)

    if case.pre is not None:
        twin["pre"] = like(_epilogue(case, acc, w, stop="pre"))
        w["pre"] = twin["pre"].float()
    if case.res is not None:
        twin["c" if case.res == "out" else "res"] = like(_epilogue(case, acc, w, stop="res"))
    if case.rowsum == "acc":
        twin["rowsum"] = like((a.sum(0) if case.a_t else a.sum(1)).float())


def views(case, bufs):
    v = {}
    for name, (rows, cols, p) in shapes(case).items():
        v[name] = bufs[name][p.top:p.top + rows, p.col:p.col + cols]
    if case.bias is not None:
        v["bias"] = bufs["bias"][case.bias[0]:case.bias[0] + case.N]
    if case.gate is not None and case.gate[0] == 0:
        v["gate"] = bufs["gate"][8:8 + case.N]
    if case.rowsum is not None:
        v["rowsum"] = bufs["rowsum"][3:3 + case.M]
    if case.res == "out":
        v["res"] = v["c"]
    return v


def twin_views(case, twin):
    v = dict(twin)
    if case.res == "out":
        v["res"] = v["c"]
    return v


def clone(bufs):
    return {k: t.clone() for k, t in bufs.items()}


# ------------------------------------------------------------------------------------------------ model
def rb(x):
    return x.to(BF).float()


def _sig(x):
    return torch.sigmoid(x)


def _act(x, kind):
    return x * _sig(x) if kind == "silu" else F.gelu(x, approximate="tanh")


def _dact(x, kind):
    if kind == "silu":
        s = _sig(x)
        return s * (1 + x * (1 - s))
    k0, k1 = math.sqrt(2 / math.pi), 0.044715            # 0.5 (1 + tanh u) = sigmoid(2u), u = k0 (x + k1 x^3)
    s = _sig(2 * k0 * (x + k1 * x ** 3))
    return s + x * 2 * s * (1 - s) * k0 * (1 + 3 * k1 * x * x)


def _epilogue(case, acc, w, gate_div=None, stop=None):
    """acc fp32 [M, N] and the input windows `w` (fp32) -> the output windows {c, aux} in bf16 (stop = "pre" | "res": the fp32
    value that pre_add / the residual is added to, instead)"""
    out = {}
    if case.glu is not None:
        N = case.N
        ua, ug, d = w["glu"][:, :N], w["glu"][:, N:], rb(acc)
        out["c"] = torch.cat([d * rb(_act(ug, "silu")), rb(d * ua) * _dact(ug, "silu")], 1).to(BF)
        return out
    if case.dact is not None:
        out["c"] = (rb(acc) * _dact(w["dact"], case.act)).to(BF)
        return out
    v = acc
    if "bias" in w:
        v = v + w["bias"]
    if stop == "pre":
        return rb(v)
    if case.pre is not None:
        v = rb(v) + w["pre"]
    if case.aux is not None or case.act != "none" or case.res is not None:
        v = rb(v)
    if case.aux is not None:
        out["aux"] = v.to(BF)
        if "own_aux" in w:                                # (a rounding tie in the aux copy does not count twice)
            v = w["own_aux"]
    if case.act != "none":
        v = _act(v, case.act)
    if case.gate is not None:
        g = w["gate"]
        if g.dim() == 2:
            rpb = gate_div or (case.gate[1] if case.gate[1] > 0 else case.M)
            g = g[torch.arange(case.M) // rpb]
        v = rb(g * v)
    if stop == "res":
        return v
    if case.res is not None:
        v = v + w["res"]
    out["c"] = v.to(BF)
    return out


def model(case, v, own=None):
    """The expected output windows {c, aux, rowsum} (bf16) from the input views `v` (taken BEFORE the launch): the product in
    fp64, rounded once to fp32, then the epilogue with the kernels' rounding points.  `own`: the launch's own aux_out window;
    the stages behind the copy then start from it, as the per-kernel tests do (test_gemm256_second_operand_pair)."""
    a, b = v["a"].double(), v["b"].double()
    acc = ((a.T if case.a_t else a) @ (b if case.b_t else b.T)).float()
    w = {k: t.float() for k, t in v.items() if k not in ("a", "b", "c", "aux", "rowsum")}
    if own is not None and case.aux is not None:
        w["own_aux"] = own.float()
    out = _epilogue(case, acc, w)
    if case.rowsum is not None:
        s = (a.sum(0) if case.a_t else a.sum(1)).float()
        out["rowsum"] = (rb(s) + v["rowsum"].float() if case.rowsum == "acc" else s).to(BF)
    return out


# ------------------------------------------------------------------------------------------------ checker
def _window_mask(case, name, buf):
    m = torch.zeros(buf.shape, dtype=torch.bool)
    if name == "rowsum":
        m[3:3 + case.M] = True
    else:
        rows, cols, p = shapes(case)[name]
        m[p.top:p.top + rows, p.col:p.col + cols] = True
    return m


def check(case, before, after, twin_out):
    """before / after: the buffers of build() around the launch on the views (CPU tensors); twin_out: name -> the output of
    the same launch on the contiguous twin.  Returns the list of failures."""
    fails = []
    v = views(case, after)
    for name in OUTPUTS:
        if name not in after:
            continue
        outside = bits(after[name])[~_window_mask(case, name, after[name])]
        bad = int((outside != bits(_sentinel(1))[0]).sum())
        if bad:
            fails.append(f"{case.name}: guard: {bad} elements of {name} outside its window were written")
        if not torch.equal(v[name], twin_out[name]):
            d = (bits(v[name]) != bits(twin_out[name])).nonzero()
            fails.append(f"{case.name}: {name} differs from the contiguous launch in {len(d)} elements, first at "
                         f"{tuple(d[0].tolist())}")
    for name in before:
        if name in OUTPUTS:
            continue
        if not torch.equal(bits(before[name]), bits(after[name])):
            fails.append(f"{case.name}: input {name} was modified")
    return fails


# ------------------------------------------------------------------------------------------------ CPU executor
FAULTS = ("past_n", "row_m", "eight_where_four", "aux_uses_ldc", "res_uses_ldc", "lda_is_k", "b_past_width", "drop_ragged_k",
          "gate_row_by_m", "rowsum_writes_m")
# what a placement cannot show (the twin makes the same mistake): seen by close(window, model) only
ARITHMETIC_FAULTS = ("drop_ragged_k", "gate_row_by_m")


def _flat(t):
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def _index(t, rows, cols, ld):
    return t.storage_offset() + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]


def raw_load(t, rows, cols, ld):
    """[rows, cols] from the base pointer of `t` with leading dimension `ld` (reads past the allocation repeat its last element)"""
    flat = _flat(t)
    return flat[_index(t, rows, cols, ld).clamp_(max=flat.numel() - 1)].float()


def raw_store(t, vals, ld):
    flat = _flat(t)
    idx = _index(t, vals.shape[0], vals.shape[1], ld)
    ok = idx < flat.numel()
    flat[idx[ok]] = vals.to(BF)[ok]


def cpu_execute(case, v, fault=None):
    """The launch in plain torch on the views `v`, in place.  Memory is addressed as the kernels address it: from each
    operand's base pointer with its leading dimension, never through the view's shape."""
    M, N, K = case.M, case.N, case.K
    ld = {k: (t.stride(0) if t.dim() == 2 else 0) for k, t in v.items()}
    ar, ac = (K, M) if case.a_t else (M, K)
    br, bc = (K, N) if case.b_t else (N, K)
    a = raw_load(v["a"], ar, ac, ac if fault == "lda_is_k" else ld["a"])
    if fault == "b_past_width":                              # one 8-element chunk further along k; A supplies zeros there
        if case.b_t:
            b = raw_load(v["b"], br + 8, bc, ld["b"])
            a = torch.cat([a, torch.zeros(8, ac)], 0) if case.a_t else torch.cat([a, torch.zeros(ar, 8)], 1)
        else:
            b = raw_load(v["b"], br, bc + 8, ld["b"])
            a = torch.cat([a, torch.zeros(8, ac)], 0) if case.a_t else torch.cat([a, torch.zeros(ar, 8)], 1)
    else:
        b = raw_load(v["b"], br, bc, ld["b"])
    a_op, b_op = (a.T if case.a_t else a), (b if case.b_t else b.T)
    if fault == "drop_ragged_k" and K % 64 and K > 64:
        a_op, b_op = a_op[:, :K - K % 64], b_op[:K - K % 64]
    acc = a_op @ b_op
    w = {}
    for name, cols in (("pre", N), ("dact", N), ("glu", 2 * N)):
        if name in v:
            w[name] = raw_load(v[name], M, cols, ld[name])
    if case.res is not None:
        w["res"] = raw_load(v["res"], M, N, ld["c"] if fault == "res_uses_ldc" else ld["res"])
    if "bias" in v:
        w["bias"] = v["bias"].float()
    if case.gate is not None:
        w["gate"] = v["gate"].float() if case.gate[0] == 0 else raw_load(v["gate"], gate_rows(case), N, ld["gate"])
    out = _epilogue(case, acc, w, gate_div=M if fault == "gate_row_by_m" else None)
    if "aux" in out:
        raw_store(v["aux"], out["aux"], ld["c"] if fault == "aux_uses_ldc" else ld["aux"])
    c = out["c"].float()
    if fault == "past_n":
        c = torch.cat([c, torch.zeros(M, 4)], 1)
    if fault == "eight_where_four" and N % 8 == 4:
        c = torch.cat([c, torch.zeros(M, 4)], 1)
    if fault == "row_m":
        c = torch.cat([c, torch.zeros(1, c.shape[1])], 0)
    raw_store(v["c"], c, ld["c"])
    if case.rowsum is not None:
        s = a_op.sum(1)
        s = rb(s) + v["rowsum"].float() if case.rowsum == "acc" else s
        if fault == "rowsum_writes_m":
            s = torch.cat([s, torch.zeros(1)])
        raw_store(v["rowsum"], s[None, :], 0)
