"""Plain references, exact inputs and case lists for the "glue" kernels (csrc/elementwise.hip, csrc/pixart_ops.hip and the row
routing of csrc/mmdit_ops.hip).  No GPU code is imported here: test_glue_ref_cpu.py proves on the CPU what
test_glue_exact_gpu.py relies on, and the GPU file compares the kernels with what this file computes -- never with
another run of a kernel.

Inputs are chosen so that the expected bits are known without device arithmetic:
  * copies carry int16 bits ``i mod 65521`` (NaN patterns, -0 and denormals included) and are compared as int16;
  * sums use position-dependent small integers, so every fp32 sum is exact in any order;
  * the activations see "saturated" integers only (``[32, 255]`` and ``[-255, -128]``), where the library's fp32 formulas
    give exactly x or -0 (the function) and 1 or -0 (the derivative);
  * rounding chains (flow_mix, ddpm_add_noise, mse_bf16_chunk, dropout) need real-valued inputs and are restated in fp32
    with a bf16 rounding after each op;
  * the dropout mask is splitmix64 in numpy uint64.
The case lists name the smallest shapes that reach each launch class; the ``*_classes`` functions replay the launch
arithmetic of the sources (256 threads per workgroup and the grid caps below).
"""
import math

import numpy as np
import torch

BF = torch.bfloat16
MOD = 65521                          # largest prime below 2^16: the copy pattern never lines up with a power-of-two stride
CANARY = 0x7FC1                      # a bf16 NaN no kernel produces
GUARD = 0x7F80 | 0x55                # input guard (a NaN): rows and columns no kernel may read as data

# grid caps restated from the sources (workgroups of 256 threads)
EW_CAP, PIX_CAP, JOINT_CAP, MSE_CAP, QKNORM_CAP = 2048, 4096, 8192, 256, 1024


# ------------------------------------------------------------------------------------------------ bits
def as_i16(a):
    """numpy integers (any width, taken mod 2^16) -> torch int16 bits"""
    return torch.from_numpy((np.asarray(a).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16).copy())


def pattern(n, start=0):
    """int16 bits ``(start + i) mod 65521`` of a copy operand"""
    return as_i16((np.arange(n, dtype=np.int64) + start) % MOD)


def fold(b):
    """bf16 bits (int16) with -0 folded onto +0"""
    return torch.where(b == -32768, torch.zeros_like(b), b)


def bf_bits(t):
    """bf16 tensor -> int16 bits"""
    return t.contiguous().view(torch.int16)


def rb(t):
    return t.to(BF).float()


def ints_bf(v):
    """small integers (numpy) -> bf16; |v| <= 256 is exact"""
    v = np.asarray(v)
    assert np.abs(v).max(initial=0) <= 256
    return torch.from_numpy(v.astype(np.float32)).to(BF)


def randn_bf(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ launch arithmetic
def grid_blocks(items, cap):
    return max(1, min(cap, (items + 255) // 256))


def stride_classes(items, cap):
    """a grid-stride loop over ``items`` work items: workgroups, passes of the slowest thread, whether the last pass is ragged"""
    g = grid_blocks(items, cap)
    per = g * 256
    return dict(blocks=g, passes=-(-items // per), ragged=items % per != 0, capped=(items + 255) // 256 > cap)


def ew_classes(n):
    c = stride_classes(n >> 3, EW_CAP)
    c.update(vectors=n >> 3, tail=n & 7)
    return c


def mse_classes(n):
    nb = min(MSE_CAP, (n + 255) // 256)
    return dict(blocks=nb, passes=-(-n // (nb * 256)), ragged=n % (nb * 256) != 0, final_passes=-(-nb // 64))


def text_classes(B, T, C, rows=None):
    """pad_mask / pack_mask: one wave per row, four rows per workgroup, 64 lanes walk C / 8 chunks"""
    rows = B * T if rows is None else rows
    return dict(chunks=C >> 3, chunk_passes=-(-(C >> 3) // 64), ragged_chunks=(C >> 3) % 64 != 0, rows_mod4=rows % 4)


# ------------------------------------------------------------------------------------------------ ew_kernel
EW_N = [1, 7, 8, 9, 2048 * 8 + 3, 4194304, 4194304 + 8, 4194304 + 8 * 257 + 5, 3 * 4194304 + 13]
ACTS = ("silu", "gelu_tanh")


def saturated(n, start=0):
    """position-dependent integers in [32, 255] and [-255, -128] (float64 numpy)"""
    v = (np.arange(n, dtype=np.int64) + start) % 352
    return np.where(v < 224, 32 + v, -128 - (v - 224)).astype(np.float64)


def ew_case(n):
    """x (saturated), dy (integers in [-6, 6]) and the expected bits of act(x) and dy * act'(x), -0 folded"""
    x = saturated(n)
    dy = ((np.arange(n, dtype=np.int64) * 7) % 13 - 6).astype(np.float64)
    fwd = np.where(x > 0, x, 0.0)
    bwd = np.where(x > 0, dy, 0.0)
    return ints_bf(x), ints_bf(dy), fold(bf_bits(ints_bf(fwd))), fold(bf_bits(ints_bf(bwd)))


def add_case(n):
    i = np.arange(n, dtype=np.int64)
    a, b = i % 97 - 48, (i * 5) % 61 - 30
    return ints_bf(a), ints_bf(b), fold(bf_bits(ints_bf(a + b)))


# fp32 model of the four activation formulas of csrc/common.hpp in numpy: exp, exp2 and the reciprocal are correctly
# rounded here where the device uses 1-ulp instructions; fma(a, b, c) is the product in fp64 (exact) plus c, rounded once
F32 = np.float32


def _fma(a, b, c):
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(F32)


def _rcp(x):
    with np.errstate(all="ignore"):
        return (F32(1.0) / x).astype(F32)


def m_sigmoid(x):
    with np.errstate(all="ignore"):
        return _rcp(F32(1.0) + np.exp(-x).astype(F32))


def m_gate(x):
    k0x2, k1 = F32(2.0) * F32(0.7978845608028654), F32(0.044715)
    with np.errstate(all="ignore"):
        u2 = (k0x2 * x) * _fma(k1 * x, x, 1.0)
        return _rcp(F32(1.0) + np.exp2(F32(-1.4426950408889634) * u2).astype(F32))


def model_f32(name, x, clamp=True, fused=True):
    """the library's fp32 formula ``name`` in {silu, dsilu, gelu_tanh, dgelu_tanh} on float32 x (before the bf16 rounding);
    ``clamp`` False is dgelu_tanh_f as it was before -inf was kept out of the product with s = 0; ``fused`` False is dsilu
    as written, 1 + x (1 - s) with a rounded product (the compiler is free to contract it into an fma or not)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        if name == "silu":
            return x * m_sigmoid(x)
        if name == "dsilu":
            s = m_sigmoid(x)
            return s * (_fma(x, F32(1.0) - s, 1.0) if fused else F32(1.0) + x * (F32(1.0) - s))
        if name == "gelu_tanh":
            return x * m_gate(x)
        k0x2, k1x3 = F32(2.0) * F32(0.7978845608028654), F32(3.0) * F32(0.044715)
        s = m_gate(x)
        t = _fma(x * (F32(1.0) - s), k0x2 * _fma(k1x3 * x, x, 1.0), 1.0)
        if clamp:
            t = np.where(t == -np.inf, -np.finfo(F32).max, t).astype(F32)
        return s * t


def ref_f64(name, x):
    """fp64 reference without cancellation: gelu = x / (1 + exp(-2u)); the derivatives from the gate and 1 / (1 + exp(2u))"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        if name in ("silu", "dsilu"):
            s, c = 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))           # sigmoid and 1 - sigmoid
            if name == "silu":
                return x * s
            return s + np.where(c == 0, 0.0, x * s * c)
        u2 = 2.0 * 0.7978845608028654 * x * (1.0 + 0.044715 * x * x)
        s, c = 1.0 / (1.0 + np.exp(-u2)), 1.0 / (1.0 + np.exp(u2))
        if name == "gelu_tanh":
            return np.where(s == 0, 0.0, x * s)
        du2 = 2.0 * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * x * x)
        tail = x * du2                                                          # finite for every finite bf16 x in fp64
        return s + np.where((s == 0) | (c == 0), 0.0, tail * s * c)


def all_bf16():
    """every bf16 bit pattern as (int16 bits tensor, float32 numpy values)"""
    u = np.arange(65536, dtype=np.uint32)
    return as_i16(u), (u << 16).view(F32)


def ulp_bf16(ref):
    """spacing of bf16 at |ref| (float64 numpy); denormal spacing 2^-133 below 2^-126"""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, np.maximum(np.where(np.asarray(ref) == 0, -1000, e) - 8, -133))


BF16_MAX = float(np.ldexp(255.0, 120))           # 3.3895e38
ACT_ABS = 2.0 ** -30                             # absorbs fp32 flush-to-zero of results below 1e-37


def act_excess(name, dy=1.0, fused=True):
    """largest distance, in bf16 ulps of the reference, of the numpy fp32 model from the fp64 reference over every finite
    bf16 input whose reference is in bf16's range -> (excess, x at the worst input)"""
    _, x = all_bf16()
    ok = np.isfinite(x)
    ref = dy * ref_f64(name, x)
    with np.errstate(all="ignore"):
        got = (F32(dy) * model_f32(name, x, fused=fused)).astype(np.float64)
        ok &= (np.abs(ref) <= BF16_MAX) & np.isfinite(got)
        d = np.where(ok, (np.abs(got - ref) - ACT_ABS) / ulp_bf16(ref), 0.0)
    k = int(np.argmax(d))
    return float(max(d[k], 0.0)), float(x[k])


ACT_MODELS = (("silu", 1.0), ("gelu_tanh", 1.0), ("dsilu", 1.0), ("dsilu", -3.0), ("dsilu", 1.0, False), ("dsilu", -3.0, False),
              ("dgelu_tanh", 1.0), ("dgelu_tanh", -3.0))
_M = []


def act_margin():
    """m of the sweep's bound (0.5 + m) ulp_bf16(ref) + 2^-30: 8 x the largest excess of the fp32 model over the reference
    (8 for v_exp_f32 and v_rcp_f32 being 1-ulp instructions where numpy rounds correctly)"""
    if not _M:
        _M.append(8.0 * max(act_excess(*a)[0] for a in ACT_MODELS))
    return _M[0]


def torch_f32(name, x):
    """torch's own fp32 CPU result (forward, or backward with dy = 1) for float32 numpy x"""
    import torch.nn.functional as Fn
    f = Fn.silu if "silu" in name else (lambda t: Fn.gelu(t, approximate="tanh"))
    t = torch.from_numpy(np.asarray(x, dtype=F32).copy()).requires_grad_(True)
    y = f(t)
    if not name.startswith("d"):
        return y.detach().numpy()
    y.backward(torch.ones_like(y))
    return t.grad.numpy()


# ------------------------------------------------------------------------------------------------ f32_to_bf16
F32_LOW = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
F32_N = [1, 524288, 524289]


def rne_table():
    """every upper half x the six lower halves -> (uint32 inputs, expected uint16 bits from integer arithmetic, NaN mask)"""
    hi = np.repeat(np.arange(65536, dtype=np.uint64), len(F32_LOW))
    lo = np.tile(np.array(F32_LOW, dtype=np.uint64), 65536)
    u = (hi << np.uint64(16)) | lo
    nan = ((u >> np.uint64(23)) & np.uint64(0xFF) == 0xFF) & (u & np.uint64(0x7FFFFF) != 0)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return u.astype(np.uint32), (r & np.uint64(0xFFFF)).astype(np.uint16), nan


def rne_case(n):
    """n inputs drawn from the table at a stride coprime to its length"""
    u, r, nan = rne_table()
    idx = (np.arange(n, dtype=np.int64) * 7919 + 5) % u.shape[0]
    return u[idx], r[idx], nan[idx]


# ------------------------------------------------------------------------------------------------ flow_mix / ddpm
FLOW_CASES = [(1, 1), (5, 280), (3, 174763)]                     # the last: 524,289 elements, one in the second pass
DDPM_CASES = [(1, 1), (5, 280), (3, 349526)]                     # the last: 1,048,578 elements, two in the second pass
COEFS = [0.957, 1.0, 0.0, 0.5117, 0.003]


def mix_case(B, per, seed=0):
    x, nz = randn_bf(B * per, 60 + seed, 0.5).view(B, per), randn_bf(B * per, 61 + seed).view(B, per)
    ca = torch.tensor([COEFS[(b + 1) % 5] for b in range(B)]).to(BF)
    cb = torch.tensor([COEFS[(b + 2) % 5] for b in range(B)]).to(BF)
    return x, nz, ca, cb


def flow_ref(x, nz, sigma):
    s = sigma.float()[:, None]
    noisy = rb(rb(rb(1.0 - s) * x.float()) + rb(s * nz.float()))
    return noisy.to(BF), rb(nz.float() - x.float()).to(BF)


def ddpm_ref(x, nz, ca, cb):
    return rb(rb(ca.float()[:, None] * x.float()) + rb(cb.float()[:, None] * nz.float())).to(BF)


# ------------------------------------------------------------------------------------------------ mse
MSE_N = [1, 255, 256, 257, 65536, 65537, 3 * 65536 + 77, 2 ** 18]
MSE_GSCALE = (1.0, 0.25)
MSE_CHUNK = [(7, 5, 11), (2, 1024, 2048), (4, 16384, 16384), (3, 16384, 32768)]


def mse_case(n):
    """pred, target (integers), d = pred - target with |d| <= 8 and the exact sum of squares"""
    i = np.arange(n, dtype=np.int64)
    d = (i * 5 + i // 256) % 17 - 8
    t = i % 31 - 15
    return ints_bf(t + d), ints_bf(t), d, int((d * d).sum())


def ulp32(v):
    _, e = np.frexp(np.abs(np.float64(v)))
    return np.ldexp(1.0, np.maximum(np.where(np.float64(v) == 0, -1000, e) - 24, -149))


def pow2(v):
    return v > 0 and math.frexp(v)[0] == 0.5


def _rbf_np(v):
    """float32 numpy -> rounded to bf16, back in float32 (RNE; finite inputs)"""
    u = np.asarray(v, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(F32)


def chunk_case(B, used, stride, real, seed=0):
    """pred [B, stride], target [B, used]: integers (sums exact) or real values (the rounding chain)"""
    if real:
        return randn_bf(B * stride, 70 + seed).view(B, stride), randn_bf(B * used, 71 + seed).view(B, used)
    i = np.arange(B * stride, dtype=np.int64).reshape(B, stride)
    j = np.arange(B * used, dtype=np.int64).reshape(B, used)
    t = j % 31 - 15
    p = i % 23 - 11
    p[:, :used] = t + ((j * 5 + j // 256) % 9 - 4)               # |d| <= 4 in the used half, anything in the other
    return ints_bf(p), ints_bf(t)


def chunk_ref(pred, target, gscale):
    """the fp32 restatement of torch's bf16 MSELoss on pred[:, :used] with a bf16 rounding after each op
    -> (dpred bf16 [B, stride], fp64 sum of the rounded squares, loss as the library's final kernel rounds it)"""
    B, stride = pred.shape
    used = target.shape[1]
    n = B * used
    d = rb(pred[:, :used].float() - target.float())
    sq = rb(d * d)
    norm_b, g_b = float(_rbf_np(F32(2.0) / F32(n))), float(_rbf_np(F32(gscale)))
    dp = torch.zeros(B, stride)
    dp[:, :used] = rb(norm_b * d) * g_b
    S = float(sq.double().sum())
    loss = float(_rbf_np(F32(S) * (F32(1.0) / F32(n))))          # exact when S is (integer inputs)
    return dp.to(BF), S, loss


# ------------------------------------------------------------------------------------------------ dropout
DROP_N = [1, 255, 524288, 524289, 3 * 524288 + 5]
DROP_P = [0.0, 2.0 ** -24, 0.3, 1.0 - 2.0 ** -24]
DROP_SEEDS = [0, 12345, 2 ** 63 + 7, 2 ** 64 - 1]
M64 = (1 << 64) - 1


def splitmix_py(seed, i):
    """the documented hash of (seed, element index) in pure-Python integers -> the 24 bits compared with the threshold"""
    z = (i + seed * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 40


def splitmix_np(seed, n, start=0):
    with np.errstate(over="ignore"):
        i = np.arange(start, start + n, dtype=np.uint64)
        z = i + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (z >> np.uint64(40)).astype(np.uint32)


def drop_thresh(p):
    return int(F32(p) * F32(16777216.0))


def drop_keep(seed, n, p):
    return torch.from_numpy(splitmix_np(seed, n) >= np.uint32(drop_thresh(p)))


def drop_inputs(n):
    x, g, io = randn_bf(n, 80), randn_bf(n, 81), randn_bf(n, 82)
    one = torch.ones((), dtype=BF)
    return torch.where(x == 0, one, x), torch.where(g == 0, one, g), io      # x, g nonzero: "dropped" and "zero" coincide


def drop_ref(x, io, keep, p):
    """forward bf16(x * inv_keep) or 0; backward_add bf16(io + that)"""
    inv_keep = float(F32(1.0) / (F32(1.0) - F32(p)))
    v = torch.where(keep, rb(x.float() * inv_keep), torch.zeros(()))
    return v.to(BF), (v + io.float()).to(BF)


# ------------------------------------------------------------------------------------------------ pad_mask / pack_mask
TEXT_C = [8, 504, 512, 520, 1032]                                # 1, 63, 64, 65 and 129 chunks
TEXT_BT = [(1, 5, [8]), (2, 3, [0, 3]), (3, 5, [1, 8, 5]), (4, 3, [3, 0, 6, 3])]     # lengths 0, 1, T and T + 3


def pack_rows_padded(B, T, lens):
    """rows_padded <, = and > B * T, each with offsets[B] = and < rows_padded where that can be"""
    total, bt = sum(lens), B * T
    return sorted({r for r in (total, total + 2, bt, bt + 3, max(total, bt - 1)) if r >= total and r > 0})


def text_case(B, T, C, lens, rows_padded=None):
    """source rows (pattern; two guard rows behind offsets[B]), offsets and the expected dst / mask / key bias / kv_len.
    rows_padded None: the padded [B * T, C] layout of pad_mask; else the packed layout of pack_mask."""
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    total = int(offs[-1])
    src = pattern((total + 2) * C, 17).view(total + 2, C).clone()
    src[total:] = np.int16(GUARD)
    if rows_padded is None:
        dst = torch.zeros(B * T, C, dtype=torch.int16)
        for b, L in enumerate(lens):
            k = min(L, T)
            dst[b * T:b * T + k] = src[offs[b]:offs[b] + k]
    else:
        dst = torch.zeros(rows_padded, C, dtype=torch.int16)
        dst[:total] = src[:total]
    mask = torch.tensor([[1 if t < L else 0 for t in range(T)] for L in lens], dtype=torch.int64).view(-1)
    bias = torch.where(mask == 1, torch.zeros(()), torch.full((), -9984.0))        # bf16(-10000) = -9984
    kvl = torch.tensor([min(L, T) for L in lens], dtype=torch.int32)
    return src, torch.from_numpy(offs), dst, mask, bias, kvl


# ------------------------------------------------------------------------------------------------ patch_rearrange
PATCH_CASES = [(2, C, 3 * p, 5 * p, p) for p in (1, 2, 4) for C in (1, 3, 4)] + [(1, 4, 514, 514, 2)]


def patch_ref(img, p, channel_major):
    """[B, C, H, W] -> token rows [B * h * w, C * p * p] by a plain permutation"""
    B, C, H, W = img.shape
    h, w = H // p, W // p
    v = img.view(B, C, h, p, w, p)
    v = v.permute(0, 2, 4, 1, 3, 5) if channel_major else v.permute(0, 2, 4, 3, 5, 1)
    return v.reshape(B * h * w, C * p * p).contiguous()


def unpatchify_ref(tok, B, C, H, W, p):
    """the reference's "nhwpqc->nchpwq" without einops"""
    h, w = H // p, W // p
    return tok.view(B, h, w, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W).contiguous()


# ------------------------------------------------------------------------------------------------ add_pos_embed
POS_CASES = [(5, 5, 8), (15, 5, 8), (7, 7, 1152), (21, 7, 1152), (7282, 331, 1152)]      # (rows, N, D)


def pos_case(rows, N, D):
    """x: integers of magnitude in [130, 190] (bf16 spacing 1 there); pos = k + 0.5: every sum is a tie, rounded to even"""
    r, c = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(D, dtype=np.int64), indexing="ij")
    x = (130 + (r * 7 + c) % 61) * np.where((r + c) % 3 == 0, -1, 1)
    pn, pc = np.meshgrid(np.arange(N, dtype=np.int64), np.arange(D, dtype=np.int64), indexing="ij")
    pos = ((pn * 3 + pc) % 17).astype(np.float32) + np.float32(0.5)
    s = x.astype(np.float32).reshape(rows // N, N, D) + pos[None]               # exact in fp32
    want = torch.from_numpy(s.reshape(rows, D)).to(BF)
    return ints_bf(x), torch.from_numpy(pos), want, s.reshape(rows, D)


# ------------------------------------------------------------------------------------------------ joint_rows
JOINT_CASES = [(2, 5, T, C) for C in (8, 1536) for T in (0, 1, 154)] + [(3, 1025, 154, 4800)]


def joint_case(B, N, T, C):
    img = pattern(B * N * C, 3).view(B * N, C)
    txt = pattern(B * T * C, 40000).view(B * T, C)
    joint = torch.cat([img.view(B, N, C), txt.view(B, T, C)], 1).reshape(B * (N + T), C)
    return img, txt, joint


# ------------------------------------------------------------------------------------------------ qknorm_concat
QKNORM_CASES = [(1, 1, 0, 1, 32), (2, 700, 330, 1, 32), (2, 24, 10, 2, 64), (1, 17, 5, 2, 128)]
QKNORM_DX_REL, QKNORM_DW_REL = 4e-3, 6e-3          # the bounds of test_sd3_gpu.py::test_qknorm_concat_fwd_bwd


def rms_ref(x, w, eps, dt):
    """diffusers RMSNorm [RECALL]: fp32 statistics and normalisation, cast to the weight dtype, then * weight."""
    v = x.float().pow(2).mean(-1, keepdim=True)
    y = x.float() * torch.rsqrt(v + eps)
    if dt == BF:
        y = y.to(BF)
    return (y * w.to(dt)).to(dt)


def qknorm_concat_ref(qkv_i, qkv_t, ws, B, N, T, H, dh, eps, dt):
    """[RMSNorm_head(q) | RMSNorm_head(k) | v] of the image rows, then the text rows, per image, on the CPU in ``dt``
    -> (joint [B * (N + T), 3D], [image leaf, text leaf], weight leaves): leaves for autograd"""
    D, L = H * dh, N + T
    xi = qkv_i.to(dt).cpu().view(B, N, 3, H, dh).requires_grad_(True)
    parts = [xi]
    w = [t.cpu().to(dt).requires_grad_(True) for t in ws]
    q = [rms_ref(xi[:, :, 0], w[0], eps, dt)]
    k = [rms_ref(xi[:, :, 1], w[1], eps, dt)]
    v = [xi[:, :, 2]]
    if T:
        xt = qkv_t.to(dt).cpu().view(B, T, 3, H, dh).requires_grad_(True)
        parts.append(xt)
        q.append(rms_ref(xt[:, :, 0], w[2], eps, dt)); k.append(rms_ref(xt[:, :, 1], w[3], eps, dt)); v.append(xt[:, :, 2])
    out = torch.stack([torch.cat(q, 1), torch.cat(k, 1), torch.cat(v, 1)], dim=2)      # [B, L, 3, H, dh]
    return out.reshape(B * L, 3 * D), parts, w


QKNORM_EPS = 1e-6
TIE_MARGIN = 2.0 ** -9               # of a bf16 ulp: 2^-17 relative or more, 16 x what an fp32 evaluation of rstd is off by


def tie_distance(x, dh, eps=QKNORM_EPS):
    """distance of every x * rstd (fp64 statistics over heads of dh) from the nearest tie between two bf16 numbers, in bf16 ulps"""
    x = x.double().reshape(-1, dh)
    y = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)).numpy()
    u = np.abs(y) / ulp_bf16(y)
    return np.abs(u - np.floor(u) - 0.5)


def qknorm_inputs(rows, D, seed, start, dh=None):
    """[rows, 3D]: real-valued q | k, the copy pattern in the v section.  With ``dh`` (the forward's operands) no normalised
    element x * rstd lies within TIE_MARGIN of a tie between two bf16 numbers: an element that does moves one bf16 step
    away from zero, until none is left.  The bf16 the kernel must store is then the same whatever order the fp32 sum of
    squares runs in and however the last bit of rsqrt falls, so the forward is compared bit for bit."""
    t = randn_bf(rows * 3 * D, seed).view(rows, 3 * D).clone()
    if dh is not None:
        qk = t[:, :2 * D].contiguous()
        for _ in range(20):
            near = torch.from_numpy(tie_distance(qk, dh) < TIE_MARGIN).view(qk.shape)
            if not near.any():
                break
            b = qk.view(torch.int16)
            b[near] += 1                                           # one step away from zero (no element is near the top)
        t[:, :2 * D] = qk
    t[:, 2 * D:] = pattern(rows * D, start).view(rows, D).view(BF)
    return t


# ------------------------------------------------------------------------------------------------ timestep_embed
TSTEP_CASES = [(1, 2), (5, 256), (3, 170), (9, 1000)]
TSTEP_T = [0.0, 2.9940121, 957.3083, 510.554, 1000.0, 0.5, 37.25, 999.0, 250.0]


def tstep_ref(t, dim):
    """[cos | sin] of t * exp(-ln(10000) j / half): frequency and argument rounded to fp32 as the kernel forms them,
    cos and sin in fp64"""
    half = dim // 2
    j = np.arange(half, dtype=F32)
    freq = np.exp((F32(-math.log(10000.0)) * j / F32(half)).astype(F32)).astype(F32)
    arg = (np.asarray(t, dtype=F32)[:, None] * freq[None]).astype(np.float64)
    return torch.from_numpy(np.concatenate([np.cos(arg), np.sin(arg)], 1))
