"""Exact inputs for the text-row kernels -- the row norms on csrc/rownorm_lpr.hpp (yat_gemma_rmsnorm, yat_t5_rmsnorm,
yat_dcae_rmsnorm_bias), clip_layernorm_kernel, rope_qk, geglu, embed_rows, clip_embed -- their references, the case lists of
test_textrow_exact_gpu.py and a Python restatement of the host dispatch.  Nothing here touches yat_amd or a GPU.

The norms, eps = 0 (every entry point accepts eps >= 0).  A row is  mu + sign * mag * 2^k  (mu = 0 for the RMS norms; k per
row in 0 .. 3) in one of two families:
  * "pow4": mag = 1.  The sum of squares is D 4^k, an exact fp32 integer in any order; the mean square is a power of 4 and
    1 / sqrtf of it the exact power of two 2^-k; x * rs is +-1.  Weights are dyadics, so each epilogue's value is known
    exactly and is rounded ONCE by the store (the CPU file asserts that no such value sits on a rounding tie).
  * "five": half of a row's entries have mag = 7, half mag = 1 (LayerNorm: a quarter of the row for each sign, so the mean
    stays mu).  The mean square is 25 4^k and its root 5 2^k, both exact; rs = fl(1 / 5) 2^-k comes from one correctly rounded
    fp32 division, and x * rs is NOT a bf16 number: T5's two roundings differ from one, DC-AE's four from fewer.
``expected_*`` restate each module with every rounding point in place: fp32 where the kernel holds fp32, bf16 where the module
rounds.  They are numpy, element by element in the order of the formula; the reductions they need are exact integers.

``lpr_of`` restates launch_rownorm_lpr / yat_clip_layernorm: lanes per row = the largest power of two dividing D / 8, at most
64; 256 / lpr rows per block.  ``NORM_D`` reaches D / 8 with lowest set bit 1, 2, .. 64 and 128 (the capped class), the
per-lane chunk loop running once and several times, and D = 8; ``norm_rows`` gives M = 1, rpb - 1, rpb, rpb + 1, 2 rpb + 1.
"""
import numpy as np
import torch

BF = torch.bfloat16
F32 = np.float32


def rbf(a):
    """fp32 / fp64 numpy -> the nearest bf16 (ties to even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(BF).float().numpy()


def to_bf(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    r = t.to(BF)
    assert torch.equal(r.double(), t), "not exact in bf16"
    return r


def on_tie(t):
    """True where the fp64 value lies exactly between two bf16 numbers"""
    m, _ = np.frexp(np.abs(np.asarray(t, dtype=np.float64)))
    return (m * 512.0) % 2.0 == 1.0                 # 8 significant bits kept: the 9th set and nothing below it


# ------------------------------------------------------------------------------------------------- host dispatch
def lpr_of(D):
    lpr = 1
    while lpr < 64 and ((D >> 3) % (lpr * 2)) == 0:
        lpr *= 2
    return lpr


def chunk_passes(D):
    return (D >> 3) // lpr_of(D)


NORM_D = (8, 24, 48, 96, 192, 384, 768, 512, 1536, 1024)       # lpr 1, 1, 2, 4, 8, 16, 32, 64, 64, 64


def norm_rows(D):
    rpb = 256 // lpr_of(D)
    return sorted({1, max(rpb - 1, 1), rpb, rpb + 1, 2 * rpb + 1})


# ------------------------------------------------------------------------------------------------- the norms
def rows(M, D, family, seed, centered=False):
    """-> (s [M, D] float64: the normed rows, exact in bf16; mu [M, 1]; k [M, 1])"""
    g = np.random.default_rng(seed)
    k = g.integers(0, 4, size=(M, 1))
    mu = g.integers(-5, 6, size=(M, 1)).astype(np.float64) if centered else np.zeros((M, 1))
    if family == "pow4":
        base = np.array([1.0, -1.0] * (D // 2))
    else:
        base = np.array(([7.0, -7.0] * (D // 4) + [1.0, -1.0] * (D // 4)))
    d = np.stack([g.permutation(base) for _ in range(M)])
    if not centered:
        d = d * g.choice([-1.0, 1.0], size=(M, D))
    return mu + d * 2.0 ** k, mu, k


def rstd(s, mu=0.0):
    """fp32 1 / sqrtf(sum((s - mu)^2) / D) as the kernels compute it (eps = 0): the sum is an exact integer"""
    D = s.shape[1]
    ss = ((s - mu) ** 2).sum(-1, keepdims=True)
    assert ss.max() < 2 ** 24 and np.array_equal(ss, np.round(ss))
    return F32(1.0) / np.sqrt(ss.astype(F32) / F32(D))


def weights(D, seed, fine=False):
    g = np.random.default_rng(seed + 1000)
    if fine:                                          # Gemma: 1 + w has 10 or 11 significant bits, never on a bf16 tie
        m = g.integers(-255, 256, size=D)
        m = np.where(on_tie(1.0 + m / 1024.0), m + 1, m)
        return m / 1024.0
    return g.integers(-64, 65, size=D) / 32.0


def coarse(shape, seed):
    """multiples of 1/32 in [-2, 2]"""
    return np.random.default_rng(seed + 2000).integers(-64, 65, size=shape) / 32.0


def split_residual(s, seed):
    """x, res with x + res = s exactly (all three integers, exact in bf16)"""
    res = np.random.default_rng(seed + 3000).integers(-6, 7, size=s.shape).astype(np.float64)
    return s - res, res


def expected_gemma(s, w, res=None):
    """Gemma2RMSNorm: bf16(x rs (1 + w)), ONE rounding; with a residual bf16(res + bf16(.))"""
    v = (s.astype(F32) * rstd(s)).astype(F32)
    t = (v * (F32(1.0) + w.astype(F32))).astype(F32)
    if res is not None:
        t = (res.astype(F32) + rbf(t)).astype(F32)
    return t                                          # (the store rounds once more)


def expected_t5(s, w):
    """T5LayerNorm: bf16(w bf16(x rs)), TWO roundings"""
    v = (s.astype(F32) * rstd(s)).astype(F32)
    return (w.astype(F32) * rbf(v)).astype(F32)


def expected_t5_one_rounding(s, w):
    v = (s.astype(F32) * rstd(s)).astype(F32)
    return (w.astype(F32) * v).astype(F32)


def expected_dcae(s, w, bias=None, res=None, relu=False):
    """diffusers RMSNorm of DC-AE: the normalised value, the weight product, the bias add and the residual add each rounded"""
    v = (s.astype(F32) * rstd(s)).astype(F32)
    t = rbf(rbf(v) * w.astype(F32))
    if bias is not None:
        t = rbf(t + bias.astype(F32))
    if res is not None:
        t = rbf(t + res.astype(F32))
    if relu:
        t = np.maximum(t, F32(0.0))
    return t


def expected_layernorm(s, mu, w, b):
    """nn.LayerNorm: bf16(fma((x - mean) rs, w, b)), ONE rounding (mean = mu exactly: the sum is an exact integer)"""
    assert np.array_equal(s.sum(-1, keepdims=True), mu * s.shape[1])
    a = ((s - mu).astype(F32) * rstd(s, mu)).astype(F32)
    return (a.astype(np.float64) * w + b).astype(F32)           # one fp32 rounding: the fp64 sum of a 32-bit product is exact


# ------------------------------------------------------------------------------------------------- rope_qk
ROPE_CASES = [(16, 3, 1, 8, (5, 1, 7)), (64, 5, 2, 24, (9, 4)), (256, 2, 1, 40, (3, 0, 6)), (64, 37, 3, 0, (70, 21)),
              (16, 2, 2, 16, (33, 1, 31))]          # (dh, heads rotated, head blocks left alone, slack columns, prompt lengths)


def rope_case(dh, heads, vheads, slack, lens, seed=0):
    """-> x [rows, ld] small integers with the v block and the slack columns as guards, positions restarting per prompt,
    cos / sin tables [max_len, dh] from {0, +-1, +-1/2}: every product and both sums are exact in bf16"""
    g = np.random.default_rng(seed + dh)
    n, max_len = sum(lens), max(lens)
    ld = (heads + vheads) * dh + slack
    x = g.integers(-8, 9, size=(n, ld)).astype(np.float64)
    pos = np.concatenate([np.arange(L) for L in lens]).astype(np.int32)
    vals = np.array([0.0, 1.0, -1.0, 0.5, -0.5])
    cos, sin = vals[g.integers(0, 5, size=(max_len, dh))], vals[g.integers(0, 5, size=(max_len, dh))]
    return x, pos, cos, sin, ld


def rope_ref(x, pos, cos, sin, heads, dh):
    """apply_rotary_pos_emb: x cos + rotate_half(x) sin on the first ``heads`` blocks, rotate_half(x) = cat(-x2, x1)"""
    out = x.copy()
    half = dh // 2
    for h in range(heads):
        blk = x[:, h * dh:(h + 1) * dh]
        rot = np.concatenate([-blk[:, half:], blk[:, :half]], axis=1)
        out[:, h * dh:(h + 1) * dh] = blk * cos[pos] + rot * sin[pos]
    return out


# ------------------------------------------------------------------------------------------------- geglu
GEGLU_CASES = [(1, 8, 8, 0), (3, 24, 16, 8), (37, 56, 24, 40), (5, 2056, 8, 16)]      # (M, N, gap and slack of ld, slack of ldo)


def geglu_case(M, N, seed=0):
    g = torch.Generator().manual_seed(seed + M * N)
    gate = (torch.randn(M, N, generator=g) * 2.0).to(BF)
    gate.view(-1)[:6] = torch.tensor([0.0, -0.0, 40.0, -40.0, 9.0, -9.0][:min(6, M * N)], dtype=BF)[:M * N]
    up = (torch.randint(-32, 33, (M, N), generator=g).float() / 8).to(BF)
    return gate, up


# ------------------------------------------------------------------------------------------------- embeddings
EMBED_CASES = [(1, 8, 3), (5, 8, 7), (37, 72, 11), (33, 200, 5)]                     # (rows, D, vocab)


def embed_case(nrows, D, vocab, npos=0, seed=0):
    g = torch.Generator().manual_seed(seed + nrows * D)
    table = torch.randn(vocab, D, generator=g).to(BF)
    ids = torch.randint(0, vocab, (nrows,), generator=g, dtype=torch.int32)
    ids[0], ids[-1] = 0, vocab - 1
    if nrows > 2:
        ids[1] = vocab - 1
    out = dict(table=table, ids=ids)
    if npos:
        out["ptab"] = torch.randn(npos, D, generator=g).to(BF)
        pos = torch.randint(0, npos, (nrows,), generator=g, dtype=torch.int32)
        pos[0], pos[-1] = npos - 1, 0
        out["pos"] = pos
    return out
