"""Selector inputs for softmax attention (csrc/sdpa.hip), their plain fp64 reference, the case lists of
test_sdpa_exact_gpu.py and a Python restatement of the host dispatch.  Nothing here touches yat_amd or a GPU.

Selector inputs (``build``): per (image, head) the head's columns are dealt three roles -- every ``period``-th column
(period 2 for dh <= 16, else 3; the phase moves with the seed, the image and the head) is a *code* column, one of those the
*constant* column, the rest are *free*.
  * A live key carries the +-1 code of its group id on the code columns (bit i mod nb on the i-th), an integer ``kc`` on
    the constant column and small integers (-3 .. 3) on the free columns, so that the keys of one group differ although
    their scores tie.  Groups have 1, 2 or 4 members, dealt from a seeded permutation of the live keys (members land in
    different 64-key tiles and 32-key halves); the last live key always belongs to the first group, and every query 0
    targets that group.  Live keys that belong to no group (``duds``) carry a random code and ``kc - 2``.
  * A query carries A = 64 / scale times its target's code, A on the constant column and 0 on the free columns.  With cc
    code columns the scaled score of a group member is 64 (cc + kc): kc = 4 - cc makes it +256 (``sign = +1``: the
    growing-maximum path, later tiles beat earlier ones by >= 128), kc = -1 - cc makes it -64 (``sign = -1``: every other
    live key is <= -192, and a zero-filled phantom key past T or past a packed image's rows would score 0 and win).  Both
    winner scores are powers of two, so -m log2e is exact in fp32 and the winners' exponentials are exactly 1.  Any other
    live key differs in a code bit or in the constant column: at least 128 lower, probability exactly 0 in fp32.
  * Keys past kv_len[b] are duplicates of live groups (same code, the winners' kc, other v) -- the first of them of the
    group of the last live key -- under the bias of the model, bf16((1 - mask) * -10000) (= -9984), written as that
    expression for even images and as the literal -9984 for odd ones.
  * v is -1 / 0 / 1 with at most 8 nonzeros per row, columns 0 and dh - 1 always among them; dout is dense -1 / 0 / 1.
    Then P is 1 / g or 0, out a multiple of 1/4, |dP - delta| <= 16 and dS a multiple of 1/16 up to 4: P, dS and out are
    exact in bf16 and every fp32 sum is an exact integer below 2^24 in units of its smallest step.  delta is exact in
    fp32.  dq, dk and dv are exact in fp32 but need not fit bf16: ROUNDED_ONCE -- the expectation is the fp64 value rounded
    once to bf16, which is what a kernel whose fp32 value is exact must store.
  * ``v_dense`` holds dense integers in [-8, 8] for a second, forward-only pass: ``out_dense`` is a multiple of 1/4 up to
    8, exact in bf16, and nonzero in almost every column of every row.

``reference`` is attention the plain way in fp64 (scores, softmax, P V, closed-form gradients, delta = rowsum(dO * O)); it
knows nothing of groups.  What selector inputs cannot show HERE: the lazy-rescale branch with a stale maximum (every score
is a winner or >= 128 below one, and sdpa's scale is the model's, so no logit is an integer in log2 units) and accuracy on
realistic score distributions; both stay with the random-data tests.  The prefill kernels that take their scale as an
argument (Gemma, CLIP) do show that branch exactly: the ladder cases of tests/prefill_attn_ref.py.
"""
import functools

import torch

BF = torch.bfloat16
ROUNDED_ONCE = ("dq", "dk", "dv")          # exact in fp32, rounded once to bf16 by the store; ``out`` is exact in bf16
MODEL_BIAS = float(((1 - torch.zeros(())).to(BF) * -10000.0).float())         # bf16((1 - mask) * -10000) at mask = 0
assert MODEL_BIAS == -9984.0


def _roles(dh, phase, pick):
    period = 2 if dh <= 16 else 3
    slots = [i for i in range(dh) if (i + phase) % period == 0]
    const = slots[pick % len(slots)]
    code = [i for i in slots if i != const]
    free = [i for i in range(dh) if i not in slots]
    return code, const, free


def build(B, N, T, H, dh, lens, seed, scale=1.0, sign=1):
    """-> dict(q [B*N, D], k, v, v_dense [B*T, D], dout [B*N, D] bf16; key_bias [B, T] fp32 and kv_len [B] int32, or None
    for both when ``lens`` is None).  lens[b] = keys that attend (a prefix), 0 = all T."""
    assert scale in (1.0, 0.5, 0.25) and sign in (1, -1) and dh % 8 == 0
    D = H * dh
    A = 64.0 / scale
    q, dout = torch.zeros(B, N, H, dh), torch.zeros(B, N, H, dh)
    k, v, vd = torch.zeros(B, T, H, dh), torch.zeros(B, T, H, dh), torch.zeros(B, T, H, dh)
    live = [T] * B if lens is None else [L if L > 0 else T for L in lens]          # keys that attend, per image
    for b in range(B):
        L = live[b]
        for h in range(H):
            g = torch.Generator().manual_seed(seed * 1000003 + b * H + h)
            code, const, free = _roles(dh, seed + b * H + h, seed + h)
            cc, nb = len(code), min(len(code), 5)
            kc = (4 - cc) if sign > 0 else (-1 - cc)
            # groups of 2, 4, 1, 2, 4, 1, ... keys from a permutation of the live keys that starts with the last one
            perm = torch.randperm(L, generator=g).tolist()
            perm.remove(L - 1)
            perm.insert(0, L - 1)
            ids = torch.randperm(2 ** nb, generator=g).tolist()
            gid = torch.randint(0, 2 ** nb, (T,), generator=g)          # duds and (overwritten) everybody else
            kcv = torch.full((T,), float(kc - 2))
            groups, at = [], 0
            while at < L and len(groups) < len(ids):
                want = (2, 4, 1)[len(groups) % 3]
                size = max(s for s in (1, 2, 4) if s <= min(want, L - at))
                members = perm[at:at + size]
                at += size
                gid[members] = ids[len(groups)]
                kcv[members] = float(kc)
                groups.append(members)
            if L < T:                                                    # masked duplicates of live groups, the winners' kc
                gid[L:] = torch.tensor(ids)[torch.arange(T - L) % len(groups)]
                kcv[L:] = float(kc)
            bit = torch.tensor([i % nb for i in range(cc)])
            kcode = ((gid[:, None] >> bit[None, :]) & 1).float() * 2 - 1
            kh, qh = k[b, :, h], q[b, :, h]                              # views [T, dh], [N, dh]
            kh[:, code] = kcode
            kh[:, const] = kcv
            kh[:, free] = torch.randint(-3, 4, (T, len(free)), generator=g).float()
            tgt = torch.randint(0, len(groups), (N,), generator=g)
            tgt[0] = 0
            tid = torch.tensor(ids)[tgt]
            qh[:, code] = A * (((tid[:, None] >> bit[None, :]) & 1).float() * 2 - 1)
            qh[:, const] = A
            cols = torch.randint(0, dh, (T, 8), generator=g)
            cols[:, 0], cols[:, 1] = 0, dh - 1
            sgn = torch.randint(0, 2, (T, 8), generator=g).float() * 2 - 1
            vv = torch.zeros(T, dh)
            vv.scatter_(1, cols, sgn)                                    # (a repeated column keeps one of its signs)
            v[b, :, h] = vv
            dout[b, :, h] = torch.randint(-1, 2, (N, dh), generator=g).float()
            vd[b, :, h] = torch.randint(-8, 9, (T, dh), generator=g).float()
    c = dict(B=B, N=N, T=T, H=H, dh=dh, scale=scale, sign=sign, lens=None if lens is None else list(lens), live=live,
             key_bias=None, kv_len=None)
    for n, t, rows in (("q", q, B * N), ("k", k, B * T), ("v", v, B * T), ("dout", dout, B * N), ("v_dense", vd, B * T)):
        c[n] = t.reshape(rows, D).to(BF)
        assert torch.equal(c[n].float(), t.reshape(rows, D)), n          # every input is exact in bf16
    if lens is not None:
        bias = torch.zeros(B, T)
        for b in range(B):
            mask = torch.zeros(T)
            mask[:live[b]] = 1
            bias[b] = ((1 - mask).to(BF) * -10000.0).float() if b % 2 == 0 else (1 - mask) * -9984.0
        c["key_bias"] = bias
        c["kv_len"] = torch.tensor(lens, dtype=torch.int32)
    return c


def packed(c):
    """packed keys of a case: the row index of every live key (image b's live rows back to back), kv_off list [B], rows"""
    B, T = c["B"], c["T"]
    idx = torch.cat([torch.arange(b * T, b * T + c["live"][b]) for b in range(B)])
    off = [0]
    for L in c["live"]:
        off.append(off[-1] + L)
    return idx, off[:B], off[-1]


def reference(c, weights=False):
    """fp64 attention and its gradients: out, lse, delta, dq, dk, dv (2-D layouts of the inputs; lse / delta [B, H, N])"""
    B, N, T, H, dh, scale = c["B"], c["N"], c["T"], c["H"], c["dh"], c["scale"]
    q, dout = (c[n].double().view(B, N, H, dh).transpose(1, 2) for n in ("q", "dout"))
    k, v = (c[n].double().view(B, T, H, dh).transpose(1, 2) for n in ("k", "v"))
    s = (q @ k.transpose(-1, -2)) * scale
    if c["key_bias"] is not None:
        s = s + c["key_bias"].double()[:, None, None, :]
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p, lse = e / l, (m + torch.log(l))[..., 0]
    out = p @ v
    delta = (dout * out).sum(-1)
    ds = p * (dout @ v.transpose(-1, -2) - delta[..., None])
    r = dict(out=out, dq=scale * (ds @ k), dk=scale * (ds.transpose(-1, -2) @ q), dv=p.transpose(-1, -2) @ dout)
    r["out_dense"] = p @ c["v_dense"].double().view(B, T, H, dh).transpose(1, 2)
    r = {n: t.transpose(1, 2).reshape(-1, H * dh) for n, t in r.items()}
    r.update(lse=lse, delta=delta)
    if weights:
        r.update(p=p, ds=ds, s=s)
    return r


def expectation(ref):
    """what the kernels must store: bf16 of the fp64 tensors (out exactly, ROUNDED_ONCE rounded once), fp32 lse and delta,
    and the rows with one winner (lse == its score exactly: log 1 = 0)"""
    e = {n: ref[n].to(BF) for n in ("out", "out_dense", "dq", "dk", "dv")}
    e["delta"] = ref["delta"].float()
    e["lse"] = ref["lse"].float()
    e["one_winner"] = ref["lse"] == ref["lse"].round()          # scores are integers; lse = score + ln g is one iff g = 1
    return e


# ------------------------------------------------------------------------------------------------- host dispatch
def dispatch(B, N, T, H, dh, bias, work=False):
    """Restates the kernel selection of ``sdpa_fwd_impl`` / ``sdpa_bwd_impl`` (csrc/sdpa.hip: the ``wide`` arithmetic,
    ``launch_fwd_nobias``, ``launch_fwd_x``, ``launch_dq``, ``launch_dkv``, ``SDPA_DISPATCH`` and ``common_params``) with
    YAT_SDPA_WIDE unset.  A restatement can drift from the C++: when that file's dispatch changes, change this too.
    -> dict(fwd=(KS, DT, QS, NOBIAS, ONES), dq=(KS, DT, QS, NOBIAS), dkv=(KS, DT, KB, NOBIAS), xcd=.., xcd_dkv=..)"""
    def cdiv(a, b):
        return -(-a // b)

    def head_class(d):
        return (1, 2) if d <= 32 else (2, 4) if d <= 64 else (3, 5) if d <= 80 else (4, 7) if d <= 112 else (4, 8)
    HB, nobias = H * B, not bias
    wide = int(cdiv(N, 128) * HB >= 1024)
    if dh <= 80 and cdiv(N, 192) * HB >= 1024:
        wide = 2
    if nobias and dh <= 80 and cdiv(N, 256) * HB >= 1024:
        wide = 3
    ones = None
    if nobias:
        ones = (1, 3) if dh == 32 else (2, 5) if dh == 64 else (3, 5) if 64 < dh < 80 else (4, 8) if dh == 112 else None
    ks, dt = ones or head_class(dh)
    if nobias and ones and ks <= 3 and wide == 3:
        qs = 4
    elif ks <= 3 and wide == 2:
        qs = 3
    else:
        qs = 2 if wide else 1
    fwd = (ks, dt, qs, nobias, ones is not None)
    ks, dt = head_class(dh)
    wq = int(cdiv(N, 128) * HB >= 1024)
    if dh <= 64 and cdiv(N, 192) * HB >= 1024:
        wq = 2
    dq = (ks, dt, 3 if (ks <= 2 and wq == 2) else 2 if wq else 1, nobias)
    wide_kv = (not work) and dh <= 80 and cdiv(T, 128) * HB >= 1024
    dkv = (ks, dt, 2 if (ks <= 3 and wide_kv) else 1, nobias)
    return dict(fwd=fwd, dq=dq, dkv=dkv, xcd=T >= 1024, xcd_dkv=T >= 1024 or bool(work))


HEAD_CLASSES = ((1, 2), (2, 4), (3, 5), (4, 7), (4, 8))
ONES_CLASSES = ((1, 3), (2, 5), (3, 5), (4, 8))
# every instantiation the host can select without YAT_SDPA_WIDE, listed from the launch templates (not from dispatch())
REACHABLE_FWD = (
    {(ks, dt, qs, False, False) for ks, dt in HEAD_CLASSES for qs in (1, 2, 3) if qs < 3 or ks <= 3}
    | {(ks, dt, qs, True, False) for ks, dt in HEAD_CLASSES for qs in (1, 2, 3) if qs < 3 or ks <= 3}
    | {(ks, dt, qs, True, True) for ks, dt in ONES_CLASSES for qs in (1, 2, 3, 4) if qs < 3 or ks <= 3})
REACHABLE_DQ = {(ks, dt, qs, nb) for ks, dt in HEAD_CLASSES for qs in (1, 2, 3) for nb in (False, True) if qs < 3 or ks <= 2}
REACHABLE_DKV = {(ks, dt, kb, nb) for ks, dt in HEAD_CLASSES for kb in (1, 2) for nb in (False, True) if kb < 2 or ks <= 3}
assert (len(REACHABLE_FWD), len(REACHABLE_DQ), len(REACHABLE_DKV)) == (40, 24, 16)


# ------------------------------------------------------------------------------------------------- the GPU file's cases
# (B, N, T, H, dh, lens or None, seed, scale, sign)
NS = (1, 15, 16, 17, 63, 64, 65, 130)
TS = (1, 63, 64, 65, 127, 128, 129, 200)
DH_BIAS = (8, 16, 24, 32, 40, 64, 72, 80, 88, 104, 112, 120, 128)
DH_NOBIAS = (32, 64, 72, 112, 8, 16, 40, 80, 88, 104, 128)         # the four ONES classes, then the fallbacks
BH = ((3, 3), (1, 3), (3, 1), (3, 3))


def _kv_lens(i, B, T):
    kinds = (0, 1, 63, 64, 65, T - 1, T)
    return [min(max(kinds[(3 * i + b) % 7], 0), T) for b in range(B)]


def _narrow():
    cases = []
    for i, dh in enumerate(DH_BIAS):
        for sign in (1, -1):
            j = 2 * i + (sign < 0)
            B, H = BH[j % 4]
            N, T = NS[j % 8], TS[(3 * j + 1) % 8]
            cases.append((B, N, T, H, dh, _kv_lens(j, B, T), 100 + j, (1.0, 0.25)[j % 2], sign))
    for i, dh in enumerate(DH_NOBIAS):
        for sign in (1, -1):
            j = 2 * i + (sign < 0)
            B, H = BH[(j + 1) % 4]
            cases.append((B, NS[(j + 3) % 8], TS[(5 * j + 2) % 8], H, dh, None, 200 + j, (0.25, 1.0)[j % 2], sign))
    return cases


NARROW = _narrow()
_RAG = [130, 129, 64, 1, 0, 65, 63, 128]          # ragged kv_len of the eight images of a wide case (T = 130)


def _wide():
    """ceil(N / W) * H * B >= 1024 with H * B = 512: N = 130 -> QS 2, N = 200 -> QS 3 (dQ: at dh <= 64), N = 258 -> QS 4
    (no bias, ONES classes), T = 130 -> KB 2 (dense dK/dV, dh <= 80); one head dim per (KS, DT) the class admits"""
    cases, s = [], 300
    for dh in (32, 64, 72, 112, 128):
        cases.append((8, 130, 130, 64, dh, _RAG, s, 1.0, -1 if dh != 64 else 1)); s += 1
    for dh in (32, 64, 72):
        cases.append((8, 200, 65, 64, dh, [min(x, 65) for x in _RAG], s, 0.25, -1 if dh == 64 else 1)); s += 1
    for dh in (32, 64, 72, 112, 16, 40, 80, 104, 128):
        cases.append((8, 130, 130 if dh <= 80 else 65, 64, dh, None, s, 1.0, -1 if dh % 16 else 1)); s += 1
    for dh in (32, 64, 72, 16, 40, 80):
        cases.append((8, 200, 65, 64, dh, None, s, 0.25, -1)); s += 1
    for dh in (32, 64, 72):
        cases.append((8, 258, 65, 64, dh, None, s, 1.0, -1 if dh != 72 else 1)); s += 1
    return cases


WIDE = _wide()
# xcd_remap (T >= 1024): grids of 17 and 102 workgroups (remainders 1 and 6 modulo 8) without a bias; with one, ragged
# kv_len (one <= 64, one = T) over (B, H) = (3, 3): forward, dQ and the dense dK/dV, then the work list (30 tiles x 3 heads)
XCD = [(1, 1030, 1030, 1, 64, None, 400, 1.0, -1), (2, 1030, 1030, 3, 40, None, 401, 0.25, -1),
       (3, 70, 1100, 3, 72, [40, 1100, 700], 402, 1.0, -1)]


def hashable(spec):
    return tuple(tuple(x) if isinstance(x, list) else x for x in spec)


NARROW, WIDE, XCD = ([hashable(c) for c in l] for l in (NARROW, WIDE, XCD))
CASES = NARROW + WIDE + XCD


def case_id(case):
    B, N, T, H, dh, lens, seed, scale, sign = case
    return f"B{B}-N{N}-T{T}-H{H}-dh{dh}-{'nobias' if lens is None else 'bias'}-{'pos' if sign > 0 else 'neg'}-s{seed}"


@functools.lru_cache(maxsize=2)
def case(spec):
    """inputs, fp64 reference and expectation of one case, computed once per process"""
    B, N, T, H, dh, lens, seed, scale, sign = spec
    c = build(B, N, T, H, dh, None if lens is None else list(lens), seed, scale, sign)
    ref = reference(c)
    return c, ref, expectation(ref)


def ulp32(x):
    """the fp32 spacing at |x| (x fp32 or fp64 tensor)"""
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().double().clamp_min(2.0 ** -126))) - 23)

