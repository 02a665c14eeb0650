"""Exact inputs for the four prefill attention kernels (csrc/attn_prefill.hpp: vae_attn_kernel of csrc/vae_kl.hip,
gemma_attn_kernel of csrc/gemma.hip, t5_attn_kernel of csrc/t5.hip, clip_attn_kernel of csrc/clip.hip), their plain fp64
reference, the case lists of test_prefill_attn_exact_gpu.py and a Python restatement of the host dispatch and of the lazy
rescale of ``online_softmax_step``.  Nothing here touches yat_amd or a GPU.

Every case is a packed batch: prompt b is the row range [off[b], off[b] + lens[b]) of one matrix, of which the first
eff[b] = min(lens[b], max_len) rows are live (the VAE kernel: B images of N rows, all live); ``TAIL`` rows of no prompt
follow the last one.  Per kv head the head's columns are dealt roles from a seeded permutation of every third column: eight
*code* columns, two *constant* columns c1 and c2, the rest *free*.  A key carries the +-1 code of its group id (bit t on
the t-th code column), ``kc1`` on c1, ``kc2`` (or its ladder level) on c2 and small integers (-3 .. 3) on the free columns; a
query carries ``Aq`` times the code of its *target* group, Aq on c1, ``q2`` on c2 and 0 on the free columns.  The raw score
is the fp32 integer  Aq (8 - 2 hamming + kc1) + q2 k[c2]:  the members of the target tie at the top, every other key is at
least 2 Aq lower.  v is dense integers in [-8, 8].

``mode``
  * "sel" -- selector inputs.  A prompt's keys are dealt into groups of 1, 2 or 4 (key 0 alone; the last live key first in
    line; every other group an adjacent pair {j, j + 1}; the other members from a permutation, so they land in different
    32-key halves, 64-key tiles and LDS stages).  A query's target is, in rotation, the group of its diagonal key, of key
    i + 1 (masked for a causal kernel: an *impostor*, the winners' score with another v), of key 0 and of a random visible
    key (bidirectional kernels: of the last live key first), always one with 1, 2 or 4 visible members.  2 Aq times the
    kernel's logit factor is at least 200 log2 units, so after the kernel's bf16 rounding of P the winners weigh exactly 1
    (equal raw scores give equal logits under every transform here) and everybody else exactly 0: l is 1, 2 or 4, the output
    a multiple of 1/4 up to 8 and exact in bf16.  ``sign`` +1 puts the winners at a positive score (the growing-maximum path:
    a later tile beats an earlier one and the rescale factor is exactly 0), -1 at a negative one (a zero-filled phantom key
    past the prompt's end, or a zeroed dead query, scores 0 and would win).  Rows past a prompt's live end -- the next prompt's
    first row (its key 0 carries the code of this prompt's last group), the rows a smaller max_len cuts off, the TAIL rows --
    are impostors of the group of the last live key.  The neighbouring head's (Gemma: kv head's) columns hold that head's own
    roles, codes and v.  The VAE and T5 kernels have no free scale, so their stale-maximum cases are these ties: a query
    whose group arrives in a late tile steps up (rescale factor 0) while the other queries of its strip have long seen theirs.
  * "bias" (T5) -- q = 0, every raw score is 0 and the table decides: ``BIAS_LOSER`` everywhere but at distance 0 and at one
    more distance d per head (``dist``), where it holds one value per head.  A query has 1 or 2 winners; an index off by one
    or a flipped direction moves them.
  * "ladder" (Gemma without cap, CLIP) -- ``scale`` = fp32(0x1.62e43p-1 * 2^-k) makes fl(scale * LOG2Ef) exactly 2^-k
    (``c_lin``; asserted below for k = 0 .. 7), so with Aq = 128 * 2^k and q2 = 2^k the logit of a key of the query's class is
    1024 + level in log2 units, an integer, and of any other key at least 242 lower.  Within a class the t-th key (in row
    order) has level max(0, t - 1): every causal prefix of a class weighs a power of two in all, at most 14 keys a class so
    that every partial sum fits fp32.  Classes are dealt at random; on top, in prompts of at least 97 rows, class E (two keys
    in the first half, eight in the second, one in the third; every query of the strips at 112 and 176) grows by exactly 8
    -- no rescale, P = 2^8 -- then by 1 more, then stays put for tiles on end, and class R (two keys in the first half, ten
    in the third; one query in each of four strips) grows by 10 in one half: the other 15 queries of its strip take the
    wave-uniform rescale with alpha = 2^-j or 1.  ``lazy_walk`` restates the rescale rule on these integers and reports which
    step kinds a case meets.  The output is a dyadic rational with a power-of-two denominator: exact in fp32, rounded once.

``reference`` is attention the plain way in fp64 -- logits, mask, softmax, P V per prompt and head -- rounded once to bf16 by
``expectation``; it knows nothing of groups, classes or tiles.  It takes the softmax in base 2 on  raw * c  with c the fp32
product the linear kernels use (``c_lin``), which is scale * log2(e) to 2^-24; the capped, VAE and T5 logits are the
formulas of the models.
"""
import collections
import functools
import math

import numpy as np
import torch

BF = torch.bfloat16
TAIL = 2                                            # rows of no prompt after the last one
LOG2E = math.log2(math.e)
LOG2E_F = np.float32(1.4426950408889634)           # csrc/attn_prefill.hpp
LAZY_LOG2 = 8.0
GAP_BOUND = 134.0                                   # below 2^-134 the bf16 rounding of P gives exactly 0
BIAS_LOSER = -256.0

Case = collections.namedtuple("Case", "kind mode lens max_len H Hkv dh sign scale cap seed dist")
CAUSAL = {"vae": False, "gemma": True, "t5": False, "clip": True}


def exact_scale(k):
    return float(np.float32(float.fromhex("0x1.62e43p-1") * 2.0 ** -k))


def c_lin(scale):
    """fl(scale * LOG2Ef), the fp32 product of the linear kernels (Gemma without cap, CLIP)"""
    return float(np.float32(scale) * LOG2E_F)


assert all(c_lin(exact_scale(k)) == 2.0 ** -k for k in range(8))


def scale_of(case):
    if case.kind == "vae":
        return float(np.float32(1.0) / np.sqrt(np.float32(case.dh)))
    if case.kind == "t5":
        return 1.0
    return exact_scale(case.scale) if isinstance(case.scale, int) else float(case.scale)


def amplitudes(case):
    """(Aq, kc1, q2, kc2): raw score = Aq (8 - 2 hamming + kc1) + q2 kc2 (ladder: q2 times the key's level)"""
    if case.mode == "ladder":
        return 128.0 * 2 ** case.scale, 0.0, float(2 ** case.scale), 0.0
    kc1 = -7.0 if case.sign > 0 else -9.0
    if case.kind == "vae":
        return 4096.0, kc1, 0.0, 0.0
    if case.kind == "t5":
        return 128.0, kc1, 0.0, 0.0
    if case.kind == "gemma" and case.cap > 0:
        # +: +-Aq saturate tanh.  -: the winners sit at -256 (tanh near -0.1), everybody else saturates at -cap
        return (2.0 ** 14, -7.0, 0.0, 0.0) if case.sign > 0 else (2.0 ** 14, -8.0, 256.0, -1.0)
    if isinstance(case.scale, int):
        return 128.0 * 2 ** case.scale, kc1, 0.0, 0.0
    return 2.0 ** math.ceil(math.log2(100.0 / c_lin(case.scale))), kc1, 0.0, 0.0


def logit2(case, raw, bias=None):
    """fp64 logits in log2 units of raw scores [.., Lq, Lk] (``bias``: T5's [Lq, Lk] gather of the table)"""
    s = scale_of(case)
    if case.kind == "vae":
        return raw * (s * LOG2E)
    if case.kind == "t5":
        return (raw + bias) * LOG2E
    if case.kind == "gemma" and case.cap > 0:
        return case.cap * torch.tanh(raw * (s / case.cap)) * LOG2E
    return raw * c_lin(s)


def _roles(dh, g):
    slots = [i for i in range(dh) if i % 3 == 0]
    pick = [slots[i] for i in torch.randperm(len(slots), generator=g)[:10].tolist()]
    code, c1, c2 = pick[:8], pick[8], pick[9]
    free = [i for i in range(dh) if i not in pick]
    return code, c1, c2, free


def _code(gid):
    """[n] group ids -> [n, 8] of +-1"""
    return ((torch.as_tensor(gid)[:, None] >> torch.arange(8)[None, :]) & 1).double() * 2 - 1


def _deal_groups(L, carry, pool, g):
    """selector groups over the keys [0, L) -> gid per key.  Key 0 alone (id ``carry``: the previous prompt's last group);
    the last key first in line; sizes 2, 4, 1 in turn, every other pair adjacent"""
    gid = [-1] * L
    gid[0] = carry if carry is not None else pool.pop()
    order = torch.randperm(L, generator=g).tolist()
    at, n = 0, 0
    for p in [L - 1] + order:
        if gid[p] >= 0:
            continue
        want = (2, 4, 1)[n % 3]
        members = [p]
        if want >= 2 and n % 2 == 0 and p + 1 < L and gid[p + 1] < 0:
            members.append(p + 1)
        while len(members) < want:
            while at < L and (gid[order[at]] >= 0 or order[at] in members):
                at += 1
            if at == L:
                break
            members.append(order[at])
        if len(members) == 3:
            members.pop()
        gi = pool.pop()
        for j in members:
            gid[j] = gi
        n += 1
    return gid


def _deal_targets(L, gid, causal, g):
    members = collections.defaultdict(list)
    for j, x in enumerate(gid):
        members[x].append(j)
    tgt = []
    for i in range(L):
        r = int(torch.randint(0, i + 1 if causal else L, (1,), generator=g))
        if causal:                                   # (for i = L - 1 the row after the end carries gid[L - 1] too)
            cand = [gid[i], gid[min(i + 1, L - 1)], gid[0], gid[r]]
        else:
            cand = [gid[L - 1], gid[0], gid[i], gid[r]]
        cand = cand[i % 4:] + cand[:i % 4] + [gid[0]]
        for c in cand:
            n = sum(1 for j in members[c] if j <= i) if causal else len(members[c])
            if n in (1, 2, 4):
                tgt.append(c)
                break
    return tgt


E_STRIPS, R_QUERIES = (112, 176), (101, 133, 149, 165)


def _deal_ladder(L, pool, g):
    """-> class id per key, level per key (the query classes: ``_requery``)"""
    K = max(2, -(-L // 10))
    cls = [-1] * L
    forced = L >= 97
    if forced:
        for j in (2, 5, 70) + tuple(33 + 3 * t for t in range(8)):
            cls[j] = K                                # E: levels 0, 0 | 1 .. 8 | 9
        for j in (3, 7) + tuple(65 + 2 * t for t in range(10)):
            cls[j] = K + 1                            # R: levels 0, 0 | - | 1 .. 10
    count = [0] * (K + 2)
    for j in range(L):
        if cls[j] < 0:
            c = int(torch.randint(0, K, (1,), generator=g))
            while count[c] >= 14:
                c = (c + 1) % K
            cls[j] = c
            count[c] += 1
    seen, level = [0] * (K + 2), []
    for j in range(L):
        level.append(max(0, seen[cls[j]] - 1))
        seen[cls[j]] += 1
    ids = [pool.pop() for _ in range(K + 2)]
    return [ids[c] for c in cls], level


def build(case):
    """-> dict(q [rows, H dh], k, v [rows, Hkv dh] fp64 (exact in bf16), off, eff, rows, table [H, 2 max_len - 1] or None)"""
    kind, mode, H, Hkv, dh = case.kind, case.mode, case.H, case.Hkv, case.dh
    causal, G = CAUSAL[kind], H // Hkv
    lens = list(case.lens)
    eff = [min(L, case.max_len) for L in lens]
    off = [0]
    for L in lens:
        off.append(off[-1] + L)
    rows = off[-1] + TAIL
    Aq, kc1, q2, kc2 = amplitudes(case)
    g0 = torch.Generator().manual_seed(case.seed)
    q = torch.zeros(rows, H, dh, dtype=torch.float64)
    k = torch.randint(-3, 4, (rows, Hkv, dh), generator=g0).double()
    v = torch.randint(-8, 9, (rows, Hkv, dh), generator=g0).double()
    table = None
    if kind == "t5":
        table = torch.zeros(H, 2 * case.max_len - 1, dtype=torch.float64)
        for h in range(H):
            if mode == "bias":
                table[h] = BIAS_LOSER
                table[h, case.max_len - 1] = table[h, case.max_len - 1 + case.dist[h]] = (0.0, 1.5, -2.0)[h % 3]
            else:
                table[h] = (-3.0, 0.5, 2.0)[h % 3]
    if mode != "bias":
        for kv in range(Hkv):
            g = torch.Generator().manual_seed(case.seed * 1000003 + kv)
            code, c1, c2, _ = _roles(dh, g)
            carry = None
            kgid, klev = [0] * rows, [kc2] * rows
            for b, (L, La) in enumerate(zip(eff, lens)):
                if L == 0:
                    continue
                pool = [x for x in torch.randperm(256, generator=g).tolist() if x != carry]
                if mode == "sel":
                    gid = _deal_groups(L, carry, pool, g)
                    level = [kc2] * L
                    tg = [_deal_targets(L, gid, causal, g) for _ in range(G)]
                else:
                    gid, level = _deal_ladder(L, pool, g)
                    tg = [_requery(L, gid, case.seed + 7 * kv + hh) for hh in range(G)]
                carry = gid[L - 1]
                kgid[off[b]:off[b] + L] = gid
                klev[off[b]:off[b] + L] = level
                # the rows max_len cuts off: impostors of the last live group (ladder: far above its top level)
                kgid[off[b] + L:off[b] + La] = [carry] * (La - L)
                klev[off[b] + L:off[b] + La] = [level[L - 1] + (20 if mode == "ladder" else 0)] * (La - L)
                for hh in range(G):
                    h = kv * G + hh
                    t = torch.tensor(tg[hh] + [carry] * (La - L))
                    q[off[b]:off[b] + La, h, code] = Aq * _code(t)
                    q[off[b]:off[b] + La, h, c1] = Aq
                    q[off[b]:off[b] + La, h, c2] = q2
            if carry is not None:
                kgid[off[-1]:] = [carry] * TAIL
                klev[off[-1]:] = [klev[off[-1] - 1] + (20 if mode == "ladder" else 0)] * TAIL
            k[:, kv, code] = _code(kgid)
            k[:, kv, c1] = kc1
            k[:, kv, c2] = torch.tensor(klev, dtype=torch.float64)
    c = dict(case=case, q=q.reshape(rows, H * dh), k=k.reshape(rows, Hkv * dh), v=v.reshape(rows, Hkv * dh), off=off, eff=eff,
             rows=rows, table=table)
    for n in ("q", "k", "v", "table"):
        assert c[n] is None or torch.equal(c[n].to(BF).double(), c[n]), n          # every input is exact in bf16
    return c


def _requery(L, gid, salt):
    """the class of each query of a ladder prompt: of a visible key, or E / R where those are forced (the two largest
    class indices, recognised by their forced key rows)"""
    g = torch.Generator().manual_seed(L * 131 + salt)
    out = []
    for i in range(L):
        r = int(torch.randint(0, i + 1, (1,), generator=g))
        c = gid[r]
        if L >= 97 and (i // 16) * 16 in E_STRIPS:
            c = gid[2]
        elif L >= 97 and i in R_QUERIES:
            c = gid[3]
        out.append(c)
    return out


def raw_scores(c):
    """yields (b, h, raw [Le, Le] fp64, bias [Le, Le] or None, v [Le, dh]) per live prompt and query head"""
    case = c["case"]
    H, Hkv, dh = case.H, case.Hkv, case.dh
    for b, Le in enumerate(c["eff"]):
        if Le == 0:
            continue
        r0 = c["off"][b]
        for h in range(H):
            kv = h // (H // Hkv)
            q = c["q"][r0:r0 + Le, h * dh:(h + 1) * dh]
            k = c["k"][r0:r0 + Le, kv * dh:(kv + 1) * dh]
            bias = None
            if c["table"] is not None:
                i, j = torch.arange(Le)[:, None], torch.arange(Le)[None, :]
                bias = c["table"][h][(j - i) + case.max_len - 1]
            yield b, h, q @ k.T, bias, c["v"][r0:r0 + Le, kv * dh:(kv + 1) * dh]


def masked_logits(c):
    """yields (b, h, t [Le, Le] fp64 log2 logits with -inf where the model masks, v)"""
    case = c["case"]
    for b, h, raw, bias, v in raw_scores(c):
        t = logit2(case, raw, bias)
        if CAUSAL[case.kind]:
            Le = t.shape[0]
            t = t.masked_fill(torch.arange(Le)[None, :] > torch.arange(Le)[:, None], float("-inf"))
        yield b, h, t, v


def reference(c):
    """plain fp64 attention -> (out [rows, H dh] fp64, NaN where no live query is; written [rows] bool)"""
    case = c["case"]
    out = torch.full((c["rows"], case.H * case.dh), float("nan"), dtype=torch.float64)
    written = torch.zeros(c["rows"], dtype=torch.bool)
    for b, h, t, v in masked_logits(c):
        p = torch.exp2(t - t.max(-1, keepdim=True).values)
        p = p / p.sum(-1, keepdim=True)
        r0 = c["off"][b]
        out[r0:r0 + t.shape[0], h * case.dh:(h + 1) * case.dh] = p @ v
        written[r0:r0 + t.shape[0]] = True
    return out, written


def expectation(ref):
    return ref.to(BF)


# ------------------------------------------------------------------------------------------------- the lazy rescale
def lazy_walk(t, causal=True):
    """Restates the decision of ``online_softmax_step`` (csrc/attn_prefill.hpp, ce = 1) on one (prompt, head)'s integer
    logits t [L, L] as the causal kernels walk them: strips of 16 queries, halves of 32 keys up to the strip's diagonal.  ->
    set of step kinds met by live class keys: ("P", e) a probability 2^e with no rescale in that step, ("alpha", j) a
    query rescaled by 2^-j (j = 0: alpha = 1) in a step only other queries of its strip forced, ("lone",) a rescale that
    one query alone forced, ("eight",) growth by exactly 8 without a rescale, ("stay", n) a maximum unchanged over n >= 3
    consecutive halves (more than one tile)."""
    L = t.shape[0]
    kinds = set()
    for sq0 in range(0, L, 16):
        qs = list(range(sq0, min(sq0 + 16, L)))
        m = {i: -1e30 for i in qs}
        calm = {i: 0 for i in qs}
        for kh0 in range(0, sq0 + 16, 32):
            mx = {}
            for i in qs:
                row = t[i, kh0:min(kh0 + 32, L)]
                mx[i] = float(row.max()) if row.numel() else -1e30
                if mx[i] == float("-inf"):
                    mx[i] = -1e30
            want = [i for i in qs if mx[i] > m[i] + LAZY_LOG2]
            for i in qs:
                top = float(t[i, :i + 1].max())       # what counts: steps inside the query's own class (within 40 of its top)
                near_m = m[i] > top - 40
                near = near_m and mx[i] > top - 40
                if want:
                    mn = max(m[i], mx[i])
                    if near_m and i not in want:
                        kinds.add(("alpha", int(mn - m[i])))
                    if near and want == [i]:
                        kinds.add(("lone",))
                    m[i] = mn
                    calm[i] = 0
                else:
                    e = int(mx[i] - m[i]) if near else 0
                    if e >= 1:
                        kinds.add(("P", e))
                    if e == 8:
                        kinds.add(("eight",))
                    if near_m and mx[i] <= m[i]:
                        calm[i] += 1
                        if calm[i] >= 3:
                            kinds.add(("stay", calm[i]))
                    elif e >= 1:
                        calm[i] = 0
    return kinds


# ------------------------------------------------------------------------------------------------- host dispatch
def gemma_instance(Hq, Hkv):
    """(NW, HPW) of ``yat_gemma_attn_fwd`` (csrc/gemma.hip); a restatement: when that dispatch changes, change this too"""
    G = Hq // Hkv
    return (8, 8) if G % 8 == 0 else (4, 4) if G % 4 == 0 else (4, 2) if G % 2 == 0 else (4, 1)


GEMMA_INSTANCES = ((8, 8), (4, 4), (4, 2), (4, 1))


def query_tile(case):
    if case.kind == "gemma":
        nw, hpw = gemma_instance(case.H, case.Hkv)
        return 16 * (nw // hpw)
    return 64


def walk(case):
    """The control-flow classes the workgroups of a case meet, from the kernels' own tile arithmetic -> set of names."""
    f = set()
    QT = query_tile(case)
    for L, La in zip([min(x, case.max_len) for x in case.lens] if case.kind != "vae" else case.lens, case.lens):
        grid_x = -(-(L if case.kind == "vae" else case.max_len) // QT)
        if La > L:
            f.add("cut_by_max_len")
        if L == 0:
            f.add("empty_prompt")
        for x in range(grid_x):
            q0 = x * QT
            if q0 >= L:
                f.add("tile_exits")
                continue
            f.add(f"len%64={L % 64}" if q0 + QT >= L else "inner_tile")
            for sq0 in range(q0, q0 + QT, 16):
                if sq0 >= L:
                    f.add("dead_strip")
                    continue
                if sq0 + 16 > L:
                    f.add("ragged_strip")
                if CAUSAL[case.kind]:
                    ntiles = q0 // 64 + 1
                    f.add(f"stages_{min(ntiles, 3)}")
                    k0 = (ntiles - 1) * 64
                    if k0 + 32 > sq0 + 15:
                        f.add("half_skipped")          # the diagonal lies in the first half of the last tile
                        f.add("diag_in_half_0")
                    else:
                        f.add("diag_in_half_1")
                elif case.kind == "t5":
                    ntiles = -(-L // 64)
                    f.add(f"stages_{min(ntiles, 3)}")
                    r = L % 64
                    f.add("end_on_edge" if r == 0 else "end_in_half_0" if r <= 32 else "end_in_half_1")
                else:
                    ntiles = -(-L // 32)
                    f.add(f"stages_{min(ntiles, 3)}")
                    f.add("last_tile_masked" if L % 32 else "last_tile_full")
    return f


# ------------------------------------------------------------------------------------------------- the GPU file's cases
VAE_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 130)
GEMMA_LENS = (1, 16, 17, 32, 33, 63, 64, 65, 129, 193)
TEXT_LENS = (1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 96, 97, 129, 193)
GEMMA_HEADS = ((8, 1), (4, 1), (8, 4), (4, 4), (3, 3))
MODEL_SCALE = {"gemma": 256 ** -0.5, "clip": 64 ** -0.5}


def _cases():
    cases, seed = [], 1
    for dh in (64, 512):
        for i, N in enumerate(VAE_N):
            signs = (1, -1) if N in (33, 130) else ((1,) if (i + dh // 512) % 2 == 0 else (-1,))
            for sign in signs:
                B = 3 if i % 3 == 0 else 1
                cases.append(Case("vae", "sel", (N,) * B, N, 1, 1, dh, sign, None, 0.0, seed, None)); seed += 1
    # (lens, max_len): every length class; an empty prompt first, in the middle and last; max_len above the longest
    # prompt (empty query tiles exit) and below one prompt's length (its rows past max_len keep their fill)
    gemma_batches = (((1, 16, 17, 32, 33), 33), ((63, 0, 64, 65), 135), ((0, 129, 193, 0), 193), ((65, 129), 100))
    for Hq, Hkv in GEMMA_HEADS:
        for i, (lens, ml) in enumerate(gemma_batches):
            for j, capped in enumerate((False, True)):
                sign = 1 if (i + Hq + j) % 2 == 0 else -1
                cap = (128.0 if sign > 0 else 160.0) if capped else 0.0
                scale = MODEL_SCALE["gemma"] if capped or i % 2 == 0 else 4
                cases.append(Case("gemma", "sel", lens, ml, Hq, Hkv, 256, sign, scale, cap, seed, None)); seed += 1
        cases.append(Case("gemma", "ladder", (193, 129, 33), 193, Hq, Hkv, 256, 1, 3, 0.0, seed, None)); seed += 1
    text_batches = (((1, 15, 16, 17, 31, 32, 33), 33), ((48, 0, 49, 63, 64), 134), ((0, 65, 96, 97), 97),
                    ((129, 193, 0), 193), ((193, 65), 150))
    for H in (1, 3):
        for i, (lens, ml) in enumerate(text_batches):
            for sign in (1, -1):
                cases.append(Case("t5", "sel", lens, ml, H, H, 64, sign, None, 0.0, seed, None)); seed += 1
                scale = MODEL_SCALE["clip"] if (i + (sign < 0)) % 2 == 0 else 2
                cases.append(Case("clip", "sel", lens, ml, H, H, 64, sign, scale, 0.0, seed, None)); seed += 1
            top = max(min(x, ml) for x in lens) - 1
            for dist in ((1, -1, 64), (-64, top, -top), (33, -2, 100 if top >= 100 else 5)):
                dist = tuple(max(-(ml - 1), min(ml - 1, d)) for d in dist[:H])
                cases.append(Case("t5", "bias", lens, ml, H, H, 64, 1, None, 0.0, seed, dist)); seed += 1
        for lens, ml in (((129, 193, 0), 193), ((0, 65, 96, 97), 97), ((193, 33), 160)):
            cases.append(Case("clip", "ladder", lens, ml, H, H, 64, 1, 1 + H, 0.0, seed, None)); seed += 1
    return cases


CASES = _cases()


def case_id(case):
    s = case.scale if not isinstance(case.scale, float) else "model"
    return (f"{case.kind}-{case.mode}-L{'_'.join(map(str, case.lens))}-max{case.max_len}-H{case.H}_{case.Hkv}-dh{case.dh}-"
            f"{'pos' if case.sign > 0 else 'neg'}-scale_{s}-cap{case.cap:g}-s{case.seed}")


@functools.lru_cache(maxsize=4)
def case(spec):
    """inputs, fp64 reference and the written-row mask of one case, computed once per process"""
    c = build(spec)
    ref, written = reference(c)
    return c, ref, written
