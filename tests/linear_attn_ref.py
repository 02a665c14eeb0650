"""Torch restatements of ReLU linear attention (csrc/linear_attn.hip) for test_linear_attn_ref_cpu.py and
test_linear_attn_gpu.py, written apart from yat_amd (it does not import yat_amd).  Everything runs on the CPU.

    reference(qkv, B, N, H, k_off, v_off, dtype)    diffusers' SanaLinearAttnProcessor2_0 in plain, differentiable torch:
                                                    dtype = torch.float64: the truth
                                                    dtype = torch.float32, results rounded to bf16: the flow (the processor
                                                    up-casts q, k, v to fp32 and returns to bf16 at the end; so does its autograd)
    make_inputs(kind, B, N, H, seed)                bf16 qkv [B*N, 3D] (q | k | v, D = 32 H) and dout [B*N, D]
    flips(x_bf16, truth64)                          elements that are not the correctly rounded fp64 result
    emulate(qkv, dout, ..., lo=True)                the kernels' arithmetic in torch fp32 (bf16 hi + lo split of S, dU, dS exactly
                                                    where the kernels split them); lo=False drops every lo half
    case(kind, B, N, H)                             inputs, truth and flow of one test case, computed once and shared
    conditions(got, c, name, flip_cap)              the per-head conditions both test files hold a result to

Layout: qkv is a [B*N, ld] matrix, q in columns [0, D), k in [k_off, k_off + D), v in [v_off, v_off + D), head h in the 32
columns from 32 h of each range.  ld is the tensor's row stride: column and row slices of wider buffers are taken as they are.
"""
import functools

import torch
import torch.nn.functional as F

from tests.gpu_common import _FAILS, as_good_as

BF = torch.bfloat16
C = 32
KINDS = ("randn", "sparse", "zeros", "offset")
DEAD_HEADS = {"sparse": (0, 1)}          # head 0: no live key, head 1: no live query
FLIP_CAP = 0.01                          # flips <= FLIP_CAP * numel + FLIP_FREE, derived in test_linear_attn_gpu.py's docstring
FLIP_FREE = 2


def _heads(x, off, B, N, H):
    """columns [off, off + 32 H) of a [B*N, ld] matrix as [B, H, N, 32]"""
    return x[:, off:off + C * H].reshape(B, N, H, C).permute(0, 2, 1, 3)


def _rows(x, B, N, H):
    """[B, H, N, 32] -> [B*N, 32 H]"""
    return x.permute(0, 2, 1, 3).reshape(B * N, C * H)


def reference(qkv, B, N, H, k_off, v_off, dtype):
    x = qkv.to(dtype)
    q, k, v = F.relu(_heads(x, 0, B, N, H)), F.relu(_heads(x, k_off, B, N, H)), _heads(x, v_off, B, N, H)
    v1 = F.pad(v, (0, 1), value=1.0)                                        # [B,H,N,33]: v padded with ones
    S = v1.transpose(-1, -2) @ k                                            # [B,H,33,32]
    U = q @ S.transpose(-1, -2)                                             # [B,H,N,33]
    return _rows(U[..., :C] / (U[..., C:] + 1e-15), B, N, H)


def reference_fwd_bwd(qkv, dout, B, N, H, k_off, v_off, dtype):
    """out [B*N, D] and the gradient of qkv (its shape; zero outside the q, k, v ranges), both in `dtype`"""
    x = qkv.detach().to(dtype).requires_grad_(True)
    out = reference(x, B, N, H, k_off, v_off, dtype)
    out.backward(dout.to(dtype))
    return out.detach(), x.grad


def make_inputs(kind, B, N, H, seed=0):
    assert kind in KINDS                        # (`sparse` with H < 3 has dead heads only)
    D = C * H
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + KINDS.index(kind))
    x = torch.randn(B, N, 3, H, C, generator=g)                             # [b, n, q|k|v, h, c]
    dout = torch.randn(B * N, D, generator=g)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]                            # views [B,N,H,32]
    if kind == "sparse":
        q -= 1.3
        k -= 1.3
        q[:, 3::7] = -q[:, 3::7].abs()                                      # tokens without a live query channel
        k[:, 3::5] = -k[:, 3::5].abs()                                      # tokens without a live key channel
        k[:, :, 0] = -k[:, :, 0].abs()                                      # head 0: S = 0, denominator 1e-15
        q[:, :, 1:2] = -q[:, :, 1:2].abs()                                  # head 1: U = 0
        q[:, 0, 2:, 0] = q[:, 0, 2:, 0].abs() + 0.25                        # heads >= 2 stay live whatever N is: token 0 has
        k[:, 0, 2:, 0] = k[:, 0, 2:, 0].abs() + 0.25                        # a live query and a live key in channel 0
    elif kind == "zeros":
        u = torch.rand(x.shape, generator=g)
        x[u < 0.1] = 0.0
        x[(u >= 0.1) & (u < 0.2)] = -0.0
    elif kind == "offset":
        q *= 4.0
        k *= 4.0
        v += 3.0
    qkv = x.reshape(B * N, 3 * D).to(BF)
    dout = dout.to(BF)
    for t in (qkv, dout):                                                   # no subnormals
        t[(t.float().abs() < 2.0 ** -126) & (t != 0)] = 0.0
    return qkv, dout


def round_bf16(x64):
    """fp64 -> bf16, correctly rounded (torch goes through fp32: a value that rounds onto a bf16 tie there would round twice)"""
    f = x64.float()
    tie = (f.view(torch.int32) & 0xFFFF) == 0x8000
    e = x64 - f.double()
    away = torch.where(e > 0, torch.full_like(f, float("inf")), torch.full_like(f, float("-inf")))
    return torch.where(tie & (e != 0), torch.nextafter(f, away), f).to(BF)


def flips(x_bf16, truth64):
    want = round_bf16(truth64.double())
    got = x_bf16.detach().cpu().to(BF)
    a, b = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    return int(((a != b) & ~((got == 0) & (want == 0))).sum())              # +0 and -0 are the same result


def _split(x, lo):
    hi = x.to(BF).float()
    return hi, ((x - hi).to(BF).float() if lo else None)


def _mm2(a, hi, lo_):
    """a (bf16 values) times a split fp32 operand: exact products, fp32 sums -- one MFMA per half"""
    y = a @ hi
    return y + a @ lo_ if lo_ is not None else y


def emulate(qkv, dout, B, N, H, k_off, v_off, lo=True):
    """out, dq, dk, dv as bf16 [B*N, D], computed the way csrc/linear_attn.hip's five kernels compute them."""
    x = qkv.float()
    q, k, v = _heads(x, 0, B, N, H), _heads(x, k_off, B, N, H), _heads(x, v_off, B, N, H)
    dO = _heads(dout.float(), 0, B, N, H)
    rq, rk = torch.where(q > 0, q, torch.zeros_like(q)), torch.where(k > 0, k, torch.zeros_like(k))
    # la_state_kernel: S = [v;1]^T relu(k), fp32 accumulation of exact products
    S = F.pad(v, (0, 1), value=1.0).transpose(-1, -2) @ rk                  # [B,H,33,32]
    shi, slo = _split(S, lo)
    # u_tiles: U = relu(q) (S_hi + S_lo)^T
    U = _mm2(rq, shi.transpose(-1, -2), slo.transpose(-1, -2) if lo else None)     # [B,H,N,33]
    inv = 1.0 / (U[..., C:] + 1e-15)
    o = U[..., :C] * inv
    out = _rows(o, B, N, H).to(BF)
    # la_bwd_q_kernel
    du = dO * inv
    du32 = -(dO * o).sum(-1, keepdim=True) * inv
    dhi, dlo = _split(du, lo)
    xhi, xlo = shi[..., :C, :], (slo[..., :C, :] if lo else None)           # rows c' < 32 of the state
    dq = dhi @ xhi
    if lo:
        dq = dq + dlo @ xhi + dhi @ xlo                                     # hi.hi + lo.hi + hi.lo; lo.lo is not computed
    dq = torch.where(q > 0, dq + S[..., C:, :] * du32, torch.zeros_like(dq))
    d33 = torch.cat([du, du32], -1)                                         # the dU image: 32 channels and dU32
    ihi, ilo = _split(d33, lo)
    dS = _mm2(ihi.transpose(-1, -2), rq, None) + (ilo.transpose(-1, -2) @ rq if lo else 0.0)    # [B,H,33,32]
    # la_bwd_kv_kernel
    ghi, glo = _split(dS[..., :C, :], lo)
    dv = _mm2(rk, ghi.transpose(-1, -2), glo.transpose(-1, -2) if lo else None)
    dk = _mm2(v, ghi, glo) + dS[..., C:, :]
    dk = torch.where(k > 0, dk, torch.zeros_like(dk))
    return out, _rows(dq, B, N, H).to(BF), _rows(dk, B, N, H).to(BF), _rows(dv, B, N, H).to(BF)


def cancelling_terms(qkv, dout, B, N, H, k_off, v_off):
    """sum of |terms| of dq = dU S + S[32] dU32 and of dk = v dS + dS[32], in fp64, as [B*N, D] each: what a rounding error
    of these sums is relative to where the terms cancel."""
    x = qkv.double()
    q, k, v = F.relu(_heads(x, 0, B, N, H)), F.relu(_heads(x, k_off, B, N, H)), _heads(x, v_off, B, N, H)
    dO = _heads(dout.double(), 0, B, N, H)
    S = F.pad(v, (0, 1), value=1.0).transpose(-1, -2) @ k
    U = q @ S.transpose(-1, -2)
    den = U[..., C:] + 1e-15
    dU = torch.cat([dO / den, -(dO * U[..., :C] / den).sum(-1, keepdim=True) / den], -1)
    dS = dU.transpose(-1, -2) @ q
    mq = dU[..., :C].abs() @ S[..., :C, :].abs() + S[..., C:, :].abs() * dU[..., C:].abs()
    mk = v.abs() @ dS[..., :C, :].abs() + dS[..., C:, :].abs()
    return _rows(mq, B, N, H), _rows(mk, B, N, H)


CANCEL_REL = 2.0 ** -15


@functools.lru_cache(maxsize=None)
def case(kind, B, N, H, seed=0):
    """One test case on the packed layout: inputs, fp64 truth and fp32 -> bf16 flow of out, dq, dk, dv (each [B*N, D])."""
    D = C * H
    qkv, dout = make_inputs(kind, B, N, H, seed)
    c = {"kind": kind, "B": B, "N": N, "H": H, "qkv": qkv, "dout": dout}
    for key, dtype in (("truth", torch.float64), ("flow", torch.float32)):
        out, g = reference_fwd_bwd(qkv, dout, B, N, H, D, 2 * D, dtype)
        r = {"out": out, "dq": g[:, :D], "dk": g[:, D:2 * D], "dv": g[:, 2 * D:]}
        c[key] = {n: (t if dtype == torch.float64 else t.to(BF)) for n, t in r.items()}
    if N == 1:
        c["cancel"] = dict(zip(("dq", "dk"), cancelling_terms(qkv, dout, B, N, H, D, 2 * D)))
    return c


def flip_rates(got, c):
    """{tensor: fraction of elements that are not the correctly rounded truth}, over all heads"""
    return {n: flips(got[n], c["truth"][n]) / c["truth"][n].numel() for n in ("out", "dq", "dk", "dv")}


def conditions(got, c, name, flip_cap=True):
    """What a result {out, dq, dk, dv: bf16 [B*N, D]} of case `c` is held to, per head and per tensor:
    (a) finite, and exactly zero on a dead head; (b) as_good_as(result, flow, truth); (c) the flip cap.
    N = 1 is the one exception, for dq and dk only: S = [v;1] relu(k)^T has rank one, so out = v whatever q and k are, and
    dq = dk = 0 in exact arithmetic -- the fp64 "truth" is its own rounding noise (1e-17) and no relative measure against
    it means anything.  There |result| <= 2^-15 * sum |terms| of the cancelling sum, per element: each of the hi + lo splits
    (S, dU, dS) leaves <= 2^-17 of its operand, the product lo.lo that dq drops is <= 2^-18 of a term, and the fp32 roundings
    around them (1 / den, dO / den, the dO.O sum) are 2^-24 each: under 2^-16 of sum |terms| together, held with a factor 2.
    A hi-only dq leaves 2^-9.  Failures are collected the way close() / as_good_as() collect them."""
    B, N, H = c["B"], c["N"], c["H"]
    for n in ("out", "dq", "dk", "dv"):
        g = got[n].detach().cpu()
        if not torch.isfinite(g.float()).all():
            _FAILS.append(f"{name} {n}: non-finite output")
            print(f"[parity] {name} {n}: NON-FINITE")
            continue
        for h in range(H):
            cols = slice(C * h, C * h + C)
            gh, fh, th = g[:, cols], c["flow"][n][:, cols], c["truth"][n][:, cols]
            tag = f"{name} {n} head {h}"
            if h in DEAD_HEADS.get(c["kind"], ()):
                bad = int((gh.float() != 0).sum())
                print(f"[parity] {tag}: dead head, {bad} non-zero elements")
                if bad:
                    _FAILS.append(f"{tag}: {bad} non-zero elements on a dead head")
                continue
            if n in c.get("cancel", ()):
                worst = (gh.double().abs() / c["cancel"][n][:, cols].clamp_min(1e-300)).max().item()
                print(f"[parity] {tag}: exactly 0 in exact arithmetic, max |result| / sum |terms| = {worst:.3e}"
                      f" (flow {(fh.double().abs() / c['cancel'][n][:, cols].clamp_min(1e-300)).max().item():.3e})")
                if worst > CANCEL_REL:
                    _FAILS.append(f"{tag}: {worst:.3e} of the cancelling terms is left > {CANCEL_REL:.3e}")
                continue
            as_good_as(gh, fh, th, tag)
            if flip_cap:
                nf, cap = flips(gh, th), FLIP_CAP * th.numel() + FLIP_FREE
                print(f"[parity] {tag}: flips {nf} of {th.numel()} (flow {flips(fh, th)}, cap {cap:.1f})")
                if nf > cap:
                    _FAILS.append(f"{tag}: {nf} elements differ from the rounded fp64 result > {cap:.1f}")
