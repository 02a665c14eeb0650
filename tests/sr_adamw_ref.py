"""numpy restatement of the stochastic-rounding AdamW step (csrc/optim.hip adamw_sr_kernel, include/yat_hip.h
yat_adamw_sr_step): Philox4x32, the assignment of its output bits to (global index, field), the rounding rule and one step in
float32 in the kernel's op order.  bf16 values travel as uint16 bit patterns.  Where the fp32 arithmetic of a step is exact (the
inputs of tests/test_sr_adamw_gpu.py), the kernel must reproduce ``adamw_sr_ref`` bit for bit."""
import math

import numpy as np

PHILOX_ROUNDS = 10          # csrc/optim.hip SR_PHILOX_ROUNDS: the two must agree
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
FIELD_P, FIELD_EXP_AVG, FIELD_EXP_AVG_SQ, FIELD_EMA = 0, 1, 2, 3
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=PHILOX_ROUNDS):
    """counter: 4 words, key: 2 words (ints or uint32 arrays that broadcast) -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in counter]
    k = [int(x) & 0xFFFFFFFF for x in key]
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & _M32]
        k = [(k[0] + PHILOX_W0) & 0xFFFFFFFF, (k[1] + PHILOX_W1) & 0xFFFFFFFF]
    return [x.astype(np.uint32) for x in c]


def sr_words(seed, rng_step, idx, rounds=PHILOX_ROUNDS):
    """The two 32-bit words (wa, wb) of the parameters at global indices ``idx``: one Philox call per pair ``idx >> 1``, the
    even parameter takes (w0, w1), the odd one (w2, w3)."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed, rng_step = int(seed) & (2 ** 64 - 1), int(rng_step) & (2 ** 64 - 1)
    key, step = (seed & 0xFFFFFFFF, seed >> 32), (rng_step & 0xFFFFFFFF, rng_step >> 32)
    n = idx.size
    if idx.ndim == 1 and n and n % 2 == 0 and int(idx[0]) % 2 == 0 and int(idx[-1]) - int(idx[0]) == n - 1 and np.all(np.diff(idx) == 1):
        j = idx[::2] >> np.uint64(1)                       # a run of whole pairs: one call each, outputs interleaved
        w = philox4x32((j & _M32, j >> np.uint64(32), *step), key, rounds)
        return np.stack([w[0], w[2]], 1).reshape(-1), np.stack([w[1], w[3]], 1).reshape(-1)
    j = idx >> np.uint64(1)
    w = philox4x32((j & _M32, j >> np.uint64(32), *step), key, rounds)
    odd = (idx & np.uint64(1)).astype(bool)
    return np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])


def field_bits(words, field):
    word = words[0] if field in (FIELD_P, FIELD_EXP_AVG) else words[1]
    return (word & np.uint32(0xFFFF)) if field in (FIELD_P, FIELD_EXP_AVG_SQ) else (word >> np.uint32(16))


def sr_bits(seed, rng_step, idx, field, rounds=PHILOX_ROUNDS):
    """The 16 random bits of ``field`` of the parameters at global indices ``idx`` -> uint32 array (< 65536)."""
    return field_bits(sr_words(seed, rng_step, idx, rounds), field)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rne_bf16(x):
    """float32 -> bf16 bits, round to nearest even; a NaN keeps its sign and top payload bits and is made quiet."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint16)
    nan = ((u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((u & np.uint32(0x007FFFFF)) != 0)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), r)


def sr_bf16_r(x, r):
    """The rule itself: finite x -> top 16 bits of (bits + r), 32-bit add; NaN / +-Inf -> round to nearest."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    finite = (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    s = (((u.astype(np.uint64) + np.asarray(r, dtype=np.uint64)) & _M32) >> np.uint64(16)).astype(np.uint16)
    return np.where(finite, s, rne_bf16(x))


def sr_bf16(x, seed, rng_step, idx, field, rounds=PHILOX_ROUNDS):
    return sr_bf16_r(x, sr_bits(seed, rng_step, idx, field, rounds))


def adam_scalars(lr, beta1, beta2, eps, weight_decay, step, ema_decay):
    """csrc/optim.hip adam_scalars: prepared in double, narrowed to float."""
    f = np.float32
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return dict(use_wd=weight_decay != 0.0, wd_mul=f(1.0 - lr * weight_decay), w1=f(1.0 - beta1), beta2=f(beta2), om_b2=f(1.0 - beta2),
                bc2_sqrt=f(math.sqrt(bc2)), neg_step_size=f(-(lr / bc1)), eps=f(eps), ema_omd=f(1.0 - ema_decay))


def adamw_sr_ref(p, g, m, v, coef, lr, beta1, beta2, eps, weight_decay, step, ema=None, ema_decay=0.0, seed=0, rng_step=0,
                 elem_offset=0, rounds=PHILOX_ROUNDS, dtype=np.float32, rounded=True, p_stored=None):
    """One step on bf16 bit patterns (uint16 arrays) -> (p, m, v, ema or None) as bit patterns.  ``dtype=np.float64,
    rounded=False`` returns the unrounded float64 values instead; the shadow then follows ``p_stored``, the bf16 parameters some
    run of the step has written (without it: the unrounded parameters)."""
    a = adam_scalars(lr, beta1, beta2, eps, weight_decay, step, ema_decay)
    T = dtype
    pf, gf, mf, vf = (bf16_to_f32(x).astype(T) for x in (p, g, m, v))
    idx = np.uint64(elem_offset) + np.arange(pf.size, dtype=np.uint64)
    with np.errstate(all="ignore"):
        gr = gf * T(coef) if coef is not None else gf
        if a["use_wd"]:
            pf = pf * T(a["wd_mul"])
        mf = mf + T(a["w1"]) * (gr - mf)
        vf = vf * T(a["beta2"])
        vf = vf + (T(a["om_b2"]) * gr) * gr
        den = np.sqrt(vf) / T(a["bc2_sqrt"]) + T(a["eps"])
        pf = pf + T(a["neg_step_size"]) * mf / den
        if rounded:
            words = sr_words(seed, rng_step, idx, rounds)
            po = sr_bf16_r(pf, field_bits(words, FIELD_P))
            mo = sr_bf16_r(mf, field_bits(words, FIELD_EXP_AVG))
            vo = sr_bf16_r(vf, field_bits(words, FIELD_EXP_AVG_SQ))
            ps = bf16_to_f32(po).astype(T)
        else:
            po, mo, vo = pf, mf, vf
            ps = pf if p_stored is None else bf16_to_f32(p_stored).astype(T)
        so = None
        if ema is not None:
            sf = bf16_to_f32(ema).astype(T)
            sf = sf - T(a["ema_omd"]) * (sf - ps)
            so = sr_bf16_r(sf, field_bits(words, FIELD_EMA)) if rounded else sf
    return po, mo, vo, so
