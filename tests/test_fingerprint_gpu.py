"""yat_fingerprint_u64 (csrc/fingerprint.hip) and ``ops.fingerprint`` against the numpy uint64 restatement below, exactly.

The restatement is the specification (include/yat_hip.h): the buffer is n little-endian 32-bit words w_i; with g = word_offset + i
and x = (g << 32) ^ (g >> 32) ^ w_i the term is the splitmix64 finalizer of x + 0x9E3779B97F4A7C15 (the multipliers and shifts of
tests/glue_ref.py's dropout mask), and the fingerprint is the sum of the terms mod 2^64.  Launch shape the sizes are chosen
around: 256 lanes x one 16-byte load = 1024 words per workgroup and pass, a grid capped at 2048 workgroups (so 2048 x 1024
words is the first wrap), four loads in flight per lane.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
WG_SPAN = 256 * 4                  # words one workgroup covers per pass
GRID_SPAN = 2048 * WG_SPAN         # words the capped grid covers per pass
U64 = np.uint64


def fp_ref(words, word_offset=0):
    """``words``: numpy uint32 -> Python int in [0, 2^64)"""
    with np.errstate(over="ignore"):
        g = np.arange(words.size, dtype=U64) + U64(word_offset & M64)
        z = ((g << U64(32)) ^ (g >> U64(32)) ^ words.astype(U64)) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        return int(z.sum(dtype=U64)) & M64


def fp_py(words, word_offset=0):
    """the same in pure-Python integers (no numpy wrap-around to trust)"""
    total = 0
    for i, w in enumerate(words):
        g = (word_offset + i) & M64
        z = ((((g << 32) & M64) ^ (g >> 32) ^ int(w)) + 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        total = (total + (z ^ (z >> 31))) & M64
    return total


def _words(n, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _dev(words):
    """uint32 words on the device, as an int32 tensor, with 64 canary words either side -> (view, whole, canary value)"""
    whole = torch.full((words.size + 128,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    whole[64:64 + words.size] = torch.from_numpy(words.view(np.int32)).cuda()
    return whole[64:64 + words.size], whole


def test_the_restatement_agrees_with_python_integers():
    for off in (0, 2 ** 32 - 1, 2 ** 40 + 5):
        w = _words(67, seed=off % 97)
        assert fp_ref(w, off) == fp_py(w.tolist(), off)


@pytest.mark.parametrize("n", [1, 3, 4, 63, 64, 65, 255, 256, 257, WG_SPAN - 1, WG_SPAN, WG_SPAN + 1, 4 * WG_SPAN + 3,
                               GRID_SPAN + 5, 4 * GRID_SPAN + WG_SPAN + 2])
def test_sizes_exact_and_canaries_untouched(n):
    from yat_amd import ops
    w = _words(n, seed=n)
    view, whole = _dev(w)
    assert ops.fingerprint(view) == fp_ref(w)
    torch.cuda.synchronize()
    assert (whole[:64] == 0x5A5A5A5A).all() and (whole[64 + n:] == 0x5A5A5A5A).all()
    assert np.array_equal(whole[64:64 + n].cpu().numpy().view(np.uint32), w)            # the input is only read


@pytest.mark.parametrize("offset", [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5])
@pytest.mark.parametrize("n", [5, 257])
def test_word_offsets(n, offset):
    from yat_amd import ops
    w = _words(n, seed=3)
    view, _ = _dev(w)
    assert ops.fingerprint(view, word_offset=offset) == fp_ref(w, offset)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
def test_views_of_other_dtypes(dtype):
    from yat_amd import ops
    w = _words(1000 + 3, seed=11)
    view, _ = _dev(w)
    t = view.view(dtype)
    assert t.numel() * t.element_size() == 4 * w.size
    assert ops.fingerprint(t) == fp_ref(w)
    assert ops.fingerprint(t.view(-1, 17) if t.numel() % 17 == 0 else t.view(1, -1)) == fp_ref(w)     # contiguous n-d


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 6, 1029])
def test_a_start_that_is_4_byte_but_not_16_byte_aligned(shift, n):
    from yat_amd import ops
    w = _words(n + 8, seed=shift)
    base = torch.from_numpy(w.view(np.int32)).cuda()
    assert base.data_ptr() % 16 == 0
    view = base[shift:shift + n]
    assert view.data_ptr() % 16 == 4 * shift
    assert ops.fingerprint(view) == fp_ref(w[shift:shift + n])


@pytest.mark.parametrize("cuts", [[700], [1, 1030], [5, 9, 1024, 1025, 2051, 3000]])
def test_additivity_over_uneven_slices(cuts):
    """fp(whole) = the sum of fp(slices), each with its own word_offset: accumulate adds them up on the device, in any order"""
    from yat_amd import ops
    n = 4099
    w = _words(n, seed=len(cuts))
    view, _ = _dev(w)
    want = fp_ref(w, 77)
    bounds = [0] + cuts + [n]
    pieces = list(zip(bounds[:-1], bounds[1:]))
    assert len(pieces) in (2, 3, 7)
    out = torch.full((1,), 123, dtype=torch.int64, device="cuda")            # (accumulate = 0 overwrites whatever is there)
    for k, (lo, hi) in enumerate(reversed(pieces)):
        ops.fingerprint(view[lo:hi], word_offset=77 + lo, out=out, accumulate=k > 0)
    assert int(out.item()) & M64 == want
    assert sum(ops.fingerprint(view[lo:hi], word_offset=77 + lo) for lo, hi in pieces) & M64 == want
    assert ops.fingerprint(view, word_offset=77) == want


def test_sensitivity():
    from yat_amd import ops
    n = 2 * WG_SPAN + 7
    w = _words(n, seed=5)
    view, _ = _dev(w)
    base = ops.fingerprint(view)
    for i, bit in ((0, 0), (n - 1, 31), (WG_SPAN + 1, 15)):
        flipped = w.copy()
        flipped[i] ^= np.uint32(1 << bit)
        v, _ = _dev(flipped)
        got = ops.fingerprint(v)
        assert got == fp_ref(flipped) and got != base
    swapped = w.copy()
    assert swapped[3] != swapped[n - 2]
    swapped[3], swapped[n - 2] = w[n - 2], w[3]
    v, _ = _dev(swapped)
    got = ops.fingerprint(v)
    assert got == fp_ref(swapped) and got != base
    z = torch.zeros(1030, dtype=torch.int32, device="cuda")
    a, b = ops.fingerprint(z[:1029]), ops.fingerprint(z)
    assert a == fp_ref(np.zeros(1029, np.uint32)) and b == fp_ref(np.zeros(1030, np.uint32)) and a != b


def test_the_wrapper_refuses_before_any_library_call(monkeypatch):
    from yat_amd import ops

    def boom():
        raise AssertionError("the library was reached")
    t = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    good = ops.fingerprint(t)
    monkeypatch.setattr(ops, "_lib", boom)
    with pytest.raises(ValueError, match="contiguous"):
        ops.fingerprint(t[::2])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.fingerprint(t[:63])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.fingerprint(t.view(torch.uint8)[:6])
    with pytest.raises(ValueError, match="4-byte aligned"):
        ops.fingerprint(t[1:63])                                          # 124 bytes from a 2-byte offset
    with pytest.raises(ValueError, match="accumulate needs out"):
        ops.fingerprint(t, accumulate=True)
    with pytest.raises(ValueError, match="word_offset"):
        ops.fingerprint(t, word_offset=-1)
    monkeypatch.undo()
    assert ops.fingerprint(t) == good == fp_ref(np.zeros(32, np.uint32))


def test_host_restatement_of_the_trainer_state_agrees():
    """common/trainer_state.py ``fingerprint_host`` (what checks a saved file without a GPU) is the same function"""
    from yat_amd import ops
    from yat_amd.common.trainer_state import fingerprint_host
    t = torch.randn(4104, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    assert fingerprint_host(t) == ops.fingerprint(t.cuda()) == fp_ref(t.view(torch.int32).numpy().view(np.uint32))
