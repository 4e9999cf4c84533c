"""The numpy reference of the engine's random streams (philox_reference.py), checked on the host: the published Random123
known-answer vectors, two independent forms of the round's multiply, the uniform's range, and the committed extreme tuples.
Nothing here looks at the kernel: the reference has to be right on its own before the device is compared with it."""
import math

import numpy as np
import pytest

import philox_reference as P

# Random123 kat_vectors, philox4x32 with 10 rounds: counter x4, key x2 -> output x4
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('mulhilo', [P.mulhilo_wide, P.mulhilo_limbs])
def test_known_answer_vectors(mulhilo):
    for counter, key, want in KAT:
        got = P.philox4x32_10(counter, key, mulhilo)
        assert got.dtype == np.uint32 and got.shape == (4,)
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]
    # vectorised over leading axes: the three at once give the three rows
    got = P.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]), mulhilo)
    assert got.tolist() == [list(k[2]) for k in KAT]


def test_two_forms_of_the_multiply_agree():
    rng = np.random.default_rng(2011)
    a = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64)
    b = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64)
    a[:4], b[:4] = (0, 0xFFFFFFFF, 0xFFFFFFFF, 1), (0, 0xFFFFFFFF, 1, 0xFFFFFFFF)
    for x, y in ((a, b), (np.uint64(P.PHILOX_M0), a), (np.uint64(P.PHILOX_M1), b)):
        h1, l1 = P.mulhilo_wide(x, y)
        h2, l2 = P.mulhilo_limbs(x, y)
        assert np.array_equal(h1, h2) and np.array_equal(l1, l2)
    assert [int(v) for v in P.mulhilo_limbs(0xFFFFFFFF, 0xFFFFFFFF)] == [0xFFFFFFFE, 0x00000001]
    counter = rng.integers(0, 2 ** 32, (100000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (100000, 2), dtype=np.uint64)
    assert np.array_equal(P.philox4x32_10(counter, key, P.mulhilo_wide), P.philox4x32_10(counter, key, P.mulhilo_limbs))


def test_every_counter_and_key_word_matters():
    """A one-bit change in any of the six input words changes the block (the reference carries no dead input)."""
    base_c, base_k = np.array([5, 6, 7, 8], np.uint64), np.array([9, 10], np.uint64)
    base = P.philox4x32_10(base_c, base_k)
    seen = {tuple(base.tolist())}
    for j in range(4):
        c = base_c.copy()
        c[j] ^= np.uint64(1)
        seen.add(tuple(P.philox4x32_10(c, base_k).tolist()))
    for j in range(2):
        k = base_k.copy()
        k[j] ^= np.uint64(1)
        seen.add(tuple(P.philox4x32_10(base_c, k).tolist()))
    assert len(seen) == 7


def test_uniform24_range_and_radius():
    tops = np.unique(np.concatenate([np.arange(0, 4096), np.arange(2 ** 23 - 4096, 2 ** 23 + 4096), np.arange(2 ** 24 - 4096, 2 ** 24),
                                     np.random.default_rng(24).integers(0, 2 ** 24, 1 << 20)])).astype(np.uint32)   # sorted
    for low in (0x00, 0xFF):                                     # the low byte is discarded
        u = P.uniform24((tops << np.uint32(8)) | np.uint32(low))
        assert u.dtype == np.float32
        assert (u > 0).all() and (u <= 1).all()
        assert np.array_equal(tops[u == 1.0], np.array([0xFFFFFF], np.uint32))
        assert (np.diff(u) >= 0).all()   # monotone (ties from round-to-even above 2^23)
    assert float(P.uniform24(0)) == 2.0 ** -25
    assert float(P.uniform24(0xFFFFFF00)) == 1.0
    assert float(P.uniform24(0xFFFFFE00)) == 1.0 - 2.0 ** -23   # 0xFFFFFE + 0.5 ties to even 0xFFFFFE = 2^24 - 2
    assert float(P.uniform24(0x80000100)) == (2 ** 23 + 2) * 2.0 ** -24   # 2^23 + 1.5 -> 2^23 + 2
    # radius: finite everywhere, largest at word 0, zero only at u = 1
    r = np.sqrt(-2.0 * np.log(P.uniform24(tops << np.uint32(8)).astype(np.float64)))
    assert np.isfinite(r).all()
    r_max = math.sqrt(-2.0 * math.log(2.0 ** -25))
    assert abs(r_max - 5.887) < 1e-3
    assert r.max() == r_max and int(tops[np.argmax(r)]) == 0
    assert np.array_equal(tops[r == 0], np.array([0xFFFFFF], np.uint32))


def test_box_muller_channels():
    words = np.array([[0x00000000, 0x00000000, 0xFFFFFFFF, 0x40000000],       # r0 max, angle ~0; r1 = 0
                      [0x80000000, 0x40000000, 0x80000000, 0x80000000]], np.uint32)
    z = P.box_muller(words)
    u = P.uniform24(words).astype(np.float64)
    assert z.shape == (2, 3) and z.dtype == np.float64
    assert abs(z[0, 0] - 5.887) < 1e-3 and abs(z[0, 1]) < 1e-5 and z[0, 2] == 0.0
    r0 = math.sqrt(-2 * math.log(u[1, 0]))
    assert z[1, 0] == r0 * math.cos(2 * math.pi * u[1, 1])       # channel 0: cosine of the SECOND word's angle
    assert z[1, 1] == r0 * math.sin(2 * math.pi * u[1, 1])       # channel 1: its sine (close to r0: a quarter turn)
    assert z[1, 1] > 0.99 * r0 and abs(z[1, 0]) < 1e-5 * r0
    assert z[1, 2] == math.sqrt(-2 * math.log(u[1, 2])) * math.cos(2 * math.pi * u[1, 3]) < 0   # half a turn


def test_randn_plane_layout_and_key():
    z = P.randn_plane(77, 3, 5, 3, 4, 6)
    assert z.shape == (3, 3, 4, 6) and z.dtype == np.float64
    # pixel (n, y, x) is counter i = n*H*W + y*W + x; a shard is a slice of the full batch
    w = P.noise_words(77, 3, 5, np.array([1 * 24 + 2 * 6 + 3], np.uint64))
    assert np.array_equal(z[1, :, 2, 3], P.box_muller(w)[0])
    assert np.array_equal(P.randn_plane(77, 3, 5, 2, 4, 6, first_image=1), z[1:])
    # the words are philox(counter = (i lo, i hi, plane, calls lo), key = (seed lo, seed hi ^ calls hi))
    seed, calls, i = 0x0123456789ABCDEF, (7 << 32) | 9, (3 << 32) | 11
    want = P.philox4x32_10([11, 3, 5, 9], [0x89ABCDEF, 0x01234567 ^ 7])
    assert np.array_equal(P.noise_words(seed, calls, 5, np.array([i], np.uint64))[0], want)
    for other in (P.randn_plane(78, 3, 5, 3, 4, 6), P.randn_plane(77 + 2 ** 32, 3, 5, 3, 4, 6), P.randn_plane(77, 4, 5, 3, 4, 6),
                  P.randn_plane(77, 3, 6, 3, 4, 6), P.randn_plane(77, 5, 3, 3, 4, 6)):
        assert not np.array_equal(other, z)
    big = P.randn_plane(1, 0, 0, 4, 256, 256)                     # sanity only: the stream looks N(0,1)
    assert abs(big.mean()) < 5 / math.sqrt(big.size) and abs(big.var() - 1) < 5 * math.sqrt(2 / big.size)


def test_dropout_keep_layout_and_key():
    assert P.dropout_threshold(0.5) == 2 ** 31
    assert P.dropout_threshold(0.2) == int(float(np.float32(0.2)) * 2 ** 32) == 858993472   # p is the fp32 the engine holds
    assert P.dropout_threshold(0.0) == 0 and P.dropout_threshold(1.0) == 2 ** 32 - 1
    seed, step, slot = 0xFEDCBA9876543210, 3, 2
    keep = P.dropout_keep(seed, step, slot, 0.5, 64)
    assert keep.dtype == np.uint8 and keep.shape == (64,) and set(keep.tolist()) <= {0, 1}
    words = P.philox4x32_10([5, 0, slot, step], [0x76543210 ^ 0x44524F50, 0xFEDCBA98])
    assert np.array_equal(keep[20:24], (words >= np.uint32(2 ** 31)).astype(np.uint8))     # quad 5 = elements 20..23
    assert np.array_equal(P.dropout_keep(seed, step, slot, 0.5, 32, first_elem=32), keep[32:])
    assert P.dropout_keep(seed, step, slot, 0.0, 64).all()
    n = 1 << 18
    a, b, c = (P.dropout_keep(seed, st, sl, 0.2, n) for st, sl in ((1, 0), (1, 1), (2, 0)))
    band = 5 * math.sqrt(0.32 * 0.68 / n)
    assert abs(a.mean() - 0.8) < 5 * math.sqrt(0.16 / n)
    assert abs((a != b).mean() - 0.32) < band and abs((a != c).mean() - 0.32) < band   # 2p(1-p): slots and steps are independent


def test_committed_extreme_tuples():
    """The tuples the GPU test visits really are what they claim: radius word >> 8 == 0 / 0xFFFFFF at that pixel of a
    (4,256,256) draw at calls = 0, one of each kind for the channel pair (word 0) and for channel 2 (word 2)."""
    assert {(k, w) for k, _, _, _, w in P.EXTREME_TUPLES} == {('zero', 0), ('zero', 2), ('ones', 0), ('ones', 2)}
    for kind, seed, plane, i, word in P.EXTREME_TUPLES:
        assert 0 <= i < 4 * 256 * 256
        w = P.noise_words(seed, 0, plane, np.array([i], np.uint64))[0]
        assert int(w[word]) >> 8 == (0 if kind == 'zero' else 0xFFFFFF), (kind, hex(int(w[word])))
        z = P.randn_plane(seed, 0, plane, 4, 256, 256).transpose(0, 2, 3, 1).reshape(-1, 3)[i]
        chans = (0, 1) if word == 0 else (2,)
        if kind == 'ones':
            assert all(z[c] == 0.0 for c in chans)
        else:
            assert abs(math.sqrt(sum(z[c] ** 2 for c in chans)) - 5.887) < (1e-3 if word == 0 else 5.887)
            assert all(abs(z[c]) <= 5.8871 for c in chans)


def test_fp32_restatement_gap_is_small_and_not_zero():
    """The bar of the device comparison is 4x this figure; it has to be a real fp32-vs-fp64 distance: above the rounding of one
    fp32 product at |z| ~ 1 and far below anything that could hide a wrong word (adjacent 24-bit uniforms move z by >= 3e-8 / u)."""
    gap = P.fp32_restatement_gap()
    print(f'fp32 restatement vs fp64 reference, 3 x 2^20 normals: max |d| = {gap:.3e}')
    assert 2.0 ** -24 < gap < 1e-5
