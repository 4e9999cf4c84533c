"""Plain-numpy reference for the engine's three random streams (no GPU, no fixtures, no hooks).

Written from Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3" (SC'11) and from the stream
description in include/fdsr.h -- not from the kernel.  Philox4x32-10: a 4-word counter, a 2-word key, ten rounds of

    (c0, c1, c2, c3) <- (mulhi(M1, c2) ^ c1 ^ k0,  mullo(M1, c2),  mulhi(M0, c0) ^ c3 ^ k1,  mullo(M0, c0))

with M0 = 0xD2511F53, M1 = 0xCD9E8D57, and the key bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.

Streams (word j of the counter / key, 32 bits each):

    stream                    counter                                   key
    sampler noise, plane p    (i lo, i hi, p, calls lo)                 (seed lo, seed hi ^ calls hi)    i = n*H*W + pixel
    self-drawn training eps   the same with p = 0
    dropout keep bytes        (quad lo, quad hi, slot, step)            (seed lo ^ 0x44524F50, seed hi)  quad = element // 4

Output words (w0, w1, w2, w3) of a noise counter give three normals by Box-Muller on 24-bit uniforms:
channel 0 = r0 cos(2 pi u1), channel 1 = r0 sin(2 pi u1), channel 2 = r1 cos(2 pi u3), r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2).
Output word e of a dropout counter decides element 4*quad + e: keep = word >= min(floor(p * 2^32), 2^32 - 1)."""
import numpy as np

PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9      # golden ratio
PHILOX_W1 = 0xBB67AE85      # sqrt(3) - 1
DROPOUT_KEY_XOR = 0x44524F50   # 'DROP'
MASK32 = 0xFFFFFFFF

_U = np.uint64
_M32 = _U(MASK32)
_S32 = _U(32)


def mulhilo_wide(a, b):
    """(high, low) 32-bit halves of the 32x32 -> 64 product, through one uint64 multiply."""
    p = np.asarray(a, _U) * np.asarray(b, _U)
    return p >> _S32, p & _M32


def mulhilo_limbs(a, b):
    """The same product from 16-bit limbs (schoolbook, no intermediate above 2^34): an independent second form."""
    a, b = np.asarray(a, _U), np.asarray(b, _U)
    m16, s16 = _U(0xFFFF), _U(16)
    a0, a1, b0, b1 = a & m16, a >> s16, b & m16, b >> s16
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s16) + (p01 & m16) + (p10 & m16)
    lo = (p00 & m16) | ((mid & m16) << s16)
    hi = p11 + (p01 >> s16) + (p10 >> s16) + (mid >> s16)
    return hi, lo


def philox4x32_10(counter, key, mulhilo=mulhilo_wide):
    """counter [..., 4], key [..., 2] (broadcast against each other over the leading axes) -> words [..., 4], uint32."""
    counter, key = np.asarray(counter, _U), np.asarray(key, _U)
    assert counter.shape[-1] == 4 and key.shape[-1] == 2
    assert (counter <= _M32).all() and (key <= _M32).all()
    c0, c1, c2, c3 = (counter[..., j] for j in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for r in range(10):
        if r:
            k0 = (k0 + _U(PHILOX_W0)) & _M32
            k1 = (k1 + _U(PHILOX_W1)) & _M32
        hi0, lo0 = mulhilo(_U(PHILOX_M0), c0)
        hi1, lo1 = mulhilo(_U(PHILOX_M1), c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def uniform24(word):
    """The uniform of one output word, in (0, 1]: (float32(word >> 8) + 0.5f) * 2^-24, both operations in fp32 ON PURPOSE.

    For word >> 8 >= 2^23 the sum is not representable and rounds to even, so 0xFFFFFF gives exactly 1.0 (radius 0).  Both operations
    are single correctly rounded IEEE operations, so this is the same number on every machine; a uniform formed in fp64 would differ
    from it by up to 2^-25 and move z by up to 1e-4 near u -> 1."""
    w = np.asarray(word, np.uint32) >> np.uint32(8)
    return (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def noise_words(seed, calls, plane, index):
    """Output words [..., 4] of the sampler stream for flat pixel indices `index` (i = n*H*W + pixel of the full batch)."""
    seed, calls, plane = int(seed), int(calls), int(plane)
    assert 0 <= seed < 2 ** 64 and 0 <= calls < 2 ** 64 and 0 <= plane < 2 ** 32
    i = np.asarray(index, _U)
    counter = np.stack([i & _M32, i >> _S32, np.full_like(i, plane), np.full_like(i, calls & MASK32)], axis=-1)
    key = np.array([seed & MASK32, (seed >> 32) ^ (calls >> 32)], _U)
    return philox4x32_10(counter, key)


def box_muller(words, dtype=np.float64):
    """words [..., 4] -> normals [..., 3].  dtype float64: the reference.  dtype float32: the same formula with every operation in
    numpy fp32 (angle = float32(2 pi) * u), used only to measure how far an fp32 evaluation sits from the fp64 one."""
    u = uniform24(words).astype(dtype)
    two_pi = dtype(2.0 * np.pi)
    r0 = np.sqrt(dtype(-2.0) * np.log(u[..., 0]))
    r1 = np.sqrt(dtype(-2.0) * np.log(u[..., 2]))
    a0, a1 = two_pi * u[..., 1], two_pi * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=-1)


def randn_plane(seed, calls, plane, B, H, W, first_image=0):
    """float64 [B, 3, H, W]: noise plane `plane` of call `calls` under `seed`, for images [first_image, first_image + B) of a batch."""
    i = np.arange(first_image * H * W, (first_image + B) * H * W, dtype=_U)
    z = box_muller(noise_words(seed, calls, plane, i))                      # [B*H*W, 3]
    return np.ascontiguousarray(z.reshape(B, H, W, 3).transpose(0, 3, 1, 2))


def dropout_threshold(p):
    """min(floor(p * 2^32), 2^32 - 1), with p the fp32 value the engine holds."""
    return min(int(float(np.float32(p)) * 4294967296.0), MASK32)


def dropout_keep(seed, step, slot, p, n_elems, first_elem=0):
    """uint8 [n_elems]: keep byte of elements [first_elem, first_elem + n_elems) of a block's NHWC activation."""
    seed, step, slot = int(seed), int(step), int(slot)
    assert n_elems % 4 == 0 and first_elem % 4 == 0
    assert 0 <= seed < 2 ** 64 and 0 <= step < 2 ** 32 and 0 <= slot < 2 ** 32
    q = np.arange(first_elem // 4, (first_elem + n_elems) // 4, dtype=_U)
    counter = np.stack([q & _M32, q >> _S32, np.full_like(q, slot), np.full_like(q, step)], axis=-1)
    key = np.array([(seed & MASK32) ^ DROPOUT_KEY_XOR, seed >> 32], _U)
    words = philox4x32_10(counter, key)                                     # [nq, 4]: word e is element 4*q + e
    return (words >= np.uint32(dropout_threshold(p))).astype(np.uint8).reshape(-1)


def fp32_restatement_gap(n_counters=1 << 20, seed=0x5EED, calls=0):
    """max |box_muller fp32 - box_muller fp64| over n_counters counters (3 normals each) of the reference's own stream: how far an
    honest fp32 evaluation of the formula sits from the fp64 one.  The device bar is four times this (tests/test_gpu_rng_reference.py)."""
    words = noise_words(seed, calls, 0, np.arange(n_counters, dtype=_U))
    z64 = box_muller(words, np.float64)
    z32 = box_muller(words, np.float32)
    assert z32.dtype == np.float32
    return float(np.abs(z32.astype(np.float64) - z64).max())


# Extreme radius words of a (4, 256, 256) draw at calls = 0, found once with this module by scanning seeds 0.. x planes 0..
# (2^18 counters per (seed, plane), budget 2^26 counters): (kind, seed, plane, flat index i, word index).  word index 0 is the radius
# of channels 0 and 1, word index 2 that of channel 2.  'zero': word >> 8 == 0 (u = 2^-25, the largest radius 5.887);
# 'ones': word >> 8 == 0xFFFFFF (u = 1, radius 0).  tests/test_philox_reference_host.py re-derives the words.
EXTREME_TUPLES = (
    ('ones', 1, 6, 147826, 0),
    ('ones', 1, 11, 181690, 2),
    ('zero', 1, 12, 38849, 0),
    ('zero', 7, 2, 137486, 2),
)


def search_extremes(n_seeds=16, n_planes=16, pixels=4 * 256 * 256):
    """The scan that produced EXTREME_TUPLES (first hit of each kind and word in scan order); about ten seconds of numpy."""
    found = {}
    i = np.arange(pixels, dtype=_U)
    for seed in range(n_seeds):
        for plane in range(n_planes):
            top = noise_words(seed, 0, plane, i) >> np.uint32(8)
            for word in (0, 2):
                for kind, val in (('zero', 0), ('ones', 0xFFFFFF)):
                    hit = np.flatnonzero(top[:, word] == val)
                    if hit.size and (kind, word) not in found:
                        found[(kind, word)] = (kind, seed, plane, int(hit[0]), word)
    return tuple(found[k] for k in sorted(found))
