"""numpy restatement of the DenseNet encoder's dropout mask (emlight_amd/csrc/eml_dropout.h), for the tests and the fixture.

The draw of output channel c (0..11) of global dense layer `layer` at flat pixel q = (b*H + h)*W + w is word c % 4 of
Philox-4x32-10(counter (q, c // 4, layer, 0), key (seed & 0xffffffff, seed >> 32)); the element is kept iff
draw >= floor(p * 2**32), and kept values are scaled by 1 / (1 - p)."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123's Philox-4x32-10 on arrays of 32-bit values (held as uint64)."""
    c = [np.asarray(v, np.uint64) & _M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    for i in range(10):
        if i:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
    return c


def draws(seed, layer, P):
    """(P, 12) uint64 array of the 32-bit draws of one layer over pixels 0..P-1."""
    q = np.arange(P, dtype=np.uint64)
    seed = int(seed)
    out = np.empty((P, 12), np.uint64)
    for grp in range(3):
        w = philox4x32_10(q, grp, layer, 0, seed & 0xFFFFFFFF, seed >> 32)
        for j in range(4):
            out[:, 4 * grp + j] = w[j]
    return out


def keep_mask(seed, layer, p, P):
    """(P, 12) bool: channel kept at pixel q."""
    return draws(seed, layer, P) >= np.uint64(int(np.floor(p * 2.0 ** 32)))


def mask_words(seed, layer, p, P):
    """(P,) uint16: bit c set iff channel c is kept (what eml_dense_dropout_mask_u16 writes)."""
    k = keep_mask(seed, layer, p, P)
    return (k.astype(np.uint16) << np.arange(12, dtype=np.uint16)).sum(1).astype(np.uint16)


def scaled_mask_nchw(seed, layer, p, B, H, W):
    """(B, 12, H, W) f64 multiplier of a layer's new channels: mask / (1 - p) (0 everywhere for p == 1)."""
    k = keep_mask(seed, layer, p, B * H * W).reshape(B, H, W, 12).transpose(0, 3, 1, 2)
    return k * (0.0 if p >= 1 else 1.0 / (1.0 - p))
