"""TEST INFRASTRUCTURE - numpy restatement of the library's dropout masks, written from the text of include/cdseg.h
("dropout") on top of oracle/philox.py (Philox4x32-10, pinned to Random123's known answers in tests/test_oracle.py).

A site is (seed, offset); W(t) = philox4x32_10((t low, t high, offset low, offset high), (seed low, seed high)) - the words
cdseg_rand_int writes at out[4 t .. 4 t + 3].  An element is kept iff its byte < T, T = floor(256 (1 - rate) + 1/2) >= 1.
  attention (patch p, head h, query slot i, key slot j): t = (j >> 2) | (i >> 2) << 8 | h << 16 | p << 32, word i & 3, byte j & 3
  element (row r, column c):                             t = (c >> 4) | r << 32,                          word (c >> 2) & 3, byte c & 3
"""
import math

import numpy as np

from oracle import philox

_M32 = 0xFFFFFFFF


def threshold(rate):
    rate = float(rate)
    assert 0.0 <= rate < 1.0
    return max(1, int(math.floor(256.0 * (1.0 - rate) + 0.5)))


def keep_prob(rate):
    return threshold(rate) / 256.0


def inv_keep(rate):
    """The fp32 factor kept values are multiplied by."""
    return np.float32(256.0) / np.float32(threshold(rate))


def counters(seed, offset, t_lo, t_hi):
    """(counter, key) arrays of the calls W(t), t = t_lo | t_hi << 32 (uint32 arrays of one shape)."""
    t_lo = np.asarray(t_lo, dtype=np.uint32)
    t_hi = np.broadcast_to(np.asarray(t_hi, dtype=np.uint32), t_lo.shape)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    ctr = np.stack([t_lo, t_hi, np.full(t_lo.shape, offset & _M32, dtype=np.uint32),
                    np.full(t_lo.shape, offset >> 32, dtype=np.uint32)], -1)
    key = np.stack([np.full(t_lo.shape, seed & _M32, dtype=np.uint32), np.full(t_lo.shape, seed >> 32, dtype=np.uint32)], -1)
    return ctr, key


def words(seed, offset, t_lo, t_hi):
    ctr, key = counters(seed, offset, t_lo, t_hi)
    return philox.philox4x32_10(ctr, key)


def attention_site(p, h, i, j):
    """(t low, t high, word, byte) of attention element (patch p, head h, query slot i, key slot j)."""
    return (j >> 2) | ((i >> 2) << 8) | (h << 16), p, i & 3, j & 3


def element_site(r, c):
    return c >> 4, r, (c >> 2) & 3, c & 3


def _bytes_of(w):
    """(..., 4 words) uint32 -> (..., 4 words, 4 bytes)"""
    return (w[..., None] >> (np.arange(4, dtype=np.uint32) * np.uint32(8))) & np.uint32(255)


def attention_bytes(seed, offset, L, p, h):
    """(L, L) uint8-valued array: the byte of (query i, key j) of patch p, head h."""
    nb = (L + 3) // 4
    ib, jb = np.meshgrid(np.arange(nb, dtype=np.uint32), np.arange(nb, dtype=np.uint32), indexing="ij")
    w = words(seed, offset, jb | (ib << np.uint32(8)) | np.uint32(h << 16), np.uint32(p))  # (nb, nb, 4)
    b = _bytes_of(w)  # (ib, jb, word = i & 3, byte = j & 3)
    return b.transpose(0, 2, 1, 3).reshape(4 * nb, 4 * nb)[:L, :L]


def attention_mask(seed, offset, rate, patch_lens, H):
    """Per patch a bool array (H, L, L): keep[h, i, j]."""
    T = threshold(rate)
    return [np.stack([attention_bytes(seed, offset, int(L), p, h) < T for h in range(H)]) for p, L in enumerate(patch_lens)]


def element_mask(seed, offset, rate, m, c):
    """bool (m, c): keep[r, col]."""
    T = threshold(rate)
    ng = (c + 15) // 16
    r, g = np.meshgrid(np.arange(m, dtype=np.uint32), np.arange(ng, dtype=np.uint32), indexing="ij")
    b = _bytes_of(words(seed, offset, g, r))  # (m, ng, 4, 4)
    return (b.reshape(m, ng * 16) < T)[:, :c]
