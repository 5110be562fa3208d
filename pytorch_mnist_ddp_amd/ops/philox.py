"""Philox-4x32-10 (Salmon et al. 2011) in numpy: the generator of the kernels (``csrc/include/device_utils.h``
``philox4x32``), so a CPU path of the package can draw the bits a kernel draws.  Vectorised over the counters."""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(c0, c1, c2, c3, seed: int) -> np.ndarray:
    """The four 32-bit words of ``philox4x32(counter = (c0, c1, c2, c3), key = (seed low, seed high))``: uint32
    [..., 4], the leading shape that of the broadcast counters (integers or integer arrays, each word < 2**32)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                  # 32 x 32 bits: the product fits 64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack((c0, c1, c2, c3), axis=-1).astype(np.uint32)
