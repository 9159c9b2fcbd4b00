"""The seeded McICA random numbers, restated in numpy: Philox4x32-10 (Salmon et al., SC'11) and the counter layout of
include/rrtmgpnn.h (rrtmgpnn_mcica_randoms).

One Philox call gives the four 32-bit words of 4 consecutive layers of one g-point of one column:
  counter (g, l >> 2, (col0 + icol) mod 2^32, stream), key (seed & 0xffffffff, seed >> 32),
  layer l takes word l & 3, converted as float32(w >> 8) * 2^-24 (exact; in [0, 1 - 2^-24]).
g, l, icol 0-based, l in array order.  Arrays are C-ordered with the Fortran shape reversed, as everywhere in the tests:
randoms(...) returns (ncol, nlay, ngpt) float32."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 arrays (broadcastable) of 32-bit values; key: 2 scalars.  Returns 4 uint32 arrays."""
    c = [np.asarray(x, np.uint64) & MASK32 for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:  # the key is bumped before rounds 2..10
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
    return [x.astype(np.uint32) for x in c]


def words(seed, stream, col0, ngpt, nlay, ncol):
    """(ncol, nlay, ngpt) uint32: the word each element takes."""
    ngrp = (nlay + 3) // 4
    g = np.arange(ngpt, dtype=np.uint64)[None, None, :]
    grp = np.arange(ngrp, dtype=np.uint64)[None, :, None]
    col = ((int(col0) + np.arange(ncol, dtype=np.uint64)) & MASK32)[:, None, None]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((g, grp, col, np.uint64(int(stream) & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, seed >> 32))
    out = np.stack(w, axis=2)  # (ncol, ngrp, 4, ngpt): layer 4 * grp + word
    return np.ascontiguousarray(out.reshape(ncol, 4 * ngrp, ngpt)[:, :nlay])


def to_float(w):
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def randoms(seed, stream, col0, ngpt, nlay, ncol):
    """(ncol, nlay, ngpt) float32 in [0, 1)."""
    return to_float(words(seed, stream, col0, ngpt, nlay, ncol))
