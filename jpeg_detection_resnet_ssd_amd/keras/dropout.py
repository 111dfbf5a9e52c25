"""Host statement of the device dropout (csrc/dj_dropout.hip, keras.layers.Dropout): numpy only, machine independent,
and equal bit for bit to what dj_dropout_fwd / dj_dropout_bwd compute.

The generator is Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the standard
multipliers 0xD2511F53 / 0xCD9E8D57 and Weyl key increments 0x9E3779B9 / 0xBB67AE85.  It keeps no state: the mask is a
pure function of (layer seed, data-parallel rank, optimizer step, element index), so the backward pass regenerates the
mask the forward pass drew and no mask tensor exists.

Packing (the only place it is stated; the kernel takes the six words as arguments):

    key     = (seed & 0xFFFFFFFF,  rank & 0xFFFFFFFF)
    counter = ((i >> 2) & 0xFFFFFFFF,  (i >> 2) >> 32,  step & 0xFFFFFFFF,  (step >> 32) & 0xFFFFFFFF)

Element i takes word (i & 3) of that block and is kept iff the word >= dropout_threshold(rate).  Nothing depends on the
tensor's size n: the mask of n elements is a prefix of the mask of any longer tensor.
"""
import numpy as np

PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85
_MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two -> four uint32 arrays, broadcast against each other."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(_MASK32) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(_MASK32) for v in key]
    assert len(c) == 4 and len(k) == 2
    m0, m1, mask = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1), np.uint64(_MASK32)
    for _ in range(10):
        p0 = m0 * c[0]          # 32 x 32 -> 64 bits: exact in uint64
        p1 = m1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
    shape = np.broadcast(*c).shape
    return [np.broadcast_to(v, shape).astype(np.uint32) for v in c]


def dropout_threshold(rate):
    """Words below it are dropped: min(int(rate * 2**32), 2**32 - 1), in Python floats / ints."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError("dropout rate must lie in [0, 1), got %r" % (rate,))
    return min(int(rate * 2 ** 32), 2 ** 32 - 1)


def dropout_scale(rate):
    """float32(1 / (1 - rate)): what kept elements are multiplied by."""
    return np.float32(1.0 / (1.0 - float(rate)))


def dropout_words(seed, rank, step):
    """-> (key0, key1, ctr2, ctr3), the words the C ABI takes besides the element index (module docstring)."""
    seed, rank, step = int(seed), int(rank), int(step)
    return seed & _MASK32, rank & _MASK32, step & _MASK32, (step >> 32) & _MASK32


def dropout_keep_host(n, rate, seed, rank, step):
    """-> bool[n]: True where element i is kept."""
    n = int(n)
    key0, key1, ctr2, ctr3 = dropout_words(seed, rank, step)
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((blocks & np.uint64(_MASK32), blocks >> np.uint64(32), ctr2, ctr3), (key0, key1))
    flat = np.stack(words, axis=1).reshape(-1)[:n]       # element i = word (i & 3) of block (i >> 2)
    return flat >= np.uint32(dropout_threshold(rate))


def dropout_host(x, rate, seed, rank, step):
    """(x * float32(1 / (1 - rate))) * keep in float32, keep as 0.0 / 1.0: a product, so an Inf or NaN at a dropped
    position gives NaN."""
    x = np.asarray(x, dtype=np.float32)
    keep = dropout_keep_host(x.size, rate, seed, rank, step).astype(np.float32).reshape(x.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x * dropout_scale(rate)) * keep
