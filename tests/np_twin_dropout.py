"""numpy restatement of the ConvBlock's dropout (include/ctpvae_radon.h states the stream, csrc/convblock.hip the kernels): the keep
decisions from tests.np_twin_hmc.philox -- the numpy Philox that is held to the oracle, NOT the library's host function -- and the
forward and backward by np.where on float32.  The pad twins are tests.np_twin_convblock's.  tests/test_dropout_cpu.py holds
ct_pvae_amd.dropout_mask to keep(); tests/test_gpu_dropout.py holds the kernels to all of it."""
import math

import numpy as np

from tests import np_twin_hmc

TAG = 0x44000000
RATES = (0.25, 0.9)


def threshold(rate):
    """T = ceil(float32(rate) * 2^24): k = w >> 8 is kept iff k >= T, i.e. iff k * 2^-24 >= float32(rate)."""
    return int(math.ceil(float(np.float32(rate)) * 2.0 ** 24))


def scale(rate):
    """float32(1 / (1 - rate)), the quotient in double."""
    return np.float32(1.0 / (1.0 - float(rate)))


def keep(n, length, rate, seed, draw, layer, first_object=0):
    """bool [n][length]: element i of object b has e = (first_object + b) * length + i (a Python integer: up to 63 bits) and takes word
    e & 3 of the block with counter (lo32(e >> 2), hi32(e >> 2), draw, 0x44000000 | layer), key = seed."""
    e0 = int(first_object) * int(length)
    e = np.uint64(e0) + np.arange(n * length, dtype=np.uint64)
    blk = e >> np.uint64(2)
    blocks, inverse = np.unique(blk, return_inverse=True)
    w4 = np_twin_hmc.philox(blocks & np.uint64(0xFFFFFFFF), blocks >> np.uint64(32), draw, TAG | int(layer), int(seed) & (2 ** 64 - 1))
    w = w4[inverse, (e & np.uint64(3)).astype(np.int64)]
    return ((w >> np.uint32(8)) >= np.uint32(threshold(rate))).reshape(n, length)


def keep_like(x, rate, seed, draw, layer, first_object=0):
    """keep() in the shape of a block input x [N][C][H][W]."""
    return keep(x.shape[0], x[0].size, rate, seed, draw, layer, first_object).reshape(x.shape)


def drop_fwd(x, k, rate):
    """where(k, x * scale, +0) on float32: one multiply; a dropped inf or NaN gives +0."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(k, x * scale(rate), np.float32(0.0)).astype(np.float32)


def drop_bwd(g, k, rate):
    """where(k, scale * g, +0): the forward's expression on the cotangent."""
    return drop_fwd(g, k, rate)
