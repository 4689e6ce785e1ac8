"""The dropout's stream on the host (ct_pvae_amd.dropout_mask, the library's own host entry point) against tests/np_twin_dropout.py,
which restates it with the numpy Philox that is held to the oracle; the rate's rules; the trainer's --dp and --ufs.  No GPU."""
import math

import numpy as np
import pytest

from ct_pvae_amd import dropout_mask
from ct_pvae_amd import trainer as tr
from tests import np_twin_dropout as td

KEYS = [(1234, 0, 0), (1234, 1, 0), (1234, 0, 1), (7, 3, 18)]          # (seed, draw, layer)
RATE_T = {0.1: 1677722, 0.25: 4194304, 0.5: 8388608, 0.9: 15099494}


@pytest.mark.parametrize("shape", [(4, 105), (1, 1), (3, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_is_the_twins_bit_for_bit(shape):
    """first_object 0, 1 (105 is odd: the Philox blocks then straddle the objects' quads) and 2^34 // 105, where e >> 2 passes 2^32
    and the second counter word is not zero."""
    n, length = shape
    for first in (0, 1, 2 ** 34 // 105):
        for rate in (0.25, 0.9):
            got = dropout_mask(n, length, rate, seed=1234, draw=5, layer=3, first_object=first)
            assert got.dtype == np.bool_ and got.shape == shape
            assert np.array_equal(got, td.keep(n, length, rate, 1234, 5, 3, first)), (first, rate)
    assert ((2 ** 34 // 105) * length) >> 2 < 2 ** 32 <= ((2 ** 34 // 105 + n) * length) >> 2 or length != 105     # the carry is inside


def test_a_batch_cut_in_two_is_the_whole_batch():
    whole = dropout_mask(4, 105, 0.25, seed=1234, draw=0, layer=0)
    assert np.array_equal(whole[2:], dropout_mask(2, 105, 0.25, seed=1234, draw=0, layer=0, first_object=2))


def test_masks_differ_between_seeds_draws_and_layers():
    base = dropout_mask(4, 105, 0.5, seed=1234, draw=0, layer=0)
    assert not np.array_equal(base, dropout_mask(4, 105, 0.5, seed=1235, draw=0, layer=0))
    assert not np.array_equal(base, dropout_mask(4, 105, 0.5, seed=1234, draw=1, layer=0))
    assert not np.array_equal(base, dropout_mask(4, 105, 0.5, seed=1234, draw=0, layer=1))
    assert not np.array_equal(base, dropout_mask(4, 105, 0.5, seed=1234 + 2 ** 32, draw=0, layer=0))      # the key's second word


@pytest.mark.parametrize("rate", sorted(RATE_T))
def test_keep_fraction(rate):
    """|kept / n - (1 - T / 2^24)| <= 4 sigma, sigma = sqrt(p (1 - p) / n), on [16][4096] for four keys; T as the header defines it."""
    T = RATE_T[rate]
    assert td.threshold(rate) == T == math.ceil(float(np.float32(rate)) * 2 ** 24)
    p = 1.0 - T / 2.0 ** 24
    n = 16 * 4096
    sigma = math.sqrt(p * (1 - p) / n)
    for seed, draw, layer in KEYS:
        kept = int(dropout_mask(16, 4096, rate, seed=seed, draw=draw, layer=layer).sum())
        z = (kept / n - p) / sigma
        print(f"rate {rate} key {(seed, draw, layer)}: kept {kept} of {n}, {z:+.2f} sigma")
        assert abs(kept / n - p) <= 4 * sigma


@pytest.mark.parametrize("rate", [0.0, 1.0, -0.1, float("nan"), 1 - 1e-9, 0, 1], ids=str)
def test_rates_outside_the_open_interval_are_refused(rate):
    assert not 0 < np.float32(rate) < 1
    with pytest.raises(ValueError):
        dropout_mask(2, 8, rate, seed=0, draw=0, layer=0)
    with pytest.raises(ValueError):
        tr.DropoutKey(rate, 0)


def test_other_argument_errors():
    with pytest.raises(ValueError):
        dropout_mask(2, 8, 0.5, seed=0, draw=0, layer=2 ** 24)
    with pytest.raises(ValueError):
        dropout_mask(2, 8, 0.5, seed=0, draw=2 ** 32, layer=0)
    with pytest.raises(ValueError):
        dropout_mask(0, 8, 0.5, seed=0, draw=0, layer=0)
    with pytest.raises(ValueError):
        dropout_mask(2, 8, 0.5, seed=0, draw=0, layer=0, first_object=2 ** 60)       # (first_object + n) * len passes 63 bits
    with pytest.raises(TypeError):
        dropout_mask(2, 8, "0.5", seed=0, draw=0, layer=0)


# ---- the trainer's flags --------------------------------------------------------------------------------------------------------
def test_dp_and_ufs_parse():
    a = tr.get_args(["--dp", "0.1", "--ufs"])
    assert a.dropout_prob == 0.1 and a.ufs is True
    a = tr.get_args([])
    assert a.dropout_prob == 0.0 and a.ufs is False
    for bad in ("1.5", "1", "-0.1", "nan"):
        with pytest.raises(SystemExit):
            tr.get_args(["--dp", bad])


def _nets(dropout_prob):
    """The two networks as PVAETrainer builds them for the default flags (--nb 3 --il 2 --nfm 20 --nfmm 1.1, fmm 2)."""
    a = tr.get_args(["--dp", str(dropout_prob)])
    fm = [int(a.nfm * a.nfmm ** i) for i in range(a.num_blocks)]
    ed = tr.DropoutKey(a.dropout_prob, a.head_seed) if a.dropout_prob > 0 else None
    dd = tr.DropoutKey(a.dropout_prob, a.head_seed) if a.dropout_prob > 0 else None
    enc = tr.EncodeNet(2, fm, 2, a.kernel_size, a.stride_encode, a.il, a.ik, dropout=ed)
    dec = tr.DecodeNet(enc.channels, 2, 1, a.kernel_size, a.stride_encode, a.il, a.ik, dropout=dd, first_layer=enc.num_layers)
    return enc, dec


def test_dropout_adds_no_parameters_and_numbers_the_blocks():
    import torch
    torch.manual_seed(0)
    e0, d0 = _nets(0)
    e1, d1 = _nets(0.1)
    want_enc = [f"blocks.{b}.{i}.ab.{w}" for b in range(3) for i in range(3) for w in ("weight", "bias")]
    want_dec = [f"ups.{b}.{i}.ab.{w}" for b in range(3) for i in range(3) for w in ("weight", "bias")] + ["head.ab.weight", "head.ab.bias"]
    assert list(e0.state_dict()) == want_enc and list(d0.state_dict()) == want_dec          # the keys of today
    assert list(e1.state_dict()) == want_enc and list(d1.state_dict()) == want_dec
    assert [tuple(v.shape) for v in e1.state_dict().values()] == [tuple(v.shape) for v in e0.state_dict().values()]
    blocks = [m for net in (e1, d1) for m in net.modules() if isinstance(m, tr.ConvBlock)]
    assert [m.layer for m in blocks] == list(range(19)) and (e1.num_layers, d1.num_layers) == (9, 10)       # the 19 c3 blocks
    assert all(m.dropout is e1.dropout for m in e1.modules() if isinstance(m, tr.ConvBlock))
    assert all(m.dropout is d1.dropout for m in d1.modules() if isinstance(m, tr.ConvBlock)) and d1.dropout is not e1.dropout
    assert all(m.dropout is None for net in (e0, d0) for m in net.modules() if isinstance(m, tr.ConvBlock))
