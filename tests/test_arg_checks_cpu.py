"""The tensor checks every fused operator makes before it looks at a device: a non-tensor, a float64 tensor, a tensor of the wrong rank,
an empty one, one of the wrong shape where the operator fixes more than the rank, and a non-contiguous one.  Each is refused with the
exception type and the FULL message written out below; CPU tensors suffice, since these checks come before the device check."""
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd._lib import RadonLibraryError

LIST = [1.0]
F64_4 = torch.zeros(2, 2, 3, 4, dtype=torch.float64)
RANK1 = torch.zeros(3)
RANK4 = torch.zeros(1, 2, 2, 2)
EMPTY4 = torch.zeros(2, 0, 3, 4)
STRIDED4 = torch.zeros(2, 2, 3, 4).transpose(2, 3)              # shape (2, 2, 4, 3), strides (24, 12, 1, 4)
STRIDED1 = torch.zeros(8)[::2]                                  # shape (4,), strides (2,)
HEAD = torch.zeros(2, 1, 4, 3)                                  # a good [n][1][X][Y]
HEAD_F64 = torch.zeros(2, 1, 4, 3, dtype=torch.float64)
HEAD_EMPTY = torch.zeros(0, 1, 4, 3)
HEAD_TWO = torch.zeros(2, 2, 4, 3)                              # two channels
HEAD_STRIDED = torch.zeros(2, 1, 3, 4).transpose(2, 3)          # shape (2, 1, 4, 3), strides (12, 12, 1, 4)

X, W, B = torch.zeros(1, 2, 4, 4), torch.zeros(4, 2, 3, 3), torch.zeros(4)
WT = torch.zeros(2, 4, 3, 3)
KEY = dict(seed=1, draw=0)


def _conv(x=X, w=W, b=B):
    return cp.periodic_conv_maxout(x, w, b, 1, (1, 1, 1, 1))


def _convt(x=X, w=WT, b=B):
    return cp.conv_transpose_maxout(x, w, b, 1, 0, 0)


def _marginals(alpha=HEAD, beta=HEAD):
    return cp.PixelMarginals((4, 3), device="cpu").add(alpha, beta, draws=1, seed=1)


CASES = [
    # periodic_conv_maxout
    (lambda: _conv(x=LIST), TypeError, "periodic_conv_maxout: x must be a torch tensor (got list)"),
    (lambda: _conv(x=F64_4), TypeError, "periodic_conv_maxout: x must be float32 (got torch.float64)"),
    (lambda: _conv(x=RANK1), ValueError, "periodic_conv_maxout: x must be a non-empty tensor of 4 axes (got (3,))"),
    (lambda: _conv(x=EMPTY4), ValueError, "periodic_conv_maxout: x must be a non-empty tensor of 4 axes (got (2, 0, 3, 4))"),
    (lambda: _conv(x=STRIDED4), ValueError, "periodic_conv_maxout: x must be contiguous (got strides (24, 12, 1, 4))"),
    (lambda: _conv(w=LIST), TypeError, "periodic_conv_maxout: weight must be a torch tensor (got list)"),
    (lambda: _conv(w=F64_4), TypeError, "periodic_conv_maxout: weight must be float32 (got torch.float64)"),
    (lambda: _conv(w=RANK1), ValueError, "periodic_conv_maxout: weight must be a non-empty tensor of 4 axes (got (3,))"),
    (lambda: _conv(w=STRIDED4), ValueError, "periodic_conv_maxout: weight must be contiguous (got strides (24, 12, 1, 4))"),
    (lambda: _conv(b=LIST), TypeError, "periodic_conv_maxout: bias must be a torch tensor (got list)"),
    (lambda: _conv(b=B.double()), TypeError, "periodic_conv_maxout: bias must be float32 (got torch.float64)"),
    (lambda: _conv(b=RANK4), ValueError, "periodic_conv_maxout: bias must be a non-empty tensor of 1 axes (got (1, 2, 2, 2))"),
    (lambda: _conv(b=torch.zeros(0)), ValueError, "periodic_conv_maxout: bias must be a non-empty tensor of 1 axes (got (0,))"),
    (lambda: _conv(b=STRIDED1), ValueError, "periodic_conv_maxout: bias must be contiguous (got strides (2,))"),
    # conv_transpose_maxout
    (lambda: _convt(x=LIST), TypeError, "conv_transpose_maxout: x must be a torch tensor (got list)"),
    (lambda: _convt(x=F64_4), TypeError, "conv_transpose_maxout: x must be float32 (got torch.float64)"),
    (lambda: _convt(x=RANK1), ValueError, "conv_transpose_maxout: x must be a non-empty tensor of 4 axes (got (3,))"),
    (lambda: _convt(x=EMPTY4), ValueError, "conv_transpose_maxout: x must be a non-empty tensor of 4 axes (got (2, 0, 3, 4))"),
    (lambda: _convt(x=STRIDED4), ValueError, "conv_transpose_maxout: x must be contiguous (got strides (24, 12, 1, 4))"),
    (lambda: _convt(w=LIST), TypeError, "conv_transpose_maxout: weight must be a torch tensor (got list)"),
    (lambda: _convt(w=F64_4), TypeError, "conv_transpose_maxout: weight must be float32 (got torch.float64)"),
    (lambda: _convt(w=RANK1), ValueError, "conv_transpose_maxout: weight must be a non-empty tensor of 4 axes (got (3,))"),
    (lambda: _convt(w=STRIDED4), ValueError, "conv_transpose_maxout: weight must be contiguous (got strides (24, 12, 1, 4))"),
    (lambda: _convt(b=LIST), TypeError, "conv_transpose_maxout: bias must be a torch tensor (got list)"),
    (lambda: _convt(b=B.double()), TypeError, "conv_transpose_maxout: bias must be float32 (got torch.float64)"),
    (lambda: _convt(b=RANK4), ValueError, "conv_transpose_maxout: bias must be a non-empty tensor of 1 axes (got (1, 2, 2, 2))"),
    (lambda: _convt(b=torch.zeros(0)), ValueError, "conv_transpose_maxout: bias must be a non-empty tensor of 1 axes (got (0,))"),
    (lambda: _convt(b=STRIDED1), ValueError, "conv_transpose_maxout: bias must be contiguous (got strides (2,))"),
    # periodic_pad
    (lambda: cp.periodic_pad(LIST, (0, 0, 0, 0)), TypeError, "periodic_pad: x must be a torch tensor (got list)"),
    (lambda: cp.periodic_pad(F64_4, (0, 0, 0, 0)), TypeError, "periodic_pad: x must be float32 (got torch.float64)"),
    (lambda: cp.periodic_pad(RANK1, (0, 0, 0, 0)), ValueError, "periodic_pad: x must be a non-empty [N][C][H][W] tensor (got (3,))"),
    (lambda: cp.periodic_pad(EMPTY4, (0, 0, 0, 0)), ValueError, "periodic_pad: x must be a non-empty [N][C][H][W] tensor (got (2, 0, 3, 4))"),
    (lambda: cp.periodic_pad(STRIDED4, (0, 0, 0, 0)), ValueError, "periodic_pad: x must be contiguous (got strides (24, 12, 1, 4))"),
    # maxout
    (lambda: cp.maxout(LIST), TypeError, "maxout: y must be a torch tensor (got list)"),
    (lambda: cp.maxout(F64_4), TypeError, "maxout: y must be float32 (got torch.float64)"),
    (lambda: cp.maxout(RANK1), ValueError, "maxout: y must be a non-empty [N][C][H][W] tensor (got (3,))"),
    (lambda: cp.maxout(EMPTY4), ValueError, "maxout: y must be a non-empty [N][C][H][W] tensor (got (2, 0, 3, 4))"),
    (lambda: cp.maxout(STRIDED4), ValueError, "maxout: y must be contiguous (got strides (24, 12, 1, 4))"),
    # dropout
    (lambda: cp.dropout(LIST, 0.5, layer=0, **KEY), TypeError, "dropout: x must be a torch tensor (got list)"),
    (lambda: cp.dropout(F64_4, 0.5, layer=0, **KEY), TypeError, "dropout: x must be float32 (got torch.float64)"),
    (lambda: cp.dropout(RANK1, 0.5, layer=0, **KEY), ValueError, "dropout: x must be a non-empty [N][C][H][W] tensor (got (3,))"),
    (lambda: cp.dropout(EMPTY4, 0.5, layer=0, **KEY), ValueError, "dropout: x must be a non-empty [N][C][H][W] tensor (got (2, 0, 3, 4))"),
    (lambda: cp.dropout(STRIDED4, 0.5, layer=0, **KEY), ValueError, "dropout: x must be contiguous (got strides (24, 12, 1, 4))"),
    # dropout_pad
    (lambda: cp.dropout_pad(LIST, (0, 0, 0, 0), 0.5, layer=0, **KEY), TypeError, "dropout_pad: x must be a torch tensor (got list)"),
    (lambda: cp.dropout_pad(F64_4, (0, 0, 0, 0), 0.5, layer=0, **KEY), TypeError, "dropout_pad: x must be float32 (got torch.float64)"),
    (lambda: cp.dropout_pad(RANK1, (0, 0, 0, 0), 0.5, layer=0, **KEY), ValueError,
     "dropout_pad: x must be a non-empty [N][C][H][W] tensor (got (3,))"),
    (lambda: cp.dropout_pad(EMPTY4, (0, 0, 0, 0), 0.5, layer=0, **KEY), ValueError,
     "dropout_pad: x must be a non-empty [N][C][H][W] tensor (got (2, 0, 3, 4))"),
    (lambda: cp.dropout_pad(STRIDED4, (0, 0, 0, 0), 0.5, layer=0, **KEY), ValueError,
     "dropout_pad: x must be contiguous (got strides (24, 12, 1, 4))"),
    # truncated_normal_head
    (lambda: cp.truncated_normal_head(LIST, HEAD, **KEY), TypeError, "truncated_normal_head: alpha must be a torch tensor (got list)"),
    (lambda: cp.truncated_normal_head(HEAD_F64, HEAD, **KEY), TypeError, "truncated_normal_head: alpha must be float32 (got torch.float64)"),
    (lambda: cp.truncated_normal_head(RANK1, HEAD, **KEY), ValueError,
     "truncated_normal_head: alpha must be [n][1][X][Y], the decoder's layout (got (3,))"),
    (lambda: cp.truncated_normal_head(HEAD_EMPTY, HEAD, **KEY), ValueError,
     "truncated_normal_head: alpha must be [n][1][X][Y], the decoder's layout (got (0, 1, 4, 3))"),
    (lambda: cp.truncated_normal_head(HEAD_TWO, HEAD, **KEY), ValueError,
     "truncated_normal_head: alpha must be [n][1][X][Y], the decoder's layout (got (2, 2, 4, 3))"),
    (lambda: cp.truncated_normal_head(HEAD_STRIDED, HEAD, **KEY), ValueError,
     "truncated_normal_head: alpha must be contiguous (got strides (12, 12, 1, 4))"),
    (lambda: cp.truncated_normal_head(HEAD, LIST, **KEY), TypeError, "truncated_normal_head: beta must be a torch tensor (got list)"),
    (lambda: cp.truncated_normal_head(HEAD, HEAD_TWO, **KEY), ValueError,
     "truncated_normal_head: beta must be [n][1][X][Y], the decoder's layout (got (2, 2, 4, 3))"),
    # beta_head
    (lambda: cp.beta_head(LIST, HEAD, **KEY), TypeError, "beta_head: alpha must be a torch tensor (got list)"),
    (lambda: cp.beta_head(HEAD_F64, HEAD, **KEY), TypeError, "beta_head: alpha must be float32 (got torch.float64)"),
    (lambda: cp.beta_head(RANK1, HEAD, **KEY), ValueError, "beta_head: alpha must be [n][1][X][Y], the decoder's layout (got (3,))"),
    (lambda: cp.beta_head(HEAD_EMPTY, HEAD, **KEY), ValueError, "beta_head: alpha must be [n][1][X][Y], the decoder's layout (got (0, 1, 4, 3))"),
    (lambda: cp.beta_head(HEAD_TWO, HEAD, **KEY), ValueError, "beta_head: alpha must be [n][1][X][Y], the decoder's layout (got (2, 2, 4, 3))"),
    (lambda: cp.beta_head(HEAD_STRIDED, HEAD, **KEY), ValueError, "beta_head: alpha must be contiguous (got strides (12, 12, 1, 4))"),
    (lambda: cp.beta_head(HEAD, LIST, **KEY), TypeError, "beta_head: beta must be a torch tensor (got list)"),
    (lambda: cp.beta_head(HEAD, HEAD_TWO, **KEY), ValueError, "beta_head: beta must be [n][1][X][Y], the decoder's layout (got (2, 2, 4, 3))"),
    # normal_latents
    (lambda: cp.normal_latents(LIST, ns=1, level=0, **KEY), TypeError, "normal_latents: skip must be a torch tensor (got list)"),
    (lambda: cp.normal_latents(F64_4, ns=1, level=0, **KEY), TypeError, "normal_latents: skip must be float32 (got torch.float64)"),
    (lambda: cp.normal_latents(RANK1, ns=1, level=0, **KEY), ValueError,
     "normal_latents: skip must be [B][channels][H][W], the encoder's layout (got (3,))"),
    (lambda: cp.normal_latents(EMPTY4, ns=1, level=0, **KEY), ValueError,
     "normal_latents: skip must be [B][channels][H][W], the encoder's layout (got (2, 0, 3, 4))"),
    (lambda: cp.normal_latents(STRIDED4, ns=1, level=0, **KEY), ValueError,
     "normal_latents: skip must be contiguous (got strides (24, 12, 1, 4))"),
    (lambda: cp.normal_latents(RANK4, ns=1, level=0, _eps=LIST, **KEY), TypeError, "normal_latents: _eps must be a torch tensor (got list)"),
    (lambda: cp.normal_latents(RANK4, ns=1, level=0, _eps=RANK1, **KEY), ValueError,
     "normal_latents: _eps must be [B][channels][H][W], the encoder's layout (got (3,))"),
    # beta_latents
    (lambda: cp.beta_latents(LIST, ns=1, level=0, **KEY), TypeError, "beta_latents: skip must be a torch tensor (got list)"),
    (lambda: cp.beta_latents(F64_4, ns=1, level=0, **KEY), TypeError, "beta_latents: skip must be float32 (got torch.float64)"),
    (lambda: cp.beta_latents(RANK1, ns=1, level=0, **KEY), ValueError,
     "beta_latents: skip must be [B][channels][H][W], the encoder's layout (got (3,))"),
    (lambda: cp.beta_latents(EMPTY4, ns=1, level=0, **KEY), ValueError,
     "beta_latents: skip must be [B][channels][H][W], the encoder's layout (got (2, 0, 3, 4))"),
    (lambda: cp.beta_latents(STRIDED4, ns=1, level=0, **KEY), ValueError, "beta_latents: skip must be contiguous (got strides (24, 12, 1, 4))"),
    # PixelMarginals.add, on a (4, 3) pixel grid
    (lambda: _marginals(alpha=LIST), TypeError, "PixelMarginals.add: alpha must be a torch tensor (got list)"),
    (lambda: _marginals(alpha=HEAD_F64), TypeError, "PixelMarginals.add: alpha must be float32 (got torch.float64)"),
    (lambda: _marginals(alpha=RANK1), ValueError, "PixelMarginals.add: alpha must be [n][1][4][3], the decoder's layout (got (3,))"),
    (lambda: _marginals(alpha=HEAD_EMPTY), ValueError, "PixelMarginals.add: alpha must be [n][1][4][3], the decoder's layout (got (0, 1, 4, 3))"),
    (lambda: _marginals(alpha=HEAD_TWO), ValueError, "PixelMarginals.add: alpha must be [n][1][4][3], the decoder's layout (got (2, 2, 4, 3))"),
    (lambda: _marginals(alpha=torch.zeros(2, 1, 3, 4)), ValueError,
     "PixelMarginals.add: alpha must be [n][1][4][3], the decoder's layout (got (2, 1, 3, 4))"),
    (lambda: _marginals(alpha=HEAD_STRIDED), ValueError, "PixelMarginals.add: alpha must be contiguous (got strides (12, 12, 1, 4))"),
    (lambda: _marginals(beta=LIST), TypeError, "PixelMarginals.add: beta must be a torch tensor (got list)"),
    (lambda: _marginals(beta=torch.zeros(2, 1, 3, 4)), ValueError,
     "PixelMarginals.add: beta must be [n][1][4][3], the decoder's layout (got (2, 1, 3, 4))"),
]

# ---- what the four sampling operators check after their tensors, still before any device: the counter words (through every module that
# takes them), the sample count and the level, the pair's shapes, the channel count, sqrt_reg, the size limits (on meta tensors: no
# memory), the test operands, and last the refusal of a CPU tensor
DRAW = "draw is one 32-bit counter word: 0 <= draw < 2^32"
FIRST = "first_object must be >= 0 (got -1)"
NS_N = "ns shares a counter word with the level: 1 <= ns <= 65535"
NS_B = "the sample index shares a counter word with the level, the gamma and the attempt: 1 <= ns <= 2048"
LEVEL = "level is one byte of a counter word: 0 <= level <= 255 (got 256)"
HEAD_3 = torch.zeros(3, 1, 4, 3)
SKIP = torch.zeros(2, 2, 3, 4)                                  # a good [B][2C][H][W]
SKIP_ODD = torch.zeros(2, 3, 3, 4)
HEAD_HUGE = torch.empty((2 ** 31, 1, 1, 1), device="meta")
SKIP_HUGE = torch.empty((2, 2, 2 ** 15, 2 ** 14), device="meta")
LKEY = dict(ns=1, level=0, **KEY)


def _marginals_key(**key):
    return cp.PixelMarginals((4, 3), device="cpu").add(HEAD, HEAD, draws=1, **key)


CASES += [
    # the counter words
    (lambda: cp.head_uniforms(1, 1, seed=1, draw=-1), ValueError, DRAW + " (got -1)"),
    (lambda: cp.head_uniforms(1, 1, seed=1, draw=2 ** 32), ValueError, DRAW + " (got 4294967296)"),
    (lambda: cp.head_uniforms(1, 1, seed=1, draw=0, first_object=-1), ValueError, FIRST),
    (lambda: cp.truncated_normal_head(HEAD, HEAD, seed=1, draw=-1), ValueError, DRAW + " (got -1)"),
    (lambda: cp.truncated_normal_head(HEAD, HEAD, first_object=-1, **KEY), ValueError, FIRST),
    (lambda: cp.beta_head(HEAD, HEAD, seed=1, draw=2 ** 32), ValueError, DRAW + " (got 4294967296)"),
    (lambda: cp.beta_head(HEAD, HEAD, first_object=-1, **KEY), ValueError, FIRST),
    (lambda: cp.beta_head_words(1, 1, seed=1, draw=-1, gamma=0, attempt=0), ValueError, DRAW + " (got -1)"),
    (lambda: cp.beta_head_words(1, 1, first_object=-1, gamma=0, attempt=0, **KEY), ValueError, FIRST),
    (lambda: cp.normal_latents(SKIP, ns=1, level=0, seed=1, draw=-1), ValueError, DRAW + " (got -1)"),
    (lambda: cp.normal_latents(SKIP, first_object=-1, **LKEY), ValueError, FIRST),
    (lambda: cp.latent_draws(1, 1, ns=1, level=0, seed=1, draw=2 ** 32), ValueError, DRAW + " (got 4294967296)"),
    (lambda: cp.latent_draws(1, 1, first_object=-1, **LKEY), ValueError, FIRST),
    (lambda: cp.beta_latents(SKIP, ns=1, level=0, seed=1, draw=-1), ValueError, DRAW + " (got -1)"),
    (lambda: cp.beta_latents(SKIP, first_object=-1, **LKEY), ValueError, FIRST),
    (lambda: cp.beta_latent_words(1, 1, level=0, s=0, gamma=0, attempt=0, seed=1, draw=-1), ValueError, DRAW + " (got -1)"),
    (lambda: cp.beta_latent_words(1, 1, level=0, s=0, gamma=0, attempt=0, first_object=-1, **KEY), ValueError, FIRST),
    (lambda: _marginals_key(seed=1, draw0=-1), ValueError, DRAW + " (got -1)"),
    (lambda: _marginals_key(seed=1, first_object=-1), ValueError, FIRST),
    (lambda: cp.dropout(X, 0.5, layer=0, seed=1, draw=2 ** 32), ValueError, DRAW + " (got 4294967296)"),
    (lambda: cp.dropout(X, 0.5, layer=0, first_object=-1, **KEY), ValueError, FIRST),
    # the sample count and the level
    (lambda: cp.normal_latents(SKIP, ns=0, level=0, **KEY), ValueError, NS_N + " (got 0)"),
    (lambda: cp.normal_latents(SKIP, ns=65536, level=0, **KEY), ValueError, NS_N + " (got 65536)"),
    (lambda: cp.normal_latents(SKIP, ns=1, level=256, **KEY), ValueError, LEVEL),
    (lambda: cp.latent_draws(1, 1, ns=0, level=0, **KEY), ValueError, NS_N + " (got 0)"),
    (lambda: cp.latent_draws(1, 1, ns=65536, level=0, **KEY), ValueError, NS_N + " (got 65536)"),
    (lambda: cp.latent_draws(1, 1, ns=1, level=256, **KEY), ValueError, LEVEL),
    (lambda: cp.beta_latents(SKIP, ns=0, level=0, **KEY), ValueError, NS_B + " (got 0)"),
    (lambda: cp.beta_latents(SKIP, ns=2049, level=0, **KEY), ValueError, NS_B + " (got 2049)"),
    (lambda: cp.beta_latents(SKIP, ns=1, level=256, **KEY), ValueError, LEVEL),
    (lambda: cp.beta_latent_words(1, 1, level=256, s=0, gamma=0, attempt=0, **KEY), ValueError, LEVEL),
    (lambda: cp.beta_latent_words(1, 1, level=0, s=2048, gamma=0, attempt=0, **KEY), ValueError, "beta_latent_words: 0 <= s < 2048 (got 2048)"),
    # the pair's shapes, the channel count, sqrt_reg
    (lambda: cp.truncated_normal_head(HEAD, HEAD_3, **KEY), ValueError,
     "truncated_normal_head: alpha and beta must have one shape (got (2, 1, 4, 3), (3, 1, 4, 3))"),
    (lambda: cp.beta_head(HEAD, HEAD_3, **KEY), ValueError, "beta_head: alpha and beta must have one shape (got (2, 1, 4, 3), (3, 1, 4, 3))"),
    (lambda: cp.normal_latents(SKIP_ODD, **LKEY), ValueError,
     "normal_latents: skip needs an even channel count, loc then log_scale (got (2, 3, 3, 4))"),
    (lambda: cp.beta_latents(SKIP_ODD, **LKEY), ValueError,
     "beta_latents: skip needs an even channel count, loc then log_scale (got (2, 3, 3, 4))"),
    (lambda: cp.beta_head(HEAD, HEAD, sqrt_reg=0.0, **KEY), ValueError, "beta_head: sqrt_reg must lie in (0, 0.5) (got 0.0)"),
    (lambda: cp.beta_head(HEAD, HEAD, sqrt_reg=0.5, **KEY), ValueError, "beta_head: sqrt_reg must lie in (0, 0.5) (got 0.5)"),
    (lambda: cp.beta_head(HEAD, HEAD, sqrt_reg=float("nan"), **KEY), ValueError, "beta_head: sqrt_reg must lie in (0, 0.5) (got nan)"),
    # the size limits
    (lambda: cp.truncated_normal_head(HEAD_HUGE, HEAD_HUGE, **KEY), ValueError,
     "truncated_normal_head: at most 2^31 - 1 pixels per call (got 2147483648)"),
    (lambda: cp.beta_head(HEAD_HUGE, HEAD_HUGE, **KEY), ValueError, "beta_head: at most 2^31 - 1 pixels per call (got 2147483648)"),
    (lambda: cp.normal_latents(SKIP_HUGE, ns=2, level=0, **KEY), ValueError,
     "normal_latents: at most 2^31 - 1 samples per call (got 2 x 1073741824)"),
    (lambda: cp.beta_latents(SKIP_HUGE, ns=2, level=0, **KEY), ValueError,
     "beta_latents: at most 2^31 - 1 samples per call (got 2 x 1073741824)"),
    # the test operands
    (lambda: cp.normal_latents(SKIP, _eps=SKIP, **LKEY), ValueError, "normal_latents: _eps must be [ns * B][C][H][W] on skip's device"),
    (lambda: cp.beta_latents(SKIP, _extras=[], **LKEY), TypeError, "beta_latents: _extras must be a dict"),
    # no CPU path
    (lambda: cp.truncated_normal_head(HEAD, HEAD, **KEY), RadonLibraryError,
     "truncated_normal_head: alpha and beta must be CUDA tensors on one device; there is no CPU path"),
    (lambda: cp.truncated_normal_head(HEAD, HEAD.to("meta"), **KEY), RadonLibraryError,
     "truncated_normal_head: alpha and beta must be CUDA tensors on one device; there is no CPU path"),
    (lambda: cp.beta_head(HEAD, HEAD, **KEY), RadonLibraryError,
     "beta_head: alpha and beta must be CUDA tensors on one device; there is no CPU path"),
    (lambda: cp.normal_latents(SKIP, **LKEY), RadonLibraryError, "normal_latents: skip must be a CUDA tensor; there is no CPU path"),
    (lambda: cp.beta_latents(SKIP, **LKEY), RadonLibraryError, "beta_latents: skip must be a CUDA tensor; there is no CPU path"),
]


@pytest.mark.parametrize("call, error, text", CASES, ids=[c[2].split(" (got")[0].replace(" ", "_") + f"-{i}" for i, c in enumerate(CASES)])
def test_tensor_check_type_and_full_text(call, error, text):
    with pytest.raises(error) as info:
        call()
    assert type(info.value) is error and str(info.value) == text
