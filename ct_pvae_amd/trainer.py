"""P-VAE training harness around the HIP projector (BASELINE config 3/4).

The reference's driver is ctvae/main_ct_vae.py (CT_VAE.train / train_step, :375-486) with the ELBO of
ctvae/helper_functions.py:204-332 and the nets of ctvae/models.py.  The nets and the driver are host code: here they
are plain PyTorch-ROCm (MIOpen convs); the physics decoder -- calculate_log_prob_M_given_R, the only differentiated
caller of the projector -- runs on the hand-written kernels.  What is reproduced from the reference, line by line:

  * `ns` decoder samples per step, each projected through `api` angles drawn per step from a shuffled stream of
    0..A-1 (ctvae/helper_functions.py:104-107, :263-295)
  * TruncatedNormal(positive_range(alpha), positive_range(beta), low=0, high=1e10) output distribution (:273)
  * log p(M|R): Normal(loc=proj*mask, scale=eps+sqrt(loc/pnm+eps)) (:360-368); pnm annealed as
    pnm * factor**iter with factor = exp(log(pnm/pnm_start)/num_iter) (ctvae/main_ct_vae.py:146-149, :392 -- the
    variable already holds the FINAL pnm, so the effective multiplier runs pnm .. pnm^2/pnm_start; kept as is)
  * loss = mean over the batch / 1e5 (:478); NaN gradients zeroed, per-tensor clip_by_norm(100), Adam(1e-4, eps 1e-7)
    (:353, :482-485); encoder input scaled by 1/300 (ctvae/helper_functions.py:239).  By default the Adam is torch's, whose epsilon
    stands INSIDE the bias correction (Keras's stands outside: with --ae 1e-7 the reference's acts as 3.2e-6 in torch's terms at the
    first step) and the clip multiplies by min(1, norm / l2); --fused_update runs the reference's own arithmetic (csrc/update.hip)
  * NaN loss stops the run (:401-402); checkpoint every save_interval and at the end (:409-415)

Data parallelism is new (the reference is single-device): every rank trains on its shard of the batch and the flat
gradient bucket (~0.7 M fp32) is summed with ONE all-reduce per step (RCCL over xGMI; gloo in the CPU tests).

Synthetic data stands in for the reference's dataset files: foam phantoms (phantoms.py) -> dense sinograms with the
TomoPy-style projector on the GPU (create_sinograms) -> dose masks and Poisson noise (ctvae/create_masks.py:45-63,
:94-95) -> initial reconstructions for the encoder by FBP on the GPU (iradon) in place of tomopy.recon
(ctvae/helper_functions.py:477-529): one ramp-filtered channel plus the unfiltered back-projection of the mask.
"""
import argparse
import math
import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import convblock, dataset_io, phantoms, sharding
from .conv import periodic_conv_maxout
from .conv_transpose import conv_transpose_maxout
from .convblock import dropout, dropout_pad, maxout, periodic_pad
from .create_masks import create_all_masks
from .fbp import iradon_all
from .forward_functions import num_proj_pix
from .helper_functions import calculate_log_prob_M_given_R, create_sinograms
from .latents import normal_latents
from .marginals import PixelMarginals
from ._sampling_common import EPS32
from .beta_head import beta_head
from .beta_latents import beta_latents
from .output_head import truncated_normal_head
from .update import FusedUpdate


# ---------------------------------------------------------------------------------------------------------
# nets (ctvae/models.py), channels-first
# ---------------------------------------------------------------------------------------------------------
def positive_range(x, offset=EPS32):
    """ctvae/helper_functions.py:198-201"""
    x = x - 1
    neg = (x < 0).to(x.dtype)
    return (torch.exp(torch.clamp(x, -1e10, 10)) + offset) * neg + (x + 1) * (1 - neg)


class _Maxout(torch.autograd.Function):
    """max of the two halves of the channel axis (ctvae/models.py:330-341, tf.maximum of two convolutions).  One
    comparison mask kept for the backward, which writes both halves of the gradient directly: 2 + 3 launches instead of
    the 14 of chunk + torch.maximum under autograd (two slice-backward fills and copies, mask, tie handling, add).
    Ties send the gradient to the first convolution, as TensorFlow's MaximumGrad does (x >= y)."""

    @staticmethod
    def forward(ctx, y):
        c = y.shape[1] // 2
        a, b = y[:, :c], y[:, c:]
        first = a >= b
        ctx.save_for_backward(first)
        return torch.where(first, a, b)

    @staticmethod
    def backward(ctx, g):
        first, = ctx.saved_tensors
        c = g.shape[1]
        gy = g.new_empty((g.shape[0], 2 * c) + tuple(g.shape[2:]))
        torch.mul(g, first, out=gy[:, :c])
        torch.sub(g, gy[:, :c], out=gy[:, c:])        # g where the second convolution won, 0 elsewhere (exact)
        return gy


class _PeriodicPad(torch.autograd.Function):
    """'periodic' padding of the two spatial axes (ctvae/models.py:219-263) as two gathers; the backward is the two
    matching scatter-adds (every source pixel receives at most two terms per axis, so the sum does not depend on the
    order).  4 + 6 launches instead of the ~20 of F.pad(mode='circular') under autograd (slice assignments forward,
    slice-backward fills, copies and adds backward)."""
    _index = {}

    @classmethod
    def index(cls, n, lo, hi, device):
        key = (n, lo, hi, str(device))
        idx = cls._index.get(key)
        if idx is None:
            idx = cls._index[key] = (torch.arange(-lo, n + hi, device=device) % n)
        return idx

    @staticmethod
    def forward(ctx, x, pads):
        wl, wr, hl, hr = pads
        ctx.ih = _PeriodicPad.index(x.shape[2], hl, hr, x.device)
        ctx.iw = _PeriodicPad.index(x.shape[3], wl, wr, x.device)
        ctx.hw = x.shape[2:]
        return x.index_select(2, ctx.ih).index_select(3, ctx.iw)

    @staticmethod
    def backward(ctx, g):
        H, W = ctx.hw
        gw = g.new_zeros(g.shape[:3] + (W,)).index_add_(3, ctx.iw, g)
        return gw.new_zeros(gw.shape[:2] + (H, W)).index_add_(2, ctx.ih, gw), None


class DropoutKey:
    """What the ConvBlocks of ONE network share of their dropout (--dp): the rate and the seed for good, the draw (the step index) and
    first_object (the offset of the network's batch in the global one) per call -- set(draw, first_object) before a training pass,
    clear() after it.  While no draw is set the blocks do not drop, in train() as in eval(): the evaluations run the networks as the
    reference's training=False does.  Not a module: dropout has no parameters and no state_dict entry."""

    def __init__(self, rate, seed):
        self.rate, self.seed = float(rate), int(seed)
        self.draw, self.first_object = None, 0
        convblock._rate_args("DropoutKey", self.rate)        # a bad rate is refused here, not at the first step

    def set(self, draw, first_object=0):
        self.draw, self.first_object = int(draw), int(first_object)
        return self

    def clear(self):
        self.draw = None


class ConvBlock(nn.Module):
    """Dropout => Conv2D => maxout of two convolutions (ctvae/models.py:267-342); 'periodic' padding for the strided/plain
    convolutions (:219-263), Conv2DTranspose(padding='same') for up-sampling.  fused_blocks: the padding and the maxout are one launch
    each way (convblock.periodic_pad / maxout, csrc/convblock.hip) instead of _PeriodicPad's and _Maxout's chains of torch launches;
    the parameters and their names are the same either way.  dropout: None, or the network's DropoutKey; `layer` is then the block's
    number in the stream.  In training mode, while the key holds a draw, the block drops its input (:283-284) -- inside the pad's launch
    with fused_blocks (convblock.dropout_pad), as convblock.dropout in front of _PeriodicPad without, and in front of the transposed
    convolution, which has no pad, either way.  The mask is a function of (seed, draw, layer, global object, element): no generator
    state, nothing stored for the backward.  fused_conv: a non-transposed block is ONE launch, conv.periodic_conv_maxout on ab's own
    weight and bias (csrc/conv.hip: padding, convolution and maxout with every sum in one stated order), after convblock.dropout
    where the block drops -- the bits of dropout_pad followed by that convolution; a transposed block is untouched by it.
    fused_convt: a transposed block is ONE launch, conv_transpose.conv_transpose_maxout on ab's own weight, bias, stride, padding and
    output_padding (csrc/conv_transpose.hip: transposed convolution and maxout with every sum in one stated order), after
    convblock.dropout where the block drops; a non-transposed block ignores it.  Parameters, names, initialisation and checkpoints
    are the same with and without either flag."""

    def __init__(self, cin, cout, k, stride, transpose, fused_blocks=False, dropout=None, layer=0, fused_conv=False, fused_convt=False):
        super().__init__()
        self.k, self.stride, self.transpose, self.fused_blocks = k, stride, transpose, bool(fused_blocks)
        self.fused_conv, self.fused_convt = bool(fused_conv), bool(fused_convt)
        self.dropout, self.layer = dropout, int(layer)
        # the two convolutions of the maxout are ONE convolution with 2 * cout output channels (half the launches);
        # each half is initialised as its own GlorotUniform layer
        if transpose:
            pad = (k - stride + 1) // 2
            opad = stride + 2 * pad - k
            if not 0 <= opad < stride:             # e.g. the toy recipe's --ks 2 --se 1: one pixel too many, cropped by the decoder
                pad = max((k - stride) // 2, 0)
                opad = min(max(stride + 2 * pad - k, 0), stride - 1)
            self.ab = nn.ConvTranspose2d(cin, 2 * cout, k, stride=stride, padding=pad, output_padding=opad)
            halves = self.ab.weight.data.chunk(2, dim=1)        # ConvTranspose2d weight: [cin][cout][k][k]
        else:
            self.ab = nn.Conv2d(cin, 2 * cout, k, stride=stride, padding=0)
            halves = self.ab.weight.data.chunk(2, dim=0)        # Conv2d weight: [cout][cin][k][k]
        for h in halves:
            nn.init.xavier_uniform_(h)             # GlorotUniform (fan-in / fan-out of ONE of the two convolutions)
        nn.init.zeros_(self.ab.bias)

    def forward(self, x):
        d = self.dropout if self.training and self.dropout is not None and self.dropout.draw is not None else None
        key = dict(seed=d.seed, draw=d.draw, layer=self.layer, first_object=d.first_object) if d is not None else None
        if self.transpose:
            if d is not None:
                x = dropout(x.contiguous(), d.rate, **key)
            if self.fused_convt:
                return conv_transpose_maxout(x.contiguous(), self.ab.weight, self.ab.bias, self.ab.stride[0], self.ab.padding[0],
                                             self.ab.output_padding[0])
        else:
            pads = []
            for n in (x.shape[-1], x.shape[-2]):   # last axis first, as torch.nn.functional.pad orders them
                p = self.k - (n % self.stride if n % self.stride else self.stride)
                pads += [p // 2 + p % 2, p // 2]
            if self.fused_conv:
                x = x.contiguous()
                if d is not None:
                    x = dropout(x, d.rate, **key)
                return periodic_conv_maxout(x, self.ab.weight, self.ab.bias, self.stride, tuple(pads))
            if d is None:
                x = periodic_pad(x.contiguous(), tuple(pads)) if self.fused_blocks else _PeriodicPad.apply(x, tuple(pads))
            elif self.fused_blocks:
                x = dropout_pad(x.contiguous(), tuple(pads), d.rate, **key)
            else:
                x = _PeriodicPad.apply(dropout(x.contiguous(), d.rate, **key), tuple(pads))
        return maxout(self.ab(x).contiguous()) if self.fused_blocks else _Maxout.apply(self.ab(x))


class EncodeNet(nn.Module):
    """create_encode_net, ctvae/models.py:23-108: returns the list of skips (the first one is the repeated input)."""

    def __init__(self, cin, feature_maps, fmm, kernel, stride, inter_layers, inter_kernel, fused_blocks=False, dropout=None, first_layer=0,
                 fused_conv=False, fused_convt=False):
        super().__init__()
        self.fmm = fmm
        c = cin * fmm
        self.channels = [c]
        self.blocks = nn.ModuleList()
        self.dropout = dropout
        layer = iter(range(first_layer, 2 ** 24))            # the blocks' dropout layers: numbered in construction order
        for f in feature_maps:
            layers = [ConvBlock(c, c, inter_kernel, 1, False, fused_blocks=fused_blocks, dropout=dropout, layer=next(layer), fused_conv=fused_conv,
                                fused_convt=fused_convt) for _ in range(inter_layers)]
            layers.append(ConvBlock(c, f * fmm, kernel, stride, False, fused_blocks=fused_blocks, dropout=dropout, layer=next(layer),
                                    fused_conv=fused_conv, fused_convt=fused_convt))
            self.blocks.append(nn.Sequential(*layers))
            c = f * fmm
            self.channels.append(c)
        self.num_layers = next(layer) - first_layer

    def forward(self, x):
        x = x.repeat_interleave(self.fmm, dim=1)   # tf.repeat(output, feature_maps_multiplier, axis=-1)
        skips = [x]
        for blk in self.blocks:
            x = blk(x)
            skips.append(x)
        return skips


class DecodeNet(nn.Module):
    """create_decode_net, ctvae/models.py:112-215 (the code concatenates every skip, including the input level)."""

    def __init__(self, enc_channels, fmm, out_channels, kernel, stride, inter_layers, inter_kernel, fused_blocks=False, dropout=None,
                 first_layer=0, fused_conv=False, fused_convt=False):
        super().__init__()
        lat = [c // fmm for c in enc_channels]     # channels of the sampled latents
        self.ups = nn.ModuleList()
        self.dropout = dropout
        layer = iter(range(first_layer, 2 ** 24))            # as the encoder's; the trainer numbers the decoder's blocks after them
        c = lat[-1]
        for lvl in range(len(enc_channels) - 2, -1, -1):
            layers = [ConvBlock(c, enc_channels[lvl], kernel, stride, True, fused_blocks=fused_blocks, dropout=dropout, layer=next(layer),
                                fused_conv=fused_conv, fused_convt=fused_convt)]
            layers += [ConvBlock(enc_channels[lvl], enc_channels[lvl], inter_kernel, 1, False, fused_blocks=fused_blocks, dropout=dropout,
                                 layer=next(layer), fused_conv=fused_conv, fused_convt=fused_convt) for _ in range(inter_layers)]
            self.ups.append(nn.Sequential(*layers))
            c = enc_channels[lvl] + lat[lvl]
        self.head = ConvBlock(c, 2 * out_channels, kernel, 1, False, fused_blocks=fused_blocks, dropout=dropout, layer=next(layer),
                              fused_conv=fused_conv, fused_convt=fused_convt)
        self.num_layers = next(layer) - first_layer

    def forward(self, latents):
        x = latents[-1]
        for up, skip in zip(self.ups, reversed(latents[:-1])):
            x = up(x)
            dx, dy = x.shape[-2] - skip.shape[-2], x.shape[-1] - skip.shape[-1]
            x0, y0 = dx // 2 + dx % 2, dy // 2 + dy % 2
            x = x[..., x0:x0 + skip.shape[-2], y0:y0 + skip.shape[-1]]
            x = torch.cat([x, skip], dim=1)
        alpha, beta = self.head(x).chunk(2, dim=1)
        return alpha, beta


# ---------------------------------------------------------------------------------------------------------
# distributions
# ---------------------------------------------------------------------------------------------------------
_SQRT2 = math.sqrt(2.0)


def _ncdf(z):
    return 0.5 * (1 + torch.erf(z / _SQRT2))


class TruncatedNormal:
    """tfd.TruncatedNormal(loc, scale, low, high): reparameterised sample by inverse CDF, log_prob."""

    def __init__(self, loc, scale, low=0.0, high=1e10):
        self.loc, self.scale = loc, scale
        self.a, self.b = (low - loc) / scale, (high - loc) / scale
        self.cdf_a, self.cdf_b = _ncdf(self.a), _ncdf(self.b)
        self.Z = (self.cdf_b - self.cdf_a).clamp_min(1e-30)

    def rsample(self):
        u = torch.rand_like(self.loc)
        p = (self.cdf_a + u * self.Z).clamp(1e-7, 1 - 1e-7)
        z = torch.special.ndtri(p)
        return (self.loc + self.scale * z).clamp_min(0.0)

    def log_prob(self, x):
        z = (x - self.loc) / self.scale
        return -0.5 * z * z - 0.5 * math.log(2 * math.pi) - torch.log(self.scale) - torch.log(self.Z)


def kl_normal_std(loc, scale):
    """KL(N(loc, scale) || N(0, 1)), elementwise."""
    return 0.5 * (scale * scale + loc * loc - 1.0) - torch.log(scale)


# ---------------------------------------------------------------------------------------------------------
# ELBO (ctvae/helper_functions.py:204-332; --normal: Normal latents + TruncatedNormal output, otherwise the reference's
# default Beta latents, Beta(0.5, 0.5) prior and Beta output, :247-252, :275-285, ctvae/main_ct_vae.py:369-372)
# ---------------------------------------------------------------------------------------------------------
def find_loss_vae_unsup(proj_sample, mask, input_encode, model_encode, model_decode, poisson_noise_multiplier, sqrt_reg,
                        kl_anneal, kl_multiplier, num_samples=2, theta=None, angles_i=None, pad=True, deterministic=False,
                        use_normal=True, model="rotate", noise="gaussian", fused_head=None, fused_latents=None,
                        fused_beta_head=None, fused_beta_latents=None):
    """fused_head: None -- the output distribution is the chain of torch operations below, its uniforms from torch's global
    generator -- or (seed, draw, first_object): sample, log-density and its per-object sum come from ONE launch
    (output_head.truncated_normal_head, csrc/head.hip), the uniforms from Philox keyed by those three; --normal only.
    fused_latents: None -- the Normal latents and their KL term are the chain of torch operations below, the draws from torch's
    global generator -- or (seed, draw, first_object): per skip level ONE launch gives the ns samples and the per-object KL
    (latents.normal_latents, csrc/latent.hip), the draws from Philox keyed by those three, the level and the sample; first_object is
    the offset of this call's objects in the GLOBAL batch; --normal only, not with deterministic.
    fused_beta_head: None, or (seed, draw, first_object): the DEFAULT Beta output head (use_normal=False) -- sample, clamp, log-density
    and its per-object sum -- comes from ONE launch (beta_head.beta_head, csrc/beta_head.hip), the draws from Philox keyed by those
    three, the gradient TensorFlow's implicit one.  Allowed with deterministic=True: the reference samples the output distribution
    there too.
    fused_beta_latents: None -- the DEFAULT Beta latents and their KL term against Beta(0.5, 0.5) are the chain of torch operations
    below, the draws from torch's global generator, the gradient torch's direct Beta derivative -- or (seed, draw, first_object): per
    skip level ONE launch gives the ns samples and the per-object KL (beta_latents.beta_latents, csrc/beta_latent.hip), the draws from
    Philox keyed by those three, the level and the sample, the gradient TensorFlow's implicit one; first_object is the offset of this
    call's objects in the GLOBAL batch; use_normal=False only, not with deterministic."""
    if fused_head is not None and not use_normal:
        raise ValueError("fused_head is the TruncatedNormal output head: it needs use_normal=True (the Beta head is fused_beta_head)")
    if fused_beta_head is not None and use_normal:
        raise ValueError("fused_beta_head is the Beta output head: it needs use_normal=False (with use_normal=True the output is "
                         "TruncatedNormal: fused_head)")
    if fused_latents is not None and (not use_normal or deterministic):
        raise ValueError("fused_latents is the Normal latent block: it needs use_normal=True and deterministic=False (the Beta latents "
                         "are fused_beta_latents)")
    if fused_beta_latents is not None and (use_normal or deterministic):
        raise ValueError("fused_beta_latents is the Beta latent block: it needs use_normal=False and deterministic=False (the Normal "
                         "latents are fused_latents)")
    skips = model_encode(input_encode / 300)
    q = None
    if not deterministic and fused_latents is None and fused_beta_latents is None:
        q = []
        for sk in skips:
            loc, log_scale = sk.chunk(2, dim=1)
            if use_normal:
                q.append((loc, positive_range(log_scale) + sqrt_reg))
            else:                                                   # :252 tfd.Beta(positive_range(loc), scale)
                q.append(torch.distributions.Beta(positive_range(loc), positive_range(log_scale)))
    # The reference draws its `num_samples` latent samples in a Python loop (:263-312); they are independent, so here
    # they ride the batch axis: ONE decoder pass and ONE projector + likelihood pass over num_samples * B objects
    # (sample-major), the same estimator with half the launches at ns = 2.
    ns = 1 if deterministic else int(num_samples)
    B = input_encode.shape[0]
    if deterministic:
        q_sample = skips
    elif fused_latents is not None:
        seed, draw, first_object = fused_latents
        q_sample, level_kl = [], []
        for level, sk in enumerate(skips):
            z, kl_level = normal_latents(sk.contiguous(), ns=ns, seed=seed, draw=draw, level=level, first_object=first_object,
                                         sqrt_reg=sqrt_reg)
            q_sample.append(z)
            level_kl.append(kl_level)
    elif fused_beta_latents is not None:                            # :249-254, :267 in one launch per level
        seed, draw, first_object = fused_beta_latents
        q_sample, level_kl = [], []
        for level, sk in enumerate(skips):                          # the input level's KL is unused (:325-327): it is not computed
            z, kl_level = beta_latents(sk.contiguous(), ns=ns, seed=seed, draw=draw, level=level, first_object=first_object,
                                       want_kl=level > 0)
            q_sample.append(z)
            level_kl.append(kl_level)
    elif use_normal:
        q_sample = [loc.repeat(ns, 1, 1, 1) + scale.repeat(ns, 1, 1, 1) * torch.randn((ns * B,) + tuple(loc.shape[1:]),
                                                                                      device=loc.device, dtype=loc.dtype)
                    for loc, scale in q]
    else:                                                           # reparameterised Beta samples, sample-major
        q_sample = [d.rsample((ns,)).reshape((ns * B,) + tuple(d.concentration1.shape[1:])) for d in q]
    alpha, beta = model_decode(q_sample)
    if fused_head is not None:
        seed, draw, first_object = fused_head
        # (the decoder's alpha / beta are the two channel halves of one tensor: each is made contiguous, one copy)
        x, head_lp = truncated_normal_head(alpha.contiguous(), beta.contiguous(), seed=seed, draw=draw, first_object=first_object)
        output_sample = x.permute(0, 3, 1, 2)                            # [ns * B][1][X][Y], a view: the projector gets x itself
    elif use_normal:
        dist = TruncatedNormal(positive_range(alpha), positive_range(beta), low=0.0, high=1e10)
        output_sample = dist.rsample()                                   # [ns * B][1][X][Y]
        log_prob_R_given_z = dist.log_prob(output_sample)
    elif fused_beta_head is not None:                               # :278-285 in one launch
        seed, draw, first_object = fused_beta_head
        x, head_lp = beta_head(alpha.contiguous(), beta.contiguous(), seed=seed, draw=draw, first_object=first_object, sqrt_reg=sqrt_reg)
        output_sample = x.permute(0, 3, 1, 2)
    else:                                                           # :278-285
        dist = torch.distributions.Beta(positive_range(alpha), positive_range(beta))
        output_sample = dist.rsample()
        log_prob_R_given_z = dist.log_prob(output_sample.clamp(sqrt_reg, 1 - sqrt_reg))
    # per-object sums of the log-probabilities, reduced inside the projector launch
    lp = calculate_log_prob_M_given_R(output_sample.permute(0, 2, 3, 1), mask.repeat(ns, 1), proj_sample.repeat(ns, 1, 1),
                                      poisson_noise_multiplier, sqrt_reg, theta=theta, angles_i=angles_i, pad=pad,
                                      reduce="per_object", model=model, noise=noise)
    # :305-306 reduce_sum(..., axis=[0, 1, 2]) of the squeezed [B][A][P] and [B][X][Y] tensors: the log-likelihood of a
    # sample is ONE number for the whole batch (the batch axis is summed too), the KL below is per object; :329-330 then
    # broadcast-subtract, and train_step takes the mean over the batch -- i.e. mean_b(KL_b) - sum_b(loglik_b).
    if fused_head is None and fused_beta_head is None:
        head_lp = log_prob_R_given_z.sum(dim=(1, 2, 3))
    log_prob_M = (lp + head_lp).view(ns, B).sum(dim=1)                                    # [ns]
    recon = output_sample[(ns - 1) * B:]
    if deterministic:
        kl = lp.new_zeros(B)
    elif fused_latents is not None or fused_beta_latents is not None:
        kl = sum(level_kl[2:], level_kl[1]) if len(level_kl) > 1 else lp.new_zeros(B)   # ascending level; the input level is unused
    elif use_normal:
        kl = sum(kl_normal_std(loc, scale).sum(dim=(1, 2, 3)) for loc, scale in q[1:])   # the input level is unused
    else:                                                           # prior Beta(0.5, 0.5), ctvae/main_ct_vae.py:372
        kl = sum(torch.distributions.kl_divergence(d, torch.distributions.Beta(torch.full_like(d.concentration1, 0.5),
                                                                             torch.full_like(d.concentration1, 0.5)))
                 .sum(dim=(1, 2, 3)) for d in q[1:])
    loglik = log_prob_M.mean(dim=0)                                                       # scalar
    return kl_anneal * kl_multiplier * kl - loglik, kl, loglik, recon


# ---------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------
class AngleStream:
    """Shuffled, repeating stream of 0..A-1 in chunks of `api` (ctvae/helper_functions.py:104-107)."""

    def __init__(self, num_angles, api, seed):
        self.n, self.api, self.rng, self.buf = num_angles, api, np.random.default_rng(seed), np.empty(0, np.int64)

    def next(self):
        while self.buf.size < self.api:
            self.buf = np.concatenate([self.buf, self.rng.permutation(self.n)])
        out, self.buf = self.buf[:self.api], self.buf[self.api:]
        return out


_PIXEL_DIST_NEEDS = ("--pixel_dist adds the keyed samples of a fused output head over sampled latents: it needs --normal (the "
                     "TruncatedNormal head's marginals) or --fused_beta_head (the default Beta head's: the marginals are that keyed head's "
                     "samples, there are none of torch's generator's) and cannot be combined with --det")


def _pixel_dist_head(args):
    """The one rule of --pixel_dist (get_args, PVAETrainer and pixel_dist apply it): the PixelMarginals head of these arguments --
    "truncated_normal" with --normal, "beta" with --fused_beta_head and no --normal -- or a ValueError; never with --det."""
    if args.deterministic or not (args.use_normal or getattr(args, "fused_beta_head", False)):
        raise ValueError(_PIXEL_DIST_NEEDS)
    return "truncated_normal" if args.use_normal else "beta"


_FUSED_BETA_HEAD_NEEDS = "--fused_beta_head is the default Beta output head: it cannot be combined with --normal (there: --fused_head)"
_FUSED_LATENTS_NEEDS = ("--fused_latents is the Normal latent block: it needs --normal and cannot be combined with --det (the default Beta "
                        "latents: --fused_beta_latents)")
_FUSED_BETA_LATENTS_NEEDS = ("--fused_beta_latents is the default Beta latent block: it cannot be combined with --normal (there: "
                             "--fused_latents) or with --det")


class PVAETrainer:
    def __init__(self, args, device):
        self.args, self.dev = args, device
        if getattr(args, "fused_head", False) and not args.use_normal:
            raise ValueError("--fused_head is the TruncatedNormal output head: it needs --normal")
        if getattr(args, "fused_beta_head", False) and args.use_normal:
            raise ValueError(_FUSED_BETA_HEAD_NEEDS)
        if getattr(args, "fused_latents", False) and (not args.use_normal or args.deterministic):
            raise ValueError(_FUSED_LATENTS_NEEDS)
        if getattr(args, "fused_beta_latents", False) and (args.use_normal or args.deterministic):
            raise ValueError(_FUSED_BETA_LATENTS_NEEDS)
        if getattr(args, "pixel_dist", False):
            _pixel_dist_head(args)
        self.world, self.rank, _ = sharding.env_world()
        self.sqrt_reg = EPS32
        # the nets' shapes are static: --miopen_find lets MIOpen search its convolution algorithms once (14.9 -> 11.5 ms
        # per step at batch 5 on the MI355X, after a search that costs tens of seconds; channels-last was measured too
        # and loses)
        if getattr(args, "miopen_find", False):
            torch.backends.cudnn.benchmark = True
        # --reproducible: MIOpen's default algorithms add the convolutions' weight gradients in an order that changes from run to run
        # (measured: every conv weight's gradient differs in its last bits between two equal-seed runs, with or without --fused_head;
        # none does with this switch).  The switch is process-wide, as torch defines it, and changes every convolution's algorithm.
        if getattr(args, "reproducible", False):
            torch.backends.cudnn.deterministic = True
        torch.manual_seed(1234 + self.rank)
        a = args
        self.pnm_anneal = math.exp(math.log(a.pnm / a.pnm_start) / max(a.num_iter, 1)) if a.pnm_start else 1.0
        self._make_data()
        fm = [int(a.nfm * a.nfmm ** i) for i in range(a.num_blocks)]
        fmm = 1 if a.deterministic else 2
        fused_blocks = bool(getattr(a, "fused_blocks", False))
        fused_conv = bool(getattr(a, "fused_conv", False))
        fused_convt = bool(getattr(a, "fused_convt", False))
        # --dp: one DropoutKey per network (their batches differ: B objects in the encoder, ns * B sample-major in the decoder); the
        # blocks' layers run through the encoder, then the decoder.  With --dp 0 the networks are built exactly as without the flag.
        dp = float(getattr(a, "dropout_prob", 0.0) or 0.0)
        self.enc_drop = DropoutKey(dp, a.head_seed) if dp > 0 else None
        self.dec_drop = DropoutKey(dp, a.head_seed) if dp > 0 else None
        self.enc = EncodeNet(len(a.algorithms) + 1, fm, fmm, a.kernel_size, a.stride_encode, a.il, a.ik, fused_blocks=fused_blocks,
                             dropout=self.enc_drop, fused_conv=fused_conv, fused_convt=fused_convt).to(device)
        self.dec = DecodeNet(self.enc.channels, fmm, 1, a.kernel_size, a.stride_encode, a.il, a.ik, fused_blocks=fused_blocks,
                             dropout=self.dec_drop, first_layer=self.enc.num_layers, fused_conv=fused_conv,
                             fused_convt=fused_convt).to(device)
        if self.world > 1:   # identical initial weights on every rank
            for p in list(self.enc.parameters()) + list(self.dec.parameters()):
                torch.distributed.broadcast(p.data, 0)
        self.params = list(self.enc.parameters()) + list(self.dec.parameters())
        self._bucket = None   # the gradients' resident flat bucket (built on the first step)
        if getattr(a, "noise", "gaussian") == "poisson" and a.train_pnm:
            raise ValueError("--noise poisson takes the noise multiplier as data: it cannot be combined with --train_pnm")
        self.pnm = torch.tensor(float(a.pnm), device=device, requires_grad=bool(a.train_pnm))
        # fused: the whole Adam update in one multi-tensor launch on the device (the default foreach form is ~10)
        self.opt = torch.optim.Adam(self.params + ([self.pnm] if a.train_pnm else []), lr=a.lr, eps=a.adam_epsilon,
                                    fused=(device.type == "cuda") and os.environ.get("CTPVAE_ADAM_FUSED", "1") == "1")
        # --fused_update: the update stage is update.FusedUpdate (csrc/update.hip) over the parameters that get a gradient, built at the first
        # step (or from a restored checkpoint's entries); self.opt then only holds the parameter list and the group's settings
        self.upd = None
        self.kl_anneal = 1.0
        self.angles = AngleStream(self.num_angles, a.api, seed=7)     # same stream on every rank
        self.iter = 0

    # -- dataset: --input_path (the reference's dataset_<name>/ folder) or a synthetic foam set -----------------
    def _make_data(self):
        a, dev = self.args, self.dev
        self.pad = not a.no_pad
        if a.input_path:
            # x_train_sinograms.npy + dataset_parameters.npy as scripts/images_to_sinograms.py writes them
            # (ctvae/main_ct_vae.py:152-161); the phantoms themselves are not part of that folder
            sino_np, self.theta_np, self.P = dataset_io.get_sinograms(a.input_path)
            a.td = min(a.td, sino_np.shape[0])
            sino = torch.from_numpy(np.ascontiguousarray(sino_np[:a.td], dtype=np.float32)).to(dev)
            self.theta_np = np.asarray(self.theta_np, dtype=np.float64)
            self.num_angles = a.num_angles = len(self.theta_np)
            imgs = None
        else:
            N = a.n_pixel
            self.theta_np = phantoms.dense_theta(a.num_angles)
            self.num_angles = a.num_angles
            self.P = num_proj_pix(N, N) if self.pad else N
            imgs = phantoms.foam_batch(a.td, N, seed=0, supersample=2)
            sino = create_sinograms(torch.from_numpy(imgs).to(dev), self.theta_np, pad=self.pad).clamp_min(0)   # [td][A][P]
        # ctvae/main_ct_vae.py:156-161: --no_pad sinograms are as wide as the object
        self.x_size = self.y_size = int(math.floor(self.P / math.sqrt(2) - 2)) if self.pad else self.P
        # dose masks and sparse noisy measurements, ctvae/create_masks.py:45-95 (simulated at the FINAL pnm)
        # with --save_path the three setup arrays are written there when training and read back when not (the
        # reference's train / restore split, ctvae/create_masks.py:70,101-103, ctvae/helper_functions.py:523-526)
        drawing = bool(a.train) or not a.save_path
        # every rank draws the same arrays (same seeds); only rank 0 writes them -- concurrent np.save of one path from
        # several ranks is a truncate-and-write race
        save_here = a.save_path if (self.rank == 0 or not drawing) else None
        masks, self.proj_samples = create_all_masks(sino, a.num_angles, save_path=save_here, poisson_noise_multiplier=a.pnm,
                                                    num_sparse_angles=a.nsa, random=a.random, train=drawing, real_data=a.real_data,
                                                    toy_masks=a.toy_masks,
                                                    truncate_dataset=a.td, device=dev)
        self.masks, self.truth = masks, (torch.from_numpy(imgs).to(dev) if imgs is not None else None)
        self.sinograms = sino if getattr(a, "final_merit", False) else None           # the clean sinograms, kept for --final_merit only
        # initial reconstructions for the encoder, ctvae/helper_functions.py:477-529 with FBP on the GPU
        enc_in = iradon_all(self.proj_samples, masks, self.P, self.theta_np, list(a.algorithms), self.sqrt_reg, self.x_size,
                            self.y_size, save_path=save_here, train=drawing)          # [td][X][Y][len(algorithms) + 1]
        if self.world > 1 and drawing and a.save_path:
            torch.distributed.barrier()                                                # files complete before anyone goes on
        self.input_encode = enc_in.permute(0, 3, 1, 2).contiguous()                   # [td][2][X][Y]
        self.theta = torch.from_numpy(self.theta_np.astype(np.float32)).to(dev)
        # the projector gets the HOST angle list: its tables and gather plan are then built once, on the host's bits, and
        # every step only passes its angle subset as an index operand
        self.theta_host = np.ascontiguousarray(self.theta_np, dtype=np.float32)
        self.order = np.random.default_rng(11)

    def _batch(self):
        """Global batch of `-b` examples, the same on every rank; each rank keeps its shard."""
        idx = self.order.choice(self.args.td, size=self.args.batch_size, replace=False)
        lo, hi = sharding.shard_range(len(idx), self.rank, self.world)
        idx = self._to_device(idx[lo:hi])
        return self.proj_samples[idx], self.masks[idx], self.input_encode[idx]

    def _to_device(self, host_array):
        """Small per-step index arrays go up through pinned memory without waiting: a plain torch.as_tensor(...,
        device=) is a blocking copy that first drains the stream, i.e. idles the GPU while the host prepares a step."""
        t = torch.from_numpy(np.ascontiguousarray(host_array))
        if self.dev.type != "cuda":
            return t
        return t.pin_memory().to(self.dev, non_blocking=True)

    # -- one step (CT_VAE.train_step, ctvae/main_ct_vae.py:463-486) -------------------------------------------
    def _next_inputs(self):
        """Host side of a step: the batch, the angle subset and the two annealed scalars."""
        a = self.args
        proj_sample, mask, input_encode = self._batch()
        # the step's angle subset stays in HOST memory: the projector kernels carry it in their launch arguments (no upload,
        # nothing on the stream in front of the forward)
        angles_i = torch.from_numpy(np.ascontiguousarray(self.angles.next().astype(np.int32)))
        pnm_factor = self.pnm_anneal ** self.iter
        self.kl_anneal = min(max(self.kl_anneal * a.klaf, 0.0), 100.0)
        return proj_sample, mask, input_encode, angles_i, pnm_factor, self.kl_anneal

    def _loss_and_update(self, proj_sample, mask, input_encode, angles_i, pnm_factor, kl_anneal):
        """Device side of a step: ELBO, backward, NaN filter + clip, Adam."""
        a = self.args
        pnm_i = self.pnm * pnm_factor
        # --fused_head: the draw is the global step index (saved and restored with the checkpoint's "iter"), the objects of
        # this rank follow those of the ranks before it -- a step's samples depend on (--head_seed, step, object) alone.  (The
        # batch is sample-major, [ns][B]: object (s, b) of rank r is r * ns * B + s * B + b, NOT the s * B_global + r * B + b it
        # would be in one rank's global batch -- a run is replayable at its own world size, not across world sizes.)
        fused = None
        if getattr(a, "fused_head", False):
            fused = (a.head_seed, self.iter, self.rank * (1 if a.deterministic else a.ns) * input_encode.shape[0])
        fused_beta = None                  # --fused_beta_head: keyed exactly as --fused_head
        if getattr(a, "fused_beta_head", False):
            fused_beta = (a.head_seed, self.iter, self.rank * (1 if a.deterministic else a.ns) * input_encode.shape[0])
        # --fused_latents: the same seed and draw; the latents' objects are counted in the GLOBAL batch (the sample index is a counter
        # word of its own), so their draws are the same at every world size
        fused_lat = None
        if getattr(a, "fused_latents", False):
            fused_lat = (a.head_seed, self.iter, sharding.shard_range(a.batch_size, self.rank, self.world)[0])   # _batch's lo
        fused_beta_lat = None              # --fused_beta_latents: keyed exactly as --fused_latents
        if getattr(a, "fused_beta_latents", False):
            fused_beta_lat = (a.head_seed, self.iter, sharding.shard_range(a.batch_size, self.rank, self.world)[0])
        # --dp: seed = --head_seed, draw = the step index; the objects are counted as the head counts them (rank * B in the encoder,
        # rank * ns * B in the decoder's sample-major batch), so a run replays at its own world size.  The keys hold a draw only while
        # the training pass is built: every other caller of the networks (the evaluations, --pixel_dist) runs them without dropout.
        if self.enc_drop is not None:
            nb = input_encode.shape[0]
            self.enc_drop.set(self.iter, self.rank * nb)
            self.dec_drop.set(self.iter, self.rank * (1 if a.deterministic else a.ns) * nb)
        try:
            loss_vec, kl, loglik, _ = find_loss_vae_unsup(proj_sample, mask, input_encode, self.enc, self.dec, pnm_i,
                                                          self.sqrt_reg, kl_anneal, a.klm, num_samples=a.ns,
                                                          theta=self.theta_host, angles_i=angles_i, pad=self.pad,
                                                          deterministic=a.deterministic, use_normal=a.use_normal,
                                                          model=getattr(a, "model", "rotate"), noise=getattr(a, "noise", "gaussian"),
                                                          fused_head=fused, fused_latents=fused_lat, fused_beta_head=fused_beta,
                                                          fused_beta_latents=fused_beta_lat)
        finally:
            if self.enc_drop is not None:
                self.enc_drop.clear(), self.dec_drop.clear()
        # ctvae/main_ct_vae.py:478 reduce_mean(loss_M_VAE) / 1e5 = mean_b(KL term) - loglik, where loglik already sums
        # over the batch.  Written so that the ranks' losses ADD UP to the global one (gradients are summed over ranks):
        # each rank contributes its objects' KL / global_B and its own objects' log-likelihood.
        del loss_vec
        loss = ((kl_anneal * a.klm * kl).sum() / a.batch_size - loglik) / 1e5
        self.opt.zero_grad(set_to_none=True)
        # one calling-thread pass over the graph: the default engine hands every backward() to a per-device worker thread
        # (~50 us of hand-off, and the Python backward of the projector node then runs behind the GIL of that thread)
        with torch.autograd.set_multithreading_enabled(False):
            loss.backward()
        with_grad = [p for p in self.opt.param_groups[0]["params"] if p.grad is not None]
        grads = [p.grad for p in with_grad]
        # ONE resident flat bucket (round 4): a multi-tensor copy in, one all-reduce on that memory, the filter and the clip on its
        # slices, and p.grad pointed at the slices -- no torch.cat, no per-tensor copy back (sharding.FlatGradBucket)
        if self._bucket is None or not self._bucket.matches(grads):
            self._bucket = sharding.FlatGradBucket(grads)
        bucket = self._bucket.fill(grads).allreduce_(average=False)
        if getattr(a, "fused_update", False):
            # the reference's own arithmetic (Keras's epsilon placement, tf.clip_by_norm's form) in two launches with a stated order of
            # the norms' sums: the bucket is read only, p.grad is not pointed at it and self.opt takes no step
            self._fused_update(with_grad).step(bucket.flat)
            return loss.detach()
        # tf.where(is_nan, 0, grad), then tf.clip_by_norm(g, norm) per tensor (ctvae/main_ct_vae.py:482-484) -- in one
        # flat buffer and a handful of multi-tensor launches, with no host round trip (a Python `if norm > clip` per
        # tensor would synchronise 76 times a step)
        torch.nan_to_num_(bucket.flat, nan=0.0)
        norms = torch.stack(torch._foreach_norm(bucket.views))
        scales = (a.norm / norms).clamp_(max=1.0)                          # norm / max(l2, norm); l2 = 0 -> 1
        torch._foreach_mul_(bucket.views, list(scales.unbind()))
        bucket.attach(with_grad)
        self.opt.step()
        return loss.detach()

    def _fused_update(self, with_grad):
        """--fused_update's FusedUpdate over exactly the parameters that got a gradient this step (--train_pnm's scalar among them: a
        tensor of one element).  Should the set change between steps, the moments move over through the state dictionary."""
        a = self.args
        if self.upd is None or not self.upd.same_params(with_grad):
            state = self.optimizer_state() if self.upd is not None else None
            self.upd = FusedUpdate(with_grad, lr=a.lr, eps=a.adam_epsilon, clip_norm=a.norm)
            if state is not None:
                self._load_fused_update(state, with_grad)
        return self.upd

    def _load_fused_update(self, state, params):
        """Load the entries of `params` from a state dictionary laid out over self.opt's whole parameter list."""
        index = {id(p): i for i, p in enumerate(self.opt.param_groups[0]["params"])}
        rows = [index[id(p)] for p in params]
        self.upd.load_state_dict({"state": {k: state["state"][i] for k, i in enumerate(rows) if i in state["state"]},
                                  "param_groups": [dict(state["param_groups"][0], params=list(range(len(rows))))]})

    def optimizer_state(self):
        """The optimiser's state dictionary in torch.optim.Adam's layout over self.opt's parameter list -- with --fused_update taken
        from the FusedUpdate (step, exp_avg = m, exp_avg_sq = v of the parameters it updates), so that a checkpoint written with the
        flag restores without it and the other way round."""
        if not getattr(self.args, "fused_update", False) or self.upd is None:
            return self.opt.state_dict()
        index = {id(p): i for i, p in enumerate(self.opt.param_groups[0]["params"])}
        own = self.upd.state_dict()
        group = dict(self.opt.state_dict()["param_groups"][0], lr=self.upd.lr, betas=(self.upd.beta1, self.upd.beta2), eps=self.upd.eps)
        return {"state": {index[id(p)]: own["state"][k] for k, p in enumerate(self.upd.params) if k in own["state"]}, "param_groups": [group]}

    def train_step(self, sync=True):
        """One optimisation step.  sync=True returns the loss as a python float (a host round trip, as the reference's
        per-iteration `.numpy()`); sync=False returns it as a 0-d device tensor so that the host keeps queueing the
        next step's ~800 launches while the GPU finishes this one (`train` reads the losses back in blocks)."""
        loss = self._loss_and_update(*self._next_inputs())
        self.iter += 1
        if self.world > 1:
            loss = loss.clone()
            torch.distributed.all_reduce(loss)
        return float(loss.item()) if sync else loss

    def train(self):
        a = self.args
        losses, pending, t0 = [], [], time.time()
        every = max(a.num_iter // 10, 1)
        for it in range(a.num_iter):
            pending.append(self.train_step(sync=False))
            report = it % every == 0 or it == a.num_iter - 1
            saving = bool(a.save_path) and (it % a.si == 0 or it == a.num_iter - 1)
            if report or saving or len(pending) >= 32:
                # losses come back in blocks: one host round trip per block instead of one per iteration; the
                # reference's NaN stop (ctvae/main_ct_vae.py:401-402) therefore acts within 32 iterations
                losses += torch.stack(pending).tolist()
                pending = []
                if any(math.isnan(v) for v in losses[-32:]):
                    raise SystemExit("loss is NaN")
            if report and self.rank == 0:
                print(f"Iteration number: {it}  Training loss_M_VAE: {losses[-1]:.6f}", flush=True)
            if saving and self.rank == 0:
                self.save(os.path.join(a.save_path, "training_checkpoints", f"ckpt-{it}.pt"), losses)
                np.save(os.path.join(a.save_path, "train_loss_vec.npy"), np.asarray(losses))      # ctvae/main_ct_vae.py:413
        if a.save_path and self.rank == 0 and a.num_iter > 0:
            np.save(os.path.join(a.save_path, "training_time.npy"), (time.time() - t0) / 60)       # minutes, :421-422
        return losses, time.time() - t0

    def save(self, path, losses):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"enc": self.enc.state_dict(), "dec": self.dec.state_dict(), "opt": self.optimizer_state(),
                    "kl_anneal": self.kl_anneal, "pnm": self.pnm.detach().cpu(), "iter": self.iter, "losses": losses}, path)

    def latest_checkpoint(self):
        """Path of the newest ckpt-<iteration>.pt under --save_path/training_checkpoints."""
        folder = os.path.join(self.args.save_path or ".", "training_checkpoints")
        names = [n for n in (os.listdir(folder) if os.path.isdir(folder) else []) if n.startswith("ckpt-") and n.endswith(".pt")]
        if not names:
            raise FileNotFoundError(f"no checkpoint under {folder}")
        return os.path.join(folder, max(names, key=lambda n: int(n[5:-3])))

    def restore(self, path):
        ck = torch.load(path, map_location=self.dev)
        self.enc.load_state_dict(ck["enc"])
        self.dec.load_state_dict(ck["dec"])
        if getattr(self.args, "fused_update", False):
            # the checkpoint's entries are the parameters its run updated: the FusedUpdate is built over them (none yet: at the first step)
            full = self.opt.param_groups[0]["params"]
            if len(ck["opt"]["param_groups"]) != 1 or len(ck["opt"]["param_groups"][0]["params"]) != len(full):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            rows = sorted(ck["opt"]["state"])
            self.upd = None
            if rows:
                self.upd = FusedUpdate([full[i] for i in rows], lr=self.args.lr, eps=self.args.adam_epsilon, clip_norm=self.args.norm)
                self._load_fused_update(ck["opt"], self.upd.params)
        else:
            self.opt.load_state_dict(ck["opt"])
        self.kl_anneal, self.iter = ck["kl_anneal"], ck["iter"]      # (iter is also --fused_head's draw index)
        with torch.no_grad():
            self.pnm.copy_(ck["pnm"].to(self.dev))

    @torch.no_grad()
    def evaluate(self, n=None):
        """Mean decoder output on the first n examples vs. the phantoms (MSE), and the FBP input's MSE."""
        n = n or min(self.args.td, 16)
        skips = self.enc(self.input_encode[:n] / 300)
        if self.args.deterministic:
            lat = skips
        elif self.args.use_normal:
            lat = [s.chunk(2, dim=1)[0] for s in skips]                                   # the latents' means
        else:                                                                             # Beta(a, b): a / (a + b)
            ab = [(positive_range(s.chunk(2, dim=1)[0]), positive_range(s.chunk(2, dim=1)[1])) for s in skips]
            lat = [a_ / (a_ + b_) for a_, b_ in ab]
        alpha, beta = self.dec(lat)
        rec = positive_range(alpha)[:, 0]
        if not self.args.use_normal:
            rec = rec / (rec + positive_range(beta)[:, 0])
        if self.truth is None:                    # a dataset folder holds sinograms only
            return float("nan"), float("nan")
        return float(((rec - self.truth[:n]) ** 2).mean()), float(((self.input_encode[:n, 0] - self.truth[:n]) ** 2).mean())

    @torch.no_grad()
    def final_evaluation(self, save_path=None):
        """CT_VAE.final_evaluation (ctvae/main_ct_vae.py:427-460): the unshuffled dataset in batches of `-b`, ALL angles,
        no update; keeps every batch's loss and one sample of the output distribution per object, and writes
        loss_final.npy / reconstruction_final.npy ([n][X][Y][1]) -- the file bin/final_merit.py scores."""
        a = self.args
        # full batches of `-b` on every rank (the log-likelihood sums over the batch, so a sharded batch would change the
        # per-batch losses the reference reports); the evaluation runs once and only rank 0 writes
        nb = a.batch_size
        losses, recons = [], []
        for k in range(0, (a.td // nb) * nb, nb):
            sl = slice(k, k + nb)
            loss_vec, _, _, recon = find_loss_vae_unsup(self.proj_samples[sl], self.masks[sl], self.input_encode[sl], self.enc,
                                                        self.dec, self.pnm, self.sqrt_reg, self.kl_anneal, a.klm,
                                                        num_samples=a.ns, theta=self.theta_host, angles_i=None, pad=self.pad,
                                                        deterministic=a.deterministic, use_normal=a.use_normal,
                                                        model=getattr(a, "model", "rotate"), noise=getattr(a, "noise", "gaussian"))
            losses.append(loss_vec.mean() / 1e5)
            recons.append(recon.permute(0, 2, 3, 1))
        loss_final = torch.stack(losses).cpu().numpy()
        reconstruction_final = torch.cat(recons).cpu().numpy()
        if save_path is not None and self.rank == 0:
            os.makedirs(save_path, exist_ok=True)
            np.save(os.path.join(save_path, "loss_final.npy"), loss_final)
            np.save(os.path.join(save_path, "reconstruction_final.npy"), reconstruction_final)
        return loss_final, reconstruction_final

    def final_merit(self, save_path, ground_truth=None, seed=0):
        """bin/final_merit.py on what final_evaluation left under save_path (ct_pvae_amd/final_merit.py), when a ground truth is
        known: the synthetic set's phantoms, or `ground_truth` (a .npy path or an array).  The two baselines are reconstructed with
        gridrec, as the reference script and the command line do, whatever --algorithms feeds the encoder.  Needs --final_merit (the
        clean sinograms are kept for it).  Returns final_merit's result, or None (with a note) when there is no ground truth."""
        from .final_merit import final_merit
        if self.sinograms is None:
            raise ValueError("PVAETrainer.final_merit: the trainer was made without --final_merit, so the clean sinograms were not kept")
        truth = ground_truth if ground_truth is not None else self.truth
        if truth is None:
            print("--final_merit: no ground truth is known for this dataset (pass --ground_truth FILE); nothing scored")
            return None
        return final_merit(self.args.input_path, save_path, self.args.pnm, ground_truth=truth, algorithm="gridrec", seed=seed,
                           dataset=(self.sinograms, self.theta_np), device=self.dev)

    @torch.no_grad()
    def pixel_dist(self, example_num=0, num_repeats=10000, num_samples_1=100, save_path=None, bins=50, lo=0.005, width=0.01):
        """CT_VAE.pixel_dist (ctvae/main_ct_vae.py:648-731) without its figures: the per-pixel marginals of the network's posterior for
        one example.  The example's encoder input is repeated `-b` times (load_batch, :635-646); every repeat r draws `ns` latent
        samples per copy, decodes them and adds num_samples_1 draws of the output head per decoder output to a PixelMarginals
        (seed = --head_seed, draws r * num_samples_1 ..): num_repeats * ns * b * num_samples_1 samples per pixel, none of them stored.
        With --fused_latents the latents are normal_latents' keyed by (--head_seed, draw = r); without it they come from torch's
        global generator as in find_loss_vae_unsup.  Without --normal (with --fused_beta_head) the state is PixelMarginals(head="beta"):
        the samples are beta_head's, the latents beta_latents' keyed the same way with --fused_beta_latents and otherwise
        Beta(pr(loc), pr(log_scale)).sample((ns,)) from torch's generator, sample-major.  The encoder does not depend on r and runs
        once; the projector and the likelihood, which the reference computes and discards, are not called.  Only rank 0 runs it: it
        writes <save_path>/pixel_dist_<en>.npz, prints one line and returns the PixelMarginals (the other ranks return None)."""
        a = self.args
        head = _pixel_dist_head(a)
        example_num, num_repeats = int(example_num), int(num_repeats)
        if not 0 <= example_num < self.input_encode.shape[0]:
            raise ValueError(f"pixel_dist: example {example_num} is not one of the {self.input_encode.shape[0]} examples")
        if num_repeats < 1:
            raise ValueError(f"pixel_dist: num_repeats must be >= 1 (got {num_repeats})")
        if self.rank != 0:
            return None
        ns, B = int(a.ns), a.batch_size
        fused = bool(getattr(a, "fused_latents" if head == "truncated_normal" else "fused_beta_latents", False))
        skips = self.enc(self.input_encode[example_num:example_num + 1].repeat(B, 1, 1, 1) / 300)
        if fused:
            skips = [sk.contiguous() for sk in skips]
        elif head == "truncated_normal":
            q = [(loc.repeat(ns, 1, 1, 1), (positive_range(log_scale) + self.sqrt_reg).repeat(ns, 1, 1, 1))
                 for loc, log_scale in (sk.chunk(2, dim=1) for sk in skips)]
        else:
            q = [torch.distributions.Beta(positive_range(loc), positive_range(log_scale))
                 for loc, log_scale in (sk.chunk(2, dim=1) for sk in skips)]
        m = PixelMarginals((self.x_size, self.y_size), bins=bins, lo=lo, width=width, device=self.dev, head=head)
        for r in range(num_repeats):
            if fused and head == "truncated_normal":
                q_sample = [normal_latents(sk, ns=ns, seed=a.head_seed, draw=r, level=level, first_object=0, sqrt_reg=self.sqrt_reg)[0]
                            for level, sk in enumerate(skips)]
            elif fused:
                q_sample = [beta_latents(sk, ns=ns, seed=a.head_seed, draw=r, level=level, first_object=0, want_kl=False)[0]
                            for level, sk in enumerate(skips)]
            elif head == "truncated_normal":
                q_sample = [loc + scale * torch.randn_like(loc) for loc, scale in q]
            else:                                                       # sample-major, as in find_loss_vae_unsup
                q_sample = [d.sample((ns,)).reshape((ns * B,) + tuple(d.concentration1.shape[1:])) for d in q]
            alpha, beta = self.dec(q_sample)
            m.add(alpha.contiguous(), beta.contiguous(), draws=num_samples_1, seed=a.head_seed, draw0=r * num_samples_1)
        if save_path is not None:
            os.makedirs(save_path, exist_ok=True)
            m.save(os.path.join(save_path, f"pixel_dist_{example_num}.npz"))
        mean = m.mean()
        print(f"pixel_dist example {example_num}: {m.count} samples per pixel, per-pixel means {float(mean.min()):.6f} .. "
              f"{float(mean.max()):.6f}", flush=True)
        return m


def _dropout_prob(text):
    p = float(text)
    if not 0.0 <= p < 1.0 or (p > 0.0 and not 0.0 < float(np.float32(p)) < 1.0):
        raise argparse.ArgumentTypeError(f"--dp must satisfy 0 <= p < 1, in float32 too (got {text})")
    return p


def get_args(argv=None):
    """The reference's flags that reach the path (ctvae/main_ct_vae.py:30-116), same spellings and defaults."""
    p = argparse.ArgumentParser(description="P-VAE training with the MI355X projector")
    p.add_argument("--ae", type=float, dest="adam_epsilon", default=1e-7)
    p.add_argument("-b", type=int, dest="batch_size", default=4)
    p.add_argument("--ns", type=int, dest="ns", default=2)
    p.add_argument("--det", action="store_true", dest="deterministic")
    p.add_argument("-i", type=int, dest="num_iter", default=100)
    p.add_argument("--ik", type=int, dest="ik", default=4)
    p.add_argument("--il", type=int, dest="il", default=2)
    p.add_argument("--klaf", type=float, dest="klaf", default=1.0)
    p.add_argument("--klm", type=float, dest="klm", default=1.0)
    p.add_argument("--ks", type=int, dest="kernel_size", default=4)
    p.add_argument("--lr", type=float, dest="lr", default=1e-4)
    p.add_argument("--nb", type=int, dest="num_blocks", default=3)
    p.add_argument("--nfm", type=int, dest="nfm", default=20)
    p.add_argument("--nfmm", type=float, dest="nfmm", default=1.1)
    p.add_argument("--norm", type=float, dest="norm", default=100.0)
    p.add_argument("--normal", action="store_true", dest="use_normal",
                   help="Normal latents and a TruncatedNormal output distribution (every README recipe); without it the "
                        "reference's default Beta latents / Beta(0.5, 0.5) prior / Beta output (ctvae/main_ct_vae.py:69, :369-372)")
    p.add_argument("--nsa", type=int, dest="nsa", default=10)
    p.add_argument("--api", type=int, dest="api", default=5)
    p.add_argument("--pnm", type=float, dest="pnm", default=(2 ** 16 - 1) * 0.41)
    p.add_argument("--pnm_start", type=float, dest="pnm_start", default=None)
    p.add_argument("--train_pnm", action="store_true")
    p.add_argument("--model", choices=["rotate", "siddon"], default="rotate",
                   help="forward model of the likelihood term: the reference's rotate-and-sum, or the ray-driven projector the "
                        "datasets are made with (tomopy.project)")
    p.add_argument("--noise", choices=["gaussian", "poisson"], default="gaussian",
                   help="noise model of the likelihood term: the reference's Gaussian approximation Normal(loc, sqrt(loc / pnm)), or "
                        "the exact Poisson law the measurements are drawn from (not with --train_pnm)")
    p.add_argument("--fused_head", action="store_true",
                   help="sample the TruncatedNormal output and sum its log-density in one launch (csrc/head.hip), with Philox uniforms "
                        "keyed by (--head_seed, step index, object) instead of torch's global generator; needs --normal")
    p.add_argument("--fused_beta_head", action="store_true",
                   help="sample the default Beta output and sum its clamped log-density in one launch (csrc/beta_head.hip), with "
                        "Philox draws keyed by (--head_seed, step index, object) instead of torch's global generator and TensorFlow's "
                        "implicit reparameterisation gradient instead of torch's direct Beta derivative; not with --normal")
    p.add_argument("--fused_latents", action="store_true",
                   help="sample the Normal latents and sum their KL term in one launch per skip level (csrc/latent.hip), with Philox "
                        "draws keyed by (--head_seed, step index, level, sample, global object) instead of torch's global generator; "
                        "needs --normal, not with --det")
    p.add_argument("--fused_beta_latents", action="store_true",
                   help="sample the default Beta latents and sum their KL term against Beta(0.5, 0.5) in one launch per skip level "
                        "(csrc/beta_latent.hip), with Philox draws keyed by (--head_seed, step index, level, sample, global object) instead of "
                        "torch's global generator and TensorFlow's implicit reparameterisation gradient instead of torch's direct Beta "
                        "derivative; not with --normal, not with --det")
    p.add_argument("--fused_blocks", action="store_true",
                   help="the periodic pad in front of every ConvBlock's convolution and the maxout behind it as one launch each way "
                        "(csrc/convblock.hip) instead of chains of small torch launches; the same parameters, checkpoints and, with at most "
                        "two copies of a pixel per axis, the same values; independent of --normal and --det.  Measured at the c3 recipe "
                        "(profiles/convblock_timing.txt): alone NOT measurably faster (173.8 against 173.1 steps/s, the windows overlap); "
                        "with --fused_head --fused_latents 248.1 against 237.6 steps/s, the windows overlap too")
    p.add_argument("--fused_conv", action="store_true",
                   help="every padded (non-transposed) ConvBlock -- periodic pad, convolution, maxout -- as one forward launch and at most "
                        "four backward launches on the matrix cores with fp32 operands (csrc/conv.hip) instead of MIOpen's convolutions "
                        "between the pad and the maxout: every sum in one stated order, so these blocks give the same bits from run to run "
                        "without torch's deterministic switch; the same parameters and checkpoints; the transposed blocks stay on torch "
                        "(--reproducible still sets the switch for them) unless --fused_convt is given; combinable with every other flag.  Measured at the c3 recipe "
                        "(profiles/conv_timing.txt) on top of --fused_head --fused_latents --fused_blocks --fused_update: with "
                        "--reproducible 106.5 against 53.3 steps/s (the windows do not overlap); against the non-deterministic default "
                        "NOT faster, 106.5 against 245.0 steps/s")
    p.add_argument("--fused_convt", action="store_true",
                   help="every transposed (up-sampling) ConvBlock -- transposed convolution, maxout -- as one forward launch and at most "
                        "three backward launches on the matrix cores with fp32 operands (csrc/conv_transpose.hip) instead of MIOpen's "
                        "transposed convolution in front of the maxout: every sum in one stated order; the same parameters and "
                        "checkpoints; independent of --fused_conv and combinable with every other flag.  With --fused_conv no "
                        "convolution of the networks goes through MIOpen and two runs with equal seeds are bit-equal WITHOUT "
                        "--reproducible.  Measured at the c3 recipe (profiles/conv_transpose_timing.txt) on top of --fused_head "
                        "--fused_latents --fused_blocks --fused_update: --fused_conv --fused_convt 103.4 steps/s (103.3 .. 103.5), "
                        "--reproducible --fused_conv 106.9 (106.7 .. 106.9), neither flag 286.2 (285.4 .. 286.5); the windows do not "
                        "overlap: it is 3 %% SLOWER than --reproducible --fused_conv and NOT for runs that need no bit-equal step")
    p.add_argument("--fused_update", action="store_true",
                   help="the update stage -- NaN filter, per-tensor clip_by_norm (--norm), Adam (--lr, --ae) -- as two launches over the flat "
                        "gradient bucket (csrc/update.hip) instead of torch's chain and torch.optim.Adam: Keras's Adam, as the reference runs "
                        "it (epsilon outside the bias correction: with --ae 1e-7 it acts as 3.2e-6 in torch's terms at the first step), "
                        "tf.clip_by_norm's own form, and the norms' sums of squares in float64 in a stated order; the checkpoint's optimiser "
                        "entry keeps torch.optim.Adam's layout, so it restores with or without the flag; independent of every other flag")
    p.add_argument("--dp", type=_dropout_prob, dest="dropout_prob", default=0.0,
                   help="dropout probability of every ConvBlock's input (ctvae/main_ct_vae.py:41-42, ctvae/models.py:283-284), 0 <= p < 1; "
                        "0 (the default): no dropout, the networks and their launches as without the flag.  The masks are Philox-keyed by "
                        "(--head_seed, step index, block, object, element) (csrc/convblock.hip), not drawn from torch's global generator, "
                        "and drawn again in the backward instead of stored; with --fused_blocks they ride the pad's launches.  Training "
                        "steps only: the final evaluation, --pixel_dist and --final_merit run the networks without dropout")
    p.add_argument("--ufs", action="store_true", help="accepted and ignored: the reference parses it (use_first_skip) and never reads it")
    p.add_argument("--reproducible", action="store_true",
                   help="ask torch for deterministic convolution algorithms (torch.backends.cudnn.deterministic, process-wide): with "
                        "--fused_head two runs with equal seeds are then bit-equal; MIOpen's default weight gradients are not")
    p.add_argument("--head_seed", type=int, default=1234, help="seed of --fused_head's and --fused_beta_head's uniforms and of --fused_latents' and --fused_beta_latents' draws")
    p.add_argument("--random", action="store_true")
    p.add_argument("--save_path", default=None)
    p.add_argument("--restore", action="store_true", help="restore the latest checkpoint under --save_path before training / evaluating")
    p.add_argument("--ulc", action="store_true", dest="use_latest_ckpt", help="accepted: --restore always takes the latest checkpoint")
    p.add_argument("--input_path", default=None,
                   help="dataset folder written by scripts/images_to_sinograms.py (x_train_sinograms.npy, "
                        "dataset_parameters.npy); without it a seeded synthetic foam set of --td phantoms is made")
    p.add_argument("--real", action="store_true", dest="real_data", help="real data: no simulated noise (ctvae/main_ct_vae.py:105)")
    p.add_argument("--no_pad", action="store_true", help="sinograms have no zero-padding (ctvae/main_ct_vae.py:107)")
    p.add_argument("--toy_masks", action="store_true", help="the toy problem's two-angle masks (ctvae/main_ct_vae.py:109)")
    p.add_argument("--no_final_eval", action="store_true", help="skip the final evaluation (ctvae/main_ct_vae.py:113)")
    p.add_argument("--final_merit", action="store_true",
                   help="after the final evaluation, score reconstruction_final.npy the reference's way (bin/final_merit.py, "
                        "ct_pvae_amd/final_merit.py): <save_path>/final_ave_merit.npy, the 3 x 3 table of MSE / SSIM / PSNR, the two baselines "
                        "reconstructed with gridrec as in the reference (not with --algorithms); needs "
                        "--save_path and a ground truth: the synthetic set's own phantoms, or --ground_truth with --input_path")
    p.add_argument("--ground_truth", default=None, help="ground-truth images [n][X][Y] (.npy) of an --input_path dataset, for --final_merit")
    p.add_argument("--pixel_dist", action="store_true",
                   help="per-pixel marginals of the network's posterior for example --en (ctvae/main_ct_vae.py:103, CT_VAE.pixel_dist): "
                        "a histogram and two moments per pixel over --pixel_repeats decoder passes of 100 draws each, written to "
                        "<save_path>/pixel_dist_<en>.npz (csrc/marginals.hip, csrc/beta_marginals.hip; no sample is stored); needs --normal "
                        "(the TruncatedNormal head's marginals) or --fused_beta_head (the default Beta head's), not with --det")
    p.add_argument("--en", type=int, dest="example_num", default=0, help="the example --pixel_dist looks at")
    p.add_argument("--pixel_repeats", type=int, default=10000,
                   help="decoder passes of --pixel_dist, each over -b copies of the example and --ns latent samples (the reference's "
                        "hard-coded 10000)")
    p.add_argument("--se", type=int, dest="stride_encode", default=2)
    p.add_argument("--si", type=int, dest="si", default=100000)
    p.add_argument("--miopen_find", action="store_true",
                   help="search MIOpen's convolution algorithms once (torch.backends.cudnn.benchmark); not in the reference")
    p.add_argument("--td", type=int, dest="td", default=100)
    p.add_argument("--algorithms", nargs="+", default=["gridrec"],
                   help="initial reconstructions fed to the encoder, one channel each (ctvae/main_ct_vae.py:111-112, same "
                        "default); on the GPU: gridrec (csrc/gridrec.hip, tomopy's default parzen filter), sirt, fbp, "
                        "mlem, osem, pml_quad, pml_hybrid, ospml_quad, ospml_hybrid (ct_pvae_amd/recon.py), tv (flagged stand-in)")
    p.add_argument("--train", action="store_true")
    # synthetic-data knobs (the reference reads these from its dataset folder)
    p.add_argument("--n_pixel", type=int, default=128)
    p.add_argument("--num_angles", type=int, default=180)
    args = p.parse_args(argv)
    if args.fused_head and not args.use_normal:
        raise ValueError("--fused_head is the TruncatedNormal output head: it needs --normal")
    if args.fused_beta_head and args.use_normal:
        raise ValueError(_FUSED_BETA_HEAD_NEEDS)
    if args.fused_latents and (not args.use_normal or args.deterministic):
        raise ValueError(_FUSED_LATENTS_NEEDS)
    if args.fused_beta_latents and (args.use_normal or args.deterministic):
        raise ValueError(_FUSED_BETA_LATENTS_NEEDS)
    if args.pixel_dist:
        _pixel_dist_head(args)
    if args.final_merit and (not args.save_path or args.no_final_eval):
        raise ValueError("--final_merit scores the final evaluation's reconstruction_final.npy: it needs --save_path and cannot be "
                         "combined with --no_final_eval")
    return args


def main(argv=None):
    args = get_args(argv)
    world, rank, local = sharding.init_from_env()
    dev = torch.device("cuda", local)
    tr = PVAETrainer(args, dev)
    if args.restore:                                   # ctvae/main_ct_vae.py:363-368 (--ulc: the latest checkpoint)
        tr.restore(tr.latest_checkpoint())
    losses, secs = tr.train() if args.train else ([], 0.0)
    if args.pixel_dist:                                # ctvae/main_ct_vae.py: the trained (or restored) network's pixel marginals
        tr.pixel_dist(example_num=args.example_num, num_repeats=args.pixel_repeats, save_path=args.save_path)
    if not args.no_final_eval:
        loss_final, _ = tr.final_evaluation(args.save_path)
        if rank == 0:
            print(f"Average loss final : {float(loss_final.mean()):.6f}")
        if args.final_merit and rank == 0:
            tr.final_merit(args.save_path, ground_truth=args.ground_truth)
    if rank == 0:
        mse, mse_fbp = tr.evaluate()
        if losses:
            print(f"{len(losses)} iterations in {secs:.1f} s ({len(losses) / secs:.2f} it/s); loss {losses[0]:.5f} -> {losses[-1]:.5f}")
        print(f"MSE reconstruction {mse:.5f} (FBP input {mse_fbp:.5f})")
    return losses


if __name__ == "__main__":
    main()
