"""The bits of the four fused sampling operators (truncated_normal_head, beta_head, normal_latents, beta_latents; forward and backward)
and of PixelMarginals.add for both heads, at the smallest shapes that reach every path of the code the operators share (csrc/quad_io.h):
a ragged last quad, objects that start misaligned, a thread with a second quad, two Philox blocks per quad, every combination of
cotangents, the test operands.  For every output array it prints the shape and the sha256 of the bytes, and the LP / KL sums in hex.

    python tools/sampling_bits.py [--out FILE]

Run it on two builds in one visit and compare the outputs: a change that only moves code gives the same text.  The bits depend on the
device math library compiled in, so the text is a record of one comparison (profiles/sampling_refactor_bits.txt), not a golden."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402

SEED, DRAW = 20240607, 7
LINES = []


def emit(line):
    LINES.append(line)
    print(line)


def digest(name, t):
    a = t.detach().cpu().contiguous().numpy()
    emit(f"{name:58s} {str(tuple(a.shape)):20s} {hashlib.sha256(a.tobytes()).hexdigest()}")


def sums(name, t):
    emit(f"{name:58s} " + " ".join(float(v).hex() for v in t.detach().cpu()))


def uniform(gen, shape, lo=-3.0, hi=3.0):
    """[lo, hi) from the CPU generator: the same operands on every build; both branches of positive_range occur."""
    return (torch.rand(shape, generator=gen) * (hi - lo) + lo).cuda()


def combos(tag, outs, ins, cots, names):
    """The gradients for the first output's cotangent alone, the second's alone and both."""
    for which in ((0,), (1,), (0, 1)):
        grads = torch.autograd.grad([outs[i] for i in which], ins, [cots[i] for i in which], retain_graph=True)
        for n, g in zip(names, grads):
            digest(f"{tag} cotangents {which} {n}", g)


def heads(gen):
    for shape, fo in (((3, 1, 11, 373), 5), ((2, 1, 8, 8), 0)):
        n, _, X, Y = shape
        alpha, beta = uniform(gen, shape).requires_grad_(True), uniform(gen, shape).requires_grad_(True)
        gx, glp = torch.randn((n, X, Y, 1), generator=gen).cuda(), torch.randn((n,), generator=gen).cuda()
        u = torch.rand(shape, generator=gen).clamp_(1e-6, 1 - 1e-6).cuda()
        calls = (("tn_head", lambda: cp.truncated_normal_head(alpha, beta, seed=SEED, draw=DRAW, first_object=fo)),
                 ("tn_head _u", lambda: cp.truncated_normal_head(alpha, beta, seed=SEED, draw=DRAW, first_object=fo, _u=u)),
                 ("beta_head", lambda: cp.beta_head(alpha, beta, seed=SEED, draw=DRAW, first_object=fo)))
        for name, call in calls:
            tag = f"{name} {list(shape)} fo={fo}"
            x, lp = call()
            digest(f"{tag} x", x)
            sums(f"{tag} LP", lp)
            combos(tag, (x, lp), (alpha, beta), (gx, glp), ("g_alpha", "g_beta"))
        if X * Y == 4103:
            for head in ("truncated_normal", "beta"):
                m = cp.PixelMarginals((X, Y), bins=50, head=head).add(alpha.detach(), beta.detach(), draws=30, seed=SEED, draw0=DRAW,
                                                                      first_object=fo)
                for k in ("hist", "s1", "s2"):
                    digest(f"marginals {head} draws=30 bins=50 {k}", getattr(m, k))


def latents(gen):
    ns, level = 3, 2
    for shape, fo in (((2, 22, 373, 1), 5), ((2, 2, 4, 4), 0)):
        B, C2, H, W = shape
        skip = uniform(gen, shape).requires_grad_(True)
        gz, gkl = torch.randn((ns * B, C2 // 2, H, W), generator=gen).cuda(), torch.randn((B,), generator=gen).cuda()
        eps = torch.randn((ns * B, C2 // 2, H, W), generator=gen).cuda()
        key = dict(ns=ns, seed=SEED, draw=DRAW, level=level, first_object=fo)
        extras = {}
        calls = (("normal_latents", lambda: cp.normal_latents(skip, **key)),
                 ("normal_latents _eps", lambda: cp.normal_latents(skip, _eps=eps, **key)),
                 ("beta_latents", lambda: cp.beta_latents(skip, **key)),
                 ("beta_latents _extras", lambda: cp.beta_latents(skip, _extras=extras, **key)))
        for name, call in calls:
            tag = f"{name} {list(shape)} ns={ns} level={level} fo={fo}"
            z, kl = call()
            digest(f"{tag} z", z)
            sums(f"{tag} KL", kl)
            combos(tag, (z, kl), (skip,), (gz, gkl), ("g_skip",))
        for k in ("kl_elem", "aux"):
            digest(f"beta_latents _extras {list(shape)} {k}", extras[k])
        tag = f"beta_latents want_kl=False {list(shape)} ns={ns} level={level} fo={fo}"
        z, kl = cp.beta_latents(skip, want_kl=False, **key)
        assert kl is None
        digest(f"{tag} z", z)
        digest(f"{tag} cotangents (0,) g_skip", torch.autograd.grad(z, skip, gz)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sampling_bits.py runs the kernels: no GPU found")
    gen = torch.Generator().manual_seed(SEED)
    heads(gen)
    latents(gen)
    torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
