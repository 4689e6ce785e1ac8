"""The scoring stage of CT_PVAE on the device: bin/final_merit.py, step by step.

    python -m ct_pvae_amd.final_merit --input_path dataset_foam --save_path runs/foam --pnm 26869.35 [--ground_truth FILE]
                                      [--algorithm gridrec] [--seed 0]

reads <save_path>/reconstruction_final.npy (what the trainer's final evaluation leaves), all_proj_samples.npy and all_masks.npy, the
sinograms under --input_path and the ground truth, and writes <save_path>/final_ave_merit.npy: [3][3] float64, rows = the reconstruction
from the noisy full sinogram, from the noisy partial sinogram, and the P-VAE's; columns = MSE, SSIM, PSNR averaged over the examples.

Where the reference loops on the host, this runs on the kernels: the Poisson draw (poisson_measure), the reconstructions (recon; the
examples that were measured at the same angles share ONE call) and the 3 n comparisons (ONE image_merits call).  The Poisson counts
come from the library's counter-based sampler keyed by --seed, not from TensorFlow's generator: the distribution is the reference's."""
import argparse
import os

import numpy as np
import torch

from . import dataset_io
from .create_masks import poisson_measure
from .merit import image_merits
from .recon import recon

__all__ = ["final_merit", "default_ground_truth_path", "group_by_angles", "clamp01", "main"]

ROWS = ("noisy, full sinogram", "noisy, partial sinogram", "P-VAE from noisy, partial sinogram")


def default_ground_truth_path(input_path):
    """bin/final_merit.py:37,48: the dataset folder's name without its first 8 characters ('dataset_'), plus '_training.npy'."""
    return input_path[8:] + "_training.npy"


def group_by_angles(all_masks):
    """[(used angle indices, example indices), ...]: the examples whose set of used angles (mask > 0) is identical, in the order of
    each set's first example; the examples of a group ascending.  Every example is in exactly one group."""
    used = np.asarray(all_masks) > 0
    groups = {}
    for k, row in enumerate(used):
        groups.setdefault(row.tobytes(), []).append(k)
    return [(np.flatnonzero(used[ks[0]]), np.asarray(ks, np.int64)) for ks in groups.values()]


def clamp01(x):
    """bin/final_merit.py:62-63, :88-89: np.maximum(np.minimum(x, 1), 0), for arrays and tensors (a NaN stays)."""
    if isinstance(x, torch.Tensor):
        return torch.clamp(x, 0.0, 1.0)
    return np.maximum(np.minimum(x, 1), 0)


def _recon_cropped(sino, theta, algorithm, x_size, y_size):
    """[g][angles][P] on the device -> [g][x_size][y_size], clamped."""
    return clamp01(dataset_io.crop(recon(sino, theta, center=None, sinogram_order=True, algorithm=algorithm), x_size, y_size))


def final_merit(input_path, save_path, poisson_noise_multiplier, ground_truth=None, algorithm="gridrec", seed=0, dataset=None,
                device=None, verbose=True):
    """bin/final_merit.py.  ground_truth: None (the reference's rule, default_ground_truth_path(input_path)), a .npy path or an array
    [>= n][X][Y]; dataset: (x_train_sinograms, theta) instead of the files under input_path.  Returns (merits, recon0, recon1): the
    per-example merits [3][n][3] float64 (rows as in the file, then example, then MSE / SSIM / PSNR) and the two reconstruction stacks
    [n][X][Y] float32 that were scored, as numpy arrays; writes <save_path>/final_ave_merit.npy = merits.mean(axis=1)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    reconstruction_final = np.squeeze(np.load(os.path.join(save_path, "reconstruction_final.npy")), axis=-1)
    n, x_size, y_size = reconstruction_final.shape
    if ground_truth is None:
        ground_truth = default_ground_truth_path(input_path)
    truth = np.load(ground_truth) if isinstance(ground_truth, (str, os.PathLike)) else \
        (ground_truth.detach().cpu().numpy() if isinstance(ground_truth, torch.Tensor) else np.asarray(ground_truth))
    truth = truth[0:n]
    if truth.shape != reconstruction_final.shape:
        raise ValueError(f"final_merit: the ground truth's first {n} rows are {truth.shape}, reconstruction_final is "
                         f"{reconstruction_final.shape}")
    if dataset is None:
        x_train_sinograms, theta, _ = dataset_io.get_sinograms(input_path)
    else:
        x_train_sinograms, theta = dataset
        if isinstance(x_train_sinograms, torch.Tensor):
            x_train_sinograms = x_train_sinograms.detach()
    theta = np.asarray(theta.detach().cpu().numpy() if isinstance(theta, torch.Tensor) else theta)
    sino = torch.as_tensor(x_train_sinograms[0:n]).to(device=dev, dtype=torch.float32)
    if sino.shape[0] != n or sino.shape[1] != len(theta):
        raise ValueError(f"final_merit: need {n} sinograms of {len(theta)} angles (got {tuple(sino.shape)})")

    with torch.cuda.device(dev):
        # reconstruction from a noisy version of the full sinogram (:55-63): Poisson(sino * pnm) / pnm is the draw under a mask of ones
        noisy = poisson_measure(sino, torch.ones(sino.shape[:2], dtype=torch.float32, device=dev), poisson_noise_multiplier, seed)
        recon0 = _recon_cropped(noisy, theta, algorithm, x_size, y_size)
        # reconstruction from the noisy, partial sinogram (:68-89), one call per distinct set of used angles
        all_masks = np.asarray(np.load(os.path.join(save_path, "all_masks.npy"))[0:n], np.float32)
        samples = torch.from_numpy(np.asarray(np.load(os.path.join(save_path, "all_proj_samples.npy"))[0:n], np.float32)).to(dev)
        if all_masks.shape != (n, len(theta)) or tuple(samples.shape) != tuple(sino.shape):
            raise ValueError(f"final_merit: all_masks {all_masks.shape} / all_proj_samples {tuple(samples.shape)} do not match "
                             f"{n} sinograms {tuple(sino.shape[1:])}")
        masks = torch.from_numpy(all_masks).to(dev)
        recon1 = torch.empty((n, x_size, y_size), dtype=torch.float32, device=dev)
        for used, examples in group_by_angles(all_masks):
            if used.size == 0:
                raise ValueError(f"final_merit: examples {examples.tolist()} have no used angle in all_masks.npy")
            ex, us = torch.from_numpy(examples).to(dev), torch.from_numpy(used).to(dev)
            partial = samples[ex][:, us] / masks[ex][:, us][..., None]
            recon1[ex] = _recon_cropped(partial.contiguous(), theta[used], algorithm, x_size, y_size)
        # the merit of all three against the ground truth (:97-104): 3 n pairs, one call.  float32 pixels are widened exactly on the
        # device; anything else is scored from float64, as compare does
        dtype = torch.float32 if truth.dtype == np.float32 and reconstruction_final.dtype == np.float32 else torch.float64
        t = torch.from_numpy(np.ascontiguousarray(truth)).to(device=dev, dtype=dtype)
        final = torch.from_numpy(np.ascontiguousarray(reconstruction_final)).to(device=dev, dtype=dtype)
        merits = image_merits(torch.cat([t, t, t]), torch.cat([recon0.to(dtype), recon1.to(dtype), final])).view(3, n, 3).cpu().numpy()
    final_ave_merit = np.array([np.mean(m, axis=0) for m in merits])
    if verbose:
        print("MSE, SSIM, PSNR")
        for label, row in zip(ROWS, final_ave_merit):
            print(label)
            print(row)
    np.save(os.path.join(save_path, "final_ave_merit.npy"), final_ave_merit)
    return merits, recon0.cpu().numpy(), recon1.cpu().numpy()


def main(argv=None):
    p = argparse.ArgumentParser(description="Score reconstruction_final.npy the reference's way (bin/final_merit.py)")
    p.add_argument("--input_path", required=True, help="path to the folder containing the training data")
    p.add_argument("--save_path", required=True, help="the training run's folder; final_ave_merit.npy is written there")
    p.add_argument("--pnm", type=float, required=True, dest="poisson_noise_multiplier",
                   help="poisson noise multiplier, higher value means higher SNR")
    p.add_argument("--ground_truth", default=None, help="ground-truth images [n][X][Y] (.npy); default: the reference's rule, "
                                                        "<input_path without its first 8 characters>_training.npy")
    p.add_argument("--algorithm", default="gridrec", help="reconstruction algorithm of the two baselines (recon's names)")
    p.add_argument("--seed", type=int, default=0, help="key of the Poisson draw on the full sinogram")
    a = p.parse_args(argv)
    final_merit(a.input_path, a.save_path, a.poisson_noise_multiplier, ground_truth=a.ground_truth, algorithm=a.algorithm, seed=a.seed)


if __name__ == "__main__":
    main()
