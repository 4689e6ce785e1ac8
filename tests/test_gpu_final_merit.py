"""The scoring stage on the device (ct_pvae_amd/final_merit.py, bin/final_merit.py): 6 foams of 64 x 64 at 60 angles, the dataset
folder, masks and samples made by the package's own tools, reconstruction_final.npy written directly (clamped truth plus noise)."""
import os

import numpy as np
import pytest
import torch

from ct_pvae_amd import create_all_masks, dataset_io, phantoms
from ct_pvae_amd import final_merit as fm
from ct_pvae_amd import trainer as tr

pytestmark = pytest.mark.gpu

N, SIZE, ANGLES, NSA, PNM = 6, 64, 60, 10, 1e4
RTOL = 1e-9


@pytest.fixture(scope="module")
def truth():
    return phantoms.foam_batch(N, SIZE, seed=3, supersample=2)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, truth):
    """(root, dataset folder name relative to root): root/dataset_foam in the reference's layout and root/foam_training.npy."""
    root = tmp_path_factory.mktemp("final_merit")
    dataset_io.images_to_sinograms(truth, str(root / "dataset_foam"), theta=phantoms.dense_theta(ANGLES))
    np.save(root / "foam_training.npy", np.concatenate([truth, truth[:2]]))        # longer than the run: the first n rows count
    return root, "dataset_foam"


def make_run(root, name, random, truth):
    """A run folder: all_masks.npy, all_proj_samples.npy (create_all_masks) and reconstruction_final.npy [n][X][Y][1]."""
    run = str(root / name)
    sino, _, _ = dataset_io.get_sinograms(str(root / "dataset_foam"))
    create_all_masks(torch.from_numpy(sino).cuda(), ANGLES, save_path=run, poisson_noise_multiplier=PNM, num_sparse_angles=NSA,
                     random=random, train=True, truncate_dataset=N)
    noise = np.random.default_rng(11).standard_normal(truth.shape).astype(np.float32)
    np.save(os.path.join(run, "reconstruction_final.npy"), np.clip(truth + 0.03 * noise, 0, 1).astype(np.float32)[..., None])
    return run


@pytest.fixture(scope="module")
def runs(dataset, truth):
    root, _ = dataset
    return {"uniform": make_run(root, "run_uniform", False, truth), "random": make_run(root, "run_random", True, truth)}


@pytest.fixture
def counted(monkeypatch):
    """final_merit's recon calls, counted through a wrapper: the number of angles of each call."""
    calls = []
    real = fm.recon

    def wrapper(tomo, theta, *args, **kwargs):
        calls.append((len(theta), tomo.shape[0] if kwargs.get("sinogram_order") else tomo.shape[1]))
        return real(tomo, theta, *args, **kwargs)
    monkeypatch.setattr(fm, "recon", wrapper)
    return calls


@pytest.mark.parametrize("masks", ("uniform", "random"))
def test_table_merits_and_call_count(dataset, runs, truth, counted, masks):
    root, ds = dataset
    run = runs[masks]
    merits, recon0, recon1 = fm.final_merit(str(root / ds), run, PNM, ground_truth=str(root / "foam_training.npy"), verbose=False)
    table = np.load(os.path.join(run, "final_ave_merit.npy"))
    assert table.shape == (3, 3) and table.dtype == np.float64 and np.isfinite(table).all()
    assert merits.shape == (3, N, 3) and merits.dtype == np.float64
    np.testing.assert_array_equal(table, merits.mean(axis=1))
    final = np.load(os.path.join(run, "reconstruction_final.npy"))[..., 0]
    for row, stack in enumerate((recon0, recon1, final)):
        assert stack.shape == (N, SIZE, SIZE) and stack.min() >= 0 and stack.max() <= 1
        for k in range(N):
            np.testing.assert_allclose(merits[row, k], dataset_io.compare(truth[k], stack[k], verbose=False), rtol=RTOL)
    assert table[2, 0] < table[0, 0] < table[1, 0]              # truth + 3 % noise beats 60 noisy angles beats 10 noisy angles (MSE)
    used = np.load(os.path.join(run, "all_masks.npy")) > 0
    sets = len({row.tobytes() for row in used})
    assert counted[0] == (ANGLES, N)                             # the full sinograms: one call for all n slices
    partial = counted[1:]
    assert all(a == NSA for a, _ in partial) and sum(g for _, g in partial) == N
    assert len(partial) == sets and (sets == 1 if masks == "uniform" else sets > 1)


def test_seed_keys_the_full_sinogram_row_only(dataset, runs):
    root, ds = dataset
    run, gt = runs["uniform"], str(root / "foam_training.npy")
    path = os.path.join(run, "final_ave_merit.npy")
    fm.final_merit(str(root / ds), run, PNM, ground_truth=gt, seed=0, verbose=False)
    first = np.load(path)
    fm.final_merit(str(root / ds), run, PNM, ground_truth=gt, seed=0, verbose=False)
    np.testing.assert_array_equal(np.load(path), first)
    fm.final_merit(str(root / ds), run, PNM, ground_truth=gt, seed=1, verbose=False)
    other = np.load(path)
    np.testing.assert_array_equal(other[1:], first[1:])
    assert not np.any(other[0] == first[0])


def test_cli_writes_the_functions_file(dataset, runs, monkeypatch, capsys):
    """The command line, with the reference's ground-truth rule: run from the folder that holds dataset_foam/ and foam_training.npy."""
    root, ds = dataset
    run = runs["random"]
    path = os.path.join(run, "final_ave_merit.npy")
    fm.final_merit(str(root / ds), run, PNM, ground_truth=str(root / "foam_training.npy"), seed=4, verbose=False)
    want = np.load(path)
    os.remove(path)
    monkeypatch.chdir(root)
    fm.main(["--input_path", ds, "--save_path", run, "--pnm", str(PNM), "--seed", "4"])
    np.testing.assert_array_equal(np.load(path), want)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "MSE, SSIM, PSNR" and out[1::2][:3] == list(fm.ROWS)
    os.remove(path)
    fm.main(["--input_path", ds, "--save_path", run, "--pnm", str(PNM), "--seed", "4", "--ground_truth", str(root / "foam_training.npy"),
             "--algorithm", "gridrec"])
    np.testing.assert_array_equal(np.load(path), want)


TRAIN = "--nsa 10 --td 4 -b 2 --ns 1 --api 10 --pnm 1e4 --normal --n_pixel 64 --num_angles 60 --train"


def test_trainer_flag_leaves_the_file(tmp_path):
    out = str(tmp_path / "run")
    tr.main(f"{TRAIN} -i 3 --save_path {out} --final_merit".split())
    table = np.load(os.path.join(out, "final_ave_merit.npy"))
    assert table.shape == (3, 3) and np.isfinite(table).all()
    final = np.load(os.path.join(out, "reconstruction_final.npy"))[..., 0]
    truth = phantoms.foam_batch(4, 64, seed=0, supersample=2)
    want = np.mean([dataset_io.compare(truth[k], final[k], verbose=False) for k in range(4)], axis=0)
    np.testing.assert_allclose(table[2], want, rtol=RTOL)


def test_trainer_without_the_flag_leaves_no_file(tmp_path):
    out = str(tmp_path / "run")
    tr.main(f"{TRAIN} -i 1 --save_path {out}".split())
    assert os.path.exists(os.path.join(out, "reconstruction_final.npy")) and not os.path.exists(os.path.join(out, "final_ave_merit.npy"))
