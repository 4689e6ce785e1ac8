"""The per-pixel marginals on the device (ct_pvae_amd/marginals.py, csrc/marginals.hip): every sample IS the output head's x, so the
histogram equals bin_samples of the stacked head samples exactly, the float64 sums are bit-equal to the twin's restatement of the
stated order and inside the any-order bound of math.fsum; accumulation, splits, reproducibility, errors; the trainer's --pixel_dist.

Shapes (n, X, Y): one quad; a ragged row with unaligned objects (offsets 7 and 14: Philox blocks straddled); 3 x 3; and (2, 5, 15):
75 pixels, 11 more than the 64 one workgroup covers -- a second tile with two whole quads and a 3-pixel tail, and object 1 at the
unaligned offset 75.  The draws are cut into slices of 25: K = 25 and 26 sit either side of that cut."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import PixelMarginals, _lib, bin_samples, truncated_normal_head
from ct_pvae_amd import trainer as tr
from tests import np_twin_head as th
from tests import np_twin_marginals as tm

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
SHAPES = {"1x2x2": (1, 2, 2), "3x1x7": (3, 1, 7), "3x3x3": (3, 3, 3), "2x5x15": (2, 5, 15)}
GRID = dict(lo=0.05, width=0.1, bins=20)         # [0.05, 2.05): the operands below put samples under, inside and over it
_ops, _heads = {}, {}


def _dev():
    return torch.device("cuda", 0)


def operands(shape):
    """(alpha, beta) [n][1][X][Y] on the device: pixel p takes np_twin_head's range "trainer", "trunc" or "wide" by p % 3, so every
    shape holds all three (loc far above 0, loc next to 0 with a wide scale -- the x = 0 floor's side --, and both tails)."""
    if shape not in _ops:
        n, X, Y = SHAPES[shape]
        pix = X * Y
        kinds = [th.operands(kind, n, pix, 11 + i) for i, kind in enumerate(("trainer", "trunc", "wide"))]
        pick = np.arange(pix) % 3
        al = np.choose(pick[None, :], [k[0] for k in kinds]).astype(np.float32)
        be = np.choose(pick[None, :], [k[1] for k in kinds]).astype(np.float32)
        _ops[shape] = tuple(torch.from_numpy(v).to(_dev()).reshape(n, 1, X, Y).contiguous() for v in (al, be))
    return _ops[shape]


def head_samples(shape, K, first_object, draw0):
    """float32 numpy [K][n][pix]: the output head's own x for draw = draw0 + k (computed once per key, left unchanged)."""
    key = (shape, K, first_object, draw0)
    if key not in _heads:
        al, be = operands(shape)
        n = al.shape[0]
        xs = [truncated_normal_head(al, be, seed=SEED, draw=draw0 + k, first_object=first_object)[0].reshape(n, -1) for k in range(K)]
        _heads[key] = torch.stack(xs).cpu().numpy()
        _heads[key].setflags(write=False)
    return _heads[key]


def new_state(shape, **grid):
    _, X, Y = SHAPES[shape]
    return PixelMarginals((X, Y), device=_dev(), **(grid or GRID))


def check_moments(m, samples):
    """s1, s2 within (N - 1) 2^-53 relative of math.fsum over the samples and their exact squares, N samples per pixel."""
    flat = samples.reshape(-1, samples.shape[-1])
    N = flat.shape[0]
    f1, f2 = tm.fsum_sums(flat)
    s1, s2 = m.s1.cpu().numpy(), m.s2.cpu().numpy()
    r1 = np.max(np.abs(s1 - f1) / np.where(f1 > 0, f1, 1.0))
    r2 = np.max(np.abs(s2 - f2) / np.where(f2 > 0, f2, 1.0))
    print(f"N = {N}: worst relative distance from fsum s1 {r1:.3e}, s2 {r2:.3e}, bound {tm.fsum_bound(N):.3e}")
    assert np.all(np.abs(s1 - f1) <= tm.fsum_bound(N) * f1) and np.all(np.abs(s2 - f2) <= tm.fsum_bound(N) * f2)


@pytest.mark.parametrize("late", [False, True], ids=["draw0=0", "draw0=2^32-K"])
@pytest.mark.parametrize("first_object", [0, 5])
@pytest.mark.parametrize("K", [1, 3, 25, 26, 100])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_identity_with_the_head(shape, K, first_object, late):
    n, X, Y = SHAPES[shape]
    draw0 = 2 ** 32 - K if late else 0
    al, be = operands(shape)
    want = head_samples(shape, K, first_object, draw0)
    m = new_state(shape).add(al, be, draws=K, seed=SEED, draw0=draw0, first_object=first_object)
    assert m.count == n * K
    hist = m.hist.cpu().numpy()
    np.testing.assert_array_equal(hist, bin_samples(want, **GRID))
    np.testing.assert_array_equal(hist.sum(axis=1), np.full(X * Y, m.count))
    check_moments(m, want)
    t1, t2 = tm.ordered_sums(want)                      # the stated order, restated: bit-equal
    assert np.array_equal(m.s1.cpu().numpy().view(np.uint64), t1.view(np.uint64))
    assert np.array_equal(m.s2.cpu().numpy().view(np.uint64), t2.view(np.uint64))
    mean, std = m.mean().cpu().numpy(), m.std().cpu().numpy()
    flat = want.reshape(-1, X * Y).astype(np.float64)
    np.testing.assert_allclose(mean.ravel(), flat.mean(axis=0), rtol=1e-13)
    if m.count >= 2:
        np.testing.assert_allclose(std.ravel(), flat.std(axis=0, ddof=1), rtol=1e-6, atol=1e-9)
    else:
        assert np.isnan(std).all()


def test_the_grid_exercises_all_three_column_kinds():
    """On the head's own samples: column 0, column bins + 1 and at least two inner columns are non-empty -- then the device agrees."""
    want = head_samples("2x5x15", 100, 0, 0)
    h = bin_samples(want, **GRID)
    assert h[:, 0].sum() > 0 and h[:, -1].sum() > 0 and int((h[:, 1:-1].sum(axis=0) > 0).sum()) >= 2
    m = new_state("2x5x15").add(*operands("2x5x15"), draws=100, seed=SEED)
    np.testing.assert_array_equal(m.hist.cpu().numpy(), h)


@pytest.mark.parametrize("grid", [dict(lo=0.5, width=1.0, bins=1), dict(lo=0.01, width=0.0125, bins=254),
                                  dict(lo=0.005, width=0.01, bins=50)], ids=["bins=1", "bins=254", "reference"])
def test_other_bin_counts(grid):
    want = head_samples("2x5x15", 26, 5, 0)
    h = bin_samples(want, **grid)
    assert h[:, 0].sum() > 0 and h[:, -1].sum() > 0 and h[:, 1:-1].sum() > 0
    m = new_state("2x5x15", **grid).add(*operands("2x5x15"), draws=26, seed=SEED, first_object=5)
    assert m.hist.shape == (75, grid["bins"] + 2)
    np.testing.assert_array_equal(m.hist.cpu().numpy(), h)
    np.testing.assert_array_equal(m.hist.sum(dim=1).cpu().numpy(), np.full(75, m.count))


def test_draws_accumulate_over_calls():
    """add(K1, draw0 = 0) then add(K2, draw0 = K1) gives the hist of one add(K1 + K2); row sums equal count after every call; the
    moments stay inside the any-order bound."""
    shape, K1, K2 = "3x1x7", 30, 45
    al, be = operands(shape)
    want = head_samples(shape, K1 + K2, 0, 0)
    m = new_state(shape)
    m.add(al, be, draws=K1, seed=SEED, draw0=0)
    assert m.count == 3 * K1 and torch.equal(m.hist.sum(dim=1), torch.full((7,), m.count, device=_dev()))
    np.testing.assert_array_equal(m.hist.cpu().numpy(), bin_samples(want[:K1], **GRID))
    m.add(al, be, draws=K2, seed=SEED, draw0=K1)
    assert m.count == 3 * (K1 + K2) and torch.equal(m.hist.sum(dim=1), torch.full((7,), m.count, device=_dev()))
    one = new_state(shape).add(al, be, draws=K1 + K2, seed=SEED)
    assert torch.equal(m.hist, one.hist)
    np.testing.assert_array_equal(m.hist.cpu().numpy(), bin_samples(want, **GRID))
    check_moments(m, want)
    check_moments(one, want)
    # the state's sum is s + T per call, T in the stated order
    (a1, a2), (b1, b2) = tm.ordered_sums(want[:K1]), tm.ordered_sums(want[K1:])
    assert np.array_equal(m.s1.cpu().numpy(), (0.0 + a1) + b1) and np.array_equal(m.s2.cpu().numpy(), (0.0 + a2) + b2)


def test_objects_split_over_calls():
    """Objects [0:2] with first_object = 0, then [2:3] with first_object = 2, give the hist of the whole batch."""
    shape, K = "3x3x3", 40
    al, be = operands(shape)
    want = head_samples(shape, K, 0, 0)
    m = new_state(shape)
    m.add(al[0:2].contiguous(), be[0:2].contiguous(), draws=K, seed=SEED, first_object=0)
    assert torch.equal(m.hist.sum(dim=1), torch.full((9,), 2 * K, device=_dev()))
    m.add(al[2:3].contiguous(), be[2:3].contiguous(), draws=K, seed=SEED, first_object=2)
    whole = new_state(shape).add(al, be, draws=K, seed=SEED)
    assert m.count == whole.count == 3 * K and torch.equal(m.hist, whole.hist)
    np.testing.assert_array_equal(whole.hist.cpu().numpy(), bin_samples(want, **GRID))
    check_moments(m, want)
    check_moments(whole, want)


def test_many_units_per_lane():
    """More units than 64 groups of 16 lanes hold at once: lanes walk several units (n * ceil(K / 25) = 1040 > 1024)."""
    n, X, Y, K = 260, 1, 5, 76
    a, b = th.operands("wide", n, X * Y, 3)
    al, be = (torch.from_numpy(v).to(_dev()).reshape(n, 1, X, Y) for v in (a, b))
    want = torch.stack([truncated_normal_head(al, be, seed=SEED, draw=k, first_object=1)[0].reshape(n, -1) for k in range(K)]).cpu().numpy()
    m = PixelMarginals((X, Y), device=_dev(), **GRID).add(al, be, draws=K, seed=SEED, first_object=1)
    np.testing.assert_array_equal(m.hist.cpu().numpy(), bin_samples(want, **GRID))
    check_moments(m, want)
    t1, t2 = tm.ordered_sums(want)
    assert np.array_equal(m.s1.cpu().numpy(), t1) and np.array_equal(m.s2.cpu().numpy(), t2)


def test_the_same_calls_give_the_same_bits():
    shape = "2x5x15"
    al, be = operands(shape)
    runs = []
    for _ in range(2):
        m = new_state(shape)
        m.add(al, be, draws=100, seed=SEED, first_object=5)
        m.add(al, be, draws=26, seed=SEED + 1, draw0=100)
        m.add(al[1:2].contiguous(), be[1:2].contiguous(), draws=3, seed=SEED, draw0=2 ** 32 - 3)
        runs.append((m.hist.clone(), m.s1.clone(), m.s2.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_errors_leave_the_state_unchanged():
    shape = "3x3x3"
    al, be = operands(shape)
    m = new_state(shape).add(al, be, draws=3, seed=SEED)
    before = (m.hist.clone(), m.s1.clone(), m.s2.clone(), m.count)
    with pytest.raises(ValueError):
        m.add(al.transpose(2, 3), be, draws=3, seed=SEED)                        # not contiguous
    with pytest.raises(TypeError):
        m.add(al, be.double(), draws=3, seed=SEED)
    with pytest.raises(_lib.RadonLibraryError):
        m.add(al.cpu(), be.cpu(), draws=3, seed=SEED)
    with pytest.raises(ValueError):
        m.add(*operands("3x1x7"), draws=3, seed=SEED)                            # another pixel grid than the state's
    with pytest.raises(ValueError):
        m.add(al, be, draws=0, seed=SEED)
    with pytest.raises(ValueError):
        m.add(al, be, draws=2, seed=SEED, draw0=2 ** 32 - 1)
    torch.cuda.synchronize()
    assert torch.equal(m.hist, before[0]) and torch.equal(m.s1, before[1]) and torch.equal(m.s2, before[2]) and m.count == before[3]


def test_save_and_load_on_the_device(tmp_path):
    m = new_state("3x1x7").add(*operands("3x1x7"), draws=26, seed=SEED)
    path = str(tmp_path / "m.npz")
    m.save(path)
    back = PixelMarginals.load(path, device=_dev())
    assert back.count == m.count and torch.equal(back.hist, m.hist) and torch.equal(back.s1, m.s1) and torch.equal(back.s2, m.s2)
    back.add(*operands("3x1x7"), draws=4, seed=SEED, draw0=26)                   # a loaded state goes on accumulating
    np.testing.assert_array_equal(back.hist.cpu().numpy(), bin_samples(head_samples("3x1x7", 30, 0, 0), **GRID))


TOY = ("-b 4 --ns 2 --td 8 --nsa 1 --api 2 --ik 2 --il 5 --ks 2 --nb 3 --se 1 --no_pad --toy_masks --normal --n_pixel 2 --num_angles 2 "
       "--pixel_dist --en 1 --pixel_repeats 3")


def _toy_run(folder, extra=""):
    """An untrained trainer of the cut-down toy recipe (its weights from the trainer's own seed); without --save_path among the
    arguments its setup arrays are drawn, not read back.  Returns the arrays of the file pixel_dist wrote under `folder`."""
    args = tr.get_args((TOY + " " + extra).split())
    t = tr.PVAETrainer(args, _dev())
    m = t.pixel_dist(example_num=args.example_num, num_repeats=args.pixel_repeats, save_path=str(folder))
    assert m.count == 3 * 2 * 4 * 100
    with np.load(str(folder / "pixel_dist_1.npz")) as f:
        return {k: f[k] for k in f.files}


def test_trainer_pixel_dist_writes_its_file(tmp_path, capsys):
    """The toy recipe cut down, no training: pixel_dist_1.npz with hist [4][52], count = repeats * ns * b * 100."""
    f = _toy_run(tmp_path)
    count = 3 * 2 * 4 * 100
    assert f["hist"].shape == (4, 52) and f["hist"].dtype == np.int64 and int(f["count"]) == count
    np.testing.assert_array_equal(f["hist"].sum(axis=1), np.full(4, count))
    mean = f["s1"] / count
    assert np.isfinite(mean).all() and np.isfinite(f["s2"]).all() and (mean >= 0).all()
    assert float(f["lo"]) == 0.005 and float(f["width"]) == 0.01
    assert f"{count} samples per pixel" in capsys.readouterr().out


def test_trainer_pixel_dist_is_reproducible(tmp_path):
    """--fused_latents --fused_blocks --reproducible: the latents are keyed by (--head_seed, repeat), the head's draws by (--head_seed,
    repeat * 100 + k), the convolutions deterministic -- a second run (a new trainer, new weights from the same seed) gives an equal
    hist."""
    runs = []
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
        runs.append(_toy_run(tmp_path / name, "--fused_latents --fused_blocks --reproducible"))
    np.testing.assert_array_equal(runs[0]["hist"], runs[1]["hist"])
    assert np.array_equal(runs[0]["s1"], runs[1]["s1"]) and np.array_equal(runs[0]["s2"], runs[1]["s2"])


def test_main_runs_pixel_dist_after_the_restore(tmp_path):
    """The command line as a user runs it: train and save, then --restore --pixel_dist on the saved files."""
    base = TOY.replace(" --pixel_dist --en 1 --pixel_repeats 3", "") + f" --save_path {tmp_path} --no_final_eval -i 2"
    tr.main((base + " --train").split())
    assert not (tmp_path / "pixel_dist_1.npz").exists()
    tr.main((base + " --restore --pixel_dist --en 1 --pixel_repeats 2").split())
    with np.load(str(tmp_path / "pixel_dist_1.npz")) as f:
        assert f["hist"].shape == (4, 52) and int(f["count"]) == 2 * 2 * 4 * 100
        np.testing.assert_array_equal(f["hist"].sum(axis=1), np.full(4, int(f["count"])))
    with pytest.raises(ValueError):
        tr.PVAETrainer(tr.get_args(base.split() + ["--det"]), _dev()).pixel_dist()
