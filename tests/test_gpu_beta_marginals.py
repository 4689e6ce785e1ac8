"""The Beta head's per-pixel marginals on the device (ct_pvae_amd/marginals.py head="beta", csrc/beta_marginals.hip): every sample IS
beta_head's x, so the histogram equals bin_samples of the stacked head samples exactly, the float64 sums are bit-equal to the twin's
restatement of the stated order (tests/np_twin_marginals.py, unchanged: the order is marginals.hip's) and inside the any-order bound of
math.fsum; accumulation, splits, reproducibility, NaN operands, errors; the law of the samples through the new kernel alone; the
trainer's --pixel_dist without --normal.

Shapes (n, X, Y): one quad; a ragged row with unaligned objects (offsets 7 and 14); 3 x 3; and (2, 5, 15): 75 pixels, 11 more than the
64 one workgroup covers -- a second tile with two whole quads and a 3-pixel tail, and object 1 at the unaligned offset 75.  The draws
are cut into slices of 25: K = 25 and 26 sit either side of that cut.  Pixel p takes np_twin_beta's operand range "trainer", "small",
"large" or "mixed" by p % 4: both sides of the boost's seam at concentration 1, and samples saturated at 0 and 1."""
import math

import numpy as np
import pytest
import torch
from scipy import special

from ct_pvae_amd import PixelMarginals, _lib, beta_head, bin_samples
from ct_pvae_amd import trainer as tr
from tests import np_law
from tests import np_twin_beta as tb
from tests import np_twin_marginals as tm

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
SHAPES = {"1x2x2": (1, 2, 2), "3x1x7": (3, 1, 7), "3x3x3": (3, 3, 3), "2x5x15": (2, 5, 15)}
KINDS = ("trainer", "small", "large", "mixed")
GRID = dict(lo=0.05, width=0.045, bins=20)       # [0.05, 0.95): the operands below put samples under, inside and over it
OTHER_GRIDS = {"bins=1": dict(lo=0.5, width=0.25, bins=1), "bins=254": dict(lo=0.01, width=0.0035, bins=254),
               "reference": dict(lo=0.005, width=0.01, bins=50)}
_ops, _heads = {}, {}


def _dev():
    return torch.device("cuda", 0)


def _operands_np(n, pix):
    kinds = [tb.operands(kind, n, pix, 11 + i) for i, kind in enumerate(KINDS)]
    pick = np.arange(pix) % 4
    return (np.choose(pick[None, :], [k[0] for k in kinds]).astype(np.float32),
            np.choose(pick[None, :], [k[1] for k in kinds]).astype(np.float32))


def operands(shape):
    """(alpha, beta) [n][1][X][Y] on the device, left unchanged."""
    if shape not in _ops:
        n, X, Y = SHAPES[shape]
        _ops[shape] = tuple(torch.from_numpy(v).to(_dev()).reshape(n, 1, X, Y).contiguous() for v in _operands_np(n, X * Y))
    return _ops[shape]


def stack_of_heads(al, be, K, first_object, draw0):
    n = al.shape[0]
    return torch.stack([beta_head(al, be, seed=SEED, draw=draw0 + k, first_object=first_object)[0].reshape(n, -1)
                        for k in range(K)]).cpu().numpy()


def head_samples(shape, K, first_object, draw0):
    """float32 numpy [K][n][pix]: beta_head's own x for draw = draw0 + k (computed once per key, left unchanged)."""
    key = (shape, K, first_object, draw0)
    if key not in _heads:
        _heads[key] = stack_of_heads(*operands(shape), K, first_object, draw0)
        _heads[key].setflags(write=False)
    return _heads[key]


def new_state(shape, head="beta", **grid):
    _, X, Y = SHAPES[shape]
    return PixelMarginals((X, Y), device=_dev(), head=head, **(grid or GRID))


def check_moments(m, samples):
    """s1, s2 within (N - 1) 2^-53 relative of math.fsum over the samples and their exact squares, N samples per pixel (where a
    pixel's exact sum is 0 the device's is 0)."""
    flat = samples.reshape(-1, samples.shape[-1])
    N = flat.shape[0]
    f1, f2 = tm.fsum_sums(flat)
    s1, s2 = m.s1.cpu().numpy(), m.s2.cpu().numpy()
    r1 = np.max(np.abs(s1 - f1) / np.where(f1 > 0, f1, 1.0))
    r2 = np.max(np.abs(s2 - f2) / np.where(f2 > 0, f2, 1.0))
    print(f"N = {N}: worst relative distance from fsum s1 {r1:.3e}, s2 {r2:.3e}, bound {tm.fsum_bound(N):.3e}")
    assert np.all(np.abs(s1 - f1) <= tm.fsum_bound(N) * f1) and np.all(np.abs(s2 - f2) <= tm.fsum_bound(N) * f2)


def bits(t):
    return t.cpu().numpy().view(np.uint64)


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
    assert m.count == n * K and m.head == "beta"
    hist = m.hist.cpu().numpy()
    np.testing.assert_array_equal(hist, bin_samples(want, **GRID))
    np.testing.assert_array_equal(hist.sum(axis=1), np.full(X * Y, m.count))
    check_moments(m, want)
    t1, t2 = tm.ordered_sums(want)                      # the stated order, restated: bit-equal
    assert np.array_equal(bits(m.s1), t1.view(np.uint64)) and np.array_equal(bits(m.s2), t2.view(np.uint64))
    mean, std = m.mean().cpu().numpy(), m.std().cpu().numpy()
    flat = want.reshape(-1, X * Y).astype(np.float64)
    np.testing.assert_allclose(mean.ravel(), flat.mean(axis=0), rtol=1e-13)
    if m.count >= 2:
        np.testing.assert_allclose(std.ravel(), flat.std(axis=0, ddof=1), rtol=1e-6, atol=1e-9)
    else:
        assert np.isnan(std).all()


def test_the_grid_exercises_all_three_column_kinds():
    """On the head's own samples: column 0, column bins + 1 and at least two inner columns are non-empty, samples saturate at both
    ends -- then the device agrees."""
    want = head_samples("2x5x15", 100, 0, 0)
    h = bin_samples(want, **GRID)
    assert h[:, 0].sum() > 0 and h[:, -1].sum() > 0 and int((h[:, 1:-1].sum(axis=0) > 0).sum()) >= 2
    assert (want == 0).any() and (want == 1).any()
    m = new_state("2x5x15").add(*operands("2x5x15"), draws=100, seed=SEED)
    np.testing.assert_array_equal(m.hist.cpu().numpy(), h)


@pytest.mark.parametrize("grid", list(OTHER_GRIDS))
def test_other_bin_counts(grid):
    grid = OTHER_GRIDS[grid]
    want = head_samples("2x5x15", 26, 5, 0)
    h = bin_samples(want, **grid)
    assert h[:, 0].sum() > 0 and h[:, -1].sum() > 0 and h[:, 1:-1].sum() > 0
    m = new_state("2x5x15", **grid).add(*operands("2x5x15"), draws=26, seed=SEED, first_object=5)
    assert m.hist.shape == (75, grid["bins"] + 2)
    np.testing.assert_array_equal(m.hist.cpu().numpy(), h)
    np.testing.assert_array_equal(m.hist.sum(dim=1).cpu().numpy(), np.full(75, m.count))


def test_draws_accumulate_over_calls():
    """add(K1, draw0 = 0) then add(K2, draw0 = K1) gives the hist of one add(K1 + K2); the state's sum is (0 + T1) + T2."""
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
    al, be = (torch.from_numpy(v).to(_dev()).reshape(n, 1, X, Y) for v in _operands_np(n, X * Y))
    want = stack_of_heads(al, be, K, 1, 0)
    m = PixelMarginals((X, Y), device=_dev(), head="beta", **GRID).add(al, be, draws=K, seed=SEED, first_object=1)
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


def test_the_head_keyword_is_not_ignored():
    """A "beta" state and a "truncated_normal" state on the same operands hold other samples."""
    shape = "2x5x15"
    al, be = operands(shape)
    b = new_state(shape, head="beta").add(al, be, draws=26, seed=SEED)
    t = new_state(shape, head="truncated_normal").add(al, be, draws=26, seed=SEED)
    assert b.count == t.count and not torch.equal(b.hist, t.hist) and not torch.equal(b.s1, t.s1)
    assert float(b.mean().max()) <= 1.0 < float(t.mean().max())          # a Beta sample lies in [0, 1]; "large" locs reach 40


def test_nan_operands_touch_their_pixel_alone():
    """One NaN alpha: that pixel's n * K samples are NaN (16 refused attempts each) -- column 0 holds them all and s1, s2 are NaN --
    and every other pixel has the bits of the run without it."""
    shape, K, bad = "2x5x15", 26, 37
    n, X, Y = SHAPES[shape]
    al, be = operands(shape)
    clean = new_state(shape).add(al, be, draws=K, seed=SEED, first_object=5)
    al_nan = al.clone()
    al_nan.view(n, -1)[:, bad] = float("nan")
    m = new_state(shape).add(al_nan, be, draws=K, seed=SEED, first_object=5)
    hist = m.hist.cpu().numpy()
    assert hist[bad, 0] == n * K and hist[bad, 1:].sum() == 0
    assert math.isnan(float(m.s1[bad])) and math.isnan(float(m.s2[bad]))
    keep = np.arange(X * Y) != bad
    np.testing.assert_array_equal(hist[keep], clean.hist.cpu().numpy()[keep])
    assert np.array_equal(bits(m.s1)[keep], bits(clean.s1)[keep]) and np.array_equal(bits(m.s2)[keep], bits(clean.s2)[keep])
    assert np.isfinite(clean.s1.cpu().numpy()).all()
    # one object's NaN: the pixel's other object still adds its samples to the columns, the sums are NaN
    al_one = al.clone()
    al_one.view(n, -1)[1, bad] = float("nan")
    m1 = new_state(shape).add(al_one, be, draws=K, seed=SEED, first_object=5)
    h1 = m1.hist.cpu().numpy()
    np.testing.assert_array_equal(h1[keep], clean.hist.cpu().numpy()[keep])
    assert h1[bad].sum() == n * K and h1[bad, 0] >= K and math.isnan(float(m1.s1[bad]))


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
    assert back.head == "beta" and back.count == m.count
    assert torch.equal(back.hist, m.hist) and torch.equal(back.s1, m.s1) and torch.equal(back.s2, m.s2)
    back.add(*operands("3x1x7"), draws=4, seed=SEED, draw0=26)                   # a loaded state goes on accumulating, as a Beta state
    np.testing.assert_array_equal(back.hist.cpu().numpy(), bin_samples(head_samples("3x1x7", 30, 0, 0), **GRID))


# ---- the law, through the new kernel alone ------------------------------------------------------------------------------------------
LAW_CELLS = {"a=2,b=5": (2.0, 5.0), "boosted": (-1.0, 0.0), "a=40,b=300": (40.0, 300.0)}      # raw operands (alpha, beta)
LAW_N, LAW_K, LAW_BINS = 64, 256, 254                                                        # 64 pixels x 64 x 256 = 2^20 samples


def _law_run(cell):
    ra, rb = LAW_CELLS[cell]
    al = torch.full((LAW_N, 1, 8, 8), ra, dtype=torch.float32, device=_dev())
    be = torch.full((LAW_N, 1, 8, 8), rb, dtype=torch.float32, device=_dev())
    m = PixelMarginals((8, 8), bins=LAW_BINS, lo=0.0, width=1.0 / LAW_BINS, device=_dev(), head="beta")
    m.add(al, be, draws=LAW_K, seed=SEED + 7, first_object=3)
    pr = lambda t: t if t >= 1.0 else math.exp(t - 1.0) + tb.EPS32                          # noqa: E731  positive_range
    return m, pr(ra), pr(rb)


def _law_distance(hist, a, b, shift=0):
    """sup over the 255 nominal edges j / 254 of |F_N - I(a, b)|: F_N(edge j) is the pooled count of columns 0 .. j (under, NaN, and
    bins 1 .. j: the samples below the edge).  shift (the control): the columns moved by that many bins first."""
    pooled = hist.sum(axis=0).astype(np.float64)
    total = pooled.sum()
    assert total == 2 ** 20
    cum = np.cumsum(pooled)[:LAW_BINS + 1] / total                                          # edges 0 .. 254
    cum = np.concatenate([np.zeros(shift), cum])[:LAW_BINS + 1]
    cdf = special.betainc(a, b, np.arange(LAW_BINS + 1) / LAW_BINS)
    return float(np.max(np.abs(cum - cdf)))


def test_the_samples_follow_the_beta_law():
    """2^20 samples per cell pooled over 64 equal pixels: the cumulative histogram at every nominal edge within the DKW bound of
    scipy's regularised incomplete beta (the float32 bin rule moves an edge by about one ulp: mass below 1e-6 of the bound); each
    pixel's mean within 6 standard errors of a / (a + b) (192 assertions); the control -- the same histogram moved by one column --
    is refused in at least one cell."""
    bound = np_law.dkw(2 ** 20)
    refused = []
    for cell in LAW_CELLS:
        m, a, b = _law_run(cell)
        hist = m.hist.cpu().numpy()
        assert m.count == LAW_N * LAW_K == 16384 and (hist.sum(axis=1) == m.count).all()
        dist, moved = _law_distance(hist, a, b), _law_distance(hist, a, b, shift=1)
        print(f"{cell}: a = {a:.6g}, b = {b:.6g}: sup distance {dist:.3e}, moved by one column {moved:.3e}, bound {bound:.3e}")
        assert dist <= bound, (cell, dist, bound)
        refused.append(moved > bound)
        se = math.sqrt(a * b / ((a + b) ** 2 * (a + b + 1.0)) / m.count)
        mean = m.mean().cpu().numpy().ravel()
        worst = float(np.max(np.abs(mean - a / (a + b)))) / se
        print(f"{cell}: worst pixel mean {worst:.2f} standard errors from a / (a + b)")
        for p in range(64):
            assert abs(mean[p] - a / (a + b)) <= 6.0 * se, (cell, p, mean[p], a / (a + b), se)
    assert any(refused)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
TOY = ("-b 4 --ns 2 --td 8 --nsa 1 --api 2 --ik 2 --il 5 --ks 2 --nb 3 --se 1 --no_pad --toy_masks --n_pixel 2 --num_angles 2 "
       "--fused_beta_head --pixel_dist --en 1 --pixel_repeats 3")


def _toy_run(folder, extra=""):
    """An untrained trainer of the cut-down toy recipe WITHOUT --normal (its weights from the trainer's own seed).  Returns the arrays
    of the file pixel_dist wrote under `folder`."""
    args = tr.get_args((TOY + " " + extra).split())
    t = tr.PVAETrainer(args, _dev())
    m = t.pixel_dist(example_num=args.example_num, num_repeats=args.pixel_repeats, save_path=str(folder))
    assert m.count == 3 * 2 * 4 * 100 and m.head == "beta"
    with np.load(str(folder / "pixel_dist_1.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_trainer_pixel_dist_writes_its_file(tmp_path, capsys):
    f = _toy_run(tmp_path)
    count = 3 * 2 * 4 * 100
    assert f["hist"].shape == (4, 52) and f["hist"].dtype == np.int64 and int(f["count"]) == count
    np.testing.assert_array_equal(f["hist"].sum(axis=1), np.full(4, count))
    mean = f["s1"] / count
    assert np.isfinite(f["s2"]).all() and (mean >= 0).all() and (mean <= 1).all()
    assert float(f["lo"]) == 0.005 and float(f["width"]) == 0.01 and str(f["head"]) == "beta"
    assert f"{count} samples per pixel" in capsys.readouterr().out


def test_trainer_pixel_dist_is_reproducible(tmp_path):
    """--fused_beta_latents --fused_blocks --reproducible: the latents are keyed by (--head_seed, repeat), the head's draws by
    (--head_seed, repeat * 100 + k), the convolutions deterministic -- a second run (a new trainer) gives equal bits."""
    runs = []
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
        runs.append(_toy_run(tmp_path / name, "--fused_beta_latents --fused_blocks --reproducible"))
    np.testing.assert_array_equal(runs[0]["hist"], runs[1]["hist"])
    assert np.array_equal(runs[0]["s1"], runs[1]["s1"]) and np.array_equal(runs[0]["s2"], runs[1]["s2"])


def test_main_runs_pixel_dist_after_the_restore(tmp_path):
    """The command line as a user runs it: train and save, then --restore --pixel_dist --fused_beta_head on the saved files."""
    base = TOY.replace(" --fused_beta_head --pixel_dist --en 1 --pixel_repeats 3", "") + f" --save_path {tmp_path} --no_final_eval -i 2"
    tr.main((base + " --train").split())
    assert not (tmp_path / "pixel_dist_1.npz").exists()
    tr.main((base + " --restore --pixel_dist --fused_beta_head --en 1 --pixel_repeats 2").split())
    with np.load(str(tmp_path / "pixel_dist_1.npz"), allow_pickle=False) as f:
        assert f["hist"].shape == (4, 52) and int(f["count"]) == 2 * 2 * 4 * 100 and str(f["head"]) == "beta"
        np.testing.assert_array_equal(f["hist"].sum(axis=1), np.full(4, int(f["count"])))
    with pytest.raises(ValueError):
        tr.PVAETrainer(tr.get_args(base.split() + ["--fused_beta_head", "--det"]), _dev()).pixel_dist()
    with pytest.raises(ValueError):
        tr.PVAETrainer(tr.get_args(base.split()), _dev()).pixel_dist()                   # torch's generator draws that head
