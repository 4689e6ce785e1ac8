"""The update stage without a GPU: the host-built chunk table, the entry points' argument checks, the float32 twin against the float64
formula (tests/np_twin_update.py states the bar), the control that refuses torch's epsilon placement, and FusedUpdate's state dictionary
against torch.optim.Adam's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import np_twin_update as tw


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def C(lib):
    from ct_pvae_amd import update
    c = update.chunk_len()
    assert c == 4 * tw.THREADS and c >= 64
    return c


def _lens_cases(C):
    return [[1], [C - 1], [C], [C + 1], [2 * C + 3], [1] * 300, [1, C - 1, C, C + 1, 2 * C + 3, 5], [3, 70 * C - 5, 2]]


def test_chunk_table_covers_every_element_once(C):
    from ct_pvae_amd import update
    for lens in _lens_cases(C):
        base = [0x10000 + 0x100000 * k for k in range(len(lens))]           # made-up, 4-byte aligned addresses: nothing is dereferenced
        tab = update.chunk_table(lens, base)
        assert tab.dtype.itemsize == 32 and tab.size == sum(-(-n // C) for n in lens)
        hit = np.zeros(sum(lens), np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)])
        for r in tab:
            off, n, k = int(r["off"]), int(r["len"]), int(r["tensor"])
            assert 1 <= n <= C
            assert starts[k] <= off and off + n <= starts[k + 1]               # inside ONE tensor
            assert int(r["param"]) == base[k] + 4 * (off - starts[k])          # the parameter's element at that offset
            assert int(tab[int(r["first"])]["tensor"]) == k and (int(r["first"]) == 0 or int(tab[int(r["first"]) - 1]["tensor"]) == k - 1)
            assert int(r["count"]) == -(-lens[k] // C)
            hit[off:off + n] += 1
        assert (hit == 1).all()
        assert (np.diff(tab["off"]) > 0).all() if tab.size > 1 else True      # ascending
        want = tw.chunk_rule(lens, C)
        assert [(int(r["off"]), int(r["len"]), int(r["tensor"]), int(r["first"]), int(r["count"])) for r in tab] == want


def test_entry_points_refuse_bad_arguments_before_any_hip_call(lib, C):
    from ct_pvae_amd import update
    L = lib.load()
    lens = np.array([5, 7], np.int64)
    addr = np.array([0x1000, 0x2000], np.uint64)
    out = np.zeros(2, update.CHUNK_DTYPE)
    assert L.ctpvae_update_plan_bytes(None, 2) == lib.EINVAL and "null" in lib.last_error()
    assert L.ctpvae_update_plan_bytes(lens.ctypes.data, 0) == lib.EINVAL and "empty" in lib.last_error()
    assert L.ctpvae_update_plan_bytes(lens.ctypes.data, 2) == 64
    zero = np.array([5, 0], np.int64)
    assert L.ctpvae_update_plan_bytes(zero.ctypes.data, 2) == lib.EINVAL and "positive" in lib.last_error()
    assert L.ctpvae_update_plan_host(zero.ctypes.data, addr.ctypes.data, 2, out.ctypes.data) == lib.EINVAL and "positive" in lib.last_error()
    assert L.ctpvae_update_plan_host(lens.ctypes.data, addr.ctypes.data, 0, out.ctypes.data) == lib.EINVAL and "empty" in lib.last_error()
    for args in ((None, addr.ctypes.data, 2, out.ctypes.data), (lens.ctypes.data, None, 2, out.ctypes.data),
                 (lens.ctypes.data, addr.ctypes.data, 2, None)):
        assert L.ctpvae_update_plan_host(*args) == lib.EINVAL and "null" in lib.last_error()
    null_param = np.array([0x1000, 0], np.uint64)
    assert L.ctpvae_update_plan_host(lens.ctypes.data, null_param.ctypes.data, 2, out.ctypes.data) == lib.EINVAL and "null" in lib.last_error()
    assert L.ctpvae_update_plan_host(lens.ctypes.data, addr.ctypes.data, 2, out.ctypes.data) == 0
    # the launch entry: null pointers and bad scalars are refused before any HIP call (the made-up addresses are never touched)
    ok = dict(plan=0x1000, n_chunks=2, T=2, grad=0x2000, m=0x3000, v=0x4000, partials=0x5000, norms=0x6000, t=1, alpha=1e-4, clip=100.0,
              b1=0.9, b2=0.999, eps=1e-7, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ctpvae_update_f32(*[a[k] for k in ("plan", "n_chunks", "T", "grad", "m", "v", "partials", "norms", "t", "alpha", "clip", "b1",
                                                    "b2", "eps", "stream")])
    for name in ("plan", "grad", "m", "v", "partials", "norms"):
        assert call(**{name: None}) == lib.EINVAL and "null" in lib.last_error(), name
    for kw in (dict(T=0), dict(n_chunks=1), dict(t=0), dict(clip=0.0), dict(alpha=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0),
               dict(partials=0x5004), dict(grad=0x2002)):
        assert call(**kw) == lib.EINVAL, kw
    with pytest.raises(ValueError):
        update.chunk_table([], [])
    with pytest.raises(ValueError):
        update.chunk_table([4, 0], [0x1000, 0x2000])
    with pytest.raises(ValueError):
        update.chunk_table([4, 4], [0x1000])


def _operands(seed, lens, gscale, with_state):
    rng = np.random.default_rng(seed)
    n = sum(lens)
    g = (rng.standard_normal(n) * gscale).astype(tw.F)
    p = (0.1 * rng.standard_normal(n)).astype(tw.F)
    m = (0.1 * gscale * rng.standard_normal(n)).astype(tw.F) if with_state else np.zeros(n, tw.F)
    v = ((0.1 * gscale * rng.standard_normal(n)) ** 2).astype(tw.F) if with_state else np.zeros(n, tw.F)
    return g, p, m, v


CASES = [(t, eps, gscale, lr) for t in (1, 5, 1000) for eps in (1e-7, 1e-3) for gscale in (1e-6, 1.0, 300.0) for lr in (1e-4, 1e-2)]


def _l2_elem(g, lens, C):
    return np.repeat(tw.tensor_norms(g, lens, C), lens)


def test_float32_twin_is_the_float64_formula_to_float32_precision(C):
    lens = [1, 3, 65, C + 1, 2 * C + 3]
    worst = 0.0
    for seed, (t, eps, gscale, lr) in enumerate(CASES):
        g, p, m, v = _operands(seed, lens, gscale, with_state=t > 1)
        g[::97] = np.nan                                                     # filtered: they count as 0 in the norm too
        alpha = tw.adam_alpha(t, lr, 0.9, 0.999)
        hyper = (alpha, 100.0, 0.9, 0.999, eps)
        got = tw.twin_update(g, _l2_elem(g, lens, C), p, m, v, *hyper)
        want = tw.reference_update(g, lens, p, m, v, *hyper)
        for name, a, b, bar in zip("pmv", got, want, tw.bars(g, lens, p, m, v, *hyper)):
            r, same = tw.worst_excess(a, b, bar)
            assert same and r <= tw.MARGIN, (name, t, eps, gscale, lr, r)
            worst = max(worst, r)
    assert worst > 0.0                                                       # the bar is met, not vacuous: some element does round


def test_control_torch_epsilon_placement_is_refused(C):
    """The same comparison refuses torch.optim.Adam's formula (eps = 1e-3, t = 1: Keras's epsilon acts 31.6 times as large)."""
    lens = [1, 3, 65, C + 1]
    t, eps, lr = 1, 1e-3, 1e-4
    g, p, m, v = _operands(3, lens, 1.0, with_state=False)
    alpha = tw.adam_alpha(t, lr, 0.9, 0.999)
    hyper = (alpha, 100.0, 0.9, 0.999, eps)
    bar_p = tw.bars(g, lens, p, m, v, *hyper)[0]
    twin_p = tw.twin_update(g, _l2_elem(g, lens, C), p, m, v, *hyper)[0]
    r_ok, _ = tw.worst_excess(twin_p, tw.reference_update(g, lens, p, m, v, *hyper)[0], bar_p)
    r_torch, _ = tw.worst_excess(twin_p, tw.reference_update_torch_eps(g, lens, p, m, v, t, lr, 100.0, 0.9, 0.999, eps)[0], bar_p)
    assert r_ok <= tw.MARGIN < r_torch, (r_ok, r_torch)
    # ... and with the reference's own eps = 1e-7, where the two placements differ by 3e-6 of a step
    hyper7 = (alpha, 100.0, 0.9, 0.999, 1e-7)
    twin7 = tw.twin_update(g, _l2_elem(g, lens, C), p, m, v, *hyper7)[0]
    assert tw.worst_excess(twin7, tw.reference_update(g, lens, p, m, v, *hyper7)[0], tw.bars(g, lens, p, m, v, *hyper7)[0])[0] <= tw.MARGIN


def test_norm_order_and_filter_of_the_twin(C):
    """The documented order is a float64 sum of exact squares: within n 2^-53 of math.fsum, NaNs count as 0, an inf gives inf."""
    import math
    rng = np.random.default_rng(0)
    g = rng.standard_normal(2 * C + 3).astype(tw.F)
    g[5] = np.nan
    got = tw.tensor_norms(g, [g.size], C)[0]
    g0 = np.where(np.isnan(g), 0, g).astype(np.float64)
    exact = math.sqrt(math.fsum((g0 * g0).tolist()))
    assert abs(float(got) - exact) <= float(np.spacing(tw.F(exact)))
    g[7] = np.inf
    assert np.isposinf(tw.tensor_norms(g, [g.size], C)[0])
    assert tw.tensor_norms(np.zeros(4, tw.F), [4], C)[0] == 0.0


def test_state_dict_round_trip_with_torch_adam_on_cpu(lib):
    from ct_pvae_amd import FusedUpdate
    torch.manual_seed(0)
    shapes = [(3, 4), (5,), (), (2, 1, 3)]
    params = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    adam = torch.optim.Adam(params, lr=1e-3, eps=1e-7, foreach=True)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn_like(p)
        adam.step()
    sd = adam.state_dict()
    fu = FusedUpdate(params, lr=5e-2, eps=1e-3)
    assert fu.t == 0 and fu.state_dict()["state"] == {} and tuple(fu.norms.shape) == (4,)
    fu.load_state_dict(sd)
    assert fu.t == 2 and fu.lr == 1e-3 and fu.eps == 1e-7 and (fu.beta1, fu.beta2) == (0.9, 0.999)
    assert torch.equal(fu.m, torch.cat([sd["state"][k]["exp_avg"].reshape(-1) for k in range(4)]))
    out = fu.state_dict()
    assert sorted(out["param_groups"][0]) == sorted(sd["param_groups"][0])     # torch.optim.Adam's own keys
    fresh = torch.optim.Adam([torch.nn.Parameter(torch.zeros(s)) for s in shapes], lr=1.0)
    fresh.load_state_dict(out)
    back = fresh.state_dict()
    assert back["param_groups"][0]["lr"] == 1e-3 and back["param_groups"][0]["eps"] == 1e-7
    for k in range(4):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][k][key], sd["state"][k][key]) and back["state"][k][key].shape == sd["state"][k][key].shape
        assert float(back["state"][k]["step"]) == float(sd["state"][k]["step"]) == 2.0
    for p in fresh.param_groups[0]["params"]:                                   # and torch steps on from it
        p.grad = torch.ones_like(p)
    fresh.step()
    assert float(fresh.state_dict()["state"][0]["step"]) == 3.0
    # entries whose steps differ cannot become ONE step count
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError):
        fu.load_state_dict(sd)
    with pytest.raises(ValueError):
        FusedUpdate(params[:2]).load_state_dict(adam.state_dict())
    # there is no CPU path: a well-formed step on CPU tensors is refused by name
    with pytest.raises(lib.RadonLibraryError):
        fu.step(torch.zeros(fu.total))


def test_argument_errors_raise_before_any_launch(lib):
    from ct_pvae_amd import FusedUpdate
    params = [torch.zeros(3, 4), torch.zeros(5)]
    fu = FusedUpdate(params)
    assert fu.total == 17
    with pytest.raises(ValueError):
        fu.step(torch.zeros(16))                                                # wrong length
    with pytest.raises(ValueError):
        fu.step(torch.zeros(17, dtype=torch.float64))                           # wrong dtype
    with pytest.raises(ValueError):
        fu.step(torch.zeros(17, 1))                                             # not one row
    with pytest.raises(ValueError):
        fu.step(torch.zeros(17, device="meta"))                                 # wrong device
    with pytest.raises(TypeError):
        fu.step(np.zeros(17, np.float32))
    with pytest.raises(TypeError):
        FusedUpdate([torch.zeros(3, dtype=torch.float64)])
    with pytest.raises(TypeError):
        FusedUpdate([torch.zeros(3, dtype=torch.float16)])
    half = [torch.nn.Parameter(torch.zeros(3))]
    fu2 = FusedUpdate(half)
    half[0].data = torch.zeros(3, dtype=torch.float64)                          # a parameter that stopped being float32
    with pytest.raises(TypeError):
        fu2.step(torch.zeros(3))
    with pytest.raises(ValueError):
        FusedUpdate([])
    with pytest.raises(ValueError):
        FusedUpdate([torch.zeros(4, 4).t()])                                    # not contiguous
    for kw in (dict(lr=-1.0), dict(beta1=1.0), dict(beta2=-0.5), dict(eps=-1e-7), dict(clip_norm=0.0), dict(clip_norm=float("inf"))):
        with pytest.raises(ValueError):
            FusedUpdate(params, **kw)
    from ct_pvae_amd import adam_alpha
    assert adam_alpha(1, 1e-4, 0.9, 0.999) == float(tw.adam_alpha(1, 1e-4, 0.9, 0.999))
    assert abs(adam_alpha(1, 1e-4, 0.9, 0.999) / (1e-4 * np.sqrt(0.001) / 0.1) - 1) < 1e-6
    with pytest.raises(ValueError):
        adam_alpha(0, 1e-4, 0.9, 0.999)


def test_trainer_flag_parses_and_is_off_by_default():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).fused_update is False
    assert tr.get_args(["--fused_update"]).fused_update is True
