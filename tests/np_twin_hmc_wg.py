"""The shapes, problems and seeds of the tests of the workgroup form of the HMC sampler (ct_pvae_amd/csrc/hmc_wg.hip,
hmc_sample(form="workgroup")).  The restatement itself is tests/np_twin_hmc.py, which is generic in N: Model, draws, run,
check_against_twin, target_case and check_target are used as they stand."""
import numpy as np

from tests import np_twin_hmc as tw

# name -> (N, A).  w9: two waves, the second partly filled (81 pixels).  w12: K - 1 = 143 ends the active threads on a 16-lane DPP
# row of the third wave.  w16: four full waves.  w23: nine waves (529 pixels).  w32: the full 1024 threads.
SHAPES = {"w9": (9, 5), "w12": (12, 7), "w16": (16, 6), "w23": (23, 3), "w32": (32, 4)}
C = 64
STEP = 1e-2
L = 5
SEED = 21             # the Philox seed of the runs
CAPS = {1: 0.05, 8: 0.20}     # transitions -> the largest fraction of chains left out (tests/test_gpu_hmc.py's caps)


def problem(oracle, name):
    """np_twin_hmc.problem's recipe at (N, A) = SHAPES[name]: Poisson measurements (the oracle's sampler, pnm = 1e3) of a random
    simplex object's sinogram at theta_k = 0.3 + 0.6 k, the second angle masked out, a prior of two Dirichlets."""
    N, A = SHAPES[name]
    rng = np.random.default_rng(1000 + 17 * N + A)
    theta = (0.3 + 0.6 * np.arange(A)).astype(np.float32)
    obj = rng.dirichlet(np.full(N * N, 2.0)).astype(np.float32).reshape(1, N, N)
    sino = oracle.rotate_fwd(obj, oracle.Geometry(N, N, False), oracle.rotate_transforms(theta, N, N))
    mask = np.where(np.arange(A) % 2 == 0, 1.0, 0.5).astype(np.float32)[None]
    if A > 2:
        mask[0, 1] = 0.0
    meas = oracle.poisson_measure(sino, mask, 1e3, 5)
    prior = (np.array([0.4, 0.6]), rng.uniform(0.5, 2.0, (2, N * N)))
    return dict(N=N, A=A, theta=theta, mask=mask, meas=meas, pnm=1e3, prior=prior, obj=obj)


def random_starts(name, chains=C):
    N = SHAPES[name][0]
    return np.random.default_rng(2000).dirichlet(np.full(N * N, 3.0), chains).astype(np.float32)


def twin_runs(oracle, name, n_steps):
    """The float32 and float64 restatements of hmc_sample(..., initial_state=random_starts(name), num_adaptation_steps=0, step_size=
    STEP, num_leapfrog_steps=L, seed=SEED) on C chains of the problem `name`: (problem, starts, twin32, twin64)."""
    pb = problem(oracle, name)
    model = tw.Model(oracle, pb["theta"], pb["N"], pb["mask"], pb["meas"], pb["pnm"], *pb["prior"], chains_per_object=C)
    starts = random_starts(name)
    eps = np.full(C, STEP, np.float32)
    runs = [tw.run(model, model.inverse(starts, dt), eps, np.arange(C), SEED, n_steps, L) for dt in (np.float32, np.float64)]
    return pb, starts, runs[0], runs[1]


def first(run, n):
    """The first n steps of a twin run's per-step arrays."""
    return {k: v[:n] for k, v in run.items() if k not in ("eps", "x")}


def target_cases():
    """(N, A, M, seed) of the evaluator's cases: per N one angle, a few, more than the tie angles (N = 32: one and a few), then A N
    exactly one pass of the 64 W threads where N divides it, and the next A above one pass: 9 x 15 = 135 > 128; 12 x 16 = 192 and
    12 x 17; 16 x 16 = 256 and 16 x 17; 23 x 26 = 598 > 576; 32 x 32 = 1024 and 32 x 33.  22 cases; np_twin_hmc.target_case builds each."""
    for N in (9, 12, 16, 23, 32):
        threads = 64 * -(-N * N // 64)
        angles = {1, 3} if N == 32 else {1, 3, 11}
        if threads % N == 0:
            angles.add(threads // N)
        angles.add(threads // N + 1)
        for A in sorted(angles):
            yield N, A, 1 + (N + A) % 4, 100 * N + A
