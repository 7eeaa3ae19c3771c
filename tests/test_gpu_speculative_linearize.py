"""-m gpu: speculative linearisation of the trial step's candidate (engine.hip, the LM loop of tmi_ba_solver_solve).

Where the next linearisation is a compact one (device_view.h, DeviceView::compact) the engine linearises the candidate
(prep_c, pts_c) into a second set of linearisation buffers right after back_substitute instead of taking its trial cost:
linearize sums the same residuals -- track by track where cost_view_kernel goes view by view -- and leaves cost, sum of
squares and the invalid vote where the trial cost would.  An accepted step swaps the two sets and does not linearise
again; a rejected one leaves the current linearisation untouched, and the step after it takes the trial cost as before.
TMI_BA_SPECULATIVE_LINEARIZE=0 keeps the old sequence.

"The same residuals summed in another order" (tests/test_gpu_direct_diag.py): identical iteration, step and PCG counts and
outcomes, costs and parameters to 1e-10 relative (the bound of tests/test_gpu_compact_planes.py for the same relation),
and bit-identical results wherever the path is not taken, across reset / a second solve / evaluate on one handle, and
from run to run.

The problems are PINHOLE with the default mask (compact planes on) and hold tracks of >= 12, >= 20 and >= 96
observations: the three lane mappings of track_map (1, 16 and 64 lanes per track)."""
import functools
import os

import numpy as np
import pytest

from theiasfm_amd import abi, lib, synth

pytestmark = pytest.mark.gpu

IMPL = dict(linear_solver_type=abi.ITERATIVE_SCHUR, schur_mode=abi.SCHUR_IMPLICIT)
SWITCH = "TMI_BA_SPECULATIVE_LINEARIZE"
ENV = (SWITCH, "TMI_BA_MF_ONE_SWEEP", "TMI_BA_COMPACT_PLANES")
NO_TOL = dict(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)


class env:
    """the switch unset (on) or "0" (off); the one-sweep product below its size threshold, as the compact-plane tests do"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in ENV}
        os.environ["TMI_BA_MF_ONE_SWEEP"] = "1"
        if not self.on:
            os.environ[SWITCH] = "0"

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def with_landmarks(prob, n_long, seed):
    """+ n_long tracks near the middle of the scene that every view sees, observed where the current parameters project
    them with half a pixel of noise"""
    rng = np.random.default_rng(seed)
    nc, np0, no0 = prob.num_cameras, prob.num_points, prob.num_observations
    centre = (prob.points[:, :3] / prob.points[:, 3:4]).mean(0)
    X = np.concatenate([centre + 0.02 * np.abs(centre).max() * rng.standard_normal((n_long, 3)), np.ones((n_long, 1))], 1)
    prob.points = np.ascontiguousarray(np.concatenate([prob.points, X]))
    prob.point_constant = np.concatenate([prob.point_constant, np.zeros(n_long, np.uint8)])
    prob.obs_camera = np.concatenate([prob.obs_camera, np.tile(np.arange(nc, dtype=np.int32), n_long)])
    prob.obs_point = np.concatenate([prob.obs_point, np.repeat(np.arange(np0, np0 + n_long, dtype=np.int32), nc)])
    prob.obs_xy = np.ascontiguousarray(np.concatenate([prob.obs_xy, np.zeros((n_long * nc, 2))]))
    new = np.arange(no0, no0 + n_long * nc)
    prob.obs_xy[new] = synth.project(prob, new) + 0.5 * rng.standard_normal((new.size, 2))
    return prob


@functools.lru_cache(maxsize=None)
def _problem(seed, perturb=1.0):
    prob = with_landmarks(synth.make_problem(100, 4000, 24000, seed=seed, scene="ring", spread=0.5, heavy_tail=0.02,
                                             perturb=perturb), 3, seed + 1)
    k = np.bincount(prob.obs_point, minlength=prob.num_points)
    assert ((k >= 12) & (k < 20)).any() and ((k >= 20) & (k < 96)).any() and (k >= 96).any()
    return prob


def problem(seed, perturb=1.0):
    return _problem(seed, perturb).copy()  # (the cached one stays as made)


def solve(prob, on, **kw):
    with env(on):
        p = prob.copy()
        kw.setdefault("max_num_iterations", 8)
        kw.setdefault("use_inner_iterations", 0)
        o = abi.default_options(profile_kernels=1, **kw)
        trace = abi.attach_trace(o, kw["max_num_iterations"])
        st, s = lib.solve(p, o)
        assert st == 0, s.message
        return s, p, trace


def launches(s, cls):
    return int(s.kernel_launches[abi.KERNEL_CLASS_NAMES.index(cls)])


def same_counts_and_outcomes(a, b):
    sa, _, ta = a
    sb, _, tb = b
    assert sa.num_iterations == sb.num_iterations
    assert sa.num_successful_steps == sb.num_successful_steps
    assert sa.num_unsuccessful_steps == sb.num_unsuccessful_steps
    assert sa.num_linear_solver_iterations == sb.num_linear_solver_iterations
    n = sa.num_iterations
    assert np.array_equal(ta[:n, 3], tb[:n, 3])


def same_to_round_off(a, b, rel=1e-10):
    same_counts_and_outcomes(a, b)
    sa, pa, _ = a
    sb, pb, _ = b
    assert abs(sa.final_cost - sb.final_cost) <= rel * abs(sb.final_cost)
    for x, y in ((pa.points, pb.points), (pa.extrinsics, pb.extrinsics), (pa.intrinsics, pb.intrinsics)):
        assert np.abs(x - y).max() <= rel * np.abs(y).max()


def same_bits(a, b):
    sa, pa, ta = a
    sb, pb, tb = b
    same_counts_and_outcomes(a, b)
    assert sa.initial_cost == sb.initial_cost and sa.final_cost == sb.final_cost and sa.final_rmse == sb.final_rmse
    assert sa.termination == sb.termination and sa.num_inner_iteration_steps == sb.num_inner_iteration_steps
    assert list(sa.kernel_launches) == list(sb.kernel_launches)
    assert np.array_equal(ta, tb, equal_nan=True)
    assert np.array_equal(pa.points, pb.points) and np.array_equal(pa.extrinsics, pb.extrinsics)
    assert np.array_equal(pa.intrinsics, pb.intrinsics)


def speculated(on, off):
    """trial-cost launches the path replaced"""
    return launches(off[0], "update_cost") - launches(on[0], "update_cost")


LOSSES = {"trivial": dict(), "huber": dict(loss_function_type=abi.LOSS_HUBER, robust_loss_width=2.0)}


@pytest.mark.parametrize("dof", [3, 4])
@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_on_against_off(loss, dof):
    """compact == 1 (TRIVIAL) and 2 (HUBER), 3- and 4-dof points"""
    prob = problem(11)
    kw = dict(point_dof=dof, **LOSSES[loss], **IMPL)
    on, off = solve(prob, True, **kw), solve(prob, False, **kw)
    assert speculated(on, off) > 0  # (the path ran)
    assert on[0].num_successful_steps > 0
    same_to_round_off(on, off)


# (a start 40 times further from the generating scene than the default, where Gauss-Newton steps of radius 1e4 overshoot:
#  the oracle's outcomes are 1 0 0 0 0 1 1 1 1 1)
REJECT = dict(point_dof=3, initial_trust_region_radius=1e4, max_num_iterations=10, **NO_TOL, **IMPL)


def test_rejected_steps():
    """a start from which LM rejects steps and accepts again: a rejected speculation leaves the current linearisation
    intact, the step after a rejection takes the trial cost, speculation resumes after the next acceptance"""
    from oracle import oracle
    prob = problem(56, perturb=40.0)
    o = abi.default_options(use_inner_iterations=0, **REJECT)
    t_o = abi.attach_trace(o, REJECT["max_num_iterations"])
    ref = prob.copy()
    st_o, s_o = oracle.solve(ref, o)
    assert st_o == 0
    out = t_o[:s_o.num_iterations, 3]
    rej = np.flatnonzero(out == 0.0)
    assert rej.size > 0 and (out[rej[0]:] == 1.0).any(), out  # a rejection, an acceptance after it
    on, off = solve(prob, True, **REJECT), solve(prob, False, **REJECT)
    same_to_round_off(on, off)
    n = on[0].num_iterations
    assert np.array_equal(on[2][:n, 3], out)
    # every trial step speculates but the one right after each rejection
    after_reject = int(np.count_nonzero(out[:-1] != 1.0))
    assert speculated(on, off) == n - after_reject
    # ... and a rejected speculation is a linearize the old sequence does not have
    wasted = int(np.count_nonzero((out != 1.0) & np.concatenate([[True], out[:-1] == 1.0])))
    assert launches(on[0], "linearize") == launches(off[0], "linearize") + wasted
    # the device against the oracle (the bounds of tests/test_gpu_parity.py, assert_same_solution)
    s_d, a = on[0], on[1]
    assert abs(s_d.initial_cost - s_o.initial_cost) <= 1e-12 * s_o.initial_cost
    assert abs(s_d.final_cost - s_o.final_cost) <= 1e-9 * s_o.final_cost
    assert abs(s_d.final_rmse - s_o.final_rmse) <= 1e-9
    assert s_d.num_iterations == s_o.num_iterations and s_d.num_successful_steps == s_o.num_successful_steps
    scale = 100.0
    assert np.abs(a.extrinsics - ref.extrinsics).max() <= 1e-6 * scale
    assert np.abs(a.points - ref.points).max() <= 1e-6 * scale
    assert np.abs(a.intrinsics - ref.intrinsics).max() <= 1e-6 * max(1.0, np.abs(ref.intrinsics).max())


def test_launch_accounting():
    """K accepted steps: K trial-cost launches less, as many linearize launches"""
    K = 5
    prob = problem(11)
    kw = dict(point_dof=3, max_num_iterations=K, **NO_TOL, **IMPL)
    on, off = solve(prob, True, **kw), solve(prob, False, **kw)
    assert on[0].num_iterations == K and on[0].num_successful_steps == K
    assert launches(off[0], "update_cost") - launches(on[0], "update_cost") == K
    assert launches(on[0], "linearize") == launches(off[0], "linearize")
    i = abi.KERNEL_CLASS_NAMES.index("linearize")
    assert on[0].kernel_seconds[i] > 0.0  # (the speculative launch is timed in its class)


def shared_intrinsics_problem():
    return synth.make_problem(40, 3000, 16000, seed=21, scene="ring", spread=0.5, shared_group_size=8)


UNTOUCHED = {
    "inner_iterations": (lambda: problem(11), dict(point_dof=3, use_inner_iterations=1, max_num_iterations=4, **IMPL)),
    "explicit": (lambda: problem(11), dict(point_dof=3, linear_solver_type=abi.ITERATIVE_SCHUR, schur_mode=abi.SCHUR_EXPLICIT)),
    "sparse_schur": (lambda: problem(11), dict(point_dof=3, linear_solver_type=abi.SPARSE_SCHUR, max_num_iterations=4)),
    "shared_intrinsics": (shared_intrinsics_problem, dict(point_dof=3, **IMPL)),
    "fp32": (lambda: problem(11), dict(point_dof=3, residual_precision=32, **IMPL)),
}


@pytest.mark.parametrize("name", sorted(UNTOUCHED))
def test_untouched_paths_stay_bit_for_bit(name):
    make, kw = UNTOUCHED[name]
    prob = make()
    on, off = solve(prob, True, **dict(kw)), solve(prob, False, **dict(kw))
    same_bits(on, off)


def _handle(prob, o):
    """(Solver.download writes into the problem the handle was made from: Solver.problem)"""
    return lib.Solver(prob.copy(), o, 0, 1)


def test_handle_life_cycle():
    """solve (an odd number of swaps), reset, solve, evaluate, download on one handle against fresh handles"""
    prob = problem(11)
    kw = dict(point_dof=3, use_inner_iterations=0, **NO_TOL, **IMPL)
    o3, o4 = abi.default_options(max_num_iterations=3, **kw), abi.default_options(max_num_iterations=4, **kw)
    with env(True):
        s = _handle(prob, o3)
        try:
            assert s.operator_info()["speculative_linearize"]
            st, a = s.solve(o3)
            assert st == 0 and a.num_successful_steps == 3  # three swaps: the second set is the current one
            s.reset()
            st, b = s.solve(o4)
            assert st == 0 and b.num_successful_steps == 4
            got = s.evaluate(3)
            s.download()
            pb = s.problem
        finally:
            s.close()
        f = _handle(prob, o4)
        try:
            st, c = f.solve(o4)
            assert st == 0
            f.download()
            pc = f.problem
        finally:
            f.close()
        assert b.final_cost == c.final_cost and b.final_rmse == c.final_rmse
        assert b.num_linear_solver_iterations == c.num_linear_solver_iterations
        assert np.array_equal(pb.points, pc.points) and np.array_equal(pb.extrinsics, pc.extrinsics)
        assert np.array_equal(pb.intrinsics, pc.intrinsics)
        g = _handle(pb, o4)  # a fresh handle at the parameters the first one ended on
        try:
            want = g.evaluate(3)
        finally:
            g.close()
        assert len(got) == len(want)
        for x, y in zip(got, want):
            if isinstance(x, np.ndarray):
                assert np.array_equal(x, y)
            else:
                assert x == y
    with env(False):
        h = _handle(prob, o3)
        try:
            assert not h.operator_info()["speculative_linearize"]
        finally:
            h.close()


def test_run_to_run():
    prob = problem(11)
    kw = dict(point_dof=4, **LOSSES["huber"], **IMPL)
    same_bits(solve(prob, True, **kw), solve(prob, True, **kw))
