"""-m gpu: back-substitution from the per-track sums of the PCG solve's products (kernels.h, back_combine_kernel).

On a matrix-free LM iteration of the one-sweep product every product of the PCG solve also stores, per track,
s_k = sum_i Jp_i^T (A_i p_k); with y_c = sum_k alpha_k p_k the vector W^T y_c that back_substitute_kernel sweeps the
observations for is sum_k alpha_k s_k, and the model cost change follows from y_c.g_c, the residual PCG ended with and
sum_tracks c^T V_d^-1 c.  TMI_BA_BACKSUB_FROM_PRODUCTS=0 keeps the sweep.

Every case solves the same problem with the switch on and off and runs the CPU oracle with the same options: identical
iteration, step and PCG counts and step outcomes; final cost, parameters and the model cost change of every iteration
within a bound that comes from the sweep path's own deviation from the oracle, measured on an MI355X per case --

    relative deviation of the sweep path (switch off) from the oracle
    case          parameters after one LM iteration   final cost   model cost change (largest over the iterations)
    shapes             2.368e-14   1.135e-15   5.329e-14
    compact            1.032e-14   3.760e-16   7.051e-12
    full_planes        1.161e-14   0           2.574e-12
    huber              3.731e-13   2.603e-16   1.710e-09
    rejected           6.029e-11   4.822e-14   2.072e-10
    one_pcg_iteration  1.889e-14   5.639e-16   2.478e-13
    (one run; SWEEP_DEVIATION below and profiles/backsub_from_products_summary.md hold the same figures.  The new path
    against the oracle in that run: parameters 2.368e-14 1.126e-14 1.267e-14 3.715e-13 6.029e-11 1.877e-14, cost
    5.677e-16 1.880e-16 1.880e-16 7.808e-16 4.803e-14 3.759e-16, model cost change 5.262e-14 7.437e-12 3.229e-12 1.105e-09
    2.074e-10 3.972e-13; the two device paths against each other: parameters <= 1.546e-13, cost <= 5.677e-16, model
    cost change <= 6.042e-10)

-- the new path is allowed ten times that against the oracle (the margin is for the other summation order over k), and
the same bound holds between the two device paths.  A deviation of zero (the oracle's own bits) is taken as one unit of
fp64 round-off, 2.2e-16, before the factor.

Where the path cannot serve a solve (longer than the nine planes, a residual-reset iteration, several ranks, the
IDENTITY preconditioner) the sweep
runs and the results are bit for bit those of the switch off; operator_info says which LM iterations took the path."""
import functools
import os

import numpy as np
import pytest

from theiasfm_amd import abi, dist, lib, synth

pytestmark = pytest.mark.gpu

IMPL = dict(linear_solver_type=abi.ITERATIVE_SCHUR, schur_mode=abi.SCHUR_IMPLICIT)
SWITCH = "TMI_BA_BACKSUB_FROM_PRODUCTS"
ENV = (SWITCH, "TMI_BA_MF_ONE_SWEEP", "TMI_BA_COMPACT_PLANES", "TMI_BA_COMPACT_ROBUST", "TMI_BA_PCG_SPECULATE")
NO_TOL = dict(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
EPS = 2.2e-16

# measured on an MI355X (see the docstring): relative deviation of the sweep path from the oracle,
# (parameters after one LM iteration, final cost, model cost change of any iteration)
SWEEP_DEVIATION = {
    "shapes": (2.368e-14, 1.135e-15, 5.329e-14),
    "compact": (1.032e-14, 3.760e-16, 7.051e-12),
    "full_planes": (1.161e-14, 0.0, 2.574e-12),
    "huber": (3.731e-13, 2.603e-16, 1.710e-09),
    "rejected": (6.029e-11, 4.822e-14, 2.072e-10),
    "one_pcg_iteration": (1.889e-14, 5.639e-16, 2.478e-13),
}


class env:
    """the switch unset (on) or "0" (off); the one-sweep product below its size threshold; further variables as given"""

    def __init__(self, on, **extra):
        self.on, self.extra = on, extra

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in ENV}
        os.environ["TMI_BA_MF_ONE_SWEEP"] = "1"
        if not self.on:
            os.environ[SWITCH] = "0"
        for k, v in self.extra.items():
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def add_tracks(prob, views_of_track, seed):
    """+ one track per entry of views_of_track near the middle of the scene, observed by those views where the current
    parameters project it, with half a pixel of noise (an empty entry: a track without observations)"""
    rng = np.random.default_rng(seed)
    n = len(views_of_track)
    np0, no0 = prob.num_points, prob.num_observations
    centre = (prob.points[:, :3] / prob.points[:, 3:4]).mean(0)
    X = np.concatenate([centre + 0.02 * np.abs(centre).max() * rng.standard_normal((n, 3)), np.ones((n, 1))], 1)
    prob.points = np.ascontiguousarray(np.concatenate([prob.points, X]))
    prob.point_constant = np.concatenate([prob.point_constant, np.zeros(n, np.uint8)])
    cams = np.concatenate([np.asarray(v, np.int32) for v in views_of_track] + [np.zeros(0, np.int32)])
    pts = np.concatenate([np.full(len(v), np0 + i, np.int32) for i, v in enumerate(views_of_track)] + [np.zeros(0, np.int32)])
    prob.obs_camera = np.concatenate([prob.obs_camera, cams])
    prob.obs_point = np.concatenate([prob.obs_point, pts])
    prob.obs_xy = np.ascontiguousarray(np.concatenate([prob.obs_xy, np.zeros((cams.size, 2))]))
    new = np.arange(no0, no0 + cams.size)
    if new.size:
        prob.obs_xy[new] = synth.project(prob, new) + 0.5 * rng.standard_normal((new.size, 2))
    return prob


@functools.lru_cache(maxsize=None)
def _shapes_problem():
    """every unit shape of the product in one problem: tracks of 2, of 9-20, of >= 96 and of > 512 observations, a
    constant point, a track without observations, a view whose intrinsics are all constant (rb_cols < 0 on its block)"""
    nc = 520
    prob = synth.make_problem(nc, 3000, 14000, seed=5, scene="ring", spread=0.5, heavy_tail=0.02)
    rng = np.random.default_rng(6)
    extra = [rng.choice(nc, 2, replace=False) for _ in range(40)]
    extra += [rng.choice(nc, int(k), replace=False) for k in rng.integers(9, 21, 30)]
    extra += [rng.choice(nc, 120, replace=False), np.arange(nc), []]
    prob = add_tracks(prob, extra, 7)
    prob.point_constant[3] = 1
    g = int(prob.camera_group[17])
    assert np.count_nonzero(prob.camera_group == g) == 1
    prob.intrinsics_constant[prob.group_offset[g]:prob.group_offset[g + 1]] = 1
    k = np.bincount(prob.obs_point, minlength=prob.num_points)
    assert (k == 2).any() and ((k >= 9) & (k <= 20)).any() and ((k >= 96) & (k <= 512)).any() and (k > 512).any() and (k == 0).any()
    return prob


@functools.lru_cache(maxsize=None)
def _compact_problem(seed, perturb=1.0):
    """PINHOLE, the default mask, no constant point (compact planes possible); 1, 16 and 64 lanes per track"""
    nc = 100
    prob = synth.make_problem(nc, 4000, 24000, seed=seed, scene="ring", spread=0.5, heavy_tail=0.02, perturb=perturb)
    prob = add_tracks(prob, [np.arange(nc)] * 3, seed + 1)
    k = np.bincount(prob.obs_point, minlength=prob.num_points)
    assert ((k >= 12) & (k < 20)).any() and ((k >= 20) & (k < 96)).any() and (k >= 96).any()
    return prob


def run(prob, on, handle_solves=1, extra_env=None, **kw):
    """-> [(summary, problem, trace, LM iterations that took the path, operator_info after the solve)] of handle_solves
    solves on ONE handle with reset() between them"""
    with env(on, **(extra_env or {})):
        kw.setdefault("max_num_iterations", 6)
        kw.setdefault("use_inner_iterations", 0)
        o = abi.default_options(profile_kernels=1, **kw)
        trace = abi.attach_trace(o, kw["max_num_iterations"])
        h = lib.Solver(prob.copy(), o, 0, 1)
        out = []
        try:
            assert h.operator_info()["back_substitute_from_products"] == on
            for i in range(handle_solves):
                if i:
                    h.reset()
                trace[:] = 0.0
                st, s = h.solve(o)
                assert st == 0, s.message
                h.download()
                info = h.operator_info()
                out.append((s, h.problem.copy(), trace.copy(), info["back_substitute_from_products_iterations"], info))
        finally:
            h.close()
        return out


def run_oracle(prob, **kw):
    from oracle import oracle
    kw.setdefault("max_num_iterations", 6)
    kw.setdefault("use_inner_iterations", 0)
    o = abi.default_options(**kw)
    trace = abi.attach_trace(o, kw["max_num_iterations"])
    p = prob.copy()
    st, s = oracle.solve(p, o)
    assert st == 0
    return s, p, trace, 0


def same_counts_and_outcomes(a, b):
    sa, ta, sb, tb = a[0], a[2], b[0], b[2]
    assert sa.num_iterations == sb.num_iterations
    assert sa.num_successful_steps == sb.num_successful_steps
    assert sa.num_unsuccessful_steps == sb.num_unsuccessful_steps
    assert sa.num_linear_solver_iterations == sb.num_linear_solver_iterations
    n = sa.num_iterations
    assert np.array_equal(ta[:n, 3], tb[:n, 3])
    assert np.array_equal(ta[:n, 6], tb[:n, 6])  # PCG iterations of every LM iteration


def same_bits(a, b, launches=True):
    same_counts_and_outcomes(a, b)
    sa, pa, ta = a[:3]
    sb, pb, tb = b[:3]
    assert sa.initial_cost == sb.initial_cost and sa.final_cost == sb.final_cost and sa.final_rmse == sb.final_rmse
    assert sa.termination == sb.termination
    if launches:
        assert list(sa.kernel_launches) == list(sb.kernel_launches)
    assert np.array_equal(ta, tb, equal_nan=True)
    assert np.array_equal(pa.points, pb.points) and np.array_equal(pa.extrinsics, pb.extrinsics)
    assert np.array_equal(pa.intrinsics, pb.intrinsics)


def param_dev(a, b):
    """largest relative deviation over the three parameter arrays"""
    return max(float(np.abs(x - y).max() / np.abs(y).max())
               for x, y in ((a[1].points, b[1].points), (a[1].extrinsics, b[1].extrinsics), (a[1].intrinsics, b[1].intrinsics)))


def cost_dev(a, b):
    return abs(a[0].final_cost - b[0].final_cost) / abs(b[0].final_cost)


def mcc_dev(a, b):
    n = a[0].num_iterations
    return float(np.abs(a[2][:n, 5] / b[2][:n, 5] - 1.0).max()) if n else 0.0


def check_case(name, prob, compact, env_extra=None, **kw):
    """on / off / oracle for the whole solve and for its first LM iteration; prints every figure before it asserts.
    compact: whether the handle's last linearisation must have written compact planes (operator_info) -- the product,
    and with it the space of the stored sums, differs between the two"""
    one = dict(kw, max_num_iterations=1)
    on1, off1, ref1 = run(prob, True, extra_env=env_extra, **one)[0], run(prob, False, extra_env=env_extra, **one)[0], run_oracle(prob, **one)
    on, off, ref = run(prob, True, extra_env=env_extra, **kw)[0], run(prob, False, extra_env=env_extra, **kw)[0], run_oracle(prob, **kw)
    figures = dict(sweep_param=param_dev(off1, ref1), sweep_cost=cost_dev(off, ref), new_param=param_dev(on1, ref1),
                   new_cost=cost_dev(on, ref), paths_param=param_dev(on1, off1), paths_cost=cost_dev(on, off),
                   paths_mcc=mcc_dev(on, off), new_mcc=mcc_dev(on, ref), sweep_mcc=mcc_dev(off, ref), used=on[3],
                   iterations=on[0].num_iterations, pcg=on[0].num_linear_solver_iterations)
    print(f"[backsub-from-products] {name}: " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))
    assert off[3] == 0 and off1[3] == 0
    assert on[3] > 0 and on1[3] == 1  # (the path ran)
    for r in (on, on1, off, off1):
        assert r[4]["one_sweep_product"] and r[4]["compact_planes"] == compact, r[4]
    same_counts_and_outcomes(on, off)
    same_counts_and_outcomes(on, ref)
    same_counts_and_outcomes(on1, ref1)
    dp, dc, dm = SWEEP_DEVIATION[name]
    bp, bc, bm = 10.0 * max(dp, EPS), 10.0 * max(dc, EPS), 10.0 * max(dm, EPS)
    assert figures["new_param"] <= bp and figures["paths_param"] <= bp
    assert figures["new_cost"] <= bc and figures["paths_cost"] <= bc
    assert figures["new_mcc"] <= bm and figures["paths_mcc"] <= bm
    return on, off


def test_every_unit_shape():
    # (a constant point: the camera block is stored in full, position columns included)
    on, _ = check_case("shapes", _shapes_problem().copy(), False, point_dof=3, **IMPL)
    assert not on[4]["position_columns_formed"]


def test_compact_planes():
    check_case("compact", _compact_problem(11).copy(), True, point_dof=3, **IMPL)


def test_full_planes():
    on, _ = check_case("full_planes", _compact_problem(11).copy(), False, env_extra={"TMI_BA_COMPACT_PLANES": "0"}, point_dof=3, **IMPL)
    assert on[4]["position_columns_formed"]  # (the position columns from Jp, the rest of the block stored)


def test_huber():
    # (compact planes under a robust loss are DeviceView::compact == 2, [C p_n | r^2] per observation: there is no other
    #  compact layout for a loss that is not TRIVIAL, and TMI_BA_COMPACT_ROBUST is cleared by env)
    check_case("huber", _compact_problem(11).copy(), True, point_dof=4, loss_function_type=abi.LOSS_HUBER, robust_loss_width=2.0,
               **IMPL)


# (a start 40 times further from the generating scene than the default, where Gauss-Newton steps of radius 1e4 overshoot)
REJECT = dict(point_dof=3, initial_trust_region_radius=1e4, max_num_iterations=10, **NO_TOL, **IMPL)


def test_rejected_steps_and_reset():
    """a rejected step: the planes are refilled and the step lengths recorded anew within one solve; then two solves on
    one handle with reset() between them give the same bits"""
    prob = _compact_problem(56, perturb=40.0).copy()
    on, off = check_case("rejected", prob, True, **REJECT)
    n = on[0].num_iterations
    out = on[2][:n, 3]
    assert (out == 0.0).any() and (out == 1.0).any(), out
    a, b = run(prob, True, handle_solves=2, **REJECT)
    same_bits(a, b)
    assert a[3] == b[3] == on[3]
    same_bits(a, on)


def test_one_pcg_iteration():
    """max_linear_solver_iterations = 1: y_c = alpha_1 p_1, one plane"""
    check_case("one_pcg_iteration", _compact_problem(11).copy(), True, point_dof=3, max_linear_solver_iterations=1, **IMPL)


FALL_BACK = {  # name -> (options, every PCG solve reaches its tenth iteration)
    # longer than the nine planes: PCG runs into its tenth iteration (a residual reset, other kernels)
    "long_pcg": (dict(eta=1e-14, max_linear_solver_iterations=50), True),
    # ... and a solve that ends ON the residual-reset iteration
    "reset_iteration": (dict(eta=1e-14, max_linear_solver_iterations=10), True),
    # the IDENTITY preconditioner: PCG's recurrence residual is not held close enough to b - S y_c (engine.hip, solve)
    "identity_preconditioner": (dict(preconditioner_type=abi.PRECOND_IDENTITY), False),
}


@pytest.mark.parametrize("name", sorted(FALL_BACK))
def test_fall_back_to_the_sweep(name):
    """the sweep runs wherever the planes do not stand for it -- bit for bit the switch off (the stores of the first
    iteration's products change nothing) -- and the forecast keeps the stores off after the first long solve"""
    prob = _compact_problem(11).copy()
    opts, long_solves = FALL_BACK[name]
    kw = dict(point_dof=3, max_num_iterations=4, **opts, **IMPL)
    on, off = run(prob, True, **kw)[0], run(prob, False, **kw)[0]
    n = on[0].num_iterations
    assert n > 0 and on[0].num_linear_solver_iterations > 0
    if long_solves:
        assert (on[2][:n, 6] >= 10).all(), on[2][:n, 6]
    assert on[3] == 0 and off[3] == 0
    same_bits(on, off)


class EmulatedAllReduce:
    """the all-reduce of tests/test_gpu_sharded.py: the ranks' device buffers summed in rank order on one device"""

    def __init__(self, world):
        import threading

        import torch
        self.torch, self.world = torch, world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.calls = 0

    def hook(self, rank):
        torch = self.torch

        def fn(ptr, count, stream):
            torch.cuda.ExternalStream(stream).synchronize()
            self.slots[rank] = torch.as_tensor(dist._DevArray(ptr, count), device="cuda")
            self.barrier.wait()
            if rank == 0:
                total = self.slots[0].clone()
                for t in self.slots[1:]:
                    total += t
                for t in self.slots:
                    t.copy_(total)
                torch.cuda.synchronize()
                self.calls += 1
            self.barrier.wait()
            return 0
        return fn


def _two_ranks(prob, on, **kw):
    """an emulated two-rank solve (tests/test_gpu_sharded.py: two handles in threads on one device, the all-reduce hook
    sums their buffers in rank order) -> per rank (status, summary, downloaded problem, operator_info after the solve)"""
    import threading

    import torch
    torch.cuda.init()
    world = 2
    with env(on):
        o = abi.default_options(**kw)
        emu = EmulatedAllReduce(world)
        solvers = []
        for r in range(world):
            sv = lib.Solver(prob.copy(), o, rank=r, world=world)
            sv.set_allreduce(emu.hook(r))
            solvers.append(sv)
        results = [None] * world

        def work(r):
            results[r] = solvers[r].solve(o)

        threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        try:
            assert all(not t.is_alive() for t in threads) and emu.calls > 0
            return [(results[r][0], results[r][1], solvers[r].download().copy(), solvers[r].operator_info()) for r in range(world)]
        finally:
            for sv in solvers:
                sv.close()


def test_two_ranks_keep_the_sweep():
    """two ranks solving with the switch on: the matrix-free one-sweep product runs on both, no LM iteration takes the path
    on either, and every rank ends on the bits of the switch off"""
    prob = _compact_problem(11).copy()
    kw = dict(point_dof=3, max_num_iterations=4, use_inner_iterations=0, **IMPL)
    on, off = _two_ranks(prob, True, **kw), _two_ranks(prob, False, **kw)
    for (st_a, a, pa, ia), (st_b, b, pb, ib) in zip(on, off):
        assert st_a == 0 and st_b == 0 and a.num_iterations == 4 and a.num_linear_solver_iterations > 0
        assert ia["one_sweep_product"] and ib["one_sweep_product"]
        assert not ia["back_substitute_from_products"] and ia["back_substitute_from_products_iterations"] == 0
        assert ib["back_substitute_from_products_iterations"] == 0
        assert a.num_iterations == b.num_iterations and a.num_successful_steps == b.num_successful_steps
        assert a.num_linear_solver_iterations == b.num_linear_solver_iterations
        assert a.initial_cost == b.initial_cost and a.final_cost == b.final_cost and a.final_rmse == b.final_rmse
        assert np.array_equal(pa.points, pb.points) and np.array_equal(pa.extrinsics, pb.extrinsics)
        assert np.array_equal(pa.intrinsics, pb.intrinsics)


def test_speculative_pcg_enqueue():
    """a PCG step enqueued ahead of the stopping test returns at once when the test held and must leave the planes and the
    recorded step lengths alone: the same bits with TMI_BA_PCG_SPECULATE on and off"""
    prob = _compact_problem(11).copy()
    kw = dict(point_dof=3, **IMPL)
    a = run(prob, True, **kw)[0]
    b = run(prob, True, extra_env={"TMI_BA_PCG_SPECULATE": "0"}, **kw)[0]
    assert a[3] > 0 and a[3] == b[3]
    same_bits(a, b, launches=False)  # (a speculated step that found PCG stopped is not counted, but the classes may differ)


def test_run_to_run():
    prob = _shapes_problem().copy()
    kw = dict(point_dof=3, **IMPL)
    same_bits(run(prob, True, **kw)[0], run(prob, True, **kw)[0])
