"""-m gpu: a resident solver handle (tmi_ba_solver_create, then solve / reset / set_parameters / the side kernels) is
reused with DIFFERENT options from one solve to the next -- compact or full planes, the matrix-free product or a formed
S, PCG or the dense Cholesky, inner iterations, a robust loss -- and much of its state outlives a solve.  The engine is
bit-reproducible, so the property is exact: whatever happened earlier on a handle changes no bit of a later solve.

The reference of every comparison is a FRESH handle, created with the same arguments, that ran the later solve only;
never the reused handle itself.  Compared: the status, every field of the summary and every column of the iteration
trace that is not a time (resident_sequence_cases.SUMMARY_TIME_FIELDS: setup_time_in_seconds, solve_time_in_seconds,
kernel_seconds; the trace has no time column), and the downloaded extrinsics, intrinsics and points as bytes.
Every case is deterministic and runs once."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_sequence_cases as cases  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu


def run_solve(handle, o):
    trace = abi.attach_trace(o, cases.TRACE_ROWS)
    st, s = handle.solve(o)
    return cases.Result(st, s, trace, handle.download())


_references = {}


def reference(problem, mode, x, y, start=None, tag=None):
    """(Result, operator_info) of solve(y) on a fresh handle created with x's options from `start` (default: the
    problem as built).  Computed once per (what create reads from x's options, y[, tag]) and shared."""
    key = (cases.create_key(problem, x, mode), y, tag)
    if start is not None and tag is None:
        key = None
    if key is None or key not in _references:
        h = lib.Solver(cases.problem(problem) if start is None else start.copy(), cases.options(problem, x, mode))
        try:
            got = (run_solve(h, cases.options(problem, y, mode)), h.operator_info())
        finally:
            h.close()
        if key is None:
            return got
        _references[key] = got
    return _references[key]


def assert_equal(got, ref, what):
    diff = cases.differences(got, ref)
    assert not diff, f"{what}: differs from a fresh handle in\n  " + "\n  ".join(diff)


# ---- 1. the transition matrix ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,mode,x,y", cases.matrix(), ids=lambda v: str(v))
def test_solve_after_another_solve_and_reset(problem, mode, x, y):
    ref, _ = reference(problem, mode, x, y)
    h = lib.Solver(cases.problem(problem), cases.options(problem, x, mode))
    try:
        first = run_solve(h, cases.options(problem, x, mode))
        h.reset()
        got = run_solve(h, cases.options(problem, y, mode))
    finally:
        h.close()
    assert first.status == 0
    assert_equal(got, ref, f"{problem}/{mode}: solve({x}); reset(); solve({y})")


MODE_CONFIGS = [(p, m, c) for p in cases.PROBLEMS for m in cases.MODES for c in cases.admissible(m)]


@pytest.mark.parametrize("problem,mode,config", MODE_CONFIGS, ids=lambda v: str(v))
def test_reference_takes_the_intended_path(problem, mode, config):
    """The matrix is not vacuous: every configuration's reference ends normally and ran the kernels it stands for."""
    r, info = reference(problem, mode, config, config)
    print(problem, mode, config, r.values, r.launches, info)
    assert r.status == 0 and r.values["termination"] in (0, 1)
    assert info["implicit"] == (mode == "implicit") and info["adaptive"] == (mode == "auto" and config in cases.ITERATIVE)
    its = r.values["num_iterations"]
    free_its = r.values["num_matrix_free_iterations"]
    # handles that can run matrix-free iterations: schur_mode implicit, and auto where it chooses per iteration
    # (created for an iterative solver, no shared intrinsics blocks)
    can_be_free = mode == "implicit" or (mode == "auto" and config in cases.ITERATIVE and problem != "mixed")
    one_sweep = can_be_free and problem in cases.ONE_SWEEP
    # (resident_sequence_cases.ONE_SWEEP_MIN_OBSERVATIONS: the size from which mf_ok and direct_ok are on)
    assert info["one_sweep_product"] == one_sweep and info["direct_camera_side"] == one_sweep
    if config == "f0":
        assert its == 0 and r.values["termination"] == 1
        return
    assert its >= 1
    if config == "f1":
        assert its == 1 and r.values["termination"] == 1
    if config in cases.ITERATIVE:
        assert r.values["num_linear_solver_iterations"] > 0 and r.launches["cholesky"] == 0
        assert r.launches["spmv"] > 0 or r.launches["pcg_vector"] > 0
        if mode == "implicit":
            assert free_its == its and r.launches["schur_offdiag"] == 0
        elif can_be_free:
            # auto: the first iteration is matrix-free (no PCG length to forecast from yet), later ones by their forecast
            assert free_its >= 1 and (r.launches["schur_offdiag"] == 0) == (free_its == its)
        else:
            assert free_its == 0 and r.launches["schur_offdiag"] > 0
    else:
        assert r.launches["cholesky"] > 0 and r.launches["schur_offdiag"] > 0
        assert r.values["num_linear_solver_iterations"] == 0 and free_its == 0
    if config == "c":
        assert r.values["num_inner_iteration_steps"] > 0
    else:
        assert r.values["num_inner_iteration_steps"] == 0
    if config == "g":
        assert r.summary["effective_preconditioner_type"] == abi.PRECOND_SCHUR_JACOBI_PARAMETER_BLOCKS
    # compact planes (what the LAST linearisation of the solve wrote): the one-sweep handles of the all-PINHOLE,
    # unit-aspect problem wherever the next iteration is expected to run matrix-free; nowhere else
    if not one_sweep:
        assert not info["compact_planes"]
    elif config in ("a", "e", "f1", "g"):
        last_pcg = r.trace[its - 1, abi.TRACE_FIELDS.index("linear_iterations")]
        assert info["compact_planes"] == (mode == "implicit" or last_pcg <= info["break_even"])


@pytest.mark.parametrize("problem", list(cases.PROBLEMS))
@pytest.mark.parametrize("mode", list(cases.MODES))
def test_references_of_different_configurations_differ(problem, mode):
    """For x != y "something else happened before" must be something else: the two solves, each on a fresh handle
    created with x's options, differ in final cost, iteration count or trace."""
    same = []
    for x in cases.admissible(mode):
        for y in cases.admissible(mode):
            if x != y and not cases.trajectories_differ(reference(problem, mode, x, x)[0], reference(problem, mode, x, y)[0]):
                same.append((x, y))
    assert not same


# ---- 2. sequences without a reset -----------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,mode,x,y", cases.switch_cases(), ids=lambda v: str(v))
def test_solve_after_another_solve_without_reset(problem, mode, x, y):
    h = lib.Solver(cases.problem(problem), cases.options(problem, x, mode))
    try:
        first = run_solve(h, cases.options(problem, x, mode))
        mid = h.download().copy()
        got = run_solve(h, cases.options(problem, y, mode))
    finally:
        h.close()
    assert first.status == 0
    ref, _ = reference(problem, mode, x, y, start=mid)
    assert_equal(got, ref, f"{problem}/{mode}: solve({x}); solve({y})")


@pytest.mark.parametrize("aspect", [False, True], ids=["unit_aspect", "aspect_1.01"])
@pytest.mark.parametrize("problem,mode,x,y", cases.switch_cases(), ids=lambda v: str(v))
def test_solve_after_set_parameters(problem, mode, x, y, aspect):
    """solve(x); set_parameters(Q); solve(y) against a fresh handle created on Q.  With `aspect` one group of Q has an
    aspect ratio of 1.01: compact planes are decided from the parameters a solve starts from, so the handle must leave
    the compact path as a fresh one does."""
    Q = cases.perturbed(cases.problem(problem), aspect_group=0 if aspect else None)
    h = lib.Solver(cases.problem(problem), cases.options(problem, x, mode))
    try:
        first = run_solve(h, cases.options(problem, x, mode))
        info_first = h.operator_info()
        h.set_parameters(Q.copy())
        got = run_solve(h, cases.options(problem, y, mode))
        info = h.operator_info()
    finally:
        h.close()
    assert first.status == 0
    ref, info_ref = reference(problem, mode, x, y, start=Q, tag=("Q", aspect))
    assert_equal(got, ref, f"{problem}/{mode}: solve({x}); set_parameters(Q); solve({y})")
    assert info["compact_planes"] == info_ref["compact_planes"]
    if aspect:
        assert not info["compact_planes"]
        if problem in cases.ONE_SWEEP and mode == "implicit" and x == "a":
            assert info_first["compact_planes"]  # (it did leave the path: the solve before took it)
    elif problem in cases.ONE_SWEEP and mode == "implicit" and y in ("a", "g"):
        assert info["compact_planes"]


@pytest.mark.parametrize("problem", list(cases.PROBLEMS))
def test_iterative_exact_iterative_on_an_auto_handle(problem):
    """Three solves in a row on one schur_mode-auto handle: after an iteration has formed S and run the Cholesky the
    handle still matches a fresh one, and so does the exact solve that follows matrix-free iterations."""
    h = lib.Solver(cases.problem(problem), cases.options(problem, "a", "auto"))
    try:
        first = run_solve(h, cases.options(problem, "a", "auto"))
        p1 = h.download().copy()
        second = run_solve(h, cases.options(problem, "d", "auto"))
        p2 = h.download().copy()
        third = run_solve(h, cases.options(problem, "a", "auto"))
    finally:
        h.close()
    assert first.status == 0 and second.launches["cholesky"] > 0
    assert_equal(second, reference(problem, "auto", "a", "d", start=p1)[0], f"{problem}: solve(a); solve(d)")
    assert_equal(third, reference(problem, "auto", "a", "a", start=p2)[0], f"{problem}: solve(a); solve(d); solve(a)")


# ---- 3. calls between two solves --------------------------------------------------------------------------------------
def _read_only_calls(h, problem):
    h.evaluate(cases.PROBLEMS[problem][0])
    h.operator_info()
    h.structure_checksums()
    h.download()
    # (they take the resident parameters and return flags / a selection to the caller: nothing of the handle changes)
    h.filter_outlier_tracks(4.0, 2.0)
    h.select_good_tracks(10, 100, 100)


@pytest.mark.parametrize("problem,mode,x,y", [(p, m, x, y) for p in cases.PROBLEMS for m in cases.MODES
                                              for x, y in (("a", "a"), ("a", "b"), ("b", "a"), ("d", "a"), ("a", "d"))
                                              if x in cases.admissible(m) and y in cases.admissible(m)],
                         ids=lambda v: str(v))
def test_read_only_calls_between_two_solves(problem, mode, x, y):
    """evaluate, operator_info, structure_checksums, download (and the two track calls that only report) between
    solve(x) and reset(); solve(y) change nothing."""
    h = lib.Solver(cases.problem(problem), cases.options(problem, x, mode))
    try:
        first = run_solve(h, cases.options(problem, x, mode))
        _read_only_calls(h, problem)
        h.reset()
        got = run_solve(h, cases.options(problem, y, mode))
    finally:
        h.close()
    assert first.status == 0
    assert_equal(got, reference(problem, mode, x, y)[0], f"{problem}/{mode}: solve({x}); read-only calls; reset(); solve({y})")


@pytest.mark.parametrize("problem,mode,y", MODE_CONFIGS, ids=lambda v: str(v))
def test_evaluate_before_the_first_solve(problem, mode, y):
    """evaluate() right after create leaves its own plane state (full planes, no per-track sums) behind: the first
    solve must start as on a handle that was never evaluated."""
    h = lib.Solver(cases.problem(problem), cases.options(problem, y, mode))
    try:
        h.evaluate(cases.PROBLEMS[problem][0])
        got = run_solve(h, cases.options(problem, y, mode))
    finally:
        h.close()
    assert_equal(got, reference(problem, mode, y, y)[0], f"{problem}/{mode}: evaluate(); solve({y})")


def _adjust_tracks(h, problem):
    h.adjust_tracks(abi.default_options(point_dof=cases.PROBLEMS[problem][0], max_num_iterations=5))


def _adjust_views(h, problem):
    h.adjust_views(abi.default_options(point_dof=cases.PROBLEMS[problem][0], max_num_iterations=5))


def _estimate_tracks(h, problem):
    h.estimate_tracks(abi.track_estimator_options(), abi.default_options(point_dof=cases.PROBLEMS[problem][0]))


STATE_CHANGING = {"adjust_tracks": _adjust_tracks, "adjust_views": _adjust_views, "estimate_tracks": _estimate_tracks}


@pytest.mark.parametrize("call", list(STATE_CHANGING))
@pytest.mark.parametrize("problem,mode,x,y", [(p, m, x, y) for p in cases.PROBLEMS for m in cases.MODES
                                              for x, y in (("a", "a"), ("a", "d"), ("d", "a"), ("b", "a"))
                                              if x in cases.admissible(m) and y in cases.admissible(m)],
                         ids=lambda v: str(v))
def test_state_changing_calls_between_two_solves(problem, mode, x, y, call):
    """adjust_tracks, adjust_views and estimate_tracks move the resident points / cameras.  solve(x); the call;
    solve(y) without a reset equals a fresh handle created from download() taken after the call: download() carries
    everything these calls change (parameters only -- the flags of filter_outlier_tracks and the selection of
    select_good_tracks go to the caller and are not kept in the handle, which is why those two sit with the read-only
    calls).  The sequence that ends in reset() must not see the call at all."""
    h = lib.Solver(cases.problem(problem), cases.options(problem, x, mode))
    try:
        first = run_solve(h, cases.options(problem, x, mode))
        STATE_CHANGING[call](h, problem)
        mid = h.download().copy()
        got = run_solve(h, cases.options(problem, y, mode))
        h.reset()
        again = run_solve(h, cases.options(problem, y, mode))
    finally:
        h.close()
    assert first.status == 0
    assert_equal(got, reference(problem, mode, x, y, start=mid)[0], f"{problem}/{mode}: solve({x}); {call}; solve({y})")
    assert_equal(again, reference(problem, mode, x, y)[0], f"{problem}/{mode}: solve({x}); {call}; solve({y}); reset(); solve({y})")


# ---- 4. create-time options passed again at solve ---------------------------------------------------------------------
def _other(field, mode):
    if field == "schur_mode":
        return [v for v in cases.MODES.values() if v != cases.MODES[mode]]
    return {"residual_precision": [32], "visibility_clustering_type": [abi.SINGLE_LINKAGE], "device": [-1, 0]}[field]


@pytest.mark.parametrize("field", ["schur_mode", "residual_precision", "visibility_clustering_type", "device"])
@pytest.mark.parametrize("mode", list(cases.MODES))
def test_create_time_options_are_ignored_by_solve(mode, field):
    """schur_mode, residual_precision, device and (outside the cluster preconditioners) visibility_clustering_type are
    fixed at tmi_ba_solver_create (theia_mi355_ba.h, tmi_ba_solver_solve): a solve whose options say otherwise gives the
    bits of create's values."""
    ref, _ = reference("pinhole", mode, "a", "a")
    create = cases.options("pinhole", "a", mode)
    if field == "device":
        create.device = 0
    for value in _other(field, mode):
        h = lib.Solver(cases.problem("pinhole"), create)
        try:
            got = run_solve(h, cases.options("pinhole", "a", mode, **{field: value}))
        finally:
            h.close()
        assert_equal(got, ref, f"{mode}: created with {field} = {getattr(create, field)}, solved with {value}")
