"""The case table and the comparator of tests/test_gpu_resident_sequences.py, checked without a GPU: the matrix is
complete, the comparator leaves out nothing but times, and the CPU oracle confirms that the configurations really are
different solves on the test problems (so "another solve ran before" is another solve)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_sequence_cases as cases  # noqa: E402
from oracle import oracle  # noqa: E402
from theiasfm_amd import abi  # noqa: E402


def test_configurations_are_the_ones_asked_for():
    o = {k: cases.options("small", k) for k in cases.CONFIGS}
    for k in ("a", "b", "c", "e", "f0", "f1", "g"):
        assert o[k].linear_solver_type == abi.ITERATIVE_SCHUR
    assert o["a"].loss_function_type == abi.LOSS_TRIVIAL and o["a"].preconditioner_type == abi.PRECOND_JACOBI
    assert o["a"].jacobi_scaling == 1 and o["a"].use_inner_iterations == 0
    assert o["b"].loss_function_type == abi.LOSS_HUBER and o["b"].preconditioner_type == abi.PRECOND_JACOBI
    assert o["c"].preconditioner_type == abi.PRECOND_SCHUR_JACOBI and o["c"].use_inner_iterations == 1
    assert o["d"].linear_solver_type in (abi.SPARSE_SCHUR, abi.DENSE_SCHUR)
    assert o["e"].jacobi_scaling == 0 and o["e"].loss_function_type == abi.LOSS_TRIVIAL
    assert (o["f0"].max_num_iterations, o["f1"].max_num_iterations) == (0, 1)
    assert o["g"].preconditioner_type == abi.PRECOND_SCHUR_JACOBI_PARAMETER_BLOCKS
    assert 0 < o["g"].max_linear_solver_iterations <= 5
    assert all(0 <= v.max_num_iterations <= 4 for v in o.values())
    assert cases.TRACE_ROWS > cases.MAX_ITERATIONS
    # e and the f's are a with one field changed
    for k, field in (("e", "jacobi_scaling"), ("f0", "max_num_iterations"), ("f1", "max_num_iterations")):
        for name, _ in abi.COptions._fields_:
            if name not in (field, "iteration_trace"):
                assert getattr(o[k], name) == getattr(o["a"], name), (k, name)


def test_matrix_holds_every_ordered_pair_on_every_admissible_mode():
    m = cases.matrix()
    assert len(m) == len(set(m))
    assert set(cases.MODES) == {"implicit", "explicit", "auto"}
    assert cases.MODES == {"implicit": abi.SCHUR_IMPLICIT, "explicit": abi.SCHUR_EXPLICIT, "auto": abi.SCHUR_AUTO}
    for mode in cases.MODES:
        # an exact solver on a handle created for the implicit operator is refused by tmi_ba_solver_solve; everything
        # else runs everywhere
        want = set(cases.CONFIGS) - ({"d"} if mode == "implicit" else set())
        assert set(cases.admissible(mode)) == want
        for p in cases.PROBLEMS:
            got = {(x, y) for (pp, mm, x, y) in m if pp == p and mm == mode}
            assert got == set(itertools.product(want, want))
    assert len(m) == len(cases.PROBLEMS) * (7 * 7 + 8 * 8 + 8 * 8)
    for p, mode, x, y in cases.switch_cases():
        assert (p, mode, x, y) in m
    pairs = {(x, y) for _, mode, x, y in cases.switch_cases() if mode == "auto"}
    assert pairs == {("a", "d"), ("d", "a"), ("a", "b"), ("b", "a"), ("c", "a"), ("f0", "a"), ("f1", "a"), ("a", "g")}


def test_problems_are_what_the_paths_need():
    P = cases.problem("pinhole")
    assert P.num_observations >= cases.ONE_SWEEP_MIN_OBSERVATIONS  # the one-sweep product's gate (engine.hip)
    for name in ("pinhole", "small", "dof4"):
        P = cases.problem(name)
        assert (P.group_model == abi.PINHOLE).all() and P.num_groups == P.num_cameras
        K = P.intrinsics.reshape(-1, 7)
        assert (K[:, 1] == 1.0).all() and (K[:, 2] == 0.0).all()  # unit aspect, zero skew: compact planes possible
        mask = abi.intrinsics_constant_mask(abi.PINHOLE, abi.INTRINSICS_DEFAULT)
        assert (P.intrinsics_constant.reshape(-1, 7) == mask).all()
    assert cases.PROBLEMS["dof4"][0] == 4 and cases.PROBLEMS["pinhole"][0] == 3
    M = cases.problem("mixed")
    assert len(set(M.group_model.tolist())) >= 2 and M.num_groups < M.num_cameras  # mixed models, shared groups
    # a private copy every time
    assert cases.problem("small").points is not cases.problem("small").points
    Q = cases.perturbed(cases.problem("small"), aspect_group=0)
    assert Q.intrinsics[Q.group_offset[0] + 1] != 1.0
    assert (cases.perturbed(cases.problem("small")).intrinsics.reshape(-1, 7)[:, 1] == 1.0).all()


def test_create_key_separates_what_create_reads():
    keys = {c: cases.create_key("small", c, "auto") for c in cases.CONFIGS}
    assert keys["a"] == keys["b"] == keys["e"] == keys["f0"] == keys["f1"]
    assert len({keys["a"], keys["c"], keys["d"], keys["g"]}) == 4
    assert cases.create_key("small", "a", "auto") != cases.create_key("small", "a", "implicit")
    assert cases.create_key("small", "a", "auto") != cases.create_key("dof4", "a", "auto")
    # the fields left out of the key are solve-time fields: the ones tmi_ba_solver_create never reads
    assert set(cases.CREATE_FIELDS) == {"linear_solver_type", "preconditioner_type", "point_dof", "device",
                                        "residual_precision", "schur_mode", "visibility_clustering_type"}


def _result(**changes):
    s = abi.CSummary()
    s.initial_cost, s.final_cost, s.num_iterations = 10.0, 1.0, 3
    trace = np.full((cases.TRACE_ROWS, abi.TRACE_STRIDE), np.nan)
    trace[:3] = np.arange(24.0).reshape(3, 8)
    P = cases.problem("small")
    for name, value in changes.items():
        if name == "trace":
            trace[value] += 1.0
        elif name in ("extrinsics", "intrinsics", "points"):
            getattr(P, name).reshape(-1)[value] = np.nextafter(getattr(P, name).reshape(-1)[value], np.inf)
        elif name == "status":
            pass
        elif isinstance(getattr(s, name), C.Array):
            getattr(s, name)[value[0]] = value[1]
        else:
            setattr(s, name, value)
    return cases.Result(changes.get("status", 0), s, trace, P)


def test_comparator_excludes_only_time_columns():
    assert cases.SUMMARY_TIME_FIELDS == ("setup_time_in_seconds", "solve_time_in_seconds", "kernel_seconds")
    assert cases.TRACE_TIME_COLUMNS == ()
    names = [n for n, _ in abi.CSummary._fields_]
    assert set(cases.SUMMARY_FIELDS) | set(cases.SUMMARY_TIME_FIELDS) == set(names)
    assert all("time" not in n and "seconds" not in n for n in cases.SUMMARY_FIELDS)
    assert all("time" in n or "seconds" in n for n in cases.SUMMARY_TIME_FIELDS)
    assert cases.TRACE_COLUMNS == tuple(range(abi.TRACE_STRIDE))
    assert not any("time" in n or "seconds" in n for n in abi.TRACE_FIELDS)
    base = _result()
    assert cases.differences(_result(), base) == []
    # the three time fields are ignored ...
    assert cases.differences(_result(setup_time_in_seconds=1.0, solve_time_in_seconds=2.0, kernel_seconds=(3, 0.5)), base) == []
    # ... and a change of one bit anywhere else is seen
    one = {"success": 1, "initial_cost": np.nextafter(10.0, 11.0), "final_cost": np.nextafter(1.0, 2.0), "status": 7,
           "termination": 1, "num_iterations": 4, "num_successful_steps": 1, "num_unsuccessful_steps": 1,
           "num_linear_solver_iterations": 1, "final_rmse": 5e-324, "initial_rmse": 5e-324, "num_reduced_blocks": 1,
           "reduced_block_dim": 9, "num_schur_blocks": 1, "num_schur_pairs": 1, "num_inner_iteration_steps": 1,
           "num_matrix_free_iterations": 1, "kernel_launches": (11, 1), "message": b"x",
           "effective_preconditioner_type": 2}
    assert set(one) | {"status"} == set(cases.SUMMARY_FIELDS) | {"status"}
    for name, value in one.items():
        assert cases.differences(_result(**{name: value}), base), name
    for col in range(abi.TRACE_STRIDE):
        assert cases.differences(_result(trace=(1, col)), base), col
    for name in ("extrinsics", "intrinsics", "points"):
        assert cases.differences(_result(**{name: -1}), base) == [f"downloaded {name}"]
    # bits, not values: -0.0 against 0.0 differs, NaN against the same NaN does not
    assert cases.differences(_result(final_cost=-0.0), _result(final_cost=0.0))
    assert cases.differences(_result(final_cost=float("nan")), _result(final_cost=float("nan"))) == []


@pytest.mark.parametrize("problem", ["small", "mixed", "dof4"])
def test_oracle_runs_distinct_trajectories(problem):
    """The CPU LM on the small problems: every configuration ends normally, and any two of them differ in final cost,
    iteration count or trace -- the condition under which a pair (x, y), x != y, of the GPU matrix tests anything."""
    got = {}
    for config in cases.CONFIGS:
        o = cases.options(problem, config)
        trace = abi.attach_trace(o, cases.TRACE_ROWS)
        P = cases.problem(problem)
        st, s = oracle.solve(P, o)
        assert st == 0 and s.termination in (0, 1), config
        got[config] = cases.Result(st, s, trace, P)
    assert got["f0"].values["num_iterations"] == 0 and got["f1"].values["num_iterations"] == 1
    assert got["c"].values["num_inner_iteration_steps"] > 0
    assert got["d"].values["num_linear_solver_iterations"] == 0 < got["a"].values["num_linear_solver_iterations"]
    for x, y in itertools.combinations(cases.CONFIGS, 2):
        assert cases.trajectories_differ(got[x], got[y]), (x, y)
