"""Cases and comparator of tests/test_gpu_resident_sequences.py: one resident handle, several solves whose options differ.

The property under test needs no tolerance: the engine is bit-reproducible, so whatever happened earlier on a handle
(another solve, a side kernel, a read-only call) may not change one bit of a later solve.  The reference of every
comparison is a FRESH handle that was created alike and ran the later solve only.

This module has no GPU code: tests/test_resident_sequence_cases_cpu.py checks the tables below without one.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from theiasfm_amd import abi, synth

MAX_ITERATIONS = 4
TRACE_ROWS = 8  # > MAX_ITERATIONS: the unused rows must stay NaN on both handles

# ---- solve-time configurations (the letters are the issue's) ---------------------------------------------------------
# Every entry: overrides of abi.default_options(point_dof=<the problem's>, max_num_iterations=MAX_ITERATIONS,
# use_inner_iterations=0).
_ITER = dict(linear_solver_type=abi.ITERATIVE_SCHUR, preconditioner_type=abi.PRECOND_JACOBI)
CONFIGS = {
    # a: the compact-plane path on a matrix-free all-PINHOLE handle
    "a": dict(_ITER),
    # b: a robust loss -- the robust compact instantiation or the full planes, whichever the handle takes
    "b": dict(_ITER, loss_function_type=abi.LOSS_HUBER, robust_loss_width=2.0),
    # c: SCHUR_JACOBI with the inner-iteration sweep after every trust-region step
    "c": dict(linear_solver_type=abi.ITERATIVE_SCHUR, preconditioner_type=abi.PRECOND_SCHUR_JACOBI,
              use_inner_iterations=1),
    # d: an exact solver -- S is formed, the dense Cholesky runs
    "d": dict(linear_solver_type=abi.SPARSE_SCHUR, preconditioner_type=abi.PRECOND_JACOBI),
    # e: a without Jacobi scaling (the three-pass / fast start of a solve is skipped)
    "e": dict(_ITER, jacobi_scaling=0),
    # f0 / f1: the solve ends before / just after the first full linearisation
    "f0": dict(_ITER, max_num_iterations=0),
    "f1": dict(_ITER, max_num_iterations=1),
    # g: Ceres' parameter-block Schur-Jacobi preconditioner, PCG capped low
    "g": dict(linear_solver_type=abi.ITERATIVE_SCHUR, preconditioner_type=abi.PRECOND_SCHUR_JACOBI_PARAMETER_BLOCKS,
              max_linear_solver_iterations=3),
}
ITERATIVE = tuple(k for k, c in CONFIGS.items() if c["linear_solver_type"] == abi.ITERATIVE_SCHUR)
EXACT = tuple(k for k in CONFIGS if k not in ITERATIVE)

MODES = {"implicit": abi.SCHUR_IMPLICIT, "explicit": abi.SCHUR_EXPLICIT, "auto": abi.SCHUR_AUTO}


def admissible(mode: str):
    """Configurations a handle of this schur_mode admits, as the one that creates it and as a later solve.
    tmi_ba_solver_solve refuses an exact solver on a handle created for the implicit operator (s->implicit), and a handle
    created with schur_mode implicit under an exact solver type is not an implicit handle at all."""
    return ITERATIVE if mode == "implicit" else ITERATIVE + EXACT


# ---- problems ----------------------------------------------------------------------------------------------------------
# name -> (point_dof, builder).
# "pinhole": all-PINHOLE, default intrinsics mask, unit aspect, zero skew -- the compact-plane problem.  A handle builds
#   the one-sweep matrix-free product (and with it the direct camera side and the compact planes) from 350 000
#   observations up (engine.hip, build_mf_chunks), so that is its size: the smallest at which those paths are on.
# "small": the same at the lifecycle test's size -- the two-pass matrix-free product, full planes.
ONE_SWEEP_MIN_OBSERVATIONS = 350000


def _pinhole():
    return synth.make_problem(40, 60000, ONE_SWEEP_MIN_OBSERVATIONS, seed=6, scene="ring", spread=0.4)


def _small():
    return synth.make_problem(20, 2500, 12000, seed=6, scene="ring", spread=0.4)


def _mixed():
    # three camera models, every intrinsics group shared by two views: the generic bodies, no compact planes
    return synth.make_problem(12, 1500, 7000, seed=9, scene="ring", spread=0.4, shared_group_size=2,
                              models=[(abi.PINHOLE, 0.4), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.3), (abi.FISHEYE, 0.3)])


def _dof4():
    return synth.make_problem(12, 1500, 7000, seed=11, scene="ring", spread=0.4)


PROBLEMS = {"pinhole": (3, _pinhole), "small": (3, _small), "mixed": (3, _mixed), "dof4": (4, _dof4)}
ONE_SWEEP = ("pinhole",)  # the problems on which a matrix-free handle runs the one-sweep product and compact planes
_problem_cache = {}


def problem(name: str) -> abi.Problem:
    """A private copy: handles keep pointers into the arrays they were created from."""
    if name not in _problem_cache:
        _problem_cache[name] = PROBLEMS[name][1]()
    return _problem_cache[name].copy()


def options(problem_name: str, config: str, mode: str = "auto", **overrides) -> abi.COptions:
    kw = dict(point_dof=PROBLEMS[problem_name][0], max_num_iterations=MAX_ITERATIONS, use_inner_iterations=0,
              schur_mode=MODES[mode])
    kw.update(CONFIGS[config])
    kw.update(overrides)
    return abi.default_options(**kw)


# what tmi_ba_solver_create reads from its options (engine.hip, create): two configurations that agree on these create
# the same handle, so their references can be shared
CREATE_FIELDS = ("linear_solver_type", "preconditioner_type", "point_dof", "device", "residual_precision", "schur_mode",
                 "visibility_clustering_type")


def create_key(problem_name: str, config: str, mode: str):
    o = options(problem_name, config, mode)
    return (problem_name,) + tuple(getattr(o, f) for f in CREATE_FIELDS)


def matrix():
    """Every (problem, mode, x, y): create with x's options, solve(x), reset(), solve(y) against a handle created with
    x's options that runs solve(y) only.  All ordered pairs of the configurations the mode admits, x == y included."""
    return [(p, m, x, y) for p in PROBLEMS for m in MODES for x in admissible(m) for y in admissible(m)]


# the pairs that switch path, for the sequences that do not run the whole matrix
SWITCH_PAIRS = (("a", "d"), ("d", "a"), ("a", "b"), ("b", "a"), ("c", "a"), ("f0", "a"), ("f1", "a"), ("a", "g"))


def switch_cases():
    return [(p, m, x, y) for p in PROBLEMS for m in MODES for x, y in SWITCH_PAIRS
            if x in admissible(m) and y in admissible(m)]


# ---- comparator --------------------------------------------------------------------------------------------------------
# The ONLY fields left out of a comparison: wall-clock and device times.  The iteration trace has no time column.
SUMMARY_TIME_FIELDS = ("setup_time_in_seconds", "solve_time_in_seconds", "kernel_seconds")
TRACE_TIME_COLUMNS = ()

SUMMARY_FIELDS = tuple(name for name, _ in abi.CSummary._fields_ if name not in SUMMARY_TIME_FIELDS)
TRACE_COLUMNS = tuple(i for i, name in enumerate(abi.TRACE_FIELDS) if name not in TRACE_TIME_COLUMNS)


def _bits(value):
    if isinstance(value, float):
        return np.float64(value).tobytes()  # -0.0 != 0.0, NaN == NaN: bits, not values
    if isinstance(value, C.Array):
        return bytes(value)
    return value


class Result:
    """Everything a solve left behind, detached from the handle: summary, trace, parameters."""

    def __init__(self, status: int, summary: abi.CSummary, trace: np.ndarray, downloaded: abi.Problem):
        self.status = status
        self.summary = {name: _bits(getattr(summary, name)) for name, _ in abi.CSummary._fields_}
        self.values = {name: getattr(summary, name) for name in ("initial_cost", "final_cost", "num_iterations",
                                                                  "num_linear_solver_iterations", "termination",
                                                                  "num_inner_iteration_steps",
                                                                  "num_matrix_free_iterations")}
        self.launches = dict(zip(abi.KERNEL_CLASS_NAMES, list(summary.kernel_launches)))
        self.trace = trace.copy()
        self.extrinsics = downloaded.extrinsics.tobytes()
        self.intrinsics = downloaded.intrinsics.tobytes()
        self.points = downloaded.points.tobytes()


def differences(got: Result, ref: Result):
    """Names of everything that differs between two results, time fields aside.  Empty: equal bit for bit."""
    out = []
    if got.status != ref.status:
        out.append(f"status {got.status} != {ref.status}")
    for name in SUMMARY_FIELDS:
        if got.summary[name] != ref.summary[name]:
            out.append(f"summary.{name}: {got.values.get(name, got.summary[name])!r} != "
                       f"{ref.values.get(name, ref.summary[name])!r}")
    for col in TRACE_COLUMNS:
        if got.trace[:, col].tobytes() != ref.trace[:, col].tobytes():
            out.append(f"trace.{abi.TRACE_FIELDS[col]}: {got.trace[:, col]} != {ref.trace[:, col]}")
    for name in ("extrinsics", "intrinsics", "points"):
        if getattr(got, name) != getattr(ref, name):
            out.append(f"downloaded {name}")
    return out


def trajectories_differ(a: Result, b: Result) -> bool:
    """"Something else happened before": two references differ in final cost, iteration count or trace."""
    return (a.summary["final_cost"] != b.summary["final_cost"] or a.values["num_iterations"] != b.values["num_iterations"]
            or a.trace.tobytes() != b.trace.tobytes())


def perturbed(P: abi.Problem, aspect_group=None) -> abi.Problem:
    """New parameter values for the same structure, as test_set_parameters_on_a_resident_handle makes them;
    aspect_group: that intrinsics group also gets an aspect ratio != 1 (compact planes become impossible)."""
    Q = P.copy()
    rng = np.random.default_rng(1)
    Q.extrinsics[:, :3] += 0.02 * rng.normal(size=(Q.num_cameras, 3))
    Q.points[:, :3] += 0.02 * rng.normal(size=(Q.num_points, 3))
    Q.intrinsics[0::7] *= 1.001
    if aspect_group is not None:
        Q.intrinsics[Q.group_offset[aspect_group] + 1] = 1.01
    return Q
