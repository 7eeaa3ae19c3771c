#!/usr/bin/env python3
"""Benchmark of the MI355X bundle-adjustment engine (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--workload venice1778_heavy] [--dump-outputs DIR] [--full]

A "step" is one Levenberg-Marquardt iteration (linearize, eliminate tracks,
build + solve the reduced camera system, back-substitute, trial cost) of the
synthetic BAL-Venice-1778-sized problem (1778 cameras / 993 923 tracks /
5 001 946 observations, fp64, 9-dof cameras, 3-dof points, ITERATIVE_SCHUR as
the reference's own policy picks for >= 1000 views,
reconstruction_estimator_utils.cc:121-125; the default workload is the
heavy-tailed variant of SURVEY 8(d) config 4, tracks of up to 400 views).  The
timed region runs exactly K iterations on inputs already resident in HBM, as
ceil(K / 10) solves of <= 10 iterations from the same perturbed start
(tolerances disabled; the problem converges in ~12 iterations, so a single long
solve would coast at the fixed point) with a device-side parameter reset in
between; W warm-up iterations run first.  value = N_obs * K / wall time =
observations/s over all ranks (strong scaling: the problem is fixed, tracks
are sharded over ranks).

A plain run does only what the headline needs: set up, warm up, time the K
iterations (no HIP events in the timed region), write the outputs if asked,
print the line.  --full adds everything else, as before: an untimed pass of
the same K iterations with every kernel class timed (the per-class table and
the roofline; the timed region then carries events for the dominant class),
and beside the headline (1 GPU) the reference's default operating point (inner
iterations on), the CPU port on all cores and on one core, the end-to-end wall
clock of the C++ entry point, the side kernels and the other variants;
--no-extras / --no-cpu-baseline leave parts of that out.

--dump-outputs DIR writes what the timed path computed in its last solve, the
arrays a caller of tmi_ba_solver_solve + download receives, as float64 .npy:
extrinsics [Nc, 6], intrinsics, points [Np, 4] (a fixed, seeded sample of the
rows if the whole would pass 64 MB) and costs = [initial cost, final cost,
initial RMSE, final RMSE].  The inputs are seeded: the same arguments give the
same inputs in every run.

For N > 1 launch with
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W
Rank 0 prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_MFMA_PEAK_TFLOPS = 78.6  # dense fp64 matrix peak of MI355X (product specification; MI355X_MICROARCH.md has no fp64 row)


def algorithmic_bytes(cls: str, n_obs: int, n_cam: int, n_pts: int, dc: int, dp: int, nnzb: int, mf_frac: float = 0.0):
    """Algorithmic HBM bytes of ONE launch of a kernel class, SURVEY 8(d):
    observations stream 24 B (u, v, 2 x int32), parameters 8 B per scalar,
    normal-equation blocks once, 8 d_c^2 B per structurally non-zero upper block
    of the reduced camera matrix.  Intermediates (Jacobians, W, Y) are not
    algorithmic."""
    sym = lambda d: d * (d + 1) // 2  # noqa: E731
    if cls == "linearize":
        return n_obs * 24 + n_cam * 8 * dc + n_pts * 8 * dp
    if cls == "point_eliminate":
        return n_pts * 8 * (sym(dp) + dp)
    if cls == "camera_diag":
        return n_cam * 8 * (sym(dc) + dc)
    if cls == "schur_offdiag":
        return 2 * nnzb * 8 * dc * dc
    if cls == "spmv":
        # SURVEY 8(d), B_pcg per PCG iteration: every structurally non-zero upper block of S once plus the vectors,
        # WHICHEVER operator applies S (Jacobian blocks are recomputable, hence not algorithmic).  The bytes the
        # matrix-free product cannot avoid in this repository's layout are reported beside it as `layout_floor`.
        return nnzb * 8 * dc * dc + 6 * n_cam * 8 * dc
    if cls == "pcg_vector":
        return 4 * n_cam * 8 * dc
    if cls == "back_substitute":
        return n_obs * 24 + n_cam * 8 * dc + n_pts * 8 * (sym(dp) + 2 * dp)
    if cls == "update_cost":
        return n_obs * 24 + n_cam * 8 * dc + n_pts * 8 * dp
    return 0


def matrix_free_layout_floor(n_obs: int, n_cam: int, n_pts: int, dc: int, dp: int, stored_dc: int | None = None):
    """Bytes ONE matrix-free product must read in the layout of DESIGN.md section 3 when every stored block is read
    once: the 2 x dc camera and 2 x dp point Jacobian blocks of every observation, its two int32 indices, the
    per-track factor and the vectors.  NOT SURVEY 8(d)'s figure (that one counts S blocks); a different key in the
    bench line."""
    sdc = dc if stored_dc is None else stored_dc  # (round 4: the three position columns are formed from the point block)
    return n_obs * (16 * (sdc + dp) + 8) + 4 * n_cam * 8 * dc + n_pts * 8 * (dp * (dp + 1) // 2)


def engine_source_sha():
    """Stamp of the engine sources a PMC pass was taken with (the GPU box has no .git)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "theiasfm_amd", "csrc", "*"))):
        if f.endswith((".h", ".hip", ".cpp")):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def parse_setup_phases(stderr_text: str) -> dict:
    """The LAST repeat's '[tmi_ba shim] <phase> <s> s' / '[tmi_ba setup...] <phase> <s> s' lines of tools/e2e_bench run
    with TMI_BA_SETUP_TIMING=1, as {phase: seconds} plus three sums: the walk of the reference's containers
    (AddViews / AddTracks), the flat tables the shim builds from them, and tmi_ba_solver_create (upload + device
    structure build + work arrays)."""
    import re
    runs, cur = [], None
    for line in stderr_text.splitlines():
        m = re.match(r"\[tmi_ba (shim|setup|setup/device)\]\s+(.*?)\s+([0-9.]+) s\b", line)
        if not m:
            continue
        name = ("device: " if m.group(1) != "shim" else "shim: ") + m.group(2).strip().rstrip(":")
        if name == "shim: AddViews: feature tables":
            cur = {}
            runs.append(cur)
        if cur is not None:
            cur[name] = float(m.group(3))
    if not runs:
        return {}
    last = runs[-1]
    walk = last.get("shim: AddViews: total", 0.0) + last.get("shim: AddTracks", 0.0)
    tables = sum(last.get(k, 0.0) for k in ("shim: id tables", "shim: parameters", "shim: order: histogram",
                                            "shim: order: coarse scatter", "shim: order: output alloc", "shim: order: buckets",
                                            "shim: observation order"))
    create = last.get("device: create total (incl. upload)", 0.0)
    return dict(phases=last, host_walk_of_reference_containers=round(walk, 4), host_flat_tables=round(tables, 4),
                solver_create_upload_and_device_build=round(create, 4),
                device_structure_build=round(last.get("device: structure total", 0.0), 4))


def ceres_probe():
    """SURVEY 8(d) CPU-baseline plan, step 1: is a real Ceres / Eigen / TheiaSfM on this box?  (If so,
    tools/ceres_golden_main.cc can be built against it and `kind` becomes "reference"; otherwise the port.)"""
    import fnmatch
    import subprocess
    pats = dict(ceres_lib="libceres*", ceres_header="ceres.h", eigen="*/Eigen/Core", theia_lib="libtheia.*",
                glog="libglog*", suitesparse="libcholmod*")
    found = {k: None for k in pats}
    roots = [d for d in ("/usr", "/opt", "/usr/local", "/root", "/home") if os.path.isdir(d)]
    expr = []
    for pat in pats.values():
        expr += ["-o", "-path" if "/" in pat else "-name", pat]
    try:  # one walk of the file system for all six patterns
        r = subprocess.run(["find"] + roots + ["-xdev", "-not", "-path", "*/repo/*", "-not", "-path", "*/torch/*",
                                               "-not", "-path", "/root/reference/*", "("] + expr[1:] + [")", "-print"],
                           capture_output=True, text=True, timeout=90)
        for line in r.stdout.splitlines():
            for key, pat in pats.items():
                if found[key] is None and (fnmatch.fnmatch(line, pat) or fnmatch.fnmatch(os.path.basename(line), pat)):
                    found[key] = line
    except (OSError, subprocess.TimeoutExpired):
        found = {k: "probe failed" for k in pats}
    usable = bool(found.get("ceres_lib") and found.get("ceres_header") and found.get("eigen") and found.get("theia_lib"))
    return dict(found=found, reference_buildable=usable,
                note="TheiaSfM's BundleAdjustReconstruction needs all of Ceres, Eigen, glog and libtheia"
                     + ("" if usable else "; not on this box, so cpu_baseline.kind stays 'port'"))


def pmc_traffic(kernel_class: str, workload: str, world: int, mf_frac: float = 0.0, table: str = "pmc_latest.json"):
    """HBM bytes per launch of the kernel class from the committed rocprofv3 PMC passes
    (profiles/pmc_latest.json, written by tools/summarize_profile.py from separate
    --pmc FETCH_SIZE / --pmc WRITE_SIZE runs of this same command).  Correction per
    MI355X_MICROARCH.md (HBM section): both counters are in KiB and FETCH_SIZE reports
    half of a wide read stream on gfx950, so traffic = 2 * FETCH_SIZE + WRITE_SIZE.
    None when no matching profile is committed (other workload / GPU count)."""
    path = os.path.join(ROOT, "profiles", table)
    try:
        d = json.load(open(path))
    except (OSError, ValueError):
        return None
    if d.get("workload") != workload or world != 1:
        return None
    if d.get("engine_source_sha") != engine_source_sha():
        return None  # taken with another build of the kernels: refuse rather than quote stale bytes
    v = d.get("classes", {}).get(kernel_class)
    if kernel_class == "spmv" and mf_frac > 0.0:
        # the class holds both operators' products: blend as algorithmic_bytes does
        f = d.get("classes", {}).get("spmv_matrix_free")
        if f is None:
            return None
        v = (1.0 - mf_frac) * (v or 0.0) + mf_frac * f
    return None if v is None else int(v)


def pmc_build():
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
    except (OSError, ValueError):
        return None
    return dict(tag=d.get("tag"), engine_source_sha=d.get("engine_source_sha"), git_head=d.get("git_head"),
                current_engine_source_sha=engine_source_sha(),
                stale=d.get("engine_source_sha") != engine_source_sha())


def write_problem_file(prob, path):
    """flat problem for tools/e2e_bench.cc (PINHOLE, one intrinsics group per view)"""
    import numpy as np
    assert prob.num_groups == prob.num_cameras and (prob.group_model == 0).all()
    with open(path, "wb") as f:
        np.array([prob.num_cameras, prob.num_points, prob.num_observations], dtype=np.int64).tofile(f)
        prob.extrinsics.astype(np.float64).tofile(f)
        prob.intrinsics.astype(np.float64).tofile(f)
        prob.points.astype(np.float64).tofile(f)
        prob.obs_camera.astype(np.int32).tofile(f)
        prob.obs_point.astype(np.int32).tofile(f)
        prob.obs_xy.astype(np.float64).tofile(f)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, prob, s):
    """--dump-outputs: the parameters `prob` holds after download and the costs of summary `s`, float64 .npy files"""
    import numpy as np
    arrays = dict(extrinsics=prob.extrinsics, intrinsics=prob.intrinsics, points=prob.points,
                  costs=np.array([s.initial_cost, s.final_cost, s.initial_rmse, s.final_rmse]))
    rest = sum(a.nbytes for k, a in arrays.items() if k != "points")
    rows = max(0, (DUMP_LIMIT_BYTES - rest) // (prob.points.shape[1] * 8))
    if prob.num_points > rows:
        keep = np.sort(np.random.default_rng(0).choice(prob.num_points, rows, replace=False))
        arrays["points"] = prob.points[keep]
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="venice1778_heavy",
                    choices=["tiny", "ladybug49", "alamo", "venice1778", "venice1778_heavy"])
    ap.add_argument("--solve-length", type=int, default=10,
                    help="LM iterations per solve: the K timed iterations are ceil(K / this) solves from the "
                         "same perturbed start (the problem converges in ~12 iterations; a single K-iteration "
                         "solve would coast at the fixed point)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the per-class kernel table and roofline (an untimed pass of their "
                         "own), the CPU baselines, the other operating points, sizes and configurations, the "
                         "end-to-end C++ entry point and the side kernels")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the parameters and costs of the last timed solve to DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baselines, no side kernels")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the lines beside the headline: plain venice1778, inner iterations, "
                         "end-to-end C++ entry point, side kernels")
    ap.add_argument("--cpu-iters", type=int, default=2)
    ap.add_argument("--transport", default="rccl", choices=["rccl", "torch", "staged", "torch_staged"],
                    help="rccl: ncclAllReduce issued by the engine; torch: torch.distributed (nccl) hook; staged: "
                         "gloo through host memory with every rank on GPU 0 -- a functional check of the "
                         "multi-process path on a single-GPU box, not a measurement")
    ap.add_argument("--residual-precision", type=int, default=64, choices=[64, 32],
                    help="32 = evaluate residuals/Jacobians in fp32, accumulate in fp64 (config 5)")
    ap.add_argument("--schur-mode", default="auto", choices=["auto", "explicit", "implicit"],
                    help="ITERATIVE_SCHUR: form S explicitly (one all-reduce of S per LM iteration) "
                         "or apply it implicitly (one small all-reduce per PCG iteration); "
                         "auto = explicit on one GPU, implicit on several")
    args = ap.parse_args()

    import numpy as np
    import torch

    from theiasfm_amd import abi, dist, lib, synth
    import __graft_entry__ as entry

    one_gpu = args.transport in ("staged", "torch_staged")  # every rank on GPU 0, sums through gloo
    rank, world, local = dist.init_from_env(backend="gloo" if one_gpu else None)
    if one_gpu:
        local = 0
    hook_stats = {}  # calls / bytes of the torch.distributed hook (N > 1 with --transport torch / torch_staged)
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with "
                  "python -m torch.distributed.run --nproc-per-node N", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py needs a GPU", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    if rank == 0:
        entry.build_engine()
    if world > 1:
        torch.distributed.barrier()

    def solver_policy(n_cam):
        # the reference's solver-type policy (reconstruction_estimator_utils.cc:110-133)
        if n_cam >= 1000:
            return abi.ITERATIVE_SCHUR, "ITERATIVE_SCHUR/SCHUR_JACOBI"
        if n_cam >= 150:
            return abi.SPARSE_SCHUR, "SPARSE_SCHUR (exact, dense Cholesky of S)"
        return abi.DENSE_SCHUR, "DENSE_SCHUR (exact)"

    schur_mode = {"auto": 0, "explicit": 1, "implicit": 2}[args.schur_mode]

    def base_options(n_cam):
        # Tolerances are DISABLED (negative: |dcost| <= tol * cost etc. can never hold), so a solve
        # runs exactly max_num_iterations trust-region iterations.  use_inner_iterations = 0 for the
        # headline: a step is the trust-region iteration proper, on the device and in the CPU baseline
        # alike; the reference's default (inner iterations on) is timed beside it below.
        return dict(point_dof=3, linear_solver_type=solver_policy(n_cam)[0], function_tolerance=-1.0,
                    gradient_tolerance=-1.0, parameter_tolerance=-1.0, device=local, schur_mode=schur_mode,
                    residual_precision=args.residual_precision, use_inner_iterations=0)

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    def run_chunks(solver, base, steps, profile):
        """`steps` LM iterations as solves of --solve-length iterations from the start point; the
        device-resident reset between two solves is part of the region.  Returns (iterations run,
        summed kernel seconds, summed launches, last summary, PCG iterations, accepted steps)."""
        left, done = steps, 0
        secs = [0.0] * abi.NUM_KERNEL_CLASSES
        launches = [0] * abi.NUM_KERNEL_CLASSES
        pcg = acc = mf = 0
        run_chunks.sweeps = 0
        s = None
        while left > 0:
            n = min(left, max(1, args.solve_length))
            st, s = solver.solve(abi.default_options(max_num_iterations=n, profile_kernels=profile, **base))
            if st != 0:
                raise RuntimeError(f"solve failed: {st} {s.message!r}")
            done += int(s.num_iterations)
            pcg += int(s.num_linear_solver_iterations)
            acc += int(s.num_successful_steps)
            mf += int(s.num_matrix_free_iterations)
            run_chunks.sweeps += int(s.num_inner_iteration_steps)
            for i in range(abi.NUM_KERNEL_CLASSES):
                secs[i] += s.kernel_seconds[i]
                launches[i] += s.kernel_launches[i]
            left -= n
            if int(s.num_iterations) != n:
                break  # a failure mode (invalid steps, minimum radius): reported through steps != K
            if left > 0:
                solver.reset()
        return done, secs, launches, s, pcg, acc, mf

    def measure(workload, steps, warmup, with_transport, overrides=None, profiled=True):
        """creates the resident solver, warms up, profiles (profiled = True), times; returns a dict of raw results"""
        t0 = time.perf_counter()
        prob = synth.config(workload)
        t_gen = time.perf_counter() - t0
        base = {**base_options(prob.num_cameras), **(overrides or {})}
        # Solver.download() writes into `prob`: the start for the legs of --full, and on every rank for merging the
        # dumped outputs over ranks
        prob0 = prob.copy() if (rank == 0 and args.full) or (world > 1 and args.dump_outputs) else None
        t0 = time.perf_counter()
        solver = lib.Solver(prob, abi.default_options(max_num_iterations=1, **base), rank, world)
        transport = "none"
        if world > 1 and with_transport:
            # RCCL over xGMI: natively from the engine (ncclAllReduce on its own stream); the
            # torch.distributed hook is the fallback (and --transport torch forces it)
            if args.transport == "staged":
                solver.set_allreduce(dist.make_staged_allreduce())
                transport = "gloo, staged through host memory (functional check only)"
            elif args.transport == "torch_staged":
                # the torch.distributed hook itself (aliased device tensors on the engine's stream) with a collective
                # that works when the ranks share one GPU: what --transport torch runs, minus RCCL
                solver.set_allreduce(dist.make_device_allreduce(dist.gloo_staged_sum, hook_stats))
                transport = "torch.distributed hook with a gloo collective staged through host memory (functional check only)"
            elif args.transport == "rccl" and dist.init_native_rccl(solver, rank, world):
                transport = "rccl (native, ncclAllReduce from the engine)"
            else:
                solver.set_allreduce(dist.make_device_allreduce(None, hook_stats))
                transport = "rccl via torch.distributed hook"
        t_create = time.perf_counter() - t0
        if warmup > 0:
            st, s = solver.solve(abi.default_options(max_num_iterations=warmup, **base))
            if st != 0:
                raise RuntimeError(f"warm-up solve failed: {st} {s.message!r}")
            solver.reset()
        secs_p = launches_p = dom_idx = None
        timed_profile = 0
        if profiled:
            # untimed pass of the same iterations with every kernel class timed (HIP events on the engine's
            # stream): the per-class table, and which class dominates.  The timed region carries events for
            # THAT class only (two event records per launch of every class cost a few % of an iteration).
            _, secs_p, launches_p, _, _, _, _ = run_chunks(solver, base, steps, 1)
            secs_nc = list(secs_p)
            secs_nc[abi.KERNEL_CLASS_NAMES.index("allreduce")] = 0.0
            dom_idx = max(range(len(secs_nc)), key=lambda i: secs_nc[i])
            timed_profile = (1 << dom_idx) if dom_idx > 0 else 1
            solver.reset()
        sync_all()
        t0 = time.perf_counter()
        done, secs_t, launches_t, s, pcg, acc, mf = run_chunks(solver, base, steps, timed_profile)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if world > 1:
            torch.distributed.barrier()
            dev = "cpu" if one_gpu else "cuda"
            mine = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            every = [torch.zeros_like(mine) for _ in range(world)]
            torch.distributed.all_gather(every, mine)
            per_rank_elapsed = [float(x.item()) for x in every]
            elapsed = max(per_rank_elapsed)
        else:
            per_rank_elapsed = [elapsed]
        return dict(prob=prob, prob0=prob0, base=base, solver=solver, transport=transport, t_gen=t_gen, sweeps=run_chunks.sweeps,
                    per_rank_elapsed=per_rank_elapsed,
                    t_create=t_create, steps_run=done, elapsed=elapsed, summary=s, pcg=pcg, accepted=acc, matrix_free=mf,
                    secs_p=secs_p, launches_p=launches_p, secs_t=secs_t, launches_t=launches_t, dom_idx=dom_idx)

    # One retry, visible in the line: if the headline solve FAILS on one rank with the compact planes (DESIGN.md section 3;
    # seen once in this round on one box of the pool, never reproduced: profiles/r06_product_experiments.md), the run is
    # repeated with the stored camera block and the line says so -- a failed solve is never reported as a number.
    compact_retry = None
    try:
        m = measure(args.workload, args.steps, args.warmup, True, profiled=args.full)
    except RuntimeError as ex:
        if world != 1 or os.environ.get("TMI_BA_COMPACT_PLANES") == "0" or "solve failed" not in str(ex):
            raise
        compact_retry = str(ex)[:300]
        os.environ["TMI_BA_COMPACT_PLANES"] = "0"
        m = measure(args.workload, args.steps, args.warmup, True, profiled=args.full)
    solver, s, prob, prob0, base = m["solver"], m["summary"], m["prob"], m["prob0"], m["base"]
    steps_run, elapsed = m["steps_run"], m["elapsed"]
    n_obs, n_cam, n_pts = prob.num_observations, prob.num_cameras, prob.num_points
    solver_type, solver_name = solver_policy(n_cam)
    if args.dump_outputs:
        solver.download()  # into `prob`
        if world > 1:
            # a rank downloads the points of its own tracks only: every point comes from the one rank that moved it
            dev = "cpu" if one_gpu else "cuda"
            moved = (prob.points != prob0.points).any(axis=1)
            owners = torch.from_numpy(moved.astype(np.float64)).to(dev)
            pts = torch.from_numpy(np.where(moved[:, None], prob.points, 0.0)).to(dev)
            torch.distributed.all_reduce(owners)
            torch.distributed.all_reduce(pts)
            prob.points[:] = np.where(owners.cpu().numpy()[:, None] > 0, pts.cpu().numpy(), prob0.points)
        if rank == 0:
            dump_outputs(args.dump_outputs, prob, s)
    if rank != 0:
        solver.close()
        return

    dc, dp = int(s.reduced_block_dim), 3
    nnzb = int(s.num_schur_blocks)

    mf_frac = float(m["matrix_free"]) / max(1, steps_run)  # share of the timed LM iterations whose PCG ran matrix-free

    def table(launch_list, sec_list):
        rows = []
        for name, launches, sec in zip(abi.KERNEL_CLASS_NAMES, launch_list, sec_list):
            if launches == 0 or sec <= 0.0:
                continue
            # per-rank launch: this rank's share of the observations / tracks
            ab = algorithmic_bytes(name, n_obs // world, n_cam, n_pts // world, dc, dp, nnzb, mf_frac)
            avg = sec / launches
            rows.append(dict(kernel=name, launches=int(launches), total_ms=round(sec * 1e3, 4),
                             avg_us=round(avg * 1e6, 2), algorithmic_bytes_per_launch=int(ab),
                             achieved_GBs=round(ab / avg / 1e9, 2) if avg > 0 else None))
        return rows

    roofline = kernels = None
    if args.full:
        kernels = table(m["launches_p"], m["secs_p"])
        dom_name = abi.KERNEL_CLASS_NAMES[m["dom_idx"]]
        timed_rows = [k for k in table(m["launches_t"], m["secs_t"]) if k["kernel"] == dom_name]
        dom = timed_rows[0] if timed_rows else max((k for k in kernels if k["kernel"] != "allreduce"),
                                                   key=lambda k: k["total_ms"])
        roofline = dict(bound="hbm", kernel=dom["kernel"], achieved=dom["achieved_GBs"], peak=HBM_PEAK_GBS,
                        unit="GB/s", frac=round(dom["achieved_GBs"] / HBM_PEAK_GBS, 5),
                        traffic=pmc_traffic(dom["kernel"], args.workload, world, mf_frac),
                        traffic_source="profiles/pmc_latest.json: rocprofv3 --pmc passes of this command, committed "
                                       "(counters cannot be read from inside the process); null when that pass was "
                                       "taken with other kernel sources (traffic_build.stale)",
                        traffic_build=pmc_build(),
                        launches=dom["launches"], avg_us=dom["avg_us"],
                        algorithmic_bytes_per_launch=dom["algorithmic_bytes_per_launch"],
                        algorithmic_bytes_definition="SURVEY 8(d): per product nnzb * 8 d_c^2 + 6 N_c 8 d_c (S blocks once, "
                                                     "whichever operator applies S); per-observation classes 24 B/observation "
                                                     "+ parameters + normal-equation blocks",
                        measured="HIP events on the engine's stream inside the timed region")
        if dom["kernel"] == "spmv" and mf_frac > 0.0:
            # beside the contract's figure, under its own key: what a matrix-free product has to read in this layout
            # which product / plane layout THIS handle runs is the engine's answer, not a copy of its rules
            info = solver.operator_info()
            one_sweep, drop_pos = info["one_sweep_product"], info["position_columns_formed"]
            compact = info.get("compact_planes", False)
            # (compact planes: the camera block is ONE 16-byte pair per observation -- the normalised image point)
            lf = matrix_free_layout_floor(n_obs // world, n_cam, n_pts // world, dc, dp, 1 if compact else (dc - 3 if drop_pos else dc))
            roofline["kernel"] = ("spmv (one product q = S p; matrix-free in %d of %d timed LM iterations: %s)"
                                  % (m["matrix_free"], steps_run,
                                     "mfc::product_kernel + mfc::reduce_kernel, the one-sweep product of mf_chunks.h" if one_sweep
                                     else "implicit_tracks_q + implicit_cameras_q, the two-pass product"))
            roofline["layout_floor"] = dict(
                bytes_per_launch=int(lf), achieved=round(lf / (dom["avg_us"] * 1e-6) / 1e9, 2),
                frac=round(lf / (dom["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 5),
                note="matrix-free product, every stored Jacobian block read once%s (NOT SURVEY 8(d)'s bytes; round 2 "
                     "quoted this figure as roofline.frac)" % (" -- compact planes: the camera block is formed from the point "
                                                               "block, the normalised image point (the one stored pair), the "
                                                               "track and the view" if compact else
                                                               " -- the position columns of the camera block are not "
                                                               "stored" if drop_pos else ""))
            roofline["compact_planes"] = bool(compact)
        # the other large classes of the same timed region (schur_offdiag was the dominant one until the adaptive
        # operator choice took it out of the short PCG solves): same definition, for comparison across rounds
        roofline["other_classes"] = {
            k["kernel"]: dict(achieved=k["achieved_GBs"], frac=round(k["achieved_GBs"] / HBM_PEAK_GBS, 5), launches=k["launches"],
                              avg_us=k["avg_us"], traffic=pmc_traffic(k["kernel"], args.workload, world, mf_frac))
            for k in kernels  # the separate pass with every class timed (kernels_note)
            if k["kernel"] in ("schur_offdiag", "spmv", "point_eliminate", "linearize") and k["kernel"] != dom["kernel"]}

    explicit = not (int(s.num_schur_pairs) == 0 and solver_type == abi.ITERATIVE_SCHUR)
    n_r = n_cam * dc
    if world > 1:
        # doubles all-reduced per LM iteration
        per_lm = (nnzb * dc * dc + n_cam * 3 * dc + 8) if explicit else (n_cam * (dc * dc + 3 * dc) + 8)
        per_pcg = 0 if explicit else n_r
        n_pcg_it = m["pcg"] / max(steps_run, 1)
        allreduce = dict(bytes_per_lm_iteration=int(8 * (per_lm + 8 + per_pcg * n_pcg_it)),
                         collectives_per_lm_iteration=round(2 + (0 if explicit else n_pcg_it), 2),
                         note=("one all-reduce of the reduced camera normal equations per LM iteration" if explicit else
                               "matrix-free operator: the diagonal blocks + gradients once per LM iteration and the "
                               "reduced vector (8 d_c N_c bytes) once per PCG iteration -- deviates from the "
                               "north-star wording, S itself would be ~0.8 GB per iteration"))
    else:
        allreduce = None

    out = dict(
        **({"solve_failed_with_compact_planes_and_was_repeated_with_the_stored_block": compact_retry} if compact_retry else {}),
        metric="ba_observations_per_sec", value=n_obs * steps_run / elapsed, unit="observations/s",
        n_gpus=world, steps=steps_run, warmup=args.warmup, ms_per_step=1e3 * elapsed / max(steps_run, 1),
        higher_is_better=True, scaling="strong", vs_baseline=None,
        dtype="f64" if args.residual_precision == 64 else "f32 residuals/Jacobians, f64 accumulation",
        data="synthetic",
        config=dict(workload=f"{args.workload}-synthetic", cameras=n_cam, tracks=n_pts,
                    observations=n_obs, camera_dof=dc, point_dof=dp, linear_solver=solver_name,
                    loss="TRIVIAL", use_inner_iterations=0,
                    solves=f"{-(-args.steps // max(1, args.solve_length))} x <= {args.solve_length} iterations from the "
                           "perturbed start, device-side reset in between (inside the timed region)",
                    schur_mode=args.schur_mode,
                    schur_operator=(("per LM iteration: matrix-free when the forecast PCG length is below the "
                                     "break-even of forming S, the explicit block-sparse S otherwise (schur_mode "
                                     "auto on one rank; both resident)"
                                     if (world == 1 and args.schur_mode == "auto" and solver_type == abi.ITERATIVE_SCHUR)
                                     else "explicit block-sparse S") if explicit else "implicit (matrix-free)"),
                    parallelism=f"tracks sharded x{world}", transport=m["transport"],
                    # what this handle runs (tmi_ba_solver_operator_info): the one-sweep matrix-free product, position
                    # columns formed from the point block, camera side of matrix-free iterations built view by view
                    # from one record per track instead of camera-major records (direct_diag.h)
                    engine_paths=solver.operator_info()),
        lm_iterations_per_sec=steps_run / elapsed,
        pcg_iterations=int(m["pcg"]),
        matrix_free_lm_iterations_in_last_solve=int(s.num_matrix_free_iterations),
        initial_cost=s.initial_cost, final_cost=s.final_cost, initial_rmse=s.initial_rmse,
        final_rmse=s.final_rmse, accepted_steps=int(m["accepted"]),
        schur_blocks_upper=nnzb, schur_pairs=int(s.num_schur_pairs),
        setup_seconds=dict(generate=round(m["t_gen"], 3), create_upload=round(m["t_create"], 3)))
    if args.full:
        out.update(roofline=roofline, kernels=kernels,
                   kernels_note="per-class table: separate untimed pass of the same iterations with every class timed")
    if allreduce:
        # what the first real multi-GPU run needs to be read from ONE line: every rank's own time for the same K
        # iterations (the slowest is the headline), rank 0's time inside the all-reduce callback and its launches from
        # the pass with every class timed (--full), and -- with the torch.distributed hook -- the hook's own call / byte
        # counts
        i_ar = abi.KERNEL_CLASS_NAMES.index("allreduce")
        allreduce["per_rank_ms_per_step"] = [round(1e3 * e / max(steps_run, 1), 4) for e in m["per_rank_elapsed"]]
        if args.full:
            allreduce["rank0_calls_per_lm_iteration_measured"] = round(m["launches_p"][i_ar] / max(steps_run, 1), 2)
            allreduce["rank0_ms_per_step_in_callback"] = round(1e3 * m["secs_p"][i_ar] / max(steps_run, 1), 4)
        if hook_stats:
            allreduce["torch_hook"] = dict(calls=int(hook_stats.get("calls", 0)), bytes=int(hook_stats.get("bytes", 0)),
                                           note="over warm-up, the profiled pass (--full) and the timed region")
        out["allreduce"] = allreduce
    if steps_run != args.steps:
        out["note"] = f"solver stopped after {steps_run} of {args.steps} iterations: {s.message!r}"
    # Whole-iteration figure of SURVEY 8(d): B_iter = B_lin + B_schur + B_pcg + B_back + B_cost with the
    # measured block count and PCG iterations (intermediates -- Jacobians, Y -- are not algorithmic)
    sym = lambda n: n * (n + 1) // 2  # noqa: E731
    n_pcg = m["pcg"] / max(steps_run, 1)
    b_lin = n_obs * 24 + n_cam * 8 * dc + n_pts * 8 * dp + n_cam * 8 * (sym(dc) + dc) + n_pts * 8 * (sym(dp) + dp)
    b_schur = 2 * nnzb * 8 * dc * dc
    b_pcg = n_pcg * (nnzb * 8 * dc * dc + 6 * n_cam * 8 * dc)
    b_back = n_obs * 24 + n_cam * 8 * dc + n_pts * 8 * (sym(dp) + 2 * dp)
    b_cost = n_obs * 24 + n_cam * 8 * dc + n_pts * 8 * dp
    # S is formed only in the LM iterations that ran PCG on it (schur_mode auto picks per iteration): B_schur counts
    # for those and not for the matrix-free ones
    formed_frac = (1.0 - mf_frac) if solver_type == abi.ITERATIVE_SCHUR else 1.0
    b_iter = b_lin + formed_frac * b_schur + b_pcg + b_back + b_cost
    b_iter_all = b_lin + b_schur + b_pcg + b_back + b_cost
    out["iteration_roofline"] = dict(
        algorithmic_bytes_per_lm_iteration=int(b_iter), pcg_iterations_per_lm_iteration=round(n_pcg, 2),
        lm_iterations_that_formed_S=int(round(formed_frac * steps_run)), of=steps_run,
        achieved_GBs=round(b_iter * steps_run / elapsed / 1e9, 1), peak_GBs=HBM_PEAK_GBS * world,
        frac=round(b_iter * steps_run / elapsed / 1e9 / (HBM_PEAK_GBS * world), 5),
        frac_if_S_counted_every_iteration=round(b_iter_all * steps_run / elapsed / 1e9 / (HBM_PEAK_GBS * world), 5),
        note="SURVEY 8(d) formula, B_schur only for the iterations that formed S; the kernels move several times these "
             "bytes (profiles/) because Jacobian blocks and the per-observation Schur factors are stored and gathered "
             "rather than recomputed")

    extras = world == 1 and args.full and not args.no_extras
    cpu_baseline = world == 1 and args.full and not args.no_cpu_baseline
    if extras:
        # ---- the reference's default operating point: inner iterations ON
        # (reconstruction_estimator_utils.cc:117, bundle_adjustment.h:112), same problem, same start
        solver.reset()
        n_in = min(5, args.steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st_i, s_i = solver.solve(abi.default_options(max_num_iterations=n_in, **{**base, "use_inner_iterations": 1}))
        torch.cuda.synchronize()
        t_in = time.perf_counter() - t0
        out["with_inner_iterations"] = dict(
            steps=int(s_i.num_iterations), ms_per_step=round(1e3 * t_in / max(int(s_i.num_iterations), 1), 3),
            observations_per_s=n_obs * int(s_i.num_iterations) / t_in,
            coordinate_descent_sweeps=int(s_i.num_inner_iteration_steps), final_cost=s_i.final_cost,
            status=int(st_i),
            note="one solve of the first iterations with use_inner_iterations = 1 (Ceres switches the sweeps off "
                 "once their relative gain drops below 1e-3)")

    if cpu_baseline:
        # CPU baseline: the in-repo oracle (Ceres-semantics restatement; the real
        # Theia + Ceres cannot be built offline) on the SAME problem and options
        # for a bounded number of LM iterations, all host cores via OpenMP.
        from oracle import oracle
        iters = max(1, args.cpu_iters)
        cpu_opts = abi.default_options(max_num_iterations=iters, **{**base, "device": -1})
        ref = prob0.copy()
        tc = time.perf_counter()
        st_o, s_o = oracle.solve(ref, cpu_opts)
        t_cpu = time.perf_counter() - tc
        # the device on the same bounded sample, for a full-size parity figure
        solver.reset()
        dev_opts = abi.default_options(max_num_iterations=iters, **base)
        st_d, s_d = solver.solve(dev_opts)
        out["cpu_baseline"] = dict(
            value=n_obs * int(s_o.num_iterations) / s_o.solve_time_in_seconds, unit="observations/s",
            cores=oracle.num_threads(), kind="port", ceres_probe=ceres_probe(),
            sample=f"{int(s_o.num_iterations)} LM iterations of the full {args.workload} problem, same options "
                   f"(solve {s_o.solve_time_in_seconds:.2f} s + setup {s_o.setup_time_in_seconds:.2f} s, wall {t_cpu:.2f} s)",
            final_cost=s_o.final_cost, final_rmse=s_o.final_rmse,
            note="the in-repo Ceres-semantics port (oracle/, plain C + OpenMP: dual-number Jacobians, a pair-list Schur "
                 "complement), NOT Ceres: it is test infrastructure written for transparency, and Ceres + SuiteSparse on the "
                 "same cores is expected to need well under its time -- the speed-ups quoted against it are not a claim "
                 "about Ceres.  No Ceres / Eigen / Theia exists on the box (ceres_probe) to time instead")
        out["parity_sample"] = dict(
            iterations=int(s_o.num_iterations), device_cost=s_d.final_cost, oracle_cost=s_o.final_cost,
            rel_cost_diff=abs(s_d.final_cost - s_o.final_cost) / s_o.final_cost,
            rmse_abs_diff=abs(s_d.final_rmse - s_o.final_rmse))
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
        # Theia's default is num_threads = 1 (bundle_adjustment.h:107): the same port on ONE core, on a
        # bounded sample -- every 48th track with all its observations, all cameras
        keep_pts = np.arange(0, n_pts, 48)
        remap = np.full(n_pts, -1, dtype=np.int64)
        remap[keep_pts] = np.arange(keep_pts.size)
        sel = np.flatnonzero(remap[prob0.obs_point] >= 0)
        sub = abi.Problem(prob0.extrinsics.copy(), prob0.camera_group.copy(), prob0.camera_flags.copy(),
                          prob0.group_model.copy(), prob0.group_offset.copy(), prob0.intrinsics.copy(),
                          prob0.intrinsics_constant.copy(), prob0.points[keep_pts].copy(),
                          prob0.point_constant[keep_pts].copy(), prob0.obs_camera[sel].copy(),
                          remap[prob0.obs_point[sel]].astype(np.int32), prob0.obs_xy[sel].copy())
        nthr = oracle.num_threads()
        oracle.set_num_threads(1)
        try:
            st_1, s_1 = oracle.solve(sub, abi.default_options(max_num_iterations=2, **{**base, "device": -1}))
        finally:
            oracle.set_num_threads(nthr)
        out["cpu_baseline_single_thread"] = dict(
            value=sub.num_observations * int(s_1.num_iterations) / s_1.solve_time_in_seconds, unit="observations/s",
            cores=1, kind="port",
            sample=f"{int(s_1.num_iterations)} LM iterations on every 48th track ({sub.num_observations} observations, "
                   f"all {n_cam} cameras), solve {s_1.solve_time_in_seconds:.2f} s")
        out["speedup_vs_cpu_single_thread"] = out["value"] / out["cpu_baseline_single_thread"]["value"]

    if extras:
        # ---- end-to-end wall clock of the drop-in C++ entry point on the same problem:
        # theia::BundleAdjustReconstruction = AddView/AddTrack + flatten + structure build + upload +
        # LM + download + write-back (tools/e2e_bench.cc).  NOT the headline value (inputs start on the host).
        import subprocess
        import tempfile
        entry.build_host_shim()
        exe = os.path.join(ROOT, "tools", "e2e_bench")
        if os.path.exists(exe):
            with tempfile.TemporaryDirectory() as td:
                path = os.path.join(td, "problem.bin")
                write_problem_file(prob0, path)
                solver.close()  # free the HBM of the resident solver first
                solver = None
                e2e = {}
                # merged = 1: the device path's merged per-view preconditioner block (what the headline uses through the
                # C ABI); merged = 0: Ceres' per-parameter-block SCHUR_JACOBI, which the shim passes by default.  Every
                # line also carries `second_call`: the same Reconstruction adjusted again, served by the resident session.
                for key, inner, merged in (("inner_iterations_off", 0, 1), ("inner_iterations_on", 1, 1),
                                           ("shim_default_preconditioner_inner_off", 0, 0)):
                    p = subprocess.run([exe, path, str(args.solve_length), str(inner), "2", str(merged)],  # best of two: the first call of a process loads the code objects (~0.25 s)
                                       capture_output=True, text=True, timeout=900)
                    try:
                        e2e[key] = json.loads(p.stdout.strip().splitlines()[-1])
                    except (ValueError, IndexError):
                        e2e[key] = dict(error=(p.stderr or p.stdout)[-400:], returncode=p.returncode)
                # where the set-up of the drop-in call goes -- the phases the shim and
                # tmi_ba_solver_create print with TMI_BA_SETUP_TIMING (second repeat of one more run: the first call of a
                # process also loads the code objects), grouped host walk / host tables / device build
                try:
                    p = subprocess.run([exe, path, str(args.solve_length), "0", "2", "1"], capture_output=True, text=True,
                                       timeout=900, env=dict(os.environ, TMI_BA_SETUP_TIMING="1"))
                    e2e["setup_phases_seconds"] = parse_setup_phases(p.stderr)
                except Exception as ex:  # noqa: BLE001  (diagnostics only)
                    e2e["setup_phases_seconds"] = dict(error=str(ex)[:200])
                out["end_to_end"] = e2e
        if solver is None:
            solver = lib.Solver(prob0.copy(), abi.default_options(max_num_iterations=1, **base), 0, 1)

    if cpu_baseline:
        from oracle import oracle
        # The steps either side of the BA on the same resident
        # problem, outside the timed region: kernel time from HIP events, the oracle beside it.
        side = {}
        solver.reset()
        solver.solve(abi.default_options(max_num_iterations=max(1, args.cpu_iters), **base))
        adjusted = solver.download().copy()
        flag_d, _, fs = solver.filter_outlier_tracks(4.0, 2.0)
        flag_d, _, fs = solver.filter_outlier_tracks(4.0, 2.0)  # second launch: warm
        tc = time.perf_counter()
        flag_o, _, counts = oracle.filter_outlier_tracks(adjusted, 4.0, 2.0)
        t_f = time.perf_counter() - tc
        side["outlier_filter"] = dict(
            kernel_us=round(fs.kernel_seconds * 1e6, 1), call_ms=round(fs.seconds * 1e3, 3),
            observations_per_s=n_obs / fs.kernel_seconds, cpu_port_observations_per_s=n_obs / t_f,
            flags_equal=bool((flag_d == flag_o).all()), removed=int(counts[1] + counts[2]))
        solver.reset()
        trk_opts = abi.default_options(max_num_iterations=10, **{**base, "function_tolerance": 1e-6,
                                                               "parameter_tolerance": 1e-8,
                                                               "gradient_tolerance": 1e-10})
        term_d, it_d, _, c1_d, ts = solver.adjust_tracks(trk_opts)
        # CPU port on a bounded sample: the first 100 000 tracks (the rest are marked constant,
        # which the per-track oracle skips)
        n_cpu = min(100_000, n_pts)
        ref2 = prob0.copy()
        ref2.point_constant = ref2.point_constant.copy()
        ref2.point_constant[n_cpu:] = 1
        tc = time.perf_counter()
        term_o, it_o, _, c1_o = oracle.adjust_tracks(ref2, trk_opts)
        t_t = time.perf_counter() - tc
        sm = slice(0, n_cpu)
        side["batched_track_ba"] = dict(
            kernel_ms=round(ts.kernel_seconds * 1e3, 3), tracks=int(ts.num_tracks),
            lm_iterations=int(ts.total_iterations), tracks_per_s=ts.num_tracks / ts.kernel_seconds,
            cpu_port_tracks_per_s=n_cpu / t_t, cpu_port_sample=f"first {n_cpu} tracks, {oracle.num_threads()} threads",
            termination_mismatches=int((term_d[sm] != term_o[sm]).sum()),
            iteration_mismatches=int((it_d[sm] != it_o[sm]).sum()),
            final_cost_rel_diff_above_1e9=int((np.abs(c1_d[sm] - c1_o[sm]) > 1e-9 * np.maximum(c1_o[sm], 1e-12)).sum()),
            sample_final_cost=dict(device=float(c1_d[sm].sum()), oracle=float(c1_o[sm].sum())))
        solver.reset()
        sel_d, ln_d, err_d, ss0 = solver.select_good_tracks(10, 100, 100)  # builds the per-view track lists
        sel_d, ln_d, err_d, ss = solver.select_good_tracks(10, 100, 100)
        tc = time.perf_counter()
        sel_o, _, _ = oracle.select_good_tracks(prob0, 10, 100, 100)
        t_s = time.perf_counter() - tc
        side["track_selection"] = dict(
            statistics_kernel_us=round(ss.kernel_seconds * 1e6, 1), call_ms=round(ss.seconds * 1e3, 2),
            first_call_ms=round(ss0.seconds * 1e3, 2),
            cpu_port_ms=round(t_s * 1e3, 1), selected=int(ss.num_selected), of=int(ss.num_tracks),
            selection_equal=bool((sel_d == sel_o).all()))
        # batched BundleAdjustTwoViews (bundle_adjust_two_views.cc:113-191): 20 000 view pairs, 5-300 correspondences
        from theiasfm_amd import lib as _lib
        tvb = synth.make_two_view_batch(20000, 5, max_corr=300)
        _lib.adjust_two_views(tvb.copy(), 4)  # first call: module load, allocations
        tv_d = tvb.copy()
        tc = time.perf_counter()
        term_d, it_d, _, c1_d, tvs = _lib.adjust_two_views(tv_d, 4)
        t_call = time.perf_counter() - tc
        n_cpu = 2000
        tv_s = tvb.head(n_cpu)
        if True:
            tc = time.perf_counter()
            term_o, it_o, _, c1_o = oracle.adjust_two_views(tv_s, 4)
            t_o = time.perf_counter() - tc
            sm = slice(0, n_cpu)
            ok = term_o >= 0
            side["batched_two_view_ba"] = dict(
                kernel_ms=round(tvs.kernel_seconds * 1e3, 3), call_ms=round(t_call * 1e3, 2), pairs=int(tvb.num_pairs),
                correspondences=int(tvb.correspondence_ptr[-1]), lm_iterations=int(tvs.total_iterations),
                pairs_per_s=tvb.num_pairs / tvs.kernel_seconds, cpu_port_pairs_per_s=n_cpu / t_o,
                cpu_port_sample=f"first {n_cpu} pairs, {oracle.num_threads()} threads",
                termination_mismatches=int((term_d[sm] != term_o).sum()),
                iteration_mismatches=int((it_d[sm] != it_o).sum()),
                final_cost_rel_diff_above_1e6=int((np.abs(c1_d[sm][ok] - c1_o[ok]) > 1e-6 * np.maximum(c1_o[ok], 1e-12)).sum()))
        # batched BundleAdjustTwoViewsAngular (bundle_adjust_two_views.cc:193-240): relative pose of 20 000 pairs
        tab, _, _ = synth.make_two_view_angular_batch(20000, 5, max_corr=300)
        _lib.adjust_two_views_angular(tab.copy())
        ta_d = tab.copy()
        tc = time.perf_counter()
        term_d, it_d, _, c1_d, tas = _lib.adjust_two_views_angular(ta_d)
        t_call = time.perf_counter() - tc
        n_cpu_a = 3000
        ta_o = tab.head(n_cpu_a)
        tc = time.perf_counter()
        term_o, it_o, _, c1_o = oracle.adjust_two_views_angular(ta_o)
        t_o = time.perf_counter() - tc
        term_d, it_d = term_d[:n_cpu_a], it_d[:n_cpu_a]
        side["batched_two_view_angular_ba"] = dict(
            kernel_ms=round(tas.kernel_seconds * 1e3, 3), call_ms=round(t_call * 1e3, 2), pairs=int(tab.num_pairs),
            correspondences=int(tab.correspondence_ptr[-1]), lm_iterations=int(tas.total_iterations),
            pairs_per_s=tab.num_pairs / tas.kernel_seconds, cpu_port_pairs_per_s=n_cpu_a / t_o,
            cpu_port_sample=f"first {n_cpu_a} pairs, {oracle.num_threads()} threads",
            termination_mismatches=int((term_d != term_o).sum()), iteration_mismatches=int((it_d != it_o).sum()))
        out["side_kernels"] = side
    solver.close()

    if extras and args.workload == "venice1778_heavy":
        # the same sizes with geometric track lengths only (max 63): round 1's headline workload
        mp = measure("venice1778", args.steps, args.warmup, False)
        mp["solver"].close()
        out["variants"] = {"venice1778-synthetic": dict(
            ms_per_step=round(1e3 * mp["elapsed"] / max(mp["steps_run"], 1), 4), steps=mp["steps_run"],
            value=n_obs * mp["steps_run"] / mp["elapsed"], schur_pairs=int(mp["summary"].num_schur_pairs),
            pcg_iterations=int(mp["pcg"]), final_rmse=mp["summary"].final_rmse)}
        if world == 1:
            # ---- the reference-default operating point: what theia::BundleAdjustReconstruction solves for a caller who
            # changes nothing -- Ceres' SCHUR_JACOBI block shape (one block per parameter block: 6x6 extrinsics + NxN
            # intrinsics per view, bundle_adjustment.h:87), homogeneous points with four free coordinates
            # (bundle_adjuster.cc:379-385), inner iterations on (bundle_adjustment.h:112,
            # reconstruction_estimator_utils.cc:118).  Same problem, same timed-region rules as the headline.
            rd = dict(point_dof=4, preconditioner_type=abi.PRECOND_SCHUR_JACOBI_PARAMETER_BLOCKS, use_inner_iterations=1)
            mr = measure(args.workload, args.steps, args.warmup, False, overrides=rd)
            mr["solver"].close()
            sr = mr["summary"]
            nnzb_r, dc_r = int(sr.num_schur_blocks), int(sr.reduced_block_dim)
            mf_r = float(mr["matrix_free"]) / max(1, mr["steps_run"])
            rows_r = []
            for name, launches, sec in zip(abi.KERNEL_CLASS_NAMES, mr["launches_p"], mr["secs_p"]):
                if launches == 0 or sec <= 0.0:
                    continue
                ab = algorithmic_bytes(name, n_obs, n_cam, n_pts, dc_r, 4, nnzb_r, mf_r)
                rows_r.append(dict(kernel=name, launches=int(launches), ms_per_step=round(1e3 * sec / max(1, mr["steps_run"]), 4),
                                   avg_us=round(1e6 * sec / launches, 2), algorithmic_bytes_per_launch=int(ab),
                                   achieved_GBs=round(ab / (sec / launches) / 1e9, 2)))
            dom_r = max((k for k in rows_r if k["kernel"] != "allreduce"), key=lambda k: k["ms_per_step"])
            out["variants"]["reference_defaults"] = dict(
                settings=dict(preconditioner="SCHUR_JACOBI, one block per parameter block (Ceres' shape)", point_dof=4,
                              use_inner_iterations=1, linear_solver=solver_name, schur_mode=args.schur_mode),
                ms_per_step=round(1e3 * mr["elapsed"] / max(mr["steps_run"], 1), 4), steps=mr["steps_run"],
                value=n_obs * mr["steps_run"] / mr["elapsed"], pcg_iterations=int(mr["pcg"]),
                pcg_iterations_per_lm_iteration=round(mr["pcg"] / max(1, mr["steps_run"]), 2),
                operator_chosen_by_auto=dict(matrix_free_lm_iterations=int(mr["matrix_free"]),
                                             formed_S_lm_iterations=int(mr["steps_run"] - mr["matrix_free"])),
                coordinate_descent_sweeps=int(mr["sweeps"]), accepted_steps=int(mr["accepted"]),
                final_cost=sr.final_cost, final_rmse=sr.final_rmse,
                roofline=dict(bound="hbm", kernel=dom_r["kernel"], achieved=dom_r["achieved_GBs"], peak=HBM_PEAK_GBS,
                              unit="GB/s", frac=round(dom_r["achieved_GBs"] / HBM_PEAK_GBS, 5), avg_us=dom_r["avg_us"],
                              launches=dom_r["launches"], algorithmic_bytes_per_launch=dom_r["algorithmic_bytes_per_launch"],
                              traffic=pmc_traffic(dom_r["kernel"], "venice1778_heavy_reference_defaults", world, mf_r,
                                                  table="pmc_venice1778_heavy_reference_defaults.json"),
                              traffic_source="profiles/pmc_venice1778_heavy_reference_defaults.json (rocprofv3 --pmc passes of "
                                             "tools/refdef_probe.py refdef_auto, stamped with the kernel sources; null when stale)",
                              measured="HIP events on the engine's stream, separate pass with every class timed"),
                kernels=rows_r,
                note="the headline differs from this in three stated settings (merged 9x9 preconditioner block, w fixed, no "
                     "sweeps); with Ceres' block shape PCG needs ~5x the iterations per LM iteration")
            # ... and as a CO-HEADLINE of the top-level line: `value` is quoted on the engine's own
            # best operating point, this is what a Theia caller who changes nothing gets on the same problem
            rdv = out["variants"]["reference_defaults"]
            out["co_headline"] = dict(
                what="the same problem at the reference's default options (reconstruction_estimator_utils.cc:110-133, "
                     "bundle_adjustment.h:78-122: Ceres-shaped SCHUR_JACOBI, 4-dof homogeneous points, inner iterations on)",
                metric="ba_observations_per_sec", value=rdv["value"], ms_per_step=rdv["ms_per_step"], steps=rdv["steps"],
                pcg_iterations_per_lm_iteration=rdv["pcg_iterations_per_lm_iteration"],
                roofline_frac=rdv["roofline"]["frac"], final_rmse=rdv["final_rmse"],
                ratio_to_headline_ms_per_step=round(rdv["ms_per_step"] / max(1e-9, out["ms_per_step"]), 2))
            out["config"]["co_headline_note"] = (
                f"reference-default options on the same problem: {rdv['ms_per_step']:.2f} ms per LM iteration "
                f"({rdv['pcg_iterations_per_lm_iteration']} PCG iterations per LM iteration) -- see co_headline / "
                "variants.reference_defaults")
            # the reference's solver policy below 1000 views is an exact reduced solve
            # (reconstruction_estimator_utils.cc:110-133): SPARSE_SCHUR -> the tiled dense Cholesky of S
            ma = measure("alamo", args.steps, args.warmup, False)
            ma["solver"].close()
            pa = ma["prob"]
            out["variants"]["alamo570-synthetic"] = dict(
                cameras=pa.num_cameras, tracks=pa.num_points, observations=pa.num_observations,
                linear_solver=solver_policy(pa.num_cameras)[1],
                ms_per_step=round(1e3 * ma["elapsed"] / max(ma["steps_run"], 1), 4), steps=ma["steps_run"],
                value=pa.num_observations * ma["steps_run"] / ma["elapsed"], final_rmse=ma["summary"].final_rmse)
            # the exact solve's own roofline: the factorisation is compute, not bytes (n^3 / 3 flops + two triangular
            # solves per launch of the tile-dataflow Cholesky), priced against the dense fp64 MFMA peak
            ic = abi.KERNEL_CLASS_NAMES.index("cholesky")
            if ma["launches_p"][ic]:
                n_s = pa.num_cameras * 9  # (every view has the 9-wide block in this workload)
                fl = n_s ** 3 / 3.0 + 2.0 * n_s ** 2
                us = 1e6 * ma["secs_p"][ic] / ma["launches_p"][ic]
                out["variants"]["alamo570-synthetic"]["roofline"] = dict(
                    bound="mfma", kernel="cholesky (gather + cdf::chol_dataflow_kernel: factorisation and both substitutions)",
                    n=n_s, flops_per_launch=fl, avg_us=round(us, 2), launches=int(ma["launches_p"][ic]),
                    achieved=round(fl / (us * 1e-6) / 1e12, 3), peak=FP64_MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                    frac=round(fl / (us * 1e-6) / 1e12 / FP64_MFMA_PEAK_TFLOPS, 5),
                    share_of_iteration=round(ma["secs_p"][ic] / max(sum(ma["secs_p"]), 1e-30), 4),
                    measured="HIP events on the engine's stream, the untimed pass with every class timed")
            # ---- Venice sizes with SEQUENCE structure (synth scene "street"): neighbouring views share
            # most tracks, distant views none -- S is a band (fill below), and PCG with SCHUR_JACOBI needs tens to
            # hundreds of iterations per LM iteration where the ring scene of the headline needs five.  Headline options,
            # default tolerances (the solve converges), one solve from the perturbed start.
            pv = synth.config("venice1778_street")
            ov = dict(point_dof=3, linear_solver_type=abi.ITERATIVE_SCHUR, use_inner_iterations=0)
            sv = lib.Solver(pv.copy(), abi.default_options(max_num_iterations=2, **ov), 0, 1)
            sv.solve(abi.default_options(max_num_iterations=2, **ov))
            sv.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st_v, sm_v = sv.solve(abi.default_options(max_num_iterations=30, **ov))
            torch.cuda.synchronize()
            t_v = time.perf_counter() - t0
            sv.reset()
            _, sm_vp = sv.solve(abi.default_options(max_num_iterations=30, profile_kernels=1, **ov))
            info_v = sv.operator_info()
            sv.close()
            dv = sm_vp.as_dict()
            nv, pcg_v = int(sm_v.num_iterations), int(sm_v.num_linear_solver_iterations)
            nnzb_v, dc_v = int(sm_v.num_schur_blocks), int(sm_v.reduced_block_dim)
            rows_v = []
            for name, launches, sec in zip(abi.KERNEL_CLASS_NAMES, dv["kernel_launches"], dv["kernel_seconds"]):
                if launches == 0 or sec <= 0.0:
                    continue
                ab = algorithmic_bytes(name, pv.num_observations, pv.num_cameras, pv.num_points, dc_v, 3, nnzb_v, 0.0)
                rows_v.append(dict(kernel=name, launches=int(launches), ms_per_step=round(1e3 * sec / max(1, nv), 4),
                                   avg_us=round(1e6 * sec / launches, 2), algorithmic_bytes_per_launch=int(ab),
                                   achieved_GBs=round(ab / (sec / launches) / 1e9, 2)))
            dom_v = max(rows_v, key=lambda k: k["ms_per_step"])
            out["variants"]["venice_like"] = dict(
                workload="venice1778_street-synthetic", cameras=pv.num_cameras, tracks=pv.num_points,
                observations=pv.num_observations, schur_blocks_upper=nnzb_v,
                S_fill=round((2.0 * (nnzb_v - pv.num_cameras) + pv.num_cameras) / float(pv.num_cameras) ** 2, 4),
                steps=nv, accepted_steps=int(sm_v.num_successful_steps), ms_per_step=round(1e3 * t_v / max(1, nv), 3),
                solve_ms=round(1e3 * t_v, 2), value=pv.num_observations * nv / t_v, pcg_iterations=pcg_v,
                pcg_iterations_per_lm_iteration=round(pcg_v / max(1, nv), 1),
                us_per_pcg_iteration=round(1e6 * t_v / max(1, pcg_v), 1),
                matrix_free_lm_iterations=int(sm_v.num_matrix_free_iterations), engine_paths=info_v,
                initial_rmse=sm_v.initial_rmse, final_rmse=sm_v.final_rmse, status=int(st_v),
                termination=bytes(sm_v.message).split(b"\0")[0].decode(),
                roofline=dict(bound="hbm", kernel=dom_v["kernel"] + " (with the formed S a whole PCG solve is ONE persistent "
                              "launch, pcg_persist.h: a 'launch' of this class is one PCG iteration, product + vector part)",
                              achieved=dom_v["achieved_GBs"], peak=HBM_PEAK_GBS, unit="GB/s",
                              frac=round(dom_v["achieved_GBs"] / HBM_PEAK_GBS, 5), avg_us=dom_v["avg_us"],
                              launches=dom_v["launches"], algorithmic_bytes_per_launch=dom_v["algorithmic_bytes_per_launch"],
                              traffic=None, measured="HIP events on the engine's stream, separate pass with every class timed"),
                kernels=rows_v,
                note="what a sequence-structured collection asks of the path: the LM iteration is the PCG loop")
            # BASELINE config 1 (49 views, 31.8 k observations): DENSE_SCHUR by the reference's policy; a problem
            # this small is bound by launch and read-back latency, not by bytes
            ml = measure("ladybug49", args.steps, args.warmup, False)
            ml["solver"].close()
            pl = ml["prob"]
            out["variants"]["ladybug49-synthetic"] = dict(
                cameras=pl.num_cameras, tracks=pl.num_points, observations=pl.num_observations,
                linear_solver=solver_policy(pl.num_cameras)[1],
                ms_per_step=round(1e3 * ml["elapsed"] / max(ml["steps_run"], 1), 4), steps=ml["steps_run"],
                value=pl.num_observations * ml["steps_run"] / ml["elapsed"], final_rmse=ml["summary"].final_rmse)
            # the shim's default point parameterisation: 4 free homogeneous coordinates per point, as the
            # reference leaves them (bundle_adjuster.cc:379-385); the headline uses 3 (w fixed, the north-star's 2x3 blocks)
            o4 = dict(point_dof=4, linear_solver_type=abi.ITERATIVE_SCHUR, use_inner_iterations=0,
                      function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
            s4 = lib.Solver(prob0.copy(), abi.default_options(max_num_iterations=2, **o4))
            s4.solve(abi.default_options(max_num_iterations=2, **o4))
            s4.reset()
            _, sm4 = s4.solve(abi.default_options(max_num_iterations=10, **o4))
            s4.close()
            out["variants"]["venice1778_heavy_point_dof4-synthetic"] = dict(
                steps=int(sm4.num_iterations), ms_per_step=round(1e3 * sm4.solve_time_in_seconds / max(1, sm4.num_iterations), 3),
                pcg_iterations=int(sm4.num_linear_solver_iterations), final_rmse=sm4.final_rmse)
            # the reference's APPLICATION loss: HUBER of width 10 (applications/build_reconstruction_flags.txt:117-121) on the
            # headline problem and options -- the specialised bodies with the corrector left in and compact planes holding
            # the corrected point plus r^2; round 5 and before: the generic bodies
            oh = dict(point_dof=3, linear_solver_type=abi.ITERATIVE_SCHUR, use_inner_iterations=0, loss_function_type=abi.LOSS_HUBER,
                      robust_loss_width=10.0, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
            sh = lib.Solver(prob0.copy(), abi.default_options(max_num_iterations=2, **oh))
            sh.solve(abi.default_options(max_num_iterations=2, **oh))
            sh.reset()
            _, smh = sh.solve(abi.default_options(max_num_iterations=10, **oh))
            compact_h = sh.operator_info().get("compact_planes", False)
            sh.close()
            out["variants"]["venice1778_heavy_huber10-synthetic"] = dict(
                steps=int(smh.num_iterations), ms_per_step=round(1e3 * smh.solve_time_in_seconds / max(1, smh.num_iterations), 3),
                pcg_iterations=int(smh.num_linear_solver_iterations), final_rmse=smh.final_rmse, compact_planes=bool(compact_h),
                loss="HUBER", robust_loss_width=10.0)
            # BASELINE config 5 at Venice size (synth.config5): mixed camera models, intrinsics shared by 33 groups of 2-200
            # views, fp32 residual evaluation (fp64 accumulation); CLUSTER_JACOBI over {shared block, its views} with the
            # matrix-free operator (schur_mode auto), and SCHUR_JACOBI -- round 2's operating point -- beside it
            p5 = synth.config5()
            o5 = dict(point_dof=3, linear_solver_type=abi.ITERATIVE_SCHUR, residual_precision=32, use_inner_iterations=0,
                      function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
            v5 = dict(cameras=p5.num_cameras, observations=p5.num_observations, shared_intrinsics_groups=int(p5.num_groups),
                      largest_group=int(np.bincount(p5.camera_group).max()))
            for key, pre in (("cluster_jacobi", abi.PRECOND_CLUSTER_JACOBI), ("schur_jacobi", abi.PRECOND_SCHUR_JACOBI)):
                t0 = time.perf_counter()
                s5 = lib.Solver(p5.copy(), abi.default_options(max_num_iterations=2, preconditioner_type=pre, **o5))
                t_create5 = time.perf_counter() - t0
                s5.solve(abi.default_options(max_num_iterations=2, preconditioner_type=pre, **o5))
                s5.reset()
                _, sm5 = s5.solve(abi.default_options(max_num_iterations=8, preconditioner_type=pre, **o5))
                s5.close()
                v5[key] = dict(steps=int(sm5.num_iterations),
                               ms_per_step=round(1e3 * sm5.solve_time_in_seconds / max(1, sm5.num_iterations), 3),
                               pcg_iterations=int(sm5.num_linear_solver_iterations),
                               matrix_free_iterations=int(sm5.num_matrix_free_iterations),
                               schur_blocks_formed=int(sm5.num_schur_blocks), final_rmse=sm5.final_rmse,
                               create_seconds=round(t_create5, 3))
            out["variants"]["config5_mixed_models_shared_intrinsics_fp32-synthetic"] = v5
    print(json.dumps(out))


if __name__ == "__main__":
    main()
