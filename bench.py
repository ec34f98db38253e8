#!/usr/bin/env python3
"""
Benchmark of the MI355X hot path on BASELINE.json's headline configuration:
1e6 landmarks x 4 cameras per GPU (configs[1]); synthetic scene of SURVEY.md 8(d).

One STEP = one pass of the triangulation hot path over the rank's resident batch:
linear-LS (DLT) + Hartley-Sturm iterative-LS over all landmarks (one fused launch producing both), followed -- once the BA
kernels are built in (see `ba` in the output) -- by one Gauss-Newton iteration of bundle
adjustment (linearise + Schur + reduce + solve + back-substitute) on the same landmarks.
Inputs are resident in HBM before the timed region.  `value` = landmarks (all ranks) / step.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--landmarks L] [--cams C] [--dump-outputs DIR] [--full]

A plain run sets up, runs the steps (below), writes --dump-outputs if given and prints ONE JSON line: metric, value,
ms_per_step, config.  --full then runs every other leg as well (the objects below, `value_cold`, and at N > 1 `ba_strong`)
and prints the compact headline of them all, every leg in full going to bench_details.json and stderr.

N > 1: one rank per GPU.  `python bench.py --gpus N` starts its own ranks (child `python -m torch.distributed.run`, the
parent never touches the GPU) unless it already runs under torch.distributed.run (WORLD_SIZE set).  Landmarks shard
across ranks, no data-path collective for triangulation, one RCCL all-reduce of the reduced camera system per BA iteration,
issued from C on the kernels' stream (mqs_ba_gn_iteration_dev; `transport` in the output).
  --scaling weak    (default) every rank holds L landmarks of its own scene: BASELINE configs[1] per GPU.
  --scaling strong  ONE scene of L landmarks, rank r holds sharding.landmark_shard(L, r, N): BASELINE configs[3].
At N > 1 the weak run also reports configs[3] as `ba_strong`: the 1e6-landmark problem sharded N-way, 10 GN iterations,
with the poses checked against the same problem solved by ONE rank (<= 1e-10).

Extra objects on the JSON line under --full:
  roofline     -- the step's dominant kernel, the BA lineariser (`ba_linearize_wave_kernel<4, true>`, 0.55 of the step): counted
                  fp64 flop per launch / average launch duration from hipEvents on the launch stream against the 78.6 TFLOP/s
                  fp64 vector peak (what binds it), with the HBM view of the same launch (`roofline.hbm`: algorithmic bytes and
                  PMC traffic against 8 TB/s) beside it.
  rooflines    -- the same for every kernel of the step, the BA kernels and the matcher (MFMA bound).
  asymptote    -- SURVEY 8(d)'s second size, 1e7 landmarks x 4 cameras: the triangulation kernels and one BA iteration.
  frontend     -- corner detection + pyramidal LK on a rendered VGA frame pair (kernel time); the per-frame loop (configs[4]) on the
                  rendered sequence and on the reference's example sequence, each with the frames resident beforehand
                  (`frames_per_s`) and arriving inside the timed loop (`frames_per_s_with_upload`).
  replay       -- the per-frame SLAM loop replayed from the reference's recorded tracks (frames/s).
  cpu_baseline -- the oracle's plain-C port of the reference kernel (oracle/c/tri_oracle.c),
                  single thread as the reference ships it, same step on the same arrays
                  (rank 0, N = 1 only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_VALU_PEAK_TFLOPS = 78.6    # same guide: 256 CUs x 4 SIMDs x 16 fp64 FMA lanes x 2 flop x 2.4 GHz (vector, not matrix)


def _evidence():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evidence_stamp
    return evidence_stamp


def kernel_flops():
    """fp64 flop and VALU instructions per landmark of the fp64-bound kernels, counted from the gfx950 ISA by
    tools/isa_mix.py (static count x loop trip counts; FMA = 2 flop): profiles/kernel_flops.json.  A record whose `source`
    digest no longer matches the kernel sources of this tree is dropped (tools/evidence_stamp.py): the caller then reports
    the figure as null instead of a constant that has outlived its kernel."""
    try:
        data = json.load(open(os.path.join(ROOT, "profiles", "kernel_flops.json")))
        ev = _evidence()
        return {k: v for k, v in data.items() if isinstance(v, dict) and ev.is_current(v.get("source"))}
    except Exception:
        return {}


def pmc_traffic():
    """profiles/pmc_traffic.json with the per-kernel-family figures whose sources have changed since the PMC pass removed:
    (record, stale_families)."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        ev = _evidence()
        stale = [fam for fam in ("ba", "tri") if not ev.is_current(rec.get("sources", {}).get(fam))]
        for key in list(rec):
            if (key.startswith("ba_") and "ba" in stale) or (key.startswith(("iterative_ls", "linear_ls", "linear_eigen")) and "tri" in stale):
                rec[key] = None
        if "tri" in stale and isinstance(rec.get("valu"), dict):
            rec["valu"]["iterative_ls"] = None
        if "ba" in stale and isinstance(rec.get("valu"), dict):
            rec["valu"]["ba_linearize_schur"] = None
        return rec, stale
    except Exception:
        return {}, ["ba", "tri"]


# dmabuf IPC is the only kind this pool's driver supports: without it RCCL / peer mappings across processes fail with
# hipIpcGetMemHandle: invalid argument.  Set before anything can initialise HIP in this process (torch is imported inside main()).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def ba_strong_leg(mq, np, torch, total, C, rank, world, dev, group, dist, iters=10):
    """BASELINE configs[3]: ONE scene of `total` landmarks x C cameras, rank r holds sharding.landmark_shard(total, r, world)
    (contiguous ranges: the reference's `omp parallel for` axis, triangulation.c:70,109; graph bundle_adjust.cpp:289-298),
    `iters` Gauss-Newton iterations with one all-reduce of the reduced camera system each.  The poses every rank ends with
    are compared with the same problem solved by rank 0 alone."""
    syn, sh, D = mq.synthetic, mq.sharding, mq.device
    u_all, P, _ = syn.triangulation_problem(total, C, seed=syn.RSEED + 7)
    Pd = torch.from_numpy(np.ascontiguousarray(P)).to(dev)

    def problem(lo, hi, grp):
        us = np.ascontiguousarray(u_all[:, lo:hi])
        x0, _ = D.iterative_LS_triangulation(torch.from_numpy(us).to(dev), Pd)
        return mq.bundle_adjustment.make_benchmark_problem(us, P, x0, dev, seed=syn.RSEED, process_group=grp,
                                                           prior_first=4 if lo == 0 else 0)

    def fence():
        dist.barrier()
        torch.cuda.synchronize()

    a, b = sh.landmark_shard(total, rank, world)
    problem(a, b, group).gauss_newton_iterations(2)              # warm-up on a throw-away copy of the shard
    ba = problem(a, b, group)
    c0 = ba.total_cost()
    fence()
    t0 = time.perf_counter()
    ba.gauss_newton_iterations(iters)
    fence()
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    dt = float(dt.item())
    c1 = ba.total_cost()
    # the collective by itself: back-to-back all-reduces of the 602-double system on the kernels' stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = torch.zeros_like(ba.lin)
    red = (lambda: group.all_reduce_sum_(probe)) if isinstance(group, sh.CComm) else (lambda: dist.all_reduce(probe))
    red()
    fence()
    e0.record()
    for _ in range(20):
        red()
    e1.record()
    e1.synchronize()
    ar_us = e0.elapsed_time(e1) / 20 * 1e3
    # every rank solved the same reduced system: identical poses everywhere, and equal to the one-rank solution
    mine = ba.poses.clone()
    lo_, hi_ = mine.clone(), mine.clone()
    dist.all_reduce(lo_, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi_, op=dist.ReduceOp.MAX)
    same = bool(torch.equal(lo_, hi_))
    diff = cost_one = None
    if rank == 0:
        one = problem(0, total, None)
        one.gauss_newton_iterations(iters)
        torch.cuda.synchronize()
        diff = float((one.poses - mine).abs().max().item())
        cost_one = one.total_cost()
    fence()
    return {"workload": "BASELINE configs[3]: %d landmarks x %d cameras sharded %d-way (contiguous landmark ranges), %d Gauss-Newton "
                        "iterations, one all-reduce of (6C)^2+6C+2 doubles per iteration" % (total, C, world, iters),
            "landmarks_total": total, "landmarks_per_gpu": b - a, "iterations": iters, "ms_per_iter": round(1e3 * dt / iters, 4),
            "gn_iters_per_s": round(iters / dt, 1), "landmarks_per_s": round(total * iters / dt),
            "all_reduce_us": round(ar_us, 2), "rccl_world_size": dist.get_world_size(), "backend": dist.get_backend(),
            "cost_before": c0, "cost_after": c1, "cost_after_one_rank": cost_one,
            "poses_identical_on_all_ranks": same, "max_abs_pose_diff_vs_one_rank": diff,
            "ok": (same and diff is not None and diff <= 1e-10) if rank == 0 else None}


def headline(out, details_path):
    """The contract line: metric / value / config / roofline / cpu_baseline in full, one or two numbers of every other leg."""
    g = lambda d, *ks: (g(d.get(ks[0]), *ks[1:]) if len(ks) > 1 else d.get(ks[0])) if isinstance(d, dict) else None
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "clock_settle_steps", "ms_per_step", "ms_per_step_cold", "value_cold",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
    h = {k: out[k] for k in keep}
    r = out.get("roofline") or {}
    h["roofline"] = {k: r[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "hbm") if k in r}
    c = out.get("cpu_baseline")
    if c:
        h["cpu_baseline"] = {"value": c["value"], "unit": c["unit"], "cores": c["cores"], "kind": c["kind"], "sample": c["sample"],
                             "all_cores": g(c, "all_cores", "value"), "ba_gn_iters_per_s_all_cores": g(c, "ba", "gn_iters_per_s"),
                             "parity": c.get("parity")}
    else:
        h["cpu_baseline"] = None
    b = out.get("ba") or {}
    h["ba"] = {"gn_iters_per_s": b.get("gn_iters_per_s"), "ms_per_iter": b.get("ms_per_iter"), "landmarks_total": b.get("landmarks_total"),
               "shard_proxy": {"ms_per_iter": g(b, "shard_proxy", "ms_per_iter"), "landmarks": g(b, "shard_proxy", "landmarks")},
               "from_perturbed_start_ms_per_iter": g(b, "from_perturbed_start", "ms_per_iter")} if b else None
    rl = out.get("rooflines") or {}
    h["rooflines_frac"] = {k: v.get("frac") for k, v in rl.items() if isinstance(v, dict)}
    a = out.get("asymptote") or {}
    h["asymptote_1e7"] = {"linear_ls_GBps": g(a, "linear_ls", "GBps"), "iterative_ls_ms": g(a, "iterative_ls", "ms"), "ba_ms_per_iter": g(a, "ba_gn_iteration", "ms_per_iter"),
                          "error": a.get("error"), "skipped": a.get("skipped")} if a else None
    m = out.get("match") or {}
    h["match"] = {"f16_frac_of_peak": m.get("frac_of_peak"), "fp4_frac_of_peak": g(m, "packed_bits_fp4", "frac_of_peak"), "ms_per_pair": m.get("ms_per_pair"),
                  "fp4_ms_per_pair": g(m, "packed_bits_fp4", "ms_per_pair")}
    f = out.get("frontend") or {}
    ba60 = f.get("end_to_end_loop_device_resident_ba_per_keyframe") or {}
    icl = f.get("reference_example_sequence_icl_nuim_80_frames") or {}
    icl200 = f.get("reference_example_sequence_icl_nuim_200_frames") or {}
    icl_ba, icl200_ba = icl.get("ba_per_keyframe") or {}, icl200.get("ba_per_keyframe") or {}
    r400 = f.get("rendered_400_frames_ba_per_keyframe_with_upload") or {}
    # frames/s of the loop legs: WITH the frames arriving inside the timed loop (the reference reads every frame inside its loop,
    # slam2.py:1209-1213); `resident` beside it = every frame on the device before the clock starts
    h["loop"] = {
        "rendered_60_frames": {"plain_frames_per_s": g(f, "end_to_end_loop_device_resident", "frames_per_s_with_upload"),
                               "plain_frames_per_s_resident": g(f, "end_to_end_loop_device_resident", "frames_per_s"),
                               "ba_per_keyframe_frames_per_s": ba60.get("frames_per_s_with_upload"), "ba_per_keyframe_frames_per_s_resident": ba60.get("frames_per_s"),
                               "engine": g(ba60, "bundle_adjust_per_keyframe", "engine"),
                               "adjust_ms_median": g(ba60, "bundle_adjust_per_keyframe", "ms_per_adjustment_median", "adjust_ms"),
                               "rmse_plain": g(f, "end_to_end_loop_device_resident", "trajectory_rmse"), "rmse_ba": ba60.get("trajectory_rmse")},
        "rendered_400_frames": {"ba_per_keyframe_frames_per_s": r400.get("frames_per_s"), "engines": r400.get("engines"), "rmse_ba": r400.get("trajectory_rmse"),
                                "poses_per_adjustment_max": r400.get("poses_per_adjustment_max")} if r400 else None,
        "icl_nuim_80_frames": {"plain_frames_per_s": g(icl, "plain", "frames_per_s_with_upload"), "plain_frames_per_s_resident": g(icl, "plain", "frames_per_s"),
                               "ba_per_keyframe_frames_per_s": icl_ba.get("frames_per_s_with_upload"), "ba_per_keyframe_frames_per_s_resident": icl_ba.get("frames_per_s"),
                               "rmse_m_plain_ba_reference": [g(icl, "plain", "ours_vs_groundtruth_rmse_m"), icl_ba.get("ours_vs_groundtruth_rmse_m"),
                                                              g(icl, "plain", "reference_vs_groundtruth_rmse_m")]},
        "icl_nuim_200_frames": {"plain_frames_per_s": g(icl200, "plain", "frames_per_s_with_upload"), "plain_frames_per_s_resident": g(icl200, "plain", "frames_per_s"),
                                "ba_per_keyframe_frames_per_s": icl200_ba.get("frames_per_s_with_upload"), "ba_per_keyframe_frames_per_s_resident": icl200_ba.get("frames_per_s"),
                                "ba_every_frame_frames_per_s_resident": g(icl200, "ba_per_keyframe_every_frame", "frames_per_s"),
                                "ba_four_seeds_rmse_m": g(icl200, "ba_per_keyframe_four_seeds", "rmse_m"),
                                "rmse_m_plain_ba_reference": [g(icl200, "plain", "ours_vs_groundtruth_rmse_m"), icl200_ba.get("ours_vs_groundtruth_rmse_m"),
                                                               g(icl200, "plain", "reference_vs_groundtruth_rmse_m")]} if icl200 else None,
        "cpu_baseline": None, "cpu_baseline_note": "no CPU baseline for the loop legs (the reference's loop cannot run here): bench_details.json",
        "error": f.get("error")}
    h["sparse_ba"] = {"linearize_plus_solve_ms": g(out, "sparse_ba", "linearize+solve_ms"), "lm_ms": g(out, "sparse_ba", "lm_ms"), "n": g(out, "sparse_ba", "n")}
    t = out.get("transport")
    h["transport"] = t if t is None or len(t) <= 160 else t[:157] + "..."
    st = out.get("ba_strong")
    h["ba_strong"] = None if not st else {k: st.get(k) for k in ("landmarks_total", "landmarks_per_gpu", "iterations", "ms_per_iter", "gn_iters_per_s",
                                                                  "all_reduce_us", "rccl_world_size", "backend", "cost_before", "cost_after",
                                                                  "cost_after_one_rank", "poses_identical_on_all_ranks", "max_abs_pose_diff_vs_one_rank",
                                                                  "ok", "transport", "ba_strong_transports") if k in st}
    h["details"] = os.path.basename(details_path) if details_path else "stderr"
    return h


DUMP_ROWS = 1 << 18                 # landmarks per array in a --dump-outputs file: 3 x 6.3 MB + 2 MB + 1 MB in all at most


def dump_outputs(path, x_ls, x_it, st, ba, rows=DUMP_ROWS, seed=2024):
    """--dump-outputs: what the timed step hands its caller after its last step, as path/<name>.npy (rank 0's arrays):
    linear_ls_points / iterative_ls_points (N, 3) f64 and iterative_ls_status (N,) as f32 from the triangulation pass, and
    from the Gauss-Newton iteration ba_poses (C, 12) f64 and ba_points (N, 3) f64.  Past `rows` landmarks every per-landmark
    array holds the same fixed, seeded, sorted sample of rows, whose indices are landmark_index (f64, exact)."""
    import numpy as np
    import torch
    n = x_it.shape[0]
    idx = np.arange(n) if n <= rows else np.sort(np.random.default_rng(seed).choice(n, rows, replace=False))
    sel = torch.from_numpy(idx).to(x_it.device)
    arrays = {"landmark_index": idx.astype(np.float64),
              "linear_ls_points": x_ls[sel].double(), "iterative_ls_points": x_it[sel].double(), "iterative_ls_status": st[sel].float()}
    if ba is not None:
        arrays["ba_poses"] = ba.poses.double()
        arrays["ba_points"] = ba.points[sel].double()
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a if isinstance(a, np.ndarray) else a.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle-steps", type=int, default=400,
                    help="untimed steps before the warm-up, for the clock to reach its steady state under load (~90 ms)")
    ap.add_argument("--landmarks", type=int, default=1_000_000)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ba", action="store_true")
    ap.add_argument("--one-stream", action="store_true", help="triangulation and BA on one stream (A/B of the two-stream step)")
    ap.add_argument("--no-match", action="store_true")
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--no-frontend", action="store_true")
    ap.add_argument("--no-asymptote", action="store_true", help="skip the 1e7-landmark leg (SURVEY 8(d)'s second size)")
    ap.add_argument("--no-shard-proxy", action="store_true",
                    help="skip the 125 k-landmark legs of `ba` (profiler runs: every BA kernel then sees ONE problem size)")
    ap.add_argument("--descriptors", type=int, default=65536)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--strong-landmarks", type=int, default=1_000_000, help="total landmarks of the ba_strong leg (N > 1)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps, every other leg as well: the cold timed region, per-kernel timings and rooflines, "
                         "the 1e7 asymptote, the BA reports, matcher, replay, front-end loops, sparse BA, CPU baselines and, at N > 1, "
                         "ba_strong (the --no-* options trim this set); every leg in full goes to bench_details.json and stderr")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started by hand: become the launcher.  Nothing here has touched HIP (no torch import, no library load), and the
        # ranks are fresh child processes -- never an exec from a process that holds the GPU.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd, env=env).returncode)

    # everything that may need a compiler runs BEFORE the first GPU call (a child `make` started later would inherit an
    # initialised-GPU parent's profiler preload); both builders are no-ops when their library is up to date
    want_cpu = args.full and (not args.no_cpu_baseline) and int(os.environ.get("WORLD_SIZE", "1")) == 1
    if want_cpu:
        from oracle import c_oracle
        c_oracle.build()

    import numpy as np
    import torch
    import mqslam_amd

    if not mqslam_amd.loaded:
        raise SystemExit("libmqslam_hip.so is not available: %r" % (mqslam_amd._lib.load_error,))

    dist = None
    sh = mqslam_amd.sharding
    rank, local_rank, world = sh.init_from_env(backend="nccl")
    args.gpus = world
    transport, group = None, None
    multi = world > 1 or os.environ.get("MQS_FORCE_DIST", "0") == "1"       # the latter: the N-GPU code path with one rank (tests)
    if multi:
        import torch.distributed as dist
        group, transport = True, "torch.distributed(%s)" % dist.get_backend()
        if dist.get_backend() == "nccl" and os.environ.get("MQS_TRANSPORT", "c") in ("c", "rccl"):
            # the library's own transport: the reduced system travels as plain stores into receive buffers the ranks map from each
            # other (csrc/comm.hip: the send side rides in the lineariser's finalize kernel, the wait and the rank-ordered sum in the
            # fused solve / back-substitution kernel -- no collective launch), with an RCCL communicator in the same context for
            # what does not fit a row.  It is verified against torch.distributed's sum before use.  Every rank records its own
            # outcome and the ranks AGREE on it in collectives that all of them reach (a rank-local exception must not leave the
            # others waiting inside one); any failure keeps the torch transport (still RCCL).
            dev0 = torch.device("cuda", local_rank)
            cc, err = None, ""
            try:
                cc = sh.init_c_comm(rank, world, local_rank, peer=os.environ.get("MQS_TRANSPORT", "c") == "c")
            except Exception as e:                              # noqa: BLE001 -- init_c_comm itself agrees before it raises
                err = str(e)[:120]
            def agreed(flag):
                t = torch.tensor([1.0 if flag else 0.0], device=dev0)
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                return t.item() == 1.0

            def collective_verifies():
                """The library's all-reduce (whatever transports the context holds) against torch.distributed's, exact integers."""
                probe = torch.arange(602, dtype=torch.float64, device=dev0) * (rank + 1)
                want = probe.clone()
                dist.all_reduce(want)
                good = False
                if cc is not None:
                    try:
                        cc.all_reduce_sum_(probe)
                        torch.cuda.synchronize()
                        good = bool(torch.equal(probe, want)) and not (cc.peer_state() and cc.peer_timed_out())
                    except Exception as e:                      # noqa: BLE001
                        nonlocal_err.append(str(e)[:120])
                return agreed(good)

            def fused_iteration_verifies():
                """Three one-call Gauss-Newton iterations of a small sharded problem over the context's transport -- over the peer
                transport that is the path with the send side in the finalize kernel and the wait in the tail -- against the same
                iterations with torch.distributed's all-reduce between the two halves: poses equal to 1e-9, no timed-out row."""
                us, Ps, ps = mqslam_amd.synthetic.triangulation_problem(4096, 4, seed=mqslam_amd.synthetic.RSEED + 31 * rank)
                mk = lambda pg: mqslam_amd.bundle_adjustment.make_benchmark_problem(
                    us, Ps, ps + 0.01, dev0, seed=mqslam_amd.synthetic.RSEED, process_group=pg, prior_first=4 if rank == 0 else 0)
                # the two runs apart, the ranks agreeing in between: a rank whose peer wait gave up (MQS_E_TIMEOUT raises) must not be
                # in the agreement's collective while the others are inside the reference run's all-reduce
                ran, a = False, None
                try:
                    a = mk(cc)
                    a.gauss_newton_iterations(3)
                    torch.cuda.synchronize()
                    ran = not (cc.peer_state() and cc.peer_timed_out())
                except Exception as e:                          # noqa: BLE001
                    nonlocal_err.append(str(e)[:120])
                if not agreed(ran):
                    return False
                good = False
                try:
                    b = mk(True)
                    b.gauss_newton_iterations(3)
                    torch.cuda.synchronize()
                    good = float((a.poses - b.poses).abs().max().item()) <= 1e-9
                except Exception as e:                          # noqa: BLE001
                    nonlocal_err.append(str(e)[:120])
                return agreed(good)

            nonlocal_err = [err] if err else []
            use = collective_verifies()
            if use and cc.peer_state() and not fused_iteration_verifies():
                # the collective by itself is right but the fused path is not: drop the peer transport, keep the RCCL communicator
                mqslam_amd._lib.lib().mqs_comm_peer_close(cc.ctx.handle)
                cc.transport = "rccl"
                nonlocal_err.append("the fused peer path did not reproduce torch.distributed's iterations: peer transport closed")
                use = collective_verifies()
            if use:
                group = cc
                transport = ("peer stores over xGMI via the C ABI (mqs_comm_peer_*: send side in the finalize kernel, wait + rank-ordered "
                             "sum in the fused tail of mqs_ba_gn_iteration_dev; RCCL communicator beside it)" if cc.peer_state() else
                             "rccl via the C ABI (mqs_comm_*, all-reduce issued inside mqs_ba_gn_iteration_dev)")
                if nonlocal_err:
                    transport += " [%s]" % "; ".join(nonlocal_err)
            else:
                transport += " (C-ABI transport not used: %s)" % ("; ".join(nonlocal_err) or "its sum differs from torch.distributed's on some rank",)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    if multi and world == 1:
        torch.cuda.set_device(0)

    C = args.cams
    syn = mqslam_amd.synthetic
    strong = args.scaling == "strong" and world > 1
    if strong:
        # one scene, rank r holds its contiguous landmark range (the reference's own `omp parallel for` axis, triangulation.c:70,109)
        N_total = args.landmarks
        a, b = sh.landmark_shard(N_total, rank, world)
        u_all, P, pts_all = syn.triangulation_problem(N_total, C, seed=syn.RSEED)
        u, pts = np.ascontiguousarray(u_all[:, a:b]), pts_all[a:b]
        N = b - a
        del u_all, pts_all
    else:
        N = args.landmarks
        N_total = N * world
        u, P, pts = syn.triangulation_problem(N, C, seed=syn.RSEED + 1000 * rank)
    ud = torch.from_numpy(u).to(dev)
    Pd = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
    x_ls = torch.empty((N, 3), dtype=torch.float64, device=dev)
    x_it = torch.empty((N, 3), dtype=torch.float64, device=dev)
    st = torch.empty((N,), dtype=torch.int32, device=dev)
    D = mqslam_amd.device

    ba = None
    if not args.no_ba:
        # initial landmarks = iterative-LS output; poses are replicated, so their
        # perturbation uses the same seed on every rank
        D.iterative_LS_triangulation(ud, Pd, out=x_it, out_status=st)
        ba = mqslam_amd.bundle_adjustment.make_benchmark_problem(
            u, P, x_it, dev, seed=syn.RSEED, process_group=group if multi else None,
            prior_first=4 if (rank == 0 or not strong) else 0)

    def triangulate():
        # both least-squares methods in one pass over the observations: the first solve of the iteration (unit weights) is
        # the linear-LS system, so x_ls costs one refinement step instead of a second read (bit-identical x_it / status,
        # x_ls equal to the stand-alone kernel to rounding: tests/test_triangulation_gpu.py)
        D.linear_and_iterative_LS_triangulation(ud, Pd, out_ls=x_ls, out_it=x_it, out_status=st)

    # The triangulation pass and the BA iteration of a step are independent pipelines (the BA state was seeded from an
    # earlier triangulation): the triangulation goes to its own HIP stream, where it fills what the BA chain leaves idle
    # -- the single-wavefront reduced-system solve (12 us), the 6-workgroup finalize, the all-reduce wait at N > 1, the
    # launch gaps.  Both streams are drained by the device-wide synchronize that brackets the timed region.
    side_priority = int(os.environ.get("MQS_BENCH_SIDE_PRIORITY", "0"))      # (A/B: -1 = a high-priority stream, i.e. a hardware queue that cannot be the BA chain's)
    side = torch.cuda.Stream(device=dev, priority=side_priority) if (ba is not None and not args.one_stream) else None

    # The BA chain -- the step's critical path -- on a high-priority stream of its own: streams of different priority never share a hardware
    # queue, whatever the process has created and destroyed before (two streams on one queue run one behind the
    # other).  Measured equal to the default stream when the queues do not collide (0.1764 / 0.1765 ms per step; MQS_BENCH_BA_PRIORITY=0: A/B).
    ba_stream = torch.cuda.Stream(device=dev, priority=-1) if (side is not None and os.environ.get("MQS_BENCH_BA_PRIORITY", "-1") == "-1") else None

    def step():
        if side is not None:
            with torch.cuda.stream(side):
                triangulate()
            if ba_stream is not None:
                with torch.cuda.stream(ba_stream):
                    ba.gauss_newton_iteration()
            else:
                ba.gauss_newton_iteration()
        elif ba is not None:
            ba.gauss_newton_iteration(overlap=triangulate)     # one stream: issued inside the all-reduce window
        else:
            triangulate()

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_steps(k):
        fence()
        t0 = time.perf_counter()
        for _ in range(k):
            step()
        fence()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    # Two timed regions, both W untimed warm-up steps followed by exactly K steps between barrier + synchronize, MAX over ranks:
    #   cold     what a fresh process gives right after the contract's W warm-up steps (`ms_per_step_cold`, `value_cold`);
    #   settled  the same after `--settle-steps` further untimed steps (the same steps as the timed ones).  The part raises its
    #            clock over the first ~50-100 ms of sustained load: W = 5 warm-up steps end inside that ramp (0.223 against 0.199
    #            ms per step in round 2).  `value` / `ms_per_step` are the SETTLED figures -- the steady state a job that runs for
    #            more than a tenth of a second sees; `value_from` says so in the line and the cold figure stands beside it.
    # The cold region is timed under --full only; a plain run issues the same K steps untimed, so that the settled figure and
    # the BA state the timed steps leave (--dump-outputs) follow the same sequence of steps in both modes.
    for _ in range(args.warmup):
        step()
    if args.full:
        elapsed_cold = timed_steps(args.steps)
    else:
        for _ in range(args.steps):
            step()
    for _ in range(args.settle_steps):
        step()
    fence()
    for _ in range(args.warmup):
        step()
    elapsed = timed_steps(args.steps)

    ms_per_step = 1e3 * elapsed / args.steps
    value = N_total / (elapsed / args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, x_ls, x_it, st, ba)
    line = {
        "metric": "triangulated landmarks/sec (linear-LS DLT + iterative-LS per landmark"
                  + (" + 1 BA Gauss-Newton iteration" if ba is not None else "")
                  + "), 1e6 pts x 4 cams per GPU; BA GN iters/sec in `ba`",
        "value": round(value), "unit": "landmarks/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "clock_settle_steps": args.settle_steps, "ms_per_step": round(ms_per_step, 4),
        "value_from": "ms_per_step: %d warm-up + %d timed steps after %d untimed clock-settling steps" % (args.warmup, args.steps, args.settle_steps),
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": ("BASELINE configs[3] shape: ONE scene of %d landmarks x %d cameras sharded %d-way, linear-LS + "
                                "iterative-LS + 1 GN iteration per step" % (N_total, C, world)) if strong else
                               ("BASELINE configs[1]: %d landmarks x %d cameras per GPU, linear-LS + "
                                "iterative-LS (tol 3e-5, <=10 iterations)" % (N, C)),
                   "landmarks_per_gpu": N, "landmarks_total": N_total, "cameras": C, "sharding": "landmarks, %d-way" % world},
    }
    if not args.full:
        # a plain run: the headline and nothing else (every other leg: --full)
        if rank == 0:
            print(json.dumps(dict(line, transport=transport)), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    ms_per_step_cold = 1e3 * elapsed_cold / args.steps
    value_cold = N_total / (elapsed_cold / args.steps)

    # ---- per-kernel durations with hipEvents on the launch stream (rank 0 reports) ----
    reps = 20
    ms_it = D.time_triangulation("iterative_ls", ud, Pd, reps=reps)
    ms_ls = D.time_triangulation("linear_ls", ud, Pd, reps=reps)
    ms_eg = D.time_triangulation("linear_eigen", ud, Pd, reps=reps)
    ud32 = ud.float()                             # "also report an fp32-u variant" (widened on load)
    ms_ls32 = D.time_triangulation("linear_ls", ud32, Pd, reps=reps)
    ms_it32 = D.time_triangulation("iterative_ls", ud32, Pd, reps=reps)
    del ud32
    bytes_it = N * (16 * C + 24 + 4)            # 92 B/landmark at C = 4
    bytes_ls = N * (16 * C + 24)
    bytes_eg = N * (16 * C + 24 + 1)
    achieved = bytes_it / (ms_it * 1e-3) / 1e9
    traffic = None
    valu = None
    pmc_rec, pmc_stale = pmc_traffic()
    if pmc_rec.get("landmarks") == N and pmc_rec.get("cams") == C:
        traffic = pmc_rec.get("iterative_ls_hbm_bytes_per_launch")
        valu = pmc_rec.get("valu")
    valu_it = dict((valu or {}).get("iterative_ls") or {})
    if valu_it.get("fp64_flop_per_landmark_static_count"):
        tf = valu_it["fp64_flop_per_landmark_static_count"] * N / (ms_it * 1e-3) / 1e12
        valu_it["fp64_TFLOPs_at_measured_time"] = round(tf, 1)
        valu_it["frac_of_fp64_vector_peak_78.6TF"] = round(tf / FP64_VALU_PEAK_TFLOPS, 3)
    roofline_it = {"bound": "hbm", "kernel": "tri_kernel<%d, iterative_ls>" % C, "achieved": round(achieved, 1),
                   "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4),
                   "traffic": traffic, "algorithmic_bytes_per_launch": bytes_it, "avg_launch_ms": round(ms_it, 5),
                   "valu_pmc": valu_it or None}
    kernels = {
        "iterative_ls": {"ms": round(ms_it, 5), "landmarks_per_s": round(N / (ms_it * 1e-3)),
                         "GBps": round(bytes_it / (ms_it * 1e-3) / 1e9, 1)},
        "linear_ls": {"ms": round(ms_ls, 5), "landmarks_per_s": round(N / (ms_ls * 1e-3)),
                      "GBps": round(bytes_ls / (ms_ls * 1e-3) / 1e9, 1)},
        "linear_eigen": {"ms": round(ms_eg, 5), "landmarks_per_s": round(N / (ms_eg * 1e-3)),
                         "GBps": round(bytes_eg / (ms_eg * 1e-3) / 1e9, 1)},
        "linear_ls_f32_observations": {"ms": round(ms_ls32, 5), "landmarks_per_s": round(N / (ms_ls32 * 1e-3)),
                                       "GBps": round(N * (8 * C + 24) / (ms_ls32 * 1e-3) / 1e9, 1),
                                       "algorithmic_bytes_per_landmark": 8 * C + 24},
        "iterative_ls_f32_observations": {"ms": round(ms_it32, 5), "landmarks_per_s": round(N / (ms_it32 * 1e-3))},
    }
    # ---- "also 1e7 x 4 to show the asymptote" -- the same kernels on ten times the landmarks (rank 0, N = 1) ----
    asymptote = None
    # (not under a profiler: its launches of the SAME kernels at ten times the size would enter the per-kernel averages of the
    # kernel table that is held against this line's avg_launch_ms)
    under_profiler = any(k.startswith(("ROCP_", "ROCPROF", "ROCPROFILER")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")
    if rank == 0 and world == 1 and not args.no_asymptote and N == 1_000_000 and under_profiler:
        asymptote = {"skipped": "under a profiler (the 1e7 launches would enter the 1e6 kernels' averages); profiles/r06 holds the leg from a plain run"}
    elif rank == 0 and world == 1 and not args.no_asymptote and N == 1_000_000:
        try:
            Na = 10 * N
            ua, Pa, _ = syn.triangulation_problem(Na, C)
            uad = torch.from_numpy(ua).to(dev)
            ms = {k: D.time_triangulation(k, uad, Pd, reps=5) for k in ("linear_ls", "iterative_ls")}
            xa, _ = D.iterative_LS_triangulation(uad, Pd)
            asymptote = {"landmarks": Na, "cams": C,
                         "linear_ls": {"ms": round(ms["linear_ls"], 4), "landmarks_per_s": round(Na / (ms["linear_ls"] * 1e-3)),
                                       "GBps": round(Na * (16 * C + 24) / (ms["linear_ls"] * 1e-3) / 1e9, 1),
                                       "frac_of_hbm_peak": round(Na * (16 * C + 24) / (ms["linear_ls"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)},
                         "iterative_ls": {"ms": round(ms["iterative_ls"], 4), "landmarks_per_s": round(Na / (ms["iterative_ls"] * 1e-3)),
                                          "GBps": round(Na * (16 * C + 28) / (ms["iterative_ls"] * 1e-3) / 1e9, 1)}}
            if ba is not None:
                big = mqslam_amd.bundle_adjustment.make_benchmark_problem(ua, P, xa, dev, seed=syn.RSEED)
                ms_ba = mqslam_amd.bundle_adjustment.time_iterations(big, iters=20, warm=5)
                asymptote["ba_gn_iteration"] = {"ms_per_iter": round(ms_ba, 4), "gn_iters_per_s": round(1e3 / ms_ba, 1),
                                                "landmarks_per_s": round(Na / (ms_ba * 1e-3)), "GBps_algorithmic": round(Na * 200 / (ms_ba * 1e-3) / 1e9, 1)}
                del big
            del uad, xa, ua
            torch.cuda.empty_cache()
        except Exception as e:                                  # noqa: BLE001 -- a secondary leg must not cost the bench line
            asymptote = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    ba_out = None
    if ba is not None:
        ba_out = ba.benchmark_report(world, dist)
        if rank == 0 and world == 1:
            # "initial poses = truth o Exp(N(0, diag(0.02 rad, 0.1))), 10 GN iterations, no damping" -- a FRESH problem,
            # timed from that perturbed start (the `ba` above has long converged under the timed steps)
            fresh = mqslam_amd.bundle_adjustment.make_benchmark_problem(u, P, x_it, dev, seed=syn.RSEED)
            cf0 = fresh.total_cost()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh.gauss_newton_iterations(10)
            torch.cuda.synchronize()
            dtf = time.perf_counter() - t0
            ba_out["from_perturbed_start"] = {"iterations": 10, "ms_per_iter": round(1e2 * dtf, 4), "gn_iters_per_s": round(10 / dtf, 1),
                                              "cost_before": cf0, "cost_after": fresh.total_cost()}
            del fresh
        if rank == 0 and world == 1 and N >= 8 and not args.no_shard_proxy:
            # what ONE rank of the 8-way sharded configs[3] run holds, on this GPU alone: the serial floor of strong scaling
            ns = N // 8
            sub = mqslam_amd.bundle_adjustment.make_benchmark_problem(np.ascontiguousarray(u[:, :ns]), P, x_it[:ns].clone(), dev,
                                                                      seed=syn.RSEED)
            ba_out["shard_proxy"] = mqslam_amd.bundle_adjustment.shard_proxy_report(sub)
            del sub
            # the same shard through the peer transport with this GPU as the only rank: the launch sequence N ranks issue (finalize
            # kernel stores the row into the receive buffer, the tail waits for its flags and adds the rows) minus the xGMI hop
            try:
                cc1 = sh.init_peer_comm(0, 1, 0)
                sub = mqslam_amd.bundle_adjustment.make_benchmark_problem(np.ascontiguousarray(u[:, :ns]), P, x_it[:ns].clone(), dev,
                                                                          seed=syn.RSEED, process_group=cc1)
                ba_out["shard_proxy"]["ms_per_iter_over_the_peer_transport_one_rank"] = round(
                    mqslam_amd.bundle_adjustment.time_iterations(sub), 5)
                ba_out["shard_proxy"]["peer_timed_out"] = cc1.peer_timed_out()
                del sub
                cc1.close()
            except Exception as e:                              # noqa: BLE001 -- a secondary figure
                ba_out["shard_proxy"]["peer_transport_error"] = str(e)[:160]

    # ---- matcher (BASELINE configs[2]): one 65 536 x 65 536 x 256-bit camera pair, rank 0 reports ----
    match_out = None
    if not args.no_match:
        Mm = mqslam_amd.matching
        nd, bits = args.descriptors, 256
        tb = Mm.binary_descriptors(nd, bits, seed=7)
        qb = Mm.binary_descriptors(nd, bits, seed=8 + rank, copies_of=tb.astype(np.uint8))
        qd, td = torch.from_numpy(qb).to(dev), torch.from_numpy(tb).to(dev)
        mi = torch.empty((nd, 2), dtype=torch.int32, device=dev)
        md = torch.empty((nd, 2), dtype=torch.float32, device=dev)
        mws = torch.empty(int(mqslam_amd._lib.lib().mqs_match_knn2_f16_workspace_bytes(nd, nd)), dtype=torch.uint8,
                          device=dev)
        for _ in range(60):                               # the clock under matrix load settles over ~50-80 ms of sustained launches
            Mm.knn2_dev(qd, td, mi, md, mws)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            Mm.knn2_dev(qd, td, mi, md, mws)
        e1.record()
        e1.synchronize()
        ms_pair = e0.elapsed_time(e1) / 20
        tf = 2.0 * nd * nd * bits / (ms_pair * 1e-3) / 1e12
        match_out = {"workload": "%d x %d descriptors x %d bits as {0,1} fp16, kNN-2, one camera pair per GPU" % (nd, nd, bits),
                     "ms_per_pair": round(ms_pair, 3), "query_rows_per_s": round(nd / (ms_pair * 1e-3)),
                     "TFLOPs": round(tf, 1), "mfma_f16_dense_peak_TFLOPs": 2500.0, "frac_of_peak": round(tf / 2500.0, 4)}
        # the same camera pair as packed 256-bit descriptors on the FP4 matrix path (identical results)
        qp, tp = torch.from_numpy(Mm.pack_bits(qb)).to(dev), torch.from_numpy(Mm.pack_bits(tb)).to(dev)
        mi8, md8 = torch.empty_like(mi), torch.empty_like(md)
        mws8 = torch.empty(int(mqslam_amd._lib.lib().mqs_match_knn2_bits_workspace_bytes(nd, nd, bits)), dtype=torch.uint8, device=dev)
        for _ in range(120):                              # ~60 ms of sustained launches: the steady state of the clock (0.62 ms
            Mm.knn2_bits_dev(qp, tp, mi8, md8, mws8)      # for the first twenty launches, 0.45 from the hundredth on)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            Mm.knn2_bits_dev(qp, tp, mi8, md8, mws8)
        e1.record()
        e1.synchronize()
        ms8 = e0.elapsed_time(e1) / 20
        tops = 2.0 * nd * nd * bits / (ms8 * 1e-3) / 1e12
        # packed descriptors run on the FP4 matrix instruction (v_mfma_f32_32x32x64_f8f6f4, ~10 PF dense on MI355X);
        # `int8_peak_equivalent` prices the same work against the 5 P int8 peak it ran against until round 2
        match_out["packed_bits_fp4"] = {"ms_per_pair": round(ms8, 3), "Tops": round(tops, 1), "matrix_path": "fp4 (E2M1), fp32 accumulate",
                                         "mfma_fp4_dense_peak_Tops": 10000.0, "frac_of_peak": round(tops / 10000.0, 4),
                                         "int8_peak_equivalent": round(tops / 5000.0, 4),
                                         "equals_fp16_path": bool(torch.equal(mi, mi8) and torch.equal(md, md8))}
        # BASELINE configs[2] in full: 4 cameras x `nd` descriptors, every unordered camera pair (6), kNN-2 on the FP4
        # matrix path + the reference's ratio test / one-match-per-train-row filter on the device; pairs deal to ranks
        cams = [tp] + [torch.from_numpy(Mm.pack_bits(Mm.binary_descriptors(nd, bits, seed=20 + c, copies_of=tb.astype(np.uint8)))).to(dev)
                       for c in range(1, 4)]
        res = Mm.cross_match_dev(cams, rank, world, max_radius=8.0, max_dist_ratio=0.8)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(3):
            res = Mm.cross_match_dev(cams, rank, world, max_radius=8.0, max_dist_ratio=0.8)
        e1.record()
        e1.synchronize()
        ms_x = e0.elapsed_time(e1) / 3
        match_out["cross_match_4_cameras"] = {
            "pairs_total": 6, "pairs_this_rank": len(res), "ms_this_rank": round(ms_x, 3),
            "matches_kept_this_rank": int(sum(int((r[2] >= 0).sum().item()) for r in res.values())),
            "note": "knn2_bits + ratio/unique filter per pair, descriptors resident; pairs are independent units dealt "
                    "round-robin to ranks (no collective)"}
        del qd, td, mi, md, mws, qp, tp, mi8, md8, mws8, cams, res

    # ---- every kernel of the step against the bound that applies to it ----
    rooflines = {
        "linear_ls": {"bound": "hbm", "achieved": kernels["linear_ls"]["GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                      "frac": round(kernels["linear_ls"]["GBps"] / HBM_PEAK_GBPS, 4)},
        "iterative_ls": {"bound": "hbm", "achieved": kernels["iterative_ls"]["GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(kernels["iterative_ls"]["GBps"] / HBM_PEAK_GBPS, 4),
                         "note": "fp64 VALU issue binds before HBM (DESIGN.md)"},
        "linear_eigen": {"bound": "hbm", "achieved": kernels["linear_eigen"]["GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(kernels["linear_eigen"]["GBps"] / HBM_PEAK_GBPS, 4)},
    }
    if ba_out is not None:
        lin_gbps = N * (24 + 16 * C) / (ba_out["kernels_ms"]["linearize_schur"] * 1e-3) / 1e9
        back_gbps = N * (24 + 16 * C + 24) / (ba_out["kernels_ms"]["backsub"] * 1e-3) / 1e9
        rooflines["ba_linearize_schur"] = {"bound": "hbm", "achieved": round(lin_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                           "frac": round(lin_gbps / HBM_PEAK_GBPS, 4),
                                           "valu_pmc": (valu or {}).get("ba_linearize_schur"),
                                           "note": "fp64 VALU issue binds before HBM (DESIGN.md)"}
        rooflines["ba_backsub"] = {"bound": "hbm", "achieved": round(back_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                   "frac": round(back_gbps / HBM_PEAK_GBPS, 4)}
    # the launches the timed step actually runs besides the lineariser: the fused linear-LS + iterative-LS pass (second stream) and
    # the tail of the Gauss-Newton iteration (finalize pieces + 24 x 24 solve + retraction + back-substitution in one launch)
    def timed_ms(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    ms_fused = timed_ms(triangulate)
    bytes_fused = N * (16 * C + 24 + 24 + 4)
    rooflines["tri_ls_and_iterative_fused"] = {"bound": "hbm", "kernel": "tri_kernel<%d, 3> (the step's triangulation launch)" % C,
                                               "achieved": round(bytes_fused / (ms_fused * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                               "frac": round(bytes_fused / (ms_fused * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                               "algorithmic_bytes_per_launch": bytes_fused, "avg_launch_ms": round(ms_fused, 5),
                                               "valu_pmc": (valu or {}).get("tri_ls_and_iterative_fused"),
                                               "note": "fp64 VALU issue binds before HBM (DESIGN.md): on this data 99 % of the landmarks run all ten "
                                                       "re-weighting iterations (noise-limited depths never settle within 3e-5)"}
    if ba_out is not None and "solve_retract_backsub_one_launch" in ba_out["kernels_ms"]:
        ms_tail = ba_out["kernels_ms"]["solve_retract_backsub_one_launch"]
        bytes_tail = N * (24 + 16 * C + 24) + (8 * N if ba.prior_w is not None else 0)
        rooflines["ba_tail"] = {"bound": "hbm", "kernel": "ba_tail_kernel<%d> (the step's second BA launch: solve + retraction + back-substitution)" % C,
                                "achieved": round(bytes_tail / (ms_tail * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                "frac": round(bytes_tail / (ms_tail * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                "algorithmic_bytes_per_launch": bytes_tail, "avg_launch_ms": round(ms_tail, 5),
                                "valu_pmc": (valu or {}).get("ba_tail"),
                                "note": "13.6 M vector instructions per launch at 1e6 x 4: the SIMDs' vector units are 74 % busy (profiles/r04/02); "
                                        "two restructurings measured slower (profiles/r04/05)"}
    rooflines["iterative_ls_standalone"] = roofline_it
    roofline = roofline_it
    if ba_out is not None and C == 4:
        # the kernel with the largest share of the timed step is the BA lineariser; what binds it is fp64 vector issue
        # (its 88 B/landmark would take 11 us at HBM rate), so the headline fraction is flop / time against the fp64 VALU
        # peak, with the HBM fraction beside it.  flop per landmark: counted from the ISA (tools/isa_mix.py).
        kf = kernel_flops().get("ba_linearize_kernel<4>", {})
        ms_lin = ba_out["kernels_ms"].get("linearize_kernel_only", ba_out["kernels_ms"]["linearize_schur"])
        flop = kf.get("fp64_flop_per_landmark")
        bytes_lin = N * (24 + 16 * C) + (8 * N if ba.prior_w is not None else 0)
        hbm = {"achieved": round(bytes_lin / (ms_lin * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
               "algorithmic_bytes_per_launch": bytes_lin,
               "traffic": pmc_rec.get("ba_linearize_hbm_bytes_per_launch") if (pmc_rec.get("landmarks") == N and pmc_rec.get("cams") == C) else None}
        hbm["frac"] = round(hbm["achieved"] / HBM_PEAK_GBPS, 4)
        if flop:
            tf = flop * N / (ms_lin * 1e-3) / 1e12
            roofline = {"bound": "fp64_valu", "kernel": "ba_linearize_wave_kernel<%d, true>" % C, "achieved": round(tf, 2),
                        "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / FP64_VALU_PEAK_TFLOPS, 4),
                        "traffic": hbm["traffic"], "avg_launch_ms": round(ms_lin, 5), "fp64_flop_per_landmark": flop,
                        "valu_instructions_per_landmark": kf.get("valu_instructions_per_landmark"),
                        "valu_issue_slots_per_landmark": kf.get("valu_issue_slots_per_landmark"), "hbm": hbm,
                        "share_of_step": round(ms_lin / ms_per_step, 3),
                        "fp64_fma_rate_with_register_operands": {
                            "TFLOPs": 61.0, "frac_of_it": round(tf / 61.0, 4),
                            "source": "profiles/r04/04_valu_streams_under_pmc.json: a v_fma_f64 with three VGPR-pair sources issues every "
                                      "5.1-5.4 cycles (2.21-2.33 ns), not 4 -- what an all-FMA stream of register operands reaches on this part"},
                        "sq_wait_any_reading": "SQ_WAIT_ANY is 0.25 of this kernel's wave cycles (profiles/r03/09); straight-line fp64 streams "
                                               "WITHOUT any s_waitcnt read 0.11-0.31 by themselves (profiles/r04/04): the counter includes "
                                               "issue-side waiting, there is no hidden quarter of memory waits",
                        "note": "largest kernel of the timed step (hipEvents on the launch stream, stand-alone launches); bound by "
                                "fp64 vector issue, not HBM: `frac` = counted fp64 flop / time against the 78.6 TFLOP/s vector peak; "
                                "`hbm` is the same launch against the 8 TB/s roof SURVEY 8(d) assigns it"}
        else:
            # no current flop count for this tree's kernel (profiles/kernel_flops.json is stale or missing): the HBM view only
            roofline = dict(rooflines["ba_linearize_schur"], kernel="ba_linearize_wave_kernel<%d, true>" % C, traffic=hbm["traffic"], hbm=hbm,
                            avg_launch_ms=round(ms_lin, 5), fp64_flop_per_landmark=None,
                            stale="profiles/kernel_flops.json does not match the kernel sources (tools/evidence_stamp.py)")
        roofline["static_evidence_stale"] = pmc_stale or None
    if "hbm" not in roofline:
        roofline["hbm"] = {"achieved": roofline["achieved"], "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": roofline["frac"]}
    if match_out is not None:
        rooflines["match_knn2_f16"] = {"bound": "mfma", "achieved": match_out["TFLOPs"], "peak": 2500.0, "unit": "TFLOP/s",
                                       "frac": match_out["frac_of_peak"]}
        rooflines["match_knn2_bits_fp4"] = {"bound": "mfma", "achieved": match_out["packed_bits_fp4"]["Tops"], "peak": 10000.0,
                                            "unit": "Top/s", "frac": match_out["packed_bits_fp4"]["frac_of_peak"]}

    # ---- BASELINE configs[4] counterpart: the per-frame loop replayed from the reference's recorded tracks
    #      (committed fixture tests/golden/ba_svo: 186 frames, 1046 landmarks), rank 0 reports ----
    replay_out = None
    svo = os.path.join(ROOT, "tests", "golden", "ba_svo")
    if rank == 0 and not args.no_replay and os.path.isdir(svo):
        try:
            io = mqslam_amd.ba_io
            data = io.load_data(io.create_filenames(svo, "slam2", 1), 50)
            mqslam_amd.slam_replay.replay_frames(data)                  # warm-up
            rp = mqslam_amd.slam_replay.replay_frames(data)
            rec = np.array([data.poses[0][f][1] for f in range(len(rp["poses"]))])
            secs = sum(fr[3] for fr in rp["frames"])
            replay_out = {"workload": "slam2.py handle_new_frame replayed from recorded 2-D tracks: per frame solvePnP, on keyframes "
                                      "triangulate + refined solvePnP + re-triangulate (host-pointer C ABI, one frame at a time)",
                          "frames": len(rp["frames"]), "keyframes": sum(1 for fr in rp["frames"] if fr[2] > 0),
                          "frames_per_s": round(len(rp["frames"]) / secs, 1),
                          "frames_per_s_including_the_decoding_of_the_recording": round(len(rp["frames"]) / (secs + rp.get("prep_seconds", 0.0)), 1),
                          "decode_seconds": round(rp.get("prep_seconds", 0.0), 4),
                          "max_abs_pose_diff_vs_recorded": float(np.abs(rp["poses"] - rec).max()),
                          "landmarks_triangulated": int(np.isfinite(rp["points"][:, 0]).sum())}
        except Exception as e:                                  # noqa: BLE001 -- a secondary leg must not cost the bench line
            replay_out = {"error": "%s: %s" % (type(e).__name__, e)}

    # ---- image front-end on a rendered VGA frame pair: kernels only, device-resident ----
    frontend_out = None
    if rank == 0 and not args.no_frontend:
        try:
            import ctypes
            import gc
            if os.environ.get("MQS_BENCH_GC", "off") == "off":
                gc.collect(); gc.freeze(); gc.disable()     # (the loop legs are host-driven at ~100 us per frame: a collection over this process's objects inside one is not the loop's cost)
            rng = np.random.default_rng(5)
            Hh, Ww = 480, 640
            yy, xx = np.mgrid[0:Hh, 0:Ww].astype(np.float32)
            def render(sx, sy):
                img = np.zeros((Hh, Ww), np.float32)
                r2 = np.random.default_rng(6)
                for _ in range(500):
                    cx, cy, s, a = r2.uniform(0, Ww), r2.uniform(0, Hh), r2.uniform(1.5, 4.0), r2.uniform(-1, 1)
                    x0, x1 = int(max(0, cx - 4 * s + sx)), int(min(Ww, cx + 4 * s + sx + 1))
                    y0, y1 = int(max(0, cy - 4 * s + sy)), int(min(Hh, cy + 4 * s + sy + 1))
                    img[y0:y1, x0:x1] += a * np.exp(-((xx[y0:y1, x0:x1] - cx - sx) ** 2 + (yy[y0:y1, x0:x1] - cy - sy) ** 2) / (2 * s * s))
                return np.clip(np.rint((img + 4.0) / 8.0 * 255), 0, 255).astype(np.uint8)
            I0, I1 = render(0.0, 0.0), render(2.3, -1.1)
            Lb = mqslam_amd._lib
            dI, dJ = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
            ws1 = torch.empty(int(Lb.lib().mqs_gftt_workspace_bytes(Ww, Hh)), dtype=torch.uint8, device=dev)
            ws2 = torch.empty(int(Lb.lib().mqs_lk_workspace_bytes(Ww, Hh, 3)), dtype=torch.uint8, device=dev)
            oxy = torch.zeros((300, 2), dtype=torch.float32, device=dev)
            on = torch.zeros(1, dtype=torch.int32, device=dev)
            sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            def gftt():
                Lb.check(Lb.lib().mqs_good_features_to_track_dev(dI.data_ptr(), Ww, Hh, 300, ctypes.c_double(0.01), ctypes.c_double(7.0),
                                                                 None, oxy.data_ptr(), 300, on.data_ptr(), ws1.data_ptr(), ws1.numel(), sp))
            gftt()
            torch.cuda.synchronize()
            nc = int(on.item())
            nq = torch.empty((max(nc, 1), 2), dtype=torch.float32, device=dev)
            stt = torch.empty(max(nc, 1), dtype=torch.uint8, device=dev)
            er = torch.empty(max(nc, 1), dtype=torch.float32, device=dev)
            def lk():
                Lb.check(Lb.lib().mqs_calc_optical_flow_pyr_lk_dev(dI.data_ptr(), dJ.data_ptr(), Ww, Hh, oxy.data_ptr(), nc, 21, 21, 3, 30,
                                                                   ctypes.c_double(0.01), ctypes.c_double(1e-4), nq.data_ptr(),
                                                                   stt.data_ptr(), er.data_ptr(), ws2.data_ptr(), ws2.numel(), sp))
            def timed_us(fn, reps=30):
                fn(); torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record(); e1.synchronize()
                return e0.elapsed_time(e1) / reps * 1e3
            us_g, us_l = timed_us(gftt), (timed_us(lk) if nc else 0.0)
            flow = (nq[:nc] - oxy[:nc])[stt[:nc] == 1].cpu().numpy() if nc else np.zeros((0, 2))
            frontend_out = {"workload": "640 x 480 rendered frame pair: goodFeaturesToTrack (300 corners, quality 0.01, min distance 7) + "
                                        "pyramidal LK (21 x 21, 4 levels, <= 30 iterations) of those corners, device-resident",
                            "corners": nc, "gftt_us": round(us_g, 1), "lk_us": round(us_l, 1),
                            "tracked": int((stt[:nc] == 1).sum().item()) if nc else 0,
                            "median_flow_error_px": float(np.abs(np.median(flow, axis=0) - [2.3, -1.1]).max()) if len(flow) else None}
            # the whole loop (detect -> track -> pose -> triangulate) on the rendered plane sequence, host-pointer API
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import run_slam_loop
            run_slam_loop.run(10)
            frontend_out["end_to_end_loop"] = run_slam_loop.run_with_ba(60)
            # the same loop with its state resident on the device, one library call per frame (csrc/slam_frame.hip)
            frontend_out["end_to_end_loop_device_resident"] = run_slam_loop.run_device(60, repeats=3)
            frontend_out["end_to_end_loop_device_resident"]["frames_per_s_with_upload"] = run_slam_loop.run_device(60, repeats=3, upload="pageable")["frames_per_s"]
            # BASELINE configs[4] as written -- detect -> match -> triangulate -> BA per keyframe: the same loop with the bundle
            # adjustment of everything so far behind every keyframe (observation log on the device, sparse LM, the adjusted map and
            # poses written back into the live state) and the matcher re-associating the top-up's corners with lost landmarks
            frontend_out["end_to_end_loop_device_resident_ba_per_keyframe"] = run_slam_loop.run_device(
                60, repeats=2, bundle_adjust="keyframe", reassociate=True)
            frontend_out["end_to_end_loop_device_resident_ba_per_keyframe"]["frames_per_s_with_upload"] = run_slam_loop.run_device(
                60, repeats=2, bundle_adjust="keyframe", reassociate=True, upload="pageable")["frames_per_s"]
            # the adjustment over EVERY accepted frame (what the reference's tool does with a finished recording) beside the default
            # selection (every keyframe + the frames since the third keyframe from the end)
            frontend_out["end_to_end_loop_device_resident_ba_per_keyframe_every_frame"] = run_slam_loop.run_device(
                60, repeats=2, bundle_adjust="keyframe", reassociate=True, ba_window_keyframes=None)
            # a run longer than the resident adjuster holds poses (the reference's committed runs: 376 and 881 poses)
            r400 = run_slam_loop.run_device(400, bundle_adjust="keyframe", reassociate=True, keep=True, upload="pageable")
            s400 = r400.pop("slam")
            r400["engines"] = sorted(set(x["engine"] for x in s400.ba_reports))
            r400["poses_per_adjustment_max"] = max(x["poses"] for x in s400.ba_reports)
            r400["fallbacks"] = len(s400.ba_fallbacks)
            s400.close()
            frontend_out["rendered_400_frames_ba_per_keyframe_with_upload"] = r400
            # the reference's OWN example run (slam2.py:924-933: ICL-NUIM living room, real 640 x 480 frames) against the trajectory
            # slam2.py committed for it and against the renderer's exact one (tests/golden/icl_nuim_traj3n: the first 80 frames)
            import run_icl_nuim
            if os.path.exists(run_icl_nuim.FIX):
                run_icl_nuim.run(80)                                              # first-launch costs
                def both(frames, **kw):
                    """frames resident before the clock starts / arriving inside the timed loop (ordinary host arrays -> FrameUploader)"""
                    ra, rb = [], []
                    for _ in range(4):                                            # (interleaved: a host thread that landed badly -- the boxes are shared, load average ~30 -- does not cost ONE form all its passes)
                        ra.append(run_icl_nuim.run(frames, **kw))
                        rb.append(run_icl_nuim.run(frames, upload="pageable", **kw))
                    a, b = max(ra, key=lambda r: r["frames_per_s"]), max(rb, key=lambda r: r["frames_per_s"])      # (the same run four times: the fastest pass, like run_device's `repeats`)
                    a["frames_per_s_with_upload"] = b["frames_per_s"]
                    a["same_trajectory_with_upload"] = a["ours_vs_groundtruth_rmse_m"] == b["ours_vs_groundtruth_rmse_m"]
                    return a
                frontend_out["reference_example_sequence_icl_nuim_80_frames"] = {
                    "plain": both(80), "ba_per_keyframe": both(80, bundle_adjust="keyframe"),
                    "plain_with_the_optional_second_pass_screen_1px": run_icl_nuim.run(80, screen=1.0)}
                if os.path.exists(run_icl_nuim.FIX_REST):
                    # all 200 frames the reference commits: its own trajectory has drifted to 0.171 m by the end (the golden vector)
                    four = [run_icl_nuim.run(200, bundle_adjust="keyframe", seed=sd, upload="pageable") for sd in range(4)]
                    frontend_out["reference_example_sequence_icl_nuim_200_frames"] = {
                        "plain": both(200), "ba_per_keyframe": both(200, bundle_adjust="keyframe"),
                        "ba_per_keyframe_every_frame": run_icl_nuim.run(200, bundle_adjust="keyframe", window=None),
                        "ba_per_keyframe_four_seeds": {"rmse_m": [r["ours_vs_groundtruth_rmse_m"] for r in four],
                                                       "frames_per_s_with_upload": [r["frames_per_s"] for r in four],
                                                       "engines": sorted(set(e for r in four for e in r["engines"]))}}
            frontend_out["cpu_baseline"] = None
            frontend_out["cpu_baseline_note"] = ("the loop legs have no CPU baseline: the reference's loop (slam2.py on OpenCV 2.4 / Python 2) cannot run here, and the "
                                                 "oracle restates its kernels call by call (tests), not as a timed loop; the reference's own run of the 200 example frames is "
                                                 "the golden trajectory these legs are held against, not a speed")
        except Exception as e:                                  # noqa: BLE001 -- a secondary leg must not cost the bench line
            frontend_out = {"error": "%s: %s" % (type(e).__name__, e)}

    # ---- sparse-visibility BA (the reference's real problems: hundreds of poses) at the shape of its largest data set ----
    sparse_out = None
    if rank == 0 and not args.no_ba and not args.no_replay:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_sparse_ba
            sparse_out = bench_sparse_ba.run()
            sparse_out["workload"] = ("synthetic sequence shaped like ICL-NUIM kt2 (881 poses, 13 293 landmarks seen by 17 consecutive "
                                      "poses each): linearise (grouped, atomic-free) + banded Cholesky solve + LM to convergence")
        except Exception as e:                                  # noqa: BLE001 -- a secondary leg must not cost the bench line
            sparse_out = {"error": "%s: %s" % (type(e).__name__, e)}

    # ---- CPU baseline: the oracle's C port of the reference kernel, rank 0, N = 1 only ----
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import c_oracle
        c_oracle.build()
        ns = min(N, 1_000_000)
        us = np.ascontiguousarray(u[:, :ns])
        c_oracle.linear_LS_triangulation(us[:, :1000], P)           # page in
        t0 = time.perf_counter()
        c_oracle.linear_LS_triangulation(us, P)
        xo, so = c_oracle.iterative_LS_triangulation(us, P)
        t_cpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        c_oracle.linear_LS_triangulation(us, P, use_omp=True)
        c_oracle.iterative_LS_triangulation(us, P, use_omp=True)
        t_omp = time.perf_counter() - t0
        # parity gate run with the benchmark: GPU result vs the baseline's
        xg = x_it[:ns].cpu().numpy()
        rel = np.linalg.norm(xg - xo, axis=1) / np.maximum(np.linalg.norm(xo, axis=1), 1.0)
        ba_cpu = None
        if ba is not None:
            h = lambda t: t.cpu().numpy()
            nb = N                                                       # the full problem: no scaling of a sample
            bargs = (h(ba.poses), h(ba.calib), h(ba.sigma), h(ba.points[:nb]), np.ascontiguousarray(h(ba.obs)[:, :nb]))
            t0 = time.perf_counter()
            So, go, co, nvo = c_oracle.ba_linearize(*bargs, None, h(ba.prior_w[:nb]), h(ba.prior_xyz[:nb]), 0.0, use_omp=True)
            dpo = np.linalg.solve(So + 1e-9 * np.eye(len(go)), go)
            c_oracle.ba_backsub(*bargs, dpo, None, h(ba.prior_w[:nb]), h(ba.prior_xyz[:nb]), 0.0, use_omp=True)
            t_ba = time.perf_counter() - t0
            ba_cpu = {"gn_iters_per_s": round(1.0 / t_ba, 3), "cores": os.cpu_count(), "kind": "port",
                      "sample": "1 GN iteration (linearise + Schur + solve + back-substitute) on all %d landmarks x %d cams, "
                                "oracle/c/ba_oracle.c with OpenMP on all host cores (CPU restatement, not GTSAM)" % (nb, C)}
        # BASELINE configs[0]: 10 000 landmarks x 2 cameras -- the reference's Python path (`ref_np`: one small SVD solve per
        # point and iteration, oracle/triangulation_np.py's per-point loop, on a bounded sample) beside the same 2-view call
        # through this build's host-pointer facade (PCIe and launch inclusive)
        from oracle import triangulation_np as tnp
        u2, P2, _ = syn.triangulation_problem(10_000, 2)
        nsmp = 1500
        t0 = time.perf_counter()
        tnp.iterative_LS_triangulation_loop(u2[:, :nsmp], P2)
        t_np = time.perf_counter() - t0
        T = mqslam_amd.triangulation
        T.iterative_LS_triangulation(u2[0], P2[0], u2[1], P2[1])
        t0 = time.perf_counter()
        for _ in range(20):
            T.iterative_LS_triangulation(u2[0], P2[0], u2[1], P2[1])
        t_call = (time.perf_counter() - t0) / 20
        cfg0 = {"workload": "10 000 landmarks x 2 cameras, iterative-LS (BASELINE configs[0] shape)",
                "ref_np_landmarks_per_s": round(nsmp / t_np), "ref_np_sample": "%d landmarks, per-point numpy loop, 1 thread" % nsmp,
                "gpu_host_pointer_call_ms": round(1e3 * t_call, 4), "gpu_host_pointer_landmarks_per_s": round(10_000 / t_call)}
        # matcher: numpy Hamming all-pairs with lowest-index tie-break (`match_np`) on a bounded block of query rows
        match_cpu = None
        if match_out is not None:
            from oracle import matching_np
            nd, nq = args.descriptors, 512
            tbm = mqslam_amd.matching.binary_descriptors(nd, 256, seed=7)
            qbm = mqslam_amd.matching.binary_descriptors(nq, 256, seed=8, copies_of=tbm.astype(np.uint8))
            t0 = time.perf_counter()
            matching_np.knn2_hamming_bits(qbm, tbm)
            t_m = time.perf_counter() - t0
            match_cpu = {"query_rows_per_s": round(nq / t_m), "sample": "%d query rows x %d train rows x 256 bits, numpy (BLAS default "
                         "threads), oracle/matching_np.py" % (nq, nd), "cores": os.cpu_count()}
        cpu = {"value": round(ns / t_cpu), "unit": "landmarks/s", "cores": 1, "kind": "port", "ba": ba_cpu, "configs0": cfg0,
               "match": match_cpu,
               "sample": "linear-LS + iterative-LS over %d landmarks x %d cams (the same arrays), 1 pass, "
                         "oracle/c/tri_oracle.c, gcc -O2, single thread as the reference ships it" % (ns, C),
               "all_cores": {"value": round(ns / t_omp), "cores": os.cpu_count(),
                             "note": "same port with the reference's disabled `omp parallel for` enabled"},
               "parity": {"rel_err_p99.9": float(np.quantile(rel, 0.999)), "rel_err_median": float(np.median(rel)),
                          "status_mismatch_frac": float(np.mean(st[:ns].cpu().numpy() != so))}}

    strong_out = None
    if multi and ba is not None:
        total_strong = args.landmarks if strong else args.strong_landmarks
        strong_out = ba_strong_leg(mqslam_amd, np, torch, total_strong, C, rank, world, dev, group, dist)
        if isinstance(group, sh.CComm):
            strong_out["transport"] = group.transport
            if group.peer_state():
                # Both transports in the same run: the peer stores the step rides on by default AND the RCCL all-reduce north_star names
                # (a second library context with a communicator of its own, no peer buffers), each verified against the one-rank poses;
                # `ba_strong` is the faster one that holds, `ba_strong_transports` has both.  All ranks take the same branches.
                def holds(o, comm):
                    flag = torch.tensor([1.0 if (rank != 0 or o["ok"]) and not (comm.peer_state() and comm.peer_timed_out()) else 0.0], device=dev)
                    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                    return flag.item() == 1.0
                peer_ok = holds(strong_out, group)
                peer_leg = strong_out
                rccl_only = sh.init_c_comm(rank, world, local_rank, peer=False)
                rccl_leg = ba_strong_leg(mqslam_amd, np, torch, total_strong, C, rank, world, dev, rccl_only, dist)
                rccl_leg["transport"] = "rccl all-reduce via the C ABI (mqs_comm_all_reduce_sum_f64_dev between the two launches of an iteration)"
                rccl_ok = holds(rccl_leg, rccl_only)
                t = torch.tensor([peer_leg["ms_per_iter"], rccl_leg["ms_per_iter"]], dtype=torch.float64, device=dev)
                dist.broadcast(t, src=0)                                  # one opinion about which is faster
                take_peer = peer_ok and (not rccl_ok or t[0].item() <= t[1].item())
                strong_out = dict(peer_leg if take_peer else rccl_leg)
                strong_out["ba_strong_transports"] = {
                    "peer_stores": {"ms_per_iter": peer_leg["ms_per_iter"], "verified": bool(peer_ok), "all_reduce_us": peer_leg["all_reduce_us"]},
                    "rccl_all_reduce": {"ms_per_iter": rccl_leg["ms_per_iter"], "verified": bool(rccl_ok), "all_reduce_us": rccl_leg["all_reduce_us"]},
                    "chosen": "peer_stores" if take_peer else "rccl_all_reduce"}
                if not take_peer:
                    transport += "; ba_strong over the RCCL all-reduce (%s)" % ("faster" if peer_ok else "the peer transport did not reproduce the one-rank poses")

    if rank == 0:
        out = dict(line, **{
            "ms_per_step_cold": round(ms_per_step_cold, 4), "value_cold": round(value_cold),
            "value_from": line["value_from"] + "; ms_per_step_cold / value_cold: the same %d + %d steps first thing in the process"
                          % (args.warmup, args.steps),
            "transport": transport, "ba_strong": strong_out,
            "roofline": roofline, "rooflines": rooflines, "kernels": kernels, "asymptote": asymptote, "ba": ba_out, "match": match_out,
            "replay": replay_out, "frontend": frontend_out, "sparse_ba": sparse_out, "cpu_baseline": cpu,
        })
        # The contract's ONE line on stdout is the compact headline (round 4's line had outgrown the driver's 8 KB tail: its head,
        # `value_cold` included, was cut); every leg in full goes to bench_details.json beside this file and, as one line, to stderr.
        details_path = os.path.join(ROOT, "bench_details.json")
        try:
            with open(details_path, "w") as f:
                json.dump(out, f)
        except OSError:
            details_path = None
        print(json.dumps(out), file=sys.stderr, flush=True)
        print(json.dumps(headline(out, details_path)), flush=True)
    if dist is not None:
        dist.barrier()                      # rank 0 reports alone for a few seconds: every rank leaves the group together
        dist.destroy_process_group()
    if rank == 0 and strong_out is not None and strong_out["ok"] is False:
        raise SystemExit("ba_strong: the sharded run does not reproduce the one-rank poses (%r)" % (strong_out,))


if __name__ == "__main__":
    main()
