#!/usr/bin/env python3
"""bench.py — the BASELINE.json metric on MI355X: GP-posterior updates/sec and acquisition-evals/sec
at N=4096, d=8, fp64.

A "step" is one pass of the hot path over one batch of synthetic input (BASELINE.json configs[1]+[2]):
  (1) one GP posterior update  = Gram build + Cholesky of K+σ²I + z = L\\(y-m) + log-likelihood
      on resident (X, y)  (boss_gp_update),
  (2) one batched acquisition  = posterior mean/variance + analytic EI + arg-max over M = 8192
      resident candidates (boss_acq_ei), followed — when N>1 ranks — by the 16-byte RCCL
      all-gather that picks the global arg-max.

N>1: one process per GPU.  Under torchrun (RANK / WORLD_SIZE in the environment) this process is one rank; started
as plain `python bench.py --gpus N` it first spawns N fresh child processes of itself (before anything touches the
GPU) and relays rank 0's line.  Two records are measured:
  weak    (the top-level line, `scaling: weak`): every rank owns an independent GP (a different output slice /
          hyper-parameter sample, seeded by rank) and its own 8192 candidates; the only collective is the arg-max
          exchange.  `value` = posterior updates/s over all ranks.
  strong  (`strong_scaling`, BASELINE.json configs[2] as written: "8192 random multistarts sharded across 8×MI355X"):
          ONE N=4096 posterior replicated on every rank (the single Cholesky does not shard: replicas only), the 8192
          candidates split M/G per rank, 16-byte arg-max exchange.

Prints ONE JSON line on rank 0.  A plain run measures the headline figure alone: set-up, W warm-up steps, the K timed
steps of the weak record, and the line (`value`, `ms_per_step`, ...; the keys of what it did not measure are null).
`--full` adds everything else, each in passes of its own after the weak record: the strong record, per-kernel event
timing (`roofline`: the dominant kernel, the fused prediction kernel, measured live with HIP events on the library's
stream), the update latency distribution, the rows beyond the headline path, the batched / config-4 / config-5 blocks,
the one-process multi-device child and `cpu_baseline` (the CPU oracle, oracle/gp_oracle.py, BLAS-3 Gram + LAPACK, on
this host, rank 0, N=1).

`--dump-outputs DIR` writes what the last timed step handed its caller (rank 0), float64 .npy files of about 0.6 MB in all:
logpdf, acq (EI over the 8192 candidates), acq_argmax, acq_max, factor_z (z = L\\(y-m)) and factor_L_sample (a fixed,
seeded sample of the lower triangle of the Cholesky factor: the whole factor is 128 MB).  The inputs are seeded, so two
builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_OBS, D, M_CAND = 4096, 8, 8192
FP64_MFMA_PEAK_TFLOPS = 78.6          # AMD MI355X datasheet (vector = matrix fp64); tools/mfma_probe measures 77.6
ONE_WAVE_ISSUE_TFLOPS = 68.3          # measured: bare fp64 MFMA stream, one wave per SIMD, 256 CUs (profiles/r03_mfma_rate_probe.log)
KERNEL = "matern52"
MAX_PROCS_PER_GPU = 6                 # the GPU box's process guard


def note(msg):
    """progress on stderr (rank 0): a long run must not look hung to whoever watches it"""
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def problem(seed):
    """SURVEY §8d config 2/3 inputs."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (D, N_OBS))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(D) + 0.05 * rng.standard_normal(N_OBS)
    Xs = np.random.default_rng(seed + 1).uniform(0, 1, (D, M_CAND))
    return X, y, Xs


def factor_sample_index(N, k=1 << 16):
    """(row, column) of the factor entries --dump-outputs keeps: k fixed, seeded positions in the lower triangle."""
    rng = np.random.default_rng(2024)
    a, b = rng.integers(0, N, k), rng.integers(0, N, k)
    return np.maximum(a, b), np.minimum(a, b)


def dump_outputs(path, gp, last):
    """--dump-outputs: the arrays the last timed step returned to its caller, and the posterior it left resident."""
    os.makedirs(path, exist_ok=True)
    L, z = gp.factor()
    arrays = {"logpdf": [last["logpdf"]], "acq": last["acq"], "acq_argmax": [last["argmax"]], "acq_max": [last["max"]],
              "factor_z": z, "factor_L_sample": L[factor_sample_index(gp.N)]}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(a, dtype=np.float64))


def flops_update(N, d):
    return N ** 3 / 3 + 2 * N ** 2 + N ** 2 * (3 * d + 20) / 2


def flops_acq_eval(N, d):
    return N ** 2 + N * (3 * d + 20) + 4 * N


def pmc_traffic(kernel_substr):
    """HBM-side bytes per launch of `kernel_substr` from the rocprofv3 --pmc passes of this same command
    (profiles/*_pmc_summary.json, written by tools/pmc_summary.py): FETCH_SIZE (KB, doubled — on gfx950 it reports
    half the bytes of 16-B/lane streaming reads, MI355X_MICROARCH.md §HBM) + WRITE_SIZE (KB).  Only a summary collected
    on THIS source tree counts: each summary carries the library's source hash; anything else is refused
    (-> (None, reason))."""
    import glob
    import re
    import __graft_entry__ as entry
    want = entry.source_hash()
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")),
                   key=lambda q: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(q))])
    stale = None
    for path in reversed(paths):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        if d.get("source_hash") != want:
            stale = stale or os.path.relpath(path, ROOT)
            continue
        for k, v in d.items():
            if isinstance(v, dict) and kernel_substr in k:
                return (2.0 * v["fetch_kb_raw"] + v["write_kb"]) * 1024.0, os.path.relpath(path, ROOT)
    return None, ("no counter summary for this source tree" + (f" (newest is {stale}, collected on other sources)" if stale else ""))


def pmc_mfma(kernel_substr):
    """Matrix-pipe counters of `kernel_substr` from the third --pmc pass of tools/collect_profiles.sh (same source-hash rule as
    pmc_traffic): SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CU_CYCLES (busy cycles of the MFMA pipes, counted per SIMD, over the busy cycles of
    the kernel's CUs), MfmaUtil over the whole chip, and the fp64 FLOP the counters saw per launch (SQ_INSTS_VALU_MFMA_MOPS_F64 × 512)."""
    import glob
    import re
    import __graft_entry__ as entry
    want = entry.source_hash()
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")),
                   key=lambda q: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(q))])
    for path in reversed(paths):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        if d.get("source_hash") != want:
            continue
        for k, v in d.items():
            if isinstance(v, dict) and kernel_substr in k and v.get("mfma_busy_cycles"):
                return {"kernel": k.split("(")[0][-60:], "mfma_busy_over_busy_cu": v.get("mfma_busy_over_busy_cu"),
                        "mfma_busy_frac_per_simd": (v.get("mfma_busy_over_busy_cu") or 0.0) / 4.0, "mfma_util_chip": v.get("mfma_util_chip"),
                        "counted_fp64_flop_per_launch": (v.get("mfma_mops_f64") or 0.0) * 512.0, "launches": v.get("mfma_launches"),
                        "source": os.path.relpath(path, ROOT)}
    return None


def cpu_baseline(X, y, Xs, lam):
    """The CPU oracle on this host's cores: posterior updates the way the reference's stack computes them — pairwise
    distances in the ‖a‖²+‖b‖²−2a·b form with the cross term from one dgemm (Distances.jl; src/models/utils/kernels.jl:35),
    the radial profile broadcast over the N×N matrix, LAPACK dpotrf, two dtrsv — with BLAS threads = physical cores, and
    a bounded sample of acquisition evaluations in the reference's call pattern (one dtrsv per candidate,
    expected_improvement.jl:75,79) and in the best-effort batched pattern (one dtrsm)."""
    from oracle import gp_oracle as O
    try:
        import psutil
        cores = psutil.cpu_count(logical=False) or os.cpu_count()
    except Exception:
        cores = os.cpu_count()
    cores = min(cores, len(os.sched_getaffinity(0)))
    for qf, pf in (("/sys/fs/cgroup/cpu.max", None), ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us")):
        try:                                               # a container's CPU quota (cgroup v2 / v1)
            if pf is None:
                quota, period = open(qf).read().split()
            else:
                quota, period = open(qf).read().strip(), open(pf).read().strip()
            if quota not in ("max", "-1"):
                cores = max(1, min(cores, int(int(quota) / int(period))))
            break
        except Exception:
            pass
    from threadpoolctl import threadpool_limits
    import scipy.linalg as sla
    # BLAS threads: the physical cores, unless fewer threads factorise faster on this box (an over-subscribed or
    # bandwidth-starved host) — a 2048×2048 dpotrf probe decides; the choice is reported
    probe = np.random.default_rng(0).standard_normal((2048, 2048))
    probe = probe @ probe.T + 2048 * np.eye(2048)
    best_t, threads = None, cores
    for th in sorted({cores, min(cores, 64), min(cores, 32), min(cores, 16), min(cores, 8)}, reverse=True):
        with threadpool_limits(limits=th):
            sla.cholesky(probe, lower=True, check_finite=False)
            t0 = time.perf_counter()
            sla.cholesky(probe, lower=True, check_finite=False)
            dt = time.perf_counter() - t0
        if best_t is None or dt < 0.9 * best_t:
            best_t, threads = dt, th
    phys, cores = cores, threads
    with threadpool_limits(limits=cores):
        O.gp_fit(X, y, KERNEL, lam, 1.0, 0.05, form="blas")                # warm-up: first-touch of the big temporaries
        tm = {}
        t0 = time.perf_counter()
        reps = 0
        while reps < 3 or (time.perf_counter() - t0 < 8.0 and reps < 12):
            post = O.gp_fit(X, y, KERNEL, lam, 1.0, 0.05, form="blas", timings=tm)
            reps += 1
        t_upd = (time.perf_counter() - t0) / reps
        b = float(y.max())
        n_faithful, n_batched = 48, 2048
        t0 = time.perf_counter()
        for j in range(n_faithful):                                        # per-candidate vector form
            O.ei_acquisition([post], Xs[:, j:j + 1], [1.0], None, b)
        t_f = (time.perf_counter() - t0) / n_faithful
        t0 = time.perf_counter()
        O.ei_acquisition([post], Xs[:, :n_batched], [1.0], None, b)
        t_b = (time.perf_counter() - t0) / n_batched
        # LAPACK dpotrf called directly, in place on a Fortran-ordered buffer (no copy, no zeroing of the other triangle) — what
        # Julia's cholesky! does — and a dgemm of the same size as a health check of the BLAS on this host
        from scipy.linalg.lapack import dpotrf
        from scipy.linalg.blas import dgemm
        Kf = np.asfortranarray(O.kernelmatrix_blas(post.h, X))
        Kf[np.diag_indices(N_OBS)] += 0.05 ** 2
        t_po = []
        for _ in range(3):
            a = Kf.copy(order="F")
            t0 = time.perf_counter()
            _, info_po = dpotrf(a, lower=1, overwrite_a=1, clean=0)
            t_po.append(time.perf_counter() - t0)
        t_potrf = min(t_po)
        Bf = np.asfortranarray(Kf[:, :2048])
        dgemm(1.0, Kf, Bf)
        t0 = time.perf_counter()
        dgemm(1.0, Kf, Bf)
        t_gemm = time.perf_counter() - t0
        gf_potrf = N_OBS ** 3 / 3 / t_potrf / 1e9
        gf_gemm = 2.0 * N_OBS * N_OBS * 2048 / t_gemm / 1e9
        note = (f"dpotrf in place {gf_potrf:.0f} GF/s, dgemm {gf_gemm:.0f} GF/s on {cores} BLAS threads "
                f"({phys} cores in this container's CPU quota, {os.cpu_count()} logical CPUs on the host)")
        if gf_potrf < 60:
            note += ("; dpotrf far below the dgemm rate: OpenBLAS's blocked dpotrf is latency-bound on its panel factorisations when its "
                     "threads are time-sliced inside a cgroup quota (the probe above already picked the fastest thread count)")
    return {
        "value": 1.0 / t_upd, "unit": "updates/s", "cores": int(cores), "kind": "port",
        "dpotrf_inplace_ms": t_potrf * 1e3, "dpotrf_gflops": gf_potrf, "dgemm_gflops": gf_gemm, "blas_note": note,
        "sample": f"{reps} posterior updates at N={N_OBS} (BLAS-3 Gram + dpotrf + 2 dtrsv); {n_faithful} per-candidate (dtrsv) and "
                  f"{n_batched} batched (dtrsm) acquisition evals",
        "ms_per_update": t_upd * 1e3,
        "ms_split": {k: v / reps * 1e3 for k, v in tm.items()},
        "acq_evals_per_sec_reference_pattern": 1.0 / t_f, "acq_evals_per_sec_batched": 1.0 / t_b,
        "blas_threads": int(cores), "physical_cores_available": int(phys), "host_cpu_count": os.cpu_count(),
    }


def visible_gpus():
    """Number of GPUs this process may use, without initialising HIP.  The KFD topology lists every GPU of the HOST; only those
    whose render node (drm_render_minor -> /dev/dri/renderD<minor>) this process can open count (a container's device cgroup or
    its /dev/dri mounts hide the others).  The visibility variables can only narrow that down: each is an index list into what
    the layer below it shows, so the minimum over the ones that are set is an upper bound.  A rank whose LOCAL_RANK still turns
    out to be beyond the runtime's device count falls back to sharing device 0 (main(): `rehearsal`)."""
    n = 0
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for node in os.listdir(base):
            try:
                props = dict(l.split()[:2] for l in open(os.path.join(base, node, "properties")).read().splitlines() if len(l.split()) >= 2)
            except OSError:
                continue
            if int(props.get("simd_count", "0")) <= 0:
                continue                                       # a CPU node
            minor = props.get("drm_render_minor")
            dev = f"/dev/dri/renderD{minor}" if minor not in (None, "0", "-1") else None
            if dev is None or os.access(dev, os.R_OK | os.W_OK):
                n += 1
    except OSError:
        pass
    if n == 0:                                             # last resort (counts devices through the runtime; no context is created)
        import torch
        n = torch.cuda.device_count()
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    return n


def inproc_child(G, steps, warmup):
    """`--inproc-child G` (a fresh process): BASELINE configs[2] through the ONE-PROCESS multi-GPU entry points a Julia caller
    uses — boss_init, boss_multi_gp_update (the posterior replicated on G devices), boss_multi_acq_ei (8192 candidates split
    M/G, arg-max exchange inside the library).  Prints one JSON object."""
    import __graft_entry__ as entry
    entry.compile_library()
    from boss_jl_amd import api
    api.load_library()
    n = api.init()
    G = max(1, min(G, n))
    X, y, Xs = problem(1)
    lam = np.full(D, 0.5)
    reps = [api.GP(X, y, KERNEL, device=g) for g in range(G)]
    best = float(y.max())
    handles = [[[r]] for r in reps]
    mcand = api.MultiCandidates(Xs, G)                                # the candidate shards stay resident, as in the per-rank records
    t_u = t_a = 0.0
    am = mx = None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        api.multi_update(reps, lam, 1.0, 0.05 + 1e-4 * (i % 7))
        t1 = time.perf_counter()
        _, am, mx = api.multi_acq_ei_cand(handles, mcand, [1.0], None, best, want_acq=False)
        t2 = time.perf_counter()
        if i >= warmup:
            t_u += t1 - t0
            t_a += t2 - t1
    t0 = time.perf_counter()
    for i in range(3):                                                # the same with candidates uploaded per call (boss_multi_acq_ei)
        api.multi_acq_ei(handles, Xs, [1.0], None, best, want_acq=False)
    t_oneshot = (time.perf_counter() - t0) / 3
    ndev, rccl = api.comm_info()
    print(json.dumps({"scaling": "strong", "driver": "one process, boss_init + boss_multi_gp_update + boss_multi_acq_ei (csrc/host_multi.inc)",
                      "n_gpus": G, "devices_opened": ndev, "exchange": "rccl" if rccl and G > 1 else ("host" if G > 1 else "none"),
                      "value": steps * M_CAND / t_a, "unit": "evals/s", "ms_acq_incl_exchange": t_a / steps * 1e3,
                      "ms_update_replicated": t_u / steps * 1e3, "steps_per_sec": steps / (t_u + t_a),
                      "ms_acq_with_per_call_upload": t_oneshot * 1e3,
                      "argmax": [int(am), float(mx)], "steps": steps}), flush=True)
    mcand.close()
    for r in reps:
        r.close()
    api.shutdown()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_children(args):
    """`python bench.py --gpus N` without torchrun: N fresh child processes, one per GPU, started BEFORE this process
    touches the GPU (a process that initialised the GPU must never be replaced or re-executed).  With fewer visible
    GPUs than ranks the children share device 0 and exchange over gloo (a rehearsal of the N>1 path on a 1-GPU box:
    marked `rehearsal` in the output, at most 6 processes per GPU)."""
    n_vis = visible_gpus()                                 # (no HIP call: the launcher must not count as a GPU process)
    if n_vis < 1:
        raise SystemExit("bench.py needs a GPU (bosship has no CPU fallback)")
    env = dict(os.environ)
    if n_vis < args.gpus:
        if args.gpus > MAX_PROCS_PER_GPU * n_vis:
            raise SystemExit(f"--gpus {args.gpus}: only {n_vis} GPU(s) visible and at most {MAX_PROCS_PER_GPU} processes may share one")
        env["BOSS_BENCH_BACKEND"] = "gloo"
        env["BOSS_BENCH_REHEARSAL"] = "1"
        # (several processes on one GPU take turns on its hardware queues: where the resident chain of an update cannot run, its
        # waits give up after their size-derived budget — tens of milliseconds, once per process — and the library carries on with
        # the simpler schedule; the rehearsal runs the shipped defaults)
    import __graft_entry__ as entry
    entry.compile_library()                                # once, here (hipcc only: nothing is loaded, no GPU call)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus))
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    import tempfile
    procs = []
    out0 = tempfile.TemporaryFile()
    for r in range(args.gpus):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen(cmd, env=e, stdout=out0 if r == 0 else subprocess.DEVNULL))
    # all ranks are watched: when one dies the others would sit in a collective until the distributed timeout
    rc = 0
    alive = set(range(args.gpus))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code
                print(f"[bench] rank {r} exited with {code}: stopping the other ranks", file=sys.stderr, flush=True)
                for q in alive:
                    procs[q].terminate()
        time.sleep(0.05)
    out0.seek(0)
    sys.stdout.write(out0.read().decode())
    sys.stdout.flush()
    raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="also measure everything beyond the headline figure (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the next_rows measurements (counter-collection passes)")
    ap.add_argument("--with-config5", action="store_true", help="with --full --no-extras: still run the batched / config-5 block (counter passes of its kernels)")
    ap.add_argument("--inproc-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.inproc_child:
        inproc_child(args.inproc_child, args.steps, args.warmup)
        return

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_children(args)                                  # does not return

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (bosship has no CPU fallback)")
    # one process per GPU; BOSS_BENCH_BACKEND=gloo lets the N>1 path be rehearsed on a 1-GPU box
    # (all ranks then share device 0 and the exchange runs over gloo on CPU tensors)
    backend = os.environ.get("BOSS_BENCH_BACKEND", "nccl")
    n_vis = torch.cuda.device_count()
    dev_index = local_rank if local_rank < n_vis else local_rank % max(n_vis, 1)
    if world > n_vis and backend == "nccl":
        # RCCL refuses two ranks on one device: with fewer GPUs than ranks only the gloo rehearsal is possible
        if "BOSS_BENCH_BACKEND" in os.environ:
            raise SystemExit(f"--gpus {world}: the runtime shows {n_vis} GPU(s); RCCL needs one per rank (BOSS_BENCH_BACKEND=gloo rehearses on fewer)")
        backend = "gloo"
        os.environ["BOSS_BENCH_REHEARSAL"] = "1"
    torch.cuda.set_device(dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    import __graft_entry__ as entry
    if local_rank == 0:
        entry.build()                    # one builder per node; the others wait, then just load the .so
    if dist is not None:
        dist.barrier()
    from boss_jl_amd import api
    api.load_library()
    from boss_jl_amd import distributed as dist_util
    dev = dev_index
    lam = np.full(D, 0.5)

    def sync_all():
        api.device_sync(dev)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(step, steps, warmup):
        """W untimed warm-up steps, then exactly K steps bracketed by barrier + synchronize; max over ranks."""
        for i in range(warmup):
            step(i)
        sync_all()
        t_begin = time.perf_counter()
        t_a = t_b = 0.0
        for i in range(steps):
            a, b = step(i)
            t_a += a
            t_b += b
        sync_all()
        elapsed = time.perf_counter() - t_begin
        times = torch.tensor([elapsed, t_a, t_b], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        if dist is not None:
            dist.all_reduce(times, op=dist.ReduceOp.MAX)
        return tuple(float(v) for v in times.cpu())

    # ------------------------------------------------------------------ weak: independent slices + candidate sets
    X, y, Xs = problem(1 + 10 * rank)            # every rank: its own GP slice + its own candidate shard
    gp = api.GP(X, y, KERNEL, device=dev)
    cand = api.Candidates(Xs, device=dev)
    best = float(y.max())
    last = {}
    dump_at = args.steps - 1 if args.dump_outputs is not None and rank == 0 else -1

    def step(i, exchange=True):
        # with --dump-outputs, the step numbered as the last timed one also copies the acquisition values back (the same
        # launches; a warm-up step with that number runs before it and is overwritten)
        keep = i == dump_at
        t0 = time.perf_counter()
        # a different noise level each step so no step can reuse the previous factorisation
        lp = gp.update(lam, 1.0, 0.05 + 1e-4 * (i % 7))
        t1 = time.perf_counter()
        acq, am, mx = api.acq_ei([[gp]], cand, [1.0], None, best, want_acq=keep)
        if world > 1 and exchange:
            mx, am = dist_util.argmax_exchange(mx, am + rank * M_CAND)
        t2 = time.perf_counter()
        if keep:
            last.update(logpdf=lp, acq=acq, argmax=am, max=mx)
        return t1 - t0, t2 - t1

    note("weak record: posterior update + 8192-candidate acquisition per step")
    elapsed, t_upd, t_acq = timed(step, args.steps, args.warmup)
    note(f"  {args.steps * 1e3 / 1e3 / t_upd * world:.0f} updates/s, {elapsed / args.steps * 1e3:.3f} ms per step")
    if dump_at >= 0:
        dump_outputs(args.dump_outputs, gp, last)
        dump_at = -1                                   # (the later passes of --full that call step() keep nothing)

    # everything below measures beyond the headline figure: --full only
    # ------------------------------------------------------------------ strong: one posterior replicated, candidates M/G
    strong = None
    if args.full:
        note("strong record")
        Xr, yr, Xsr = problem(1)                      # the same problem on every rank
        lo, hi = dist_util.shard_range(M_CAND, rank, world)
        gps = gp if world == 1 else api.GP(Xr, yr, KERNEL, device=dev)
        cand_s = cand if world == 1 else api.Candidates(Xsr[:, lo:hi], device=dev)
        best_s = float(yr.max())
        winner = {}

        def step_strong(i):
            t0 = time.perf_counter()
            gps.update(lam, 1.0, 0.05 + 1e-4 * (i % 7))
            t1 = time.perf_counter()
            _, am, mx = api.acq_ei([[gps]], cand_s, [1.0], None, best_s, want_acq=False)
            if world > 1:
                mx, am = dist_util.argmax_exchange(mx, am + lo)
            t2 = time.perf_counter()
            winner[i % 7] = (am, mx)
            return t1 - t0, t2 - t1

        s_elapsed, s_upd, s_acq = timed(step_strong, args.steps, args.warmup)
        # the same step as ONE call per rank where the shard is small enough for the substitution to ride along the replicated update
        # (boss_gp_update_acq, csrc/rider.hpp): at G = 8 every rank holds 1024 candidates
        fused_strong = None
        if hi - lo <= 4096:
            rode = []

            def step_fused(i):
                t0 = time.perf_counter()
                r = gps.update_acq(lam, 1.0, 0.05 + 1e-4 * (i % 7), cand_s, best=best_s)
                am, mx = r["argmax"], r["max"]
                if world > 1:
                    mx, am = dist_util.argmax_exchange(mx, am + lo)
                rode.append(r["fused"])
                return time.perf_counter() - t0, 0.0
            f_elapsed, _, _ = timed(step_fused, args.steps, args.warmup)
            fused_strong = {"ms_per_step": f_elapsed / args.steps * 1e3, "steps_per_sec": args.steps / f_elapsed,
                            "rode_along": bool(all(rode)), "speedup_over_two_calls": s_elapsed / f_elapsed}
        strong = {
            "scaling": "strong", "metric": "acq_evals_per_sec, 8192 candidates of ONE N=4096 posterior sharded M/G (+ replicated update)",
            "value": args.steps * M_CAND / s_acq, "unit": "evals/s", "n_gpus": world, "M_per_gpu": hi - lo,
            "ms_acq_shard_incl_exchange": s_acq / args.steps * 1e3, "ms_update_replicated": s_upd / args.steps * 1e3,
            "ms_per_step": s_elapsed / args.steps * 1e3, "steps_per_sec": args.steps / s_elapsed,
            "prediction_path": "fused kernel (one workgroup per 32 candidates)" if hi - lo > 4096 else
                               "256-row substitution steps spread over the chip (few-candidates path, first call on a factorisation)",
            "argmax": [int(winner[0][0]), float(winner[0][1])],
            "exchange": "none" if world == 1 else f"16-byte all-gather over {backend}",
            "one_call_per_step": fused_strong,
        }

    # ---- per-kernel HIP-event timing of the dominant kernels (separate pass, events on the library's stream)
    roof = roof_potrf = None
    if rank == 0 and args.full:
        note("per-kernel event timing")
        # (a) the dominant kernel inside the UNSERIALISED step: the update runs as always (resident chain, side stream), the event
        # pair is switched on for the acquisition call alone — two hipEventRecord around predict_kernel on the library's stream
        api.prof_reset(dev)
        for i in range(10):
            gp.update(lam, 1.0, 0.05 + 1e-4 * (i % 7))
            api.prof_enable(dev, True)
            api.acq_ei([[gp]], cand, [1.0], None, best, want_acq=False)
            api.prof_enable(dev, False)
        ms_pred, n_pred = api.prof_get(dev, "predict")
        # (b) the factorisation's kernel classes, from a serialised pass (events around every launch: one stream, no look-ahead)
        api.prof_enable(dev, True)
        api.prof_reset(dev)
        reps = 5
        for i in range(reps):
            step(i, exchange=False)          # rank-0-only pass: must not contain a collective
        ms_syrk, n_syrk = api.prof_get(dev, "potrf_syrk")
        ms_diag, n_diag = api.prof_get(dev, "potrf_diag")
        ms_trsm, n_trsm = api.prof_get(dev, "potrf_trsm")
        api.prof_enable(dev, False)
        fl_pred = M_CAND * flops_acq_eval(N_OBS, D)                         # algorithmic flops per launch
        ach = fl_pred / (ms_pred / n_pred * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic("predict_kernel")
        roof = {"kernel": "predict_kernel", "bound": "mfma", "achieved": ach, "peak": FP64_MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": ach / FP64_MFMA_PEAK_TFLOPS, "traffic": traffic,
                "traffic_unit": "bytes/launch (rocprofv3 --pmc FETCH_SIZE x2 [gfx950 16-B/lane correction] + WRITE_SIZE, x1024)",
                "traffic_source": traffic_src,
                "avg_launch_ms": ms_pred / n_pred, "launches_timed": int(n_pred), "flops_per_launch": fl_pred,
                "timing": "HIP events around predict_kernel on the library's stream inside unserialised update + acquisition steps "
                          "(includes the two event records: a few µs); rocprofv3 --kernel-trace average of the same command under profiles/",
                # a dependence-free fp64 MFMA stream with ONE wave per SIMD (this kernel's register budget) retires 68.3 TFLOP/s
                # on 256 CUs (profiles/r03_mfma_rate_probe.log; four waves: 76.6)
                "one_wave_per_simd_issue_rate_tflops": ONE_WAVE_ISSUE_TFLOPS,
                "frac_vs_one_wave_issue_rate": ach / ONE_WAVE_ISSUE_TFLOPS,
                # matrix-pipe counters of the same command (third --pmc pass; null until collected on these sources)
                "mfma_counters": pmc_mfma("predict_kernel<"),
                "mfma_busy_frac": (pmc_mfma("predict_kernel<") or {}).get("mfma_busy_frac_per_simd")}
        # the factorisation: N^3/3 over the whole posterior update (two-stream look-ahead; the
        # per-class event times below come from the serialised profiling pass)
        fl_potrf = N_OBS ** 3 / 3
        t_upd_s = t_upd / args.steps
        ach2 = fl_potrf / t_upd_s / 1e12
        roof_potrf = {"kernel": "posterior update (gram + look-ahead Cholesky + logdet)", "bound": "mfma", "achieved": ach2,
                      "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach2 / FP64_MFMA_PEAK_TFLOPS,
                      "ms_per_update": t_upd_s * 1e3,
                      "serialised_ms_diag": ms_diag / reps, "serialised_ms_trsm": ms_trsm / reps,
                      "serialised_ms_syrk": ms_syrk / reps,
                      "mfma_counters": {"potrf_colupd_kernel": pmc_mfma("potrf_colupd_kernel"),
                                        "potrf_syrk_kernel<2,true>": pmc_mfma("potrf_syrk_kernel<2, true>") or pmc_mfma("potrf_syrk_kernel<2"),
                                        "predict_kernel_set": pmc_mfma("predict_kernel_set")},
                      "mfma_busy_frac": (pmc_mfma("potrf_colupd_kernel") or {}).get("mfma_busy_frac_per_simd")}

    # ---- latency distribution of the posterior update (the resident chain's tail latency): 2000 back-to-back updates, every launch
    # of each stamped on the host (csrc/host_factor.inc, LaunchStamps): an update beyond 2 ms reports where its submission stood still
    upd_dist = None
    if rank == 0 and args.full:
        note("update latency distribution")
        import ctypes as C
        lib = api.load_library()
        lib.boss_debug_launch_stamps.argtypes = [C.c_int, C.c_double]
        lib.boss_debug_stall_report.argtypes = [C.c_char_p, C.c_int]
        lib.boss_debug_launch_stamps(1, 2.0)
        rep = C.create_string_buffer(8192)
        lib.boss_debug_stall_report(rep, 8192)                      # (clears what the serialised profiling pass above left)
        nlat = 2000
        ts = np.empty(nlat)
        for i in range(nlat):
            t0 = time.perf_counter()
            gp.update(lam, 1.0, 0.05 + 1e-4 * (i % 7))
            ts[i] = time.perf_counter() - t0
        lib.boss_debug_stall_report(rep, 8192)
        lib.boss_debug_launch_stamps(0, 0.0)
        ts = np.sort(ts) * 1e3
        upd_dist = {"n": int(ts.size), "update_ms_p50": float(np.percentile(ts, 50)), "update_ms_p90": float(np.percentile(ts, 90)),
                    "update_ms_p99": float(np.percentile(ts, 99)), "update_ms_p999": float(np.percentile(ts, 99.9)),
                    "update_ms_max": float(ts[-1]), "update_ms_min": float(ts[0]), "update_ms_mean": float(ts.mean()),
                    "max_over_p50": float(ts[-1] / np.percentile(ts, 50)),
                    "updates_beyond_2ms": int((ts > 2.0).sum()),
                    "stall_reports": [ln for ln in rep.value.decode(errors="replace").splitlines() if ln][:8]}

    # ---- SURVEY §8f rows built beyond the headline path (rank 0, N=1 only; a fraction of a second)
    extras = None
    if rank == 0 and world == 1 and args.full and not args.no_extras:
        note("next rows (gradients, appends, small sizes, gradient observations)")
        gp.update(lam, 1.0, 0.05)
        gp.predict_grad(Xs)                                          # first gradient call on a handle: lazy allocations (transposed factor, 138 MB)
        gp.update(lam, 1.0, 0.05)
        t0 = time.perf_counter()
        for _ in range(3):
            gp.predict_grad(Xs)
        t_grad = (time.perf_counter() - t0) / 3
        note("  appends")
        rng = np.random.default_rng(7)
        g2 = api.GP(X, y, KERNEL, device=dev)
        g2.update(lam, 1.0, 0.05)
        g2.reserve(N_OBS + 64)
        g2.update(lam, 1.0, 0.05)
        t0 = time.perf_counter()
        g2.append(rng.uniform(0, 1, D), 0.0)                       # first append after an update: block path
        t_app = time.perf_counter() - t0
        g2.append(rng.uniform(0, 1, D), 0.0)                       # second: builds the inverse factors
        ts = []
        for _ in range(16):                                        # from then on: rank-one path
            t0 = time.perf_counter()
            g2.append(rng.uniform(0, 1, D), 0.0)
            ts.append(time.perf_counter() - t0)
        t_app1 = float(np.median(ts))
        g2.close()
        note("  likelihood gradients, single-candidate predictions")
        gp.update(lam, 1.0, 0.05)
        gp.loglike_grad()
        t0 = time.perf_counter()
        for i in range(3):
            gp.update(lam, 1.0, 0.05 + 1e-4 * i)
            gp.loglike_grad()
        t_llg = (time.perf_counter() - t0) / 3
        gp.predict(Xs[:, :1])                                      # substitution path (first call on a factorisation)
        t0 = time.perf_counter()
        gp.predict(Xs[:, 1:2])                                     # second call: builds the explicit inverse
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i in range(200):
            gp.predict(Xs[:, i:i + 1])
        t_one = (time.perf_counter() - t0) / 200
        extras = {"single_candidate_predicts_per_sec": 1.0 / t_one, "ms_single_candidate_predict": t_one * 1e3,
                  "ms_second_call_building_the_inverse": t_build * 1e3,
                  "loglike_with_hyperparameter_gradient_per_sec": 1.0 / t_llg, "ms_update_plus_loglike_grad": t_llg * 1e3,
                  "block_cholesky_append_ms": t_app * 1e3, "rank_one_append_ms": t_app1 * 1e3,
                  "append_vs_refactorisation": (t_upd / args.steps) / t_app1,
                  "posterior_gradient_evals_per_sec": M_CAND / t_grad, "ms_gradient_batch": t_grad * 1e3}
        note("  N = 20")
        # BASELINE.json configs[0] regime (examples/example.jl: N≈20, d=1): one posterior update
        rs = np.random.default_rng(555)
        x1 = rs.uniform(0, 20, (1, 20))
        y1 = np.exp(x1[0] / 10) * np.cos(2 * x1[0]) + 0.1 * rs.standard_normal(20)
        gs = api.GP(x1, y1, "matern32", device=dev)
        gs.update([1.5], 1.0, 0.1)
        t0 = time.perf_counter()
        for i in range(200):
            gs.update([1.5], 1.0, 0.1 + 1e-4 * (i % 7))
        extras["ms_update_N20_example_jl"] = (time.perf_counter() - t0) / 200 * 1e3
        gs.loglike_grad()
        t0 = time.perf_counter()
        for i in range(200):                      # what one objective + gradient evaluation of a model fitter costs there
            gs.update([1.5], 1.0, 0.1 + 1e-4 * (i % 7))
            gs.loglike_grad()
        extras["ms_update_plus_loglike_grad_N20"] = (time.perf_counter() - t0) / 200 * 1e3
        gs.close()
        # gradient observations (GradientGaussianProcess, §8f4): the n(1+d) = 36 864-row augmented system of the same
        # N=4096, d=8 data — 10.9 GB resident, 1.67e13 flops per update
        note("  gradient observations (36 864 rows)")
        w = np.linspace(1.0, 2.0, D)[:, None]
        yg = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(D)
        dYg = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(D)
        gg = api.GradGP(X, yg, dYg, KERNEL, device=dev)
        gg.update(np.full(D, 0.4), 1.2, 1e-3, 1e-2)
        t0 = time.perf_counter()
        gg.update(np.full(D, 0.41), 1.2, 1e-3, 1e-2)
        t_gu = time.perf_counter() - t0
        gg.predict(Xs)
        t0 = time.perf_counter()
        gg.predict(Xs)
        t_gp = time.perf_counter() - t0
        na = N_OBS * (1 + D)
        extras["gradient_gp"] = {"n": N_OBS, "d": D, "augmented_rows": na, "ms_update": t_gu * 1e3,
                                 "update_tflops": na ** 3 / 3 / t_gu / 1e12, "ms_predict_8192": t_gp * 1e3,
                                 "predict_tflops": float(na) ** 2 * M_CAND / t_gp / 1e12}
        gg.close()

    # ---- what DESIGN.md claims beyond the single-matrix chain, in the driver's own record (rank 0; N=1 only for the device work)
    batched = acq_by_m = None
    if rank == 0 and world == 1 and args.full and (not args.no_extras or args.with_config5):
        note("batched updates, config 5, acquisition by call size")
        batched = {}
        rs = np.random.default_rng(4)
        for S in (2, 4, 8, 32):                                        # boss_gp_loglike_batch at N=4096: S hyper-parameter sets per call
            lamS = np.exp(rs.normal(-0.7, 0.3, (D, S)))
            ampS, sigS = np.exp(rs.normal(0.0, 0.3, S)), np.exp(rs.normal(-3.0, 0.3, S))
            api.loglike_batch(X, y, KERNEL, lamS, ampS, sigS, device=dev)
            t0 = time.perf_counter()
            nrep = 3
            for _ in range(nrep):
                ll, st = api.loglike_batch(X, y, KERNEL, lamS, ampS, sigS, device=dev)
            dt = (time.perf_counter() - t0) / nrep
            batched[f"N4096_S{S}"] = {"updates_per_sec": S / dt, "ms_per_call": dt * 1e3, "tflops": S * flops_update(N_OBS, D) / dt / 1e12,
                                      "frac_of_fp64_mfma_peak": S * flops_update(N_OBS, D) / dt / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                                      "all_positive_definite": bool((st == 0).all())}
        N5, S5 = 1024, 512                                             # BASELINE configs[4]: 512 hyper-parameter samples, N=1024 each
        X5 = rs.uniform(0, 1, (D, N5))
        y5 = np.sin(2 * np.pi * X5).sum(0) / np.sqrt(D) + 0.05 * rs.standard_normal(N5)
        lam5 = np.exp(rs.normal(-0.7, 0.3, (D, S5)))
        amp5, sig5 = np.exp(rs.normal(0.0, 0.3, S5)), np.exp(rs.normal(-3.0, 0.3, S5))
        api.loglike_batch(X5, y5, KERNEL, lam5, amp5, sig5, device=dev)
        t0 = time.perf_counter()
        for _ in range(3):
            ll5, st5 = api.loglike_batch(X5, y5, KERNEL, lam5, amp5, sig5, device=dev)
        dt = (time.perf_counter() - t0) / 3
        batched["config5_512xN1024"] = {"factorisations_per_sec": S5 / dt, "ms_per_call": dt * 1e3, "tflops": S5 * flops_update(N5, D) / dt / 1e12,
                                        "frac_of_fp64_mfma_peak": S5 * flops_update(N5, D) / dt / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                                        "all_positive_definite": bool((st5 == 0).all())}
        note("  config 5 end to end (512 resident posteriors)")
        # BASELINE configs[4] end to end: the 512 posteriors RESIDENT out of one batched factorisation (boss_gp_fit_batch), then the
        # acquisition averaged over all of them at 8192 candidates (one prediction launch over candidate tiles × samples)
        t0 = time.perf_counter()
        gps5, ll5b, st5b = api.fit_batch(X5, y5, KERNEL, lam5, amp5, sig5, device=dev)
        t_fit_first = time.perf_counter() - t0
        for g5 in gps5:
            g5.close()
        t0 = time.perf_counter()
        gps5, ll5b, st5b = api.fit_batch(X5, y5, KERNEL, lam5, amp5, sig5, device=dev)
        t_fit = time.perf_counter() - t0
        h5 = [[g5] for g5 in gps5]
        best5 = float(y5.max())
        api.acq_ei(h5, cand, [1.0], None, best5, want_acq=False)
        t0 = time.perf_counter()
        for _ in range(2):
            _, am5, mx5 = api.acq_ei(h5, cand, [1.0], None, best5, want_acq=False)
        t_acq5 = (time.perf_counter() - t0) / 2
        fl5 = S5 * M_CAND * flops_acq_eval(N5, D)
        batched["config5_acq_S512"] = {"fit_batch_ms": t_fit * 1e3, "fit_batch_first_call_ms": t_fit_first * 1e3,
                                       "fit_tflops": S5 * flops_update(N5, D) / t_fit / 1e12,
                                       "all_positive_definite": bool((st5b == 0).all()),
                                       "loglike_equal_to_loglike_batch": bool(np.array_equal(ll5b, ll5)),
                                       "resident_posteriors": len(gps5), "candidates": M_CAND,
                                       "ms_per_averaged_acquisition": t_acq5 * 1e3, "evals_per_sec": S5 * M_CAND / t_acq5,
                                       "tflops": fl5 / t_acq5 / 1e12, "frac_of_fp64_mfma_peak": fl5 / t_acq5 / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                                       "argmax": [int(am5), float(mx5)]}
        for g5 in gps5:
            g5.close()
        # acquisition over M candidates of the N=4096 posterior: the first call on a fresh factorisation (what one step of a BO
        # loop or one shard of configs[2] at G = 8192/M GPUs pays) and a later call on the same factorisation
        acq_by_m = {}
        for M in ((1024, 2048, 4096, 8192) if not args.no_extras else ()):
            cm = api.Candidates(Xs[:, :M], device=dev)
            first, later = [], []
            for i in range(4):
                gp.update(lam, 1.0, 0.05 + 1e-4 * i)
                t0 = time.perf_counter()
                api.acq_ei([[gp]], cm, [1.0], None, best, want_acq=False)
                first.append(time.perf_counter() - t0)
                api.acq_ei([[gp]], cm, [1.0], None, best, want_acq=False)
                t0 = time.perf_counter()
                api.acq_ei([[gp]], cm, [1.0], None, best, want_acq=False)
                later.append(time.perf_counter() - t0)
            # the same pair as ONE call (boss_gp_update_acq: the candidates' substitution rides along the factorisation) against the
            # two calls timed together — what one BO iteration with a fixed / sampled candidate set costs from parameters to arg-max
            two, one, rode = [], [], []
            for i in range(12):
                t0 = time.perf_counter()
                gp.update(lam, 1.0, 0.05 + 1e-4 * (i % 7))
                api.acq_ei([[gp]], cm, [1.0], None, best, want_acq=False)
                two.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                rr = gp.update_acq(lam, 1.0, 0.05 + 1e-4 * (i % 7), cm, best=best)
                one.append(time.perf_counter() - t0)
                rode.append(bool(rr["fused"]))
            t2, t1 = float(np.median(two[2:])), float(np.median(one[2:]))
            tf, tl = float(np.median(first[1:])), float(np.median(later[1:]))
            fl = M * flops_acq_eval(N_OBS, D)
            acq_by_m[str(M)] = {"update_plus_first_call_ms": t2 * 1e3, "fused_update_plus_acq_ms": t1 * 1e3,
                                "fused_rode_along": bool(all(rode)), "fused_frac_of_peak": (flops_update(N_OBS, D) + fl) / t1 / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                                "first_call_ms": tf * 1e3, "first_call_evals_per_sec": M / tf, "first_call_frac_of_peak": fl / tf / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                                "later_call_ms": tl * 1e3, "later_call_evals_per_sec": M / tl, "later_call_frac_of_peak": fl / tl / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                                "path_first_call": "fused kernel (one workgroup per 32 candidates)" if M > 4096 else
                                                   "256-row substitution steps spread over the chip (few-candidates path)",
                                "path_later_calls": "fused kernel" if M > 4096 else "resident inverse factors (two GEMMs, built on the second call)"}
            cm.close()

    # ---- BASELINE configs[3]: semiparametric model (parametric mean + GP), 2 constrained outputs, N = 2048, d = 6, 8192 candidates
    config4 = None
    if rank == 0 and world == 1 and args.full and not args.no_extras:
        note("config 4 (two outputs, semiparametric)")
        N4, D4, P4 = 2048, 6, 2
        r4 = np.random.default_rng(3)
        X4 = r4.uniform(0, 1, (D4, N4))
        Xs4 = r4.uniform(0, 1, (D4, M_CAND))
        th = np.array([[0.2, 0.3, -0.1, 0.0, 0.1, 0.2, -0.2], [-0.1, 0.1, 0.2, -0.3, 0.0, 0.1, 0.1]])      # m_p(x; θ) = θ_p0 + θ_p1..6 · x, evaluated on the host
        mX4 = [th[p, 0] + th[p, 1:] @ X4 for p in range(P4)]
        mXs4 = np.stack([th[p, 0] + th[p, 1:] @ Xs4 for p in range(P4)])
        Y4 = np.stack([mX4[p] + np.sin(2 * np.pi * X4).sum(0) / np.sqrt(D4) * (1.0 - 0.5 * p) + 0.05 * r4.standard_normal(N4) for p in range(P4)])
        g4 = [api.GP(X4, Y4[p], KERNEL, device=dev) for p in range(P4)]
        c4 = api.Candidates(Xs4, device=dev)
        lam4 = np.full(D4, 0.5)
        ymax4 = [np.inf, 0.5]
        feas = Y4[1] <= 0.5
        best4 = float(Y4[0][feas].max()) if feas.any() else None

        def upd_pair(i, nosync):
            for p in range(P4):
                g4[p].update(lam4, 1.0, 0.05 + 1e-4 * (i % 7), mean_X=mX4[p], sync=not nosync)
            if nosync:
                for p in range(P4):
                    g4[p].sync()
        res4 = {}
        for nosync in (False, True):
            tu, ta = [], []
            for i in range(12):
                t0 = time.perf_counter()
                upd_pair(i, nosync)
                t1 = time.perf_counter()
                _, am4, mx4 = api.acq_ei([g4], c4, [1.0, 0.0], ymax4, best4, mean_Xs=mXs4[None], want_acq=False)
                t2 = time.perf_counter()
                tu.append(t1 - t0)
                ta.append(t2 - t1)
            res4["enqueued_back_to_back" if nosync else "one_after_the_other"] = {
                "ms_two_output_update": float(np.median(tu[2:])) * 1e3, "ms_ei_times_feasibility_pass": float(np.median(ta[2:])) * 1e3}
        tu = res4["enqueued_back_to_back"]["ms_two_output_update"] * 1e-3
        ta = res4["enqueued_back_to_back"]["ms_ei_times_feasibility_pass"] * 1e-3
        config4 = {"workload": "Semiparametric (parametric mean + GP), P = 2 outputs (y_max = [Inf, 0.5]), N = 2048, d = 6, 8192 candidates; mean vectors evaluated on the host",
                   **res4, "two_output_updates_per_sec": 1.0 / tu, "acq_evals_per_sec": M_CAND / ta,
                   "update_frac_of_fp64_mfma_peak": P4 * flops_update(N4, D4) / tu / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                   "acq_frac_of_fp64_mfma_peak": P4 * M_CAND * flops_acq_eval(N4, D4) / ta / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                   "argmax": [int(am4), float(mx4)],
                   "note": "the two outputs' factorisations share one context (one resident chain): enqueued back to back (BOSS_FIT_NO_SYNC) the second "
                           "starts behind the first without a host round trip; they do not overlap"}
        c4.close()
        for g in g4:
            g.close()

    # ---- configs[2] through the one-process multi-GPU entry points (a fresh child process: this one stays alive and idle meanwhile)
    inproc = None
    if rank == 0 and args.full and not args.no_extras:
        note("one-process multi-device entry points (child process)")
        try:
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--inproc-child", str(world), "--steps", str(args.steps),
                                "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
            inproc = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else {"error": (r.stderr or r.stdout)[-400:]}
        except Exception as e:                                         # never fails the bench line
            inproc = {"error": repr(e)}

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        note("CPU baseline (oracle on the host cores)")
        cpu = cpu_baseline(X, y, Xs, lam)

    if rank == 0 and acq_by_m:
        # configs[2] as written shards 8192 candidates over EIGHT GPUs: every rank repeats the update and takes M/8 = 1024 candidates on
        # the fresh factorisation.  What one step then costs per rank, from this run's own single-GPU measurements (the exchange is a
        # 16-byte all-gather, priced at 0.03 ms: an assumption, no multi-GPU box has been available) — the design ceiling of the strong record.
        ms_u = s_upd / args.steps * 1e3
        for G in (2, 4, 8):
            e = acq_by_m.get(str(M_CAND // G))
            if e:
                ms2 = ms_u + e["first_call_ms"] + 0.03
                ms = e["fused_update_plus_acq_ms"] + 0.03
                strong.setdefault("predicted_from_single_gpu", {})[f"G={G}"] = {
                    "ms_per_step": ms, "acq_evals_per_sec": M_CAND / max(ms - ms_u, 1e-3) * 1e3, "steps_per_sec": 1e3 / ms,
                    "speedup_of_the_step_over_G=1": (s_elapsed / args.steps * 1e3) / ms,
                    "ms_per_step_two_calls": ms2, "speedup_two_calls": (s_elapsed / args.steps * 1e3) / ms2,
                    "note": "replicated update (not sharded: 'replicas only') with the M/G candidates of the rank riding along "
                            "(boss_gp_update_acq) + 16-byte exchange; *_two_calls: boss_gp_update then boss_acq_ei"}

    if rank == 0:
        upd_rate = world * args.steps / t_upd
        acq_rate = world * args.steps * M_CAND / t_acq
        out = {
            "metric": "gp_posterior_updates_per_sec (+ acq_evals_per_sec), N=4096 d=8 fp64",
            "value": upd_rate, "unit": "updates/s",
            "acq_evals_per_sec": acq_rate,
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "ms_update": t_upd / args.steps * 1e3, "ms_acq_batch": t_acq / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "d=8 synthetic blackbox, GaussianProcess(Matern52) surrogate, N=4096 fp64 posterior update "
                                   "+ ExpectedImprovement over 8192 candidates per GPU (BASELINE.json configs[1]+[2])",
                       "N": N_OBS, "d": D, "M_per_gpu": M_CAND, "kernel": KERNEL,
                       "parallelism": "single GPU: no exchange" if world == 1 else
                                      f"{world} independent GP slices + candidate shards, 16-byte arg-max all-gather over {backend}"},
            "frac_of_fp64_mfma_roofline": {"update": flops_update(N_OBS, D) * upd_rate / world / (FP64_MFMA_PEAK_TFLOPS * 1e12),
                                           "acq": flops_acq_eval(N_OBS, D) * acq_rate / world / (FP64_MFMA_PEAK_TFLOPS * 1e12)},
            "roofline": roof, "roofline_potrf": roof_potrf, "update_latency": upd_dist, "strong_scaling": strong, "strong_scaling_inproc": inproc,
            "batched_updates": batched, "acq_by_M": acq_by_m, "config4": config4, "cpu_baseline": cpu, "next_rows": extras,
            # BASELINE config 5 end to end (also inside batched_updates, next to the bare batched likelihood it is compared with)
            "config5_acq_S512": (batched or {}).get("config5_acq_S512"),
        }
        if os.environ.get("BOSS_BENCH_REHEARSAL"):
            out["rehearsal"] = f"{world} ranks share {n_vis} GPU(s), exchange over gloo — a functional rehearsal of the N>1 path, not a scaling measurement"
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
