#!/usr/bin/env python3
"""North-star benchmark: pod-fail → checkpoint latency (p50/p99) and events/s at
10k concurrent jobs (BASELINE.json ``metric``), one supervised GPU-job slot per rank.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR] [--jobs 10000]
                    [--events 1000] [--transport wire|inproc] [--profile uncapped|reference]

A plain run sets up, warms up, times ``--steps`` steps and prints the result line.  ``--full``
adds what the headline figure does not need: a real HBM-OOM on the rank's GPU for the synthetic
failures' text, the open-loop latency probe, the read-back of every timed row from the store
and the GPU monitor's cost per sample.  ``--dump-outputs DIR``
writes what the last timed step left in the store as ``DIR/<name>.npy``.

One process per GPU (``torch.distributed.run`` for N>1).  Each rank runs one
supervisor replica that owns the shard of runs hashed to it (``sharding``), split
into ``--procs`` shard-worker processes (``runtime.worker-processes``), with
its GPU-job slot's telemetry on ``cuda:LOCAL_RANK`` (native amd-smi monitor; the
HIP OOM message and VRAM peak of a real HBM-OOM on that GPU seed the synthetic
hbm-oom failures).  Per-rank work is fixed (weak scaling): ``--jobs`` live runs,
``--events`` pod failures per step.

A *step* = ``--events`` pod failures (plus replacement-run churn) pushed through
the watch → informer → classify → keyed pipeline → checkpoint store path, timed
until the last of them is acknowledged by the store.  ``--transport wire`` (the
default) runs the real protocols: a fake kube-apiserver streams the watch over
HTTP (the native ``nexus-kubesim``) and the native CQL server (``nexus-cqlsrv``)
holds ``nexus.checkpoints``;
``inproc`` feeds informers directly and uses the in-memory store.

Rank 0 prints one JSON line; ``value`` = total events/s over all ranks
(total events ÷ max rank time), ``vs_baseline`` against the reference's derived
10 decisions/s ceiling (Helm defaults: 10 eps, burst 100, 2 workers).
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

REFERENCE_EPS = 10.0  # derived throughput ceiling at Helm defaults
METRIC = "pod-fail→checkpoint p50/p99 latency + events/sec at 10k concurrent jobs"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: a real HBM-OOM on the rank's "
                         "GPU whose text the synthetic hbm-oom failures carry (real_hbm_oom), the open-loop latency "
                         "probe (--probe-events, latency_at_rate), the read-back of every timed row from the store "
                         "(readback) and the GPU monitor's CPU per sample (config.monitor)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps write DIR/<name>.npy (float32): the lifecycle stage the store holds "
                         "for every run the last timed step failed (last_step_failed_stage) and started "
                         "(last_step_started_stage), numbered as bench/runner.py STAGE_CODES, in the seeded "
                         "workload's order")
    ap.add_argument("--jobs", type=int, default=None,
                    help="concurrent live jobs per rank (default 10,000; node mode: 10,000 over the node's slots)")
    ap.add_argument("--events", type=int, default=None,
                    help="pod-fail events per step per rank (default 6,000: the driver's 20 steps time at least 5 s on "
                         "one MI355X box; node mode: 6,000 over the node's slots)")
    ap.add_argument("--transport", choices=("wire", "inproc"), default="wire")
    ap.add_argument("--profile", choices=("uncapped", "reference"), default="uncapped",
                    help="reference = Helm defaults (10 eps, burst 100, 2 workers)")
    ap.add_argument("--workers", type=int, default=256)
    ap.add_argument("--procs", type=int, default=0,
                    help="supervisor shard-worker processes per replica (runtime.worker-processes; wire transport); "
                         "0 = auto: the rank's CPU share minus 4 for the harness, at most 7 (the measured "
                         "knee: auto_procs)")
    ap.add_argument("--inflight", type=int, default=4, help="steps pushed ahead of acknowledgement")
    ap.add_argument("--no-pregen", action="store_true",
                    help="generate each step's synthetic traffic on demand instead of before the timed region")
    ap.add_argument("--kube-connections", type=int, default=256)
    ap.add_argument("--probe-events", type=int, default=600,
                    help="--full, after the timed steps: open-loop latency probe with this many single failures, Poisson "
                         "arrivals (0 = off); 600 at 1000/min take ~36 s and make p99 a real quantile")
    ap.add_argument("--probe-rate", type=float, default=1000.0, help="probe rate, pod failures per minute (BASELINE config 4)")
    ap.add_argument("--no-real-oom", action="store_true",
                    help="--full: skip the real HBM-OOM on the rank's GPU (its message and VRAM peak seed the synthetic "
                         "hbm-oom failures; a plain run uses the recorded text of one, workload.DEFAULT_HIP_OOM)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json-out", default="")
    ap.add_argument("--pprof-out", default="", help="write a pprof profile of the timed steps (rank 0)")
    ap.add_argument("--pprof-hz", type=int, default=199, help="pprof sampling rate (CPU-time Hz)")
    ap.add_argument("--cql-latency-us", type=int, default=0, help="inject CQL server response latency")
    ap.add_argument("--cql-lwt-latency-us", type=int, default=-1,
                    help="extra CQL server latency of a conditional write (a Paxos round: ~4 round trips where a "
                         "plain write takes 1); -1 = 3 x --cql-latency-us")
    ap.add_argument("--no-shard-label", action="store_true",
                    help="shared cluster: every replica watches the whole namespace (filtered before decode) "
                         "instead of only its shard's Pods/Jobs by the sharding.shard-label selector")
    ap.add_argument("--hbm-shape", choices=("default-pod", "termination-message"), default="default-pod",
                    help="synthetic HBM-OOM failures: a default pod (empty termination message, the real HIP OOM "
                         "text in the container log, read over pods/log) or the text in the termination message")
    ap.add_argument("--workload", choices=("lifecycle", "failures"), default="lifecycle",
                    help="lifecycle (default): every failed run is replaced by a new run that goes Pending -> "
                         "scheduled -> Running with the kubelet's Events (its Started is a ToRunning decision: "
                         "checkpoint read + RUNNING upsert), failures carry their Job / Event traffic and Events "
                         "expire; failures: the round-4 shape (failure traffic only, new runs never start)")
    ap.add_argument("--cpu-affinity", default="auto", choices=("auto", "none", "numa", "numa-cores"),
                    help="CPU placement of the bench's processes (utils/affinity.py): auto = the rank GPU's NUMA "
                         "node, one hardware thread per core (numa-cores) when that leaves >= 16 CPUs; none = "
                         "the scheduler's")
    ap.add_argument("--diag-no-thp", action="store_true",
                    help="diagnostic: disable transparent huge pages for the bench and every process it starts")
    ap.add_argument("--diag-probe-timeline", action="store_true",
                    help="diagnostic: every second of the probe, each bench process's CPU, the host's busy CPUs and the "
                         "cgroup's CFS throttling (latency_at_rate.cpu_timeline)")
    ap.add_argument("--diag-step-timeline", action="store_true",
                    help="diagnostic: each bench process's CPU every 0.2 s of the timed steps, and which one was "
                         "closest to a full core in their steady part (config.step_timeline)")
    ap.add_argument("--diag-slow-callback-ms", type=float, default=0.0,
                    help="diagnostic: count the event-loop callbacks (parent and workers) that run at least this "
                         "long and list the probe's in latency_at_rate.slow_callbacks (obs/loopwatch.py)")
    ap.add_argument("--api-latency-us", type=int, default=0,
                    help="simulated kube-apiserver answer latency of object requests (Job DELETE / GET / PATCH): "
                         "the etcd write + admission a real apiserver spends; LIST / WATCH unaffected")
    ap.add_argument("--api-write-qps", type=float, default=0.0,
                    help="APF-like cap on the simulator's mutating requests: the excess is answered 429 + "
                         "Retry-After (0 = no cap)")
    ap.add_argument("--kube-qps", type=float, default=1_000_000.0,
                    help="the supervisor's client-side kube-qps bucket (kube-burst = the same number); the "
                         "production default is 50 / 100")
    ap.add_argument("--actuation", choices=("auto", "fused", "two-step"), default="auto",
                    help="compat.fused-write: auto (one conditional write per decision only under HA, else read + "
                         "write), fused (always one conditional write), two-step (the reference's read + write)")
    ap.add_argument("--two-step-write", action="store_true", help="alias of --actuation two-step")
    ap.add_argument("--conditional-update", choices=("auto", "always", "never"), default="auto",
                    help="compat.conditional-update of the two-step path (never = the reference's plain writes)")
    ap.add_argument("--slot-mode", choices=("auto", "node", "replica"), default="auto",
                    help="node (auto for N>1): ONE supervisor replica and ONE GPU monitor on rank 0 supervise every "
                         "GPU slot of the node — each rank is a slot whose runs are on its GPU and whose real "
                         "HBM-OOM must be attributed to that physical GPU (the production shape: one HA "
                         "supervisor, one node agent); replica: one replica + monitor + apiserver per slot")
    ap.add_argument("--gpu-evidence", choices=("local", "agent"), default="local",
                    help="local: the supervisor reads the GPU monitor in-process (an in-node supervisor); agent: "
                         "the chart's deployment — the node agent as its own process (amd-smi monitor) annotates "
                         "each failed pod and the supervisor, with no local telemetry, holds the decision up to "
                         "gpu.evidence-wait (2s) for it (wire transport; HBM-OOM text in the termination message)")
    ap.add_argument("--cluster", choices=("auto", "shared", "per-rank"), default="auto",
                    help="per-rank (default) = each GPU-job slot's replica has its own namespace shard, apiserver "
                         "simulator and CQL server; shared = one apiserver + one CQL server for all ranks, each "
                         "replica watching the whole namespace and owning its shard (a single-threaded simulator "
                         "then caps the whole curve: profiles/r3_kubesim_threads_ab)")
    return ap.parse_args(argv)


BENCH_WORKERS_KNEE = 7


def auto_procs(local_world: int) -> int:
    """Shard-worker processes per replica: the rank's CPU share minus 4 (simulated
    apiserver, CQL server, bench driver + watch hub, cluster process), within [1, 7].

    The rule, measured: add workers while they buy throughput the box resolves without
    raising the CPU per failure, and keep the single-threaded apiserver simulator clear of
    saturation (the line must measure the supervisor, not the harness).  Round 4, default-pod
    workload (profiles/r4_procs_ab/, same box, interleaved, probe on): 6 workers 34.1k
    failures/s (31.1-34.7k) at 152 µs of replica CPU per failure, probe 0.56 / 1.30 ms; 8
    workers 33.3k (32.7-33.7k) at 188 µs, probe 0.66 / 1.43 ms.  Another box
    (profiles/r4_sweep_final/, probe off) had 8 workers ahead (36.7k vs 31.4k) and 10 at
    39.5k with the simulator at 0.87 of a core.  Rounds 2-3 found six the knee as well
    (profiles/r3_cpu_ab/, profiles/r4_sweep/): past six the CPU per failure rises 15-40 %
    while the throughput gain stays inside the box-to-box spread.  On the compiled hot path
    (profiles/r4_procs_ab_compiled/, same box, interleaved, probe on): 6 workers 38.5k at
    115 µs, 8 workers 42.3k at 145 µs — +10 % throughput for +26 % CPU per failure.
    Round 6, lifecycle workload, the Event watch's noise selector and NUMA placement
    (profiles/r6/bench_r6{p,q,r}_*, interleaved on three boxes, probe off): 6 workers 21.4-22.9k
    at 251-268 µs, 7 workers 23.2-24.1k at 257-261 µs (+6 %), 8 workers 22.5-24.2k at 249-271 µs
    with the workers at 0.68-0.72 of a core — past seven the simulator paces the line."""
    from nexus_supervisor_amd.utils.cpus import cpu_share

    return max(1, min(BENCH_WORKERS_KNEE, int(cpu_share() / max(local_world, 1)) - 4))


def _harness_bound(cpu) -> dict:
    """Did a harness process limit the run?  The traffic generator by its CPU share, the
    apiserver simulator by its busiest serial part (event loop, apply port, store lock, GC thread), the
    sharded CQL server by its per-shard CPU."""
    util = {k[:-5]: v for k, v in cpu.items() if k in ("kubesim_util", "cqlsrv_util", "cluster_util")}
    limit = dict(util)
    if "cqlsrv" in limit:
        limit["cqlsrv"] = util["cqlsrv"] / max(1, int(cpu.get("cqlsrv_shards") or 1))
    if "kubesim" in limit and cpu.get("kubesim_serial_util") is not None:
        # the simulator is multi-threaded: its serial parts (event loop, apply port, store
        # lock, GC thread), not its process CPU, say whether it saturated
        limit["kubesim"] = cpu["kubesim_serial_util"]
    bound = any(v >= 0.9 for v in limit.values())
    out = {"bound": bound, "util": util, "limit_util": {k: round(v, 3) for k, v in limit.items()}}
    if bound:
        out["note"] = "a harness process was saturated: value is a lower bound of the supervisor's throughput"
    return out


def real_hbm_oom(local_rank: int, workdir: str):
    """Run the HIP stress workload to a real HBM OOM on this rank's GPU; returns its
    termination message (None when unavailable)."""
    try:
        from nexus_supervisor_amd._build import binary

        exe = binary("gpu_stress")
    except Exception as exc:  # noqa: BLE001
        print(f"[bench] gpu_stress unavailable: {exc}", file=sys.stderr)
        return None
    log = os.path.join(workdir, f"termination-{local_rank}.log")
    env = dict(os.environ, HIP_VISIBLE_DEVICES=str(local_rank))
    try:
        p = subprocess.run([exe, "hbm-oom", "--chunk-gib", "8", "--linger", "0.6", "--termination-log", log,
                            "--max-gib", "400"], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        print("[bench] gpu_stress hbm-oom timed out", file=sys.stderr)
        return None
    if p.returncode != 1 or not os.path.exists(log):
        print(f"[bench] gpu_stress rc={p.returncode}: {p.stderr[-400:]}", file=sys.stderr)
        return None
    with open(log) as f:
        return f.read().strip()


def main(argv=None) -> int:
    args = parse_args(argv)
    import faulthandler
    import signal

    try:  # diagnostics: `kill -USR1 <pid>` dumps the stacks
        faulthandler.register(signal.SIGUSR1, all_threads=True)
    except (ValueError, OSError, AttributeError):  # stderr without a file descriptor (pytest capture)
        pass
    if args.diag_slow_callback_ms > 0:  # read by the replica parent and inherited by its workers
        os.environ["NEXUS_SLOW_CALLBACK_MS"] = str(args.diag_slow_callback_ms)
    if args.diag_no_thp:
        # PR_SET_THP_DISABLE: no transparent huge pages for this process and every child
        # (inherited over fork and exec) — khugepaged collapses take the address-space lock
        import ctypes

        ctypes.CDLL(None, use_errno=True).prctl(41, 1, 0, 0, 0)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # before anything touches the GPU or starts a process: every child inherits the placement
    from nexus_supervisor_amd.utils import affinity

    visible = [v for v in os.environ.get("HIP_VISIBLE_DEVICES", "").split(",") if v.strip().isdigit()]
    gpu_index = int(visible[local_rank]) if local_rank < len(visible) else local_rank
    try:
        # the host is shared: leave out the cores another tenant keeps busy right now
        busy = affinity.cpu_busy(0.25) if args.cpu_affinity != "none" else None
        placed = affinity.apply(affinity.plan(args.cpu_affinity, gpu_index, busy=busy))
    except OSError as exc:  # a restricted sandbox: keep the scheduler's placement
        print(f"[bench] cpu affinity not applied: {exc}", file=sys.stderr)
        placed = None
    slot_mode = args.slot_mode if args.slot_mode != "auto" else (
        "node" if world > 1 and args.transport == "wire" else "replica")
    if slot_mode == "node" and args.transport != "wire":
        raise SystemExit("--slot-mode node needs --transport wire")
    if args.gpu_evidence == "agent":
        if args.transport != "wire":
            raise SystemExit("--gpu-evidence agent needs --transport wire")
        if args.cluster == "shared" and world > 1:
            raise SystemExit("--gpu-evidence agent: one agent per apiserver (per-rank cluster or node mode)")
    # Node mode is ONE replica and ONE simulator for the whole node: the north-star namespace
    # (10k concurrent jobs, 6,000 failures a step) is split over the slots, so N slots measure
    # the same supervisor on the same total work — strong scaling.  Replica mode keeps the
    # per-slot work fixed (weak scaling: N replicas, N clusters).
    node_split = slot_mode == "node" and world > 1
    if args.jobs is None:
        args.jobs = -(-10_000 // world) if node_split else 10_000
    if args.events is None:
        args.events = -(-6000 // world) if node_split else 6000
    if args.procs <= 0:
        # node mode: the one replica gets the node's CPU share (the other ranks only run GPU work)
        args.procs = auto_procs(1 if slot_mode == "node" else int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))

    import torch

    has_gpu = torch.cuda.is_available()
    dist = None
    if world > 1:
        import torch.distributed as dist  # noqa: F811

        backend = "nccl" if has_gpu else "gloo"
        if has_gpu:
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend)
    device = torch.device(f"cuda:{local_rank}") if has_gpu else torch.device("cpu")

    from nexus_supervisor_amd.bench.runner import BenchConfig, mark, run_rank

    mark("torch imported, device chosen")
    workdir = tempfile.mkdtemp(prefix=f"nexus-bench-r{rank}-")
    hip_msg = None
    if has_gpu and args.full and not args.no_real_oom:
        hip_msg = real_hbm_oom(local_rank, workdir)
        mark("real HBM-OOM done")

    def barrier_sync():
        if dist is not None:
            if has_gpu:
                dist.barrier(device_ids=[local_rank])
            else:
                dist.barrier()
        if has_gpu:
            torch.cuda.synchronize(device)

    def share(obj):
        """rank 0's object on every rank (shared-cluster rendezvous)."""
        if dist is None:
            return obj
        box = [obj]
        dist.broadcast_object_list(box, src=0)
        return box[0]

    def oom_phase():
        """Node mode, every rank at once: a real HBM-OOM on this rank's GPU (the text a
        default pod on it would log), gathered on every rank."""
        barrier_sync()
        t0 = time.time()
        msg = real_hbm_oom(local_rank, workdir) if has_gpu else None
        mine = {"slot": rank, "message": msg, "real": bool(msg), "t0": t0, "t1": time.time()}
        if dist is None:
            return [mine]
        out = [None] * world
        dist.all_gather_object(out, mine)
        return out

    cluster = args.cluster if args.cluster != "auto" else "per-rank"
    if slot_mode == "node" and world > 1:
        cluster = "node"
    cfg = BenchConfig(rank=rank, world=world, local_rank=local_rank, jobs=args.jobs, events=args.events,
                      steps=args.steps, warmup=args.warmup, transport=args.transport, profile=args.profile,
                      workers=args.workers, seed=args.seed, hip_oom_message=hip_msg, telemetry="amdsmi" if has_gpu else "fake",
                      workdir=workdir, cql_latency_us=args.cql_latency_us, inflight=args.inflight,
                      api_latency_us=args.api_latency_us, api_write_qps=args.api_write_qps, kube_qps=args.kube_qps,
                      shard_label="" if args.no_shard_label else "nexus.amd.com/shard",
                      hbm_shape=args.hbm_shape if args.transport == "wire" else "termination-message",
                      fused_write={"auto": "auto", "fused": "true", "two-step": "false"}[
                          "two-step" if args.two_step_write else args.actuation],
                      conditional_update=args.conditional_update, cql_lwt_latency_us=args.cql_lwt_latency_us,
                      kube_connections=args.kube_connections, probe_events=args.probe_events,
                      probe_rate_per_min=args.probe_rate, procs=args.procs if args.transport == "wire" else 1,
                      pregen=not args.no_pregen, cluster=cluster, run_starts=args.workload == "lifecycle",
                      pprof_out=args.pprof_out if rank == 0 else "", pprof_hz=args.pprof_hz, slot_mode=slot_mode,
                      gpu_evidence=args.gpu_evidence, probe_timeline=args.diag_probe_timeline,
                      step_timeline=args.diag_step_timeline, full=args.full, dump_outputs=bool(args.dump_outputs))
    res = asyncio.run(run_rank(cfg, barrier_sync, share, oom_phase if slot_mode == "node" and world > 1 else None))

    if args.dump_outputs and res.get("outputs"):
        import numpy as np

        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, values in res["outputs"].items():  # a few thousand numbers each
            np.save(os.path.join(args.dump_outputs, f"{name}.npy" if world == 1 else f"{name}.rank{rank}.npy"),
                    np.asarray(values, dtype=np.float32))

    elapsed = res["elapsed"]
    rb = res.get("readback") or {}
    wobj = res.get("watch_objects_per_failure")
    stats = torch.tensor([elapsed, float(res["events"]), float(res["errors"]), float(res["wrong_stage"]),
                          float(rb.get("checked", 0)), float(rb.get("wrong", 0)), float(res.get("starts", 0)),
                          float(res.get("failures", 0)), float(wobj if wobj is not None else 0.0),
                          1.0 if wobj is not None else 0.0],
                         dtype=torch.float64, device=device)

    def gather_all(values):
        """Every rank's latency samples, concatenated (ranks hold different counts)."""
        t = torch.tensor(values, dtype=torch.float64, device=device)
        if dist is None:
            return t.cpu()
        sizes = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor([t.numel()], dtype=torch.int64, device=device))
        mlen = max(1, int(max(x.item() for x in sizes)))
        padded = torch.full((mlen,), float("nan"), dtype=torch.float64, device=device)
        padded[: t.numel()] = t
        gathered = [torch.empty(mlen, dtype=torch.float64, device=device) for _ in range(world)]
        dist.all_gather(gathered, padded)
        cat = torch.cat(gathered)
        return cat[~torch.isnan(cat)].cpu()

    allat = gather_all(res["latencies_ms"])
    start_lat = gather_all(res.get("start_latencies_ms") or [])
    if dist is not None:
        mx = stats.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = stats.clone()
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        max_elapsed, total_events, total_errors = mx[0].item(), sm[1].item(), sm[2].item()
        wrong_stage, rb_checked, rb_wrong = sm[3].item(), sm[4].item(), sm[5].item()
        # the mean over the ranks that measured it (node mode: rank 0's simulator only)
        total_starts, total_failures = sm[6].item(), sm[7].item()
        watch_objects = sm[8].item() / sm[9].item() if sm[9].item() else None
    else:
        max_elapsed, total_events, total_errors = elapsed, float(res["events"]), float(res["errors"])
        wrong_stage, rb_checked, rb_wrong = float(res["wrong_stage"]), float(rb.get("checked", 0)), float(rb.get("wrong", 0))
        total_starts, total_failures, watch_objects = float(res.get("starts", 0)), float(res.get("failures", 0)), wobj
    mine = {"rank": rank, "supervisor_cpu_us_per_event": (res.get("cpu") or {}).get("supervisor_cpu_us_per_event"),
            "harness_bound": _harness_bound(res.get("cpu") or {})}
    per_rank = [mine]
    if dist is not None:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)

    if rank == 0:
        eps = total_events / max_elapsed if max_elapsed > 0 else 0.0
        q = torch.quantile(allat, torch.tensor([0.5, 0.99], dtype=torch.float64)).tolist() if allat.numel() else [None, None]
        qs = (torch.quantile(start_lat, torch.tensor([0.5, 0.99], dtype=torch.float64)).tolist()
              if start_lat.numel() else [None, None])
        hb = dict(_harness_bound(res.get("cpu") or {}))
        bound_ranks = [r["rank"] for r in per_rank if r["harness_bound"]["bound"]]
        if world > 1:
            hb["bound"] = bool(bound_ranks)
            hb["bound_ranks"] = bound_ranks
            if bound_ranks and "note" not in hb:
                hb["note"] = "a harness process was saturated: value is a lower bound of the supervisor's throughput"
        if hb["bound"]:
            print(f"[bench] WARNING: harness-bound run ({hb['limit_util']}): {hb['note']}", file=sys.stderr, flush=True)
        out = {
            "metric": METRIC,
            # pod failures decided and acknowledged per second (each brings its replacement
            # run's start: decisions_per_s counts both)
            "value": round(eps, 2),
            "unit": "pod-failures/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * max_elapsed / max(args.steps, 1), 3),
            "higher_is_better": True,
            "scaling": "strong" if cluster == "node" else "weak",
            "vs_baseline": round(eps / REFERENCE_EPS, 2),
            "dtype": "n/a (control plane, no GPU compute)",
            "data": "synthetic pod-failure events, random job ids (no cluster / dataset)",
            # latency of the timed (saturating) steps: 1000-failure bursts queue behind each other
            "p50_ms": round(q[0], 3) if q[0] is not None else None,
            "p99_ms": round(q[1], 3) if q[1] is not None else None,
            # every decision the timed steps carried: the failures plus the replacement runs'
            # ToRunning (Started Event -> checkpoint read + RUNNING upsert, the reference's most
            # frequent decision)
            "decisions_per_s": round((total_failures + total_starts) / max_elapsed, 2) if max_elapsed > 0 else 0.0,
            "starts_per_s": round(total_starts / max_elapsed, 2) if max_elapsed > 0 else 0.0,
            "start_p50_ms": round(qs[0], 3) if qs[0] is not None else None,
            "start_p99_ms": round(qs[1], 3) if qs[1] is not None else None,
            # Events / Pods / Jobs the namespace's watches carried per pod failure (apiserver
            # resourceVersion growth over the timed steps, the supervisor's DELETEs included)
            "watch_objects_per_failure": round(watch_objects, 2) if watch_objects else None,
            # open-loop latency at the north-star churn rate (1000 pod-fail events/min), rank 0
            "latency_at_rate": res.get("probe"),
            "errors": int(total_errors),
            # correctness of what was measured: decisions whose written stage differs from the
            # workload's expected stage, and timed rows read back from the store afterwards
            "wrong_stage": int(wrong_stage),
            "readback": {"checked": int(rb_checked), "wrong": int(rb_wrong),
                         "examples_rank0": rb.get("examples", [])[:3] + res.get("wrong_examples", [])[:3]},
            "supervisor_cpu_us_per_event_rank0": (res.get("cpu") or {}).get("supervisor_cpu_us_per_event"),
            # replica CPU (parent + shard workers) per pod failure, every rank
            "supervisor_cpu_us_per_event_by_rank": [r["supervisor_cpu_us_per_event"] for r in per_rank],
            # which side limited the run: a harness process (apiserver simulator / CQL server /
            # traffic generator) near a full core means the value is the harness's ceiling
            "harness_bound": hb,
            "config": {
                "model": "nexus-supervisor (informer→classify→CQL write), 1 replica-shard per GPU-job slot",
                "global_batch": args.events * world,
                "seq_len": None,
                "parallelism": (f"node{world}slots:1replica:{args.procs}proc" if cluster == "node" else
                                f"shard{world}x{args.procs if args.transport == 'wire' else 1}proc"),
                "slot_mode": slot_mode,
                "full": args.full,
                "cpu_affinity": placed,
                # GPU monitors over the node's GPUs: one (rank 0's, the node agent's role) in
                # node mode, one per rank otherwise
                "gpu_monitors": 1 if cluster == "node" or world == 1 else world,
                "monitor": res.get("monitor"),
                # node mode: every slot's real HBM-OOM, at once, attributed to its physical GPU
                "attribution": res.get("attribution"),
                # where the supervisor's GPU evidence comes from: its own monitor, or the node
                # agent's pod annotation (with the agent's cost and the waits that expired)
                "gpu_evidence": res.get("gpu_evidence"),
                "cluster": cluster if args.transport == "wire" else "in-process",
                "shard_label": (not args.no_shard_label) if cluster == "shared" and world > 1 else None,
                "concurrent_jobs_per_rank": args.jobs,
                "events_per_step_per_rank": args.events,
                "workload": args.workload,
                "transport": args.transport,
                "profile": args.profile,
                "store": res.get("store"),
                "workers": res.get("workers"),
                "worker_processes": args.procs if args.transport == "wire" else 1,
                "inflight_steps": args.inflight,
                "pregenerated_input": not args.no_pregen and args.transport == "wire",
                "rate_limit_eps": res.get("eps"),
                "kube_qps": res.get("kube_qps"),
                # hot-path modules running as C extensions (nexus_supervisor_amd/compiled.py)
                "compiled_modules": len(__import__("nexus_supervisor_amd.compiled", fromlist=["loaded"]).loaded()),
                "gpu_telemetry": res.get("telemetry"),
                "real_hbm_oom": bool(hip_msg),
                "hbm_oom_shape": args.hbm_shape if args.transport == "wire" else "termination-message",
                "cql_latency_us": args.cql_latency_us,
                "api_latency_us": args.api_latency_us,
                "api_write_qps": args.api_write_qps,
                "actuation": res.get("actuation"),
                "cql_lwt_latency_us": args.cql_lwt_latency_us,
                "stages_ms": res.get("stages"),
                "cpu_util_rank0": res.get("cpu"),
                "step_done_ms_rank0": res.get("step_done_ms"),
                **({"step_timeline": res["step_timeline"]} if res.get("step_timeline") else {}),
                "baseline": "reference derived ceiling 10 decisions/s (Helm defaults; BASELINE.md)",
            },
        }
        line = json.dumps(out)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
