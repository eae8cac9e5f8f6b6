"""Command line: ``python -m nexus_supervisor_amd <command>``.

``supervisor``  the cluster supervisor (default; reference ``main.go``)
``agent``       the per-node GPU attribution agent (needs ``NODE_NAME``)
``worker``      one shard-worker process (spawned by the supervisor when
                ``runtime.worker-processes`` > 1; not started by hand)
``config``      print the effective configuration (secrets masked)
``explain``     what the supervisor would decide for ``kubectl get … -o json`` output, and why
``shadow-report`` how a dry-run (shadow) supervisor's decisions agree with the checkpoint store
``build``       build the native components in-tree
``cqlsrv``      run the native in-memory CQL server (tests / local runs)
``gpu-check``   ask one GPU whether it is bad: known-answer MFMA GEMM + HBM pattern test
                (``--device D``, ``--quick``, ``--per-cu``, ``--attention``, ``--json``; exit 1 when a
                check fails)
``version``     print the version
"""
from __future__ import annotations

import json
import os
import subprocess
import sys


def main(argv=None) -> int:
    from .utils.covtrace import install_from_env

    install_from_env()  # child-process coverage for tools/coverage_gate.py (no-op unless enabled)
    argv = list(sys.argv[1:] if argv is None else argv)
    cmd = argv.pop(0) if argv and not argv[0].startswith("-") else "supervisor"
    if cmd == "supervisor":
        from .app import main as run

        return run(argv)
    if cmd == "worker":
        from .parallel.workers import worker_main

        return worker_main()
    if cmd == "agent":
        import asyncio

        from .config import load_config
        from .gpu.agent import run_agent
        from .obs.logging import configure_logging

        cfg = load_config()
        configure_logging(cfg.log_level, static={"service": "nexus-gpu-agent"})
        node = os.environ.get("NODE_NAME", "")
        if not node:
            print("NODE_NAME is required (downward API spec.nodeName)", file=sys.stderr)
            return 1
        asyncio.run(run_agent(cfg, node))
        return 0
    if cmd == "config":
        from .config import load_config, redacted

        print(json.dumps(redacted(load_config()), indent=2, default=str))
        return 0
    if cmd == "explain":
        from .explain import main as explain

        return explain(argv)
    if cmd == "shadow-report":
        from .shadow import main as shadow_report

        return shadow_report(argv)
    if cmd == "build":
        from ._build import main as build

        return build(argv)
    if cmd == "cqlsrv":
        from ._build import binary

        # child process (never exec): keeps signal handling simple for callers
        return subprocess.call([binary("nexus-cqlsrv")] + argv)
    if cmd == "gpu-check":
        import argparse

        from .gpu.health import check_gpu, summarize

        ap = argparse.ArgumentParser(prog="nexus_supervisor_amd gpu-check")
        ap.add_argument("--device", type=int, default=0)
        ap.add_argument("--quick", action="store_true", help="1024^3 GEMM, one pass, 256 MiB of HBM")
        ap.add_argument("--json", action="store_true", help="print the whole record")
        ap.add_argument("--dtypes", default="bf16", help="GEMM formats, comma-separated: bf16[,mxfp8][,mxfp4][,fp64][,int8]")
        ap.add_argument("--all-formats", action="store_true", help="the same as --dtypes bf16,mxfp8,mxfp4; for FP64 or INT8 name it: --dtypes bf16,fp64,int8")
        ap.add_argument("--per-cu", action="store_true", help="also check every CU's LDS and matrix units, named by XCC, SE and CU")
        ap.add_argument("--attention", action="store_true",
                        help="also run a known-answer fused attention (QK^T, exp2 softmax, PV); its final division is not covered")
        a = ap.parse_args(argv)
        quick = {"gemm": (1024, 1024, 1024), "seconds": 0.0, "hbm_mib": 256.0} if a.quick else {}
        dtypes = ("bf16", "mxfp8", "mxfp4") if a.all_formats else tuple(a.dtypes.split(","))
        try:
            result = check_gpu(a.device, dtypes=dtypes, cu=a.per_cu, attn=a.attention, **quick)
        except ValueError as e:
            ap.error(str(e))
        print(json.dumps(result) if a.json else summarize(result))
        return 0 if result["ok"] else 1
    if cmd == "version":
        from .buildmeta import main as version

        return version(argv)
    print(__doc__, file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main())
