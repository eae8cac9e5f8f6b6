"""Active device check: "is GPU 3 bad, or was it the job?"

Telemetry reads what amd-smi counted; this asks the device itself.  ``bin/gpu_check``
(``csrc/health/gpu_check.hip``) runs a known-answer bf16 GEMM on the matrix units, checked
exactly by on-device checksums, and a moving-inversions sweep over HBM.  Both answers are
exact: pass and fail need no tolerance.

The checks run as child processes, one after the other.  The caller (a long-lived agent)
never opens the GPU itself, so it never shows in amd-smi's process list, and a child that
hangs is killed at its timeout, not retried.  The verdict means something only on a device
that is otherwise idle.
"""
from __future__ import annotations

import json
import subprocess
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple


def _run_step(cmd: List[str], timeout: float) -> Tuple[Dict[str, Any], Optional[str], bool]:
    """One child: (its JSON record, error text or None, whether the device may be wedged —
    the child timed out or died by signal — so nothing more should be started on it)."""
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {}, f"timeout after {timeout:g}s (killed)", True
    except OSError as e:
        return {}, f"could not start: {e}", True
    if p.returncode < 0:
        return {}, f"killed by signal {-p.returncode}", True
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    try:
        rec = json.loads(lines[-1])
        if not isinstance(rec, dict):
            raise ValueError("not an object")
    except (IndexError, ValueError):
        tail = (p.stderr.strip().splitlines() or [""])[-1]
        return {}, f"exit {p.returncode}, unparsable output{': ' + tail if tail else ''}", False
    rec["exit"] = p.returncode
    if p.returncode == 0 and rec.get("ok") is True:
        return rec, None, False
    if p.returncode == 1:
        return rec, "wrong data", False
    return rec, f"exit {p.returncode}: {rec.get('error', 'no reason given')}", False


def check_gpu(device: int = 0, *, gemm: Sequence[int] = (8192, 8192, 4096), seconds: float = 2.0,
              hbm_mib: Optional[float] = None, passes: int = 2, timeout: float = 120.0,
              binary: Optional[str] = None) -> Dict[str, Any]:
    """Run the GEMM check, then the HBM check, on ``device``.  ``hbm_mib=None`` lets the
    binary size the sweep (the smaller of 32 GiB and half of what is free); ``binary``
    overrides the built ``bin/gpu_check``.  Returns ``{"ok", "device", "gemm", "hbm",
    "elapsed_s", "error"}``: ``ok`` only if both children exited 0 and said ok; ``error``
    names the step that failed and how.  The HBM step is skipped when the GEMM step ended
    by signal or timeout."""
    if binary is None:
        from .. import _build

        binary = _build.binary("gpu_check")
    m, n, k = gemm
    steps = [
        ("gemm", [binary, "gemm", "--m", str(m), "--n", str(n), "--k", str(k), "--seconds", repr(float(seconds)),
                  "--device", str(device)]),
        ("hbm", [binary, "hbm", "--passes", str(passes), "--device", str(device)]
         + (["--mib", repr(float(hbm_mib))] if hbm_mib is not None else [])),
    ]
    out: Dict[str, Any] = {"ok": True, "device": device, "gemm": {}, "hbm": {}, "elapsed_s": 0.0, "error": None}
    errors = []
    t0 = time.monotonic()
    for name, cmd in steps:
        rec, err, wedged = _run_step(cmd, timeout)
        out[name] = rec
        if err:
            out["ok"] = False
            errors.append(f"{name}: {err}")
        if wedged:
            if name == "gemm":
                out["hbm"] = {"skipped": True}
            break
    out["elapsed_s"] = round(time.monotonic() - t0, 3)
    out["error"] = "; ".join(errors) or None
    return out


def _gemm_text(rec: Dict[str, Any]) -> str:
    if rec.get("ok") is True:
        return "gemm clean"
    mm = rec.get("mismatches") or []
    if not mm:
        return "gemm failed"
    first = mm[0]
    delta = first.get("delta", 0)
    where = {"element": "C[{i},{j}]", "row": "row {i} (column stripe {stripe})",
             "column": "column {j} (row stripe {stripe})"}.get(first.get("kind"), "?")
    text = f"gemm mismatch at {where.format(**first)} ({delta:+g}) in tile {first.get('tile')}"
    return text + (f" and {len(mm) - 1} more" if len(mm) > 1 else "")


def _hbm_text(rec: Dict[str, Any]) -> str:
    if rec.get("skipped"):
        return "hbm not run"
    if rec.get("ok") is True:
        return "hbm clean"
    mm = rec.get("mismatches") or []
    if not mm:
        return "hbm failed"
    return (f"hbm {rec.get('mismatch_count', len(mm))} bad words, first at byte {mm[0]['offset']} "
            f"(xor {mm[0]['xor']:#010x})")


def summarize(result: Dict[str, Any]) -> str:
    """The one-line cause text an operator sees, e.g.
    ``gpu 0: gemm mismatch at C[37,101] (+1) in tile 0; hbm clean``."""
    text = f"gpu {result.get('device')}: {_gemm_text(result.get('gemm') or {})}; {_hbm_text(result.get('hbm') or {})}"
    # "wrong data" is already told by the mismatch; a crash, a timeout or bad output is not
    other = [e for e in (result.get("error") or "").split("; ") if e and not e.endswith(": wrong data")]
    return text + (f" [{'; '.join(other)}]" if other else "")
