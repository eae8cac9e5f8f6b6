"""Active device check: "is GPU 3 bad, or was it the job?"

Telemetry reads what amd-smi counted; this asks the device itself.  ``bin/gpu_check``
(``csrc/health/gpu_check.hip``) runs a known-answer bf16 GEMM on the matrix units, checked
exactly by on-device checksums, and a moving-inversions sweep over HBM.  Both answers are
exact: pass and fail need no tolerance.  On request the same GEMM check also runs in the
microscaling formats (MXFP8, MXFP4) on the scaled matrix path, which the bf16 one never touches,
and in FP64 on the double-precision matrix path (``v_mfma_f64_16x16x4_f64``), where a 53-bit
significand leaves room for wide data: random 17-bit signed integers, not five small values.
``"int8"`` runs it on the integer matrix path (``v_mfma_i32_32x32x32_i8``) with bytes uniform over
all 256 values: int8 products accumulated in int32 are exact for any data, so this is the one fast
check whose operands toggle every bit.
Also on request, ``gpu_check cu`` says where on the die: one workgroup per compute unit sweeps that
CU's whole 160 KB of LDS and runs a known-answer matrix chain on each of its SIMDs, and a fault is
named by XCC, shader engine and CU, which in CPX mode is one partition and not the whole OAM.
Also on request, ``gpu_check attn`` runs a known-answer fused attention (QK^T, a base-2 online
softmax, PV): matrix accumulators fed back to the matrix unit as operands without leaving the
registers, cross-lane row reductions, ``v_exp_f32``, the fp32 -> bf16 pack, the rescale of live
accumulators.  Small integer scores make every probability a power of two, so this one is exact too.

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


# the largest K at which the binary's exactness argument holds, per microscaling format
# (``run_gemm`` in csrc/health/gpu_check.hip enforces the same)
MX_K_CAP = {"mxfp8": 8192, "mxfp4": 2048}
# the same for every format that adds a child to the bf16 one
EXTRA_K_CAP = {**MX_K_CAP, "fp64": 8192, "int8": 65536}


def check_gpu(device: int = 0, *, gemm: Sequence[int] = (8192, 8192, 4096), seconds: float = 2.0,
              hbm_mib: Optional[float] = None, passes: int = 2, timeout: float = 120.0,
              binary: Optional[str] = None, dtypes: Sequence[str] = ("bf16",), cu: bool = False,
              attn: bool = False) -> Dict[str, Any]:
    """Run the GEMM check, then the HBM check, on ``device``.  ``hbm_mib=None`` lets the
    binary size the sweep (the smaller of 32 GiB and half of what is free); ``binary``
    overrides the built ``bin/gpu_check``.  ``dtypes`` names the GEMM formats: ``"bf16"``
    always, and each of ``"mxfp8"``, ``"mxfp4"``, ``"fp64"``, ``"int8"`` adds one child after it (the
    FP64 one after the microscaling ones, the INT8 one last) with the same M and N and K capped at
    ``EXTRA_K_CAP``, its record under ``"gemm_mxfp8"`` / ``"gemm_mxfp4"`` / ``"gemm_fp64"`` /
    ``"gemm_int8"``.  ``cu=True`` adds the
    per-CU check (``gpu_check cu``: each compute unit's whole LDS and the matrix unit of each of
    its SIMDs, named by XCC, SE and CU) after the GEMM children, its record under ``"cu"``.
    ``attn=True`` adds the fused-attention check (``gpu_check attn`` at its defaults, for ``seconds``)
    after the GEMM children and before the per-CU one, its record under ``"attn"``.  Returns
    ``{"ok", "device", "gemm", "hbm", "elapsed_s", "error"}`` and those: ``ok`` only if every
    child exited 0 and said ok; ``error`` names the steps that failed and how.  After a step
    that ended by signal or timeout nothing more is started: the rest is ``{"skipped": True}``."""
    if "bf16" not in dtypes or any(d != "bf16" and d not in EXTRA_K_CAP for d in dtypes) or len(set(dtypes)) != len(dtypes):
        raise ValueError(f"dtypes must be 'bf16' and any of {sorted(EXTRA_K_CAP)}, each once: {tuple(dtypes)!r}")
    extra = [d for d in dtypes if d in MX_K_CAP] + [d for d in ("fp64", "int8") if d in dtypes]  # fp64 after the mx ones, then int8
    if binary is None:
        from .. import _build

        binary = _build.binary("gpu_check")
    m, n, k = gemm
    steps = [
        ("gemm", [binary, "gemm", "--m", str(m), "--n", str(n), "--k", str(k), "--seconds", repr(float(seconds)),
                  "--device", str(device)]),
        *((f"gemm_{d}", [binary, "gemm", "--dtype", d, "--m", str(m), "--n", str(n), "--k", str(min(k, EXTRA_K_CAP[d])),
                         "--seconds", repr(float(seconds)), "--device", str(device)]) for d in extra),
        *([("attn", [binary, "attn", "--seconds", repr(float(seconds)), "--device", str(device)])] if attn else []),
        *([("cu", [binary, "cu", "--device", str(device)])] if cu else []),
        ("hbm", [binary, "hbm", "--passes", str(passes), "--device", str(device)]
         + (["--mib", repr(float(hbm_mib))] if hbm_mib is not None else [])),
    ]
    out: Dict[str, Any] = {"ok": True, "device": device, "gemm": {}, **{f"gemm_{d}": {} for d in extra},
                           **({"attn": {}} if attn else {}), **({"cu": {}} if cu else {}), "hbm": {},
                           "elapsed_s": 0.0, "error": None}
    errors = []
    t0 = time.monotonic()
    for at, (name, cmd) in enumerate(steps):
        rec, err, wedged = _run_step(cmd, timeout)
        out[name] = rec
        if err:
            out["ok"] = False
            errors.append(f"{name}: {err}")
        if wedged:
            for later, _ in steps[at + 1:]:
                out[later] = {"skipped": True}
            break
    out["elapsed_s"] = round(time.monotonic() - t0, 3)
    out["error"] = "; ".join(errors) or None
    return out


def _gemm_text(rec: Dict[str, Any], label: str = "gemm") -> str:
    if rec.get("skipped"):
        return f"{label} not run"
    if rec.get("ok") is True:
        return f"{label} clean"
    mm = rec.get("mismatches") or []
    if not mm:
        return f"{label} failed"
    first = mm[0]
    delta = first.get("delta", 0)
    where = {"element": "C[{i},{j}]", "row": "row {i} (column stripe {stripe})",
             "column": "column {j} (row stripe {stripe})"}.get(first.get("kind"), "?")
    text = f"{label} mismatch at {where.format(**first)} ({delta:+g}) in tile {first.get('tile')}"
    return text + (f" and {len(mm) - 1} more" if len(mm) > 1 else "")


def _attn_text(rec: Dict[str, Any]) -> str:
    if rec.get("skipped"):
        return "attn not run"
    if rec.get("ok") is True:
        return "attn clean"
    mm = rec.get("mismatches") or []
    if not mm:
        return "attn failed"
    first = mm[0]
    where = {"o": "O[{i},{c}]", "l": "l[{i}]", "m": "m[{i}]"}.get(first.get("kind"), "?").format(**first)
    delta = first.get("delta", 0)  # in units of 2^-12; INT32_MIN marks a value that is no multiple of the unit
    size = "not a multiple of 2^-12" if delta == -2 ** 31 else f"{delta:+d} x 2^-12"
    more = rec.get("mismatch_count", len(mm)) - 1
    return f"attn mismatch at head {first.get('head')} {where} ({size})" + (f" and {more} more" if more > 0 else "")


def _cu_text(rec: Dict[str, Any]) -> str:
    if rec.get("skipped"):
        return "cu not run"
    if rec.get("ok") is True:
        return "cu clean"
    bad = rec.get("bad") or []
    if not bad:
        if rec.get("error") != "coverage":
            return "cu failed"
        if rec.get("covered") != rec.get("cus"):
            return f"cu reached {rec.get('covered')} of {rec.get('cus')} CUs"
        return f"cu reached {rec.get('simds')} of {4 * rec.get('cus', 0)} SIMDs"
    first = bad[0]
    what = []
    if "lds" in first:
        lds = first["lds"]
        what.append(f"lds {lds['count']} bad word{'s' if lds['count'] != 1 else ''} at byte {lds['offset']} "
                    f"(xor {lds['xor']:#010x})")
    if "mfma" in first:
        mfma = first["mfma"]
        what.append(f"matrix unit simd {mfma['simd']} wrong at [{mfma['i']},{mfma['j']}] ({mfma['delta']:+d})")
    more = rec.get("bad_count", len(bad)) - 1
    return (f"cu xcc {first.get('xcc')} se {first.get('se')} cu {first.get('cu')}: {', '.join(what)}"
            + (f" and {more} more" if more > 0 else ""))


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
    parts = [_gemm_text(result.get("gemm") or {})]
    parts += [_gemm_text(result[f"gemm_{d}"] or {}, f"gemm {d}") for d in EXTRA_K_CAP if f"gemm_{d}" in result]
    if "attn" in result:
        parts.append(_attn_text(result["attn"] or {}))
    if "cu" in result:
        parts.append(_cu_text(result["cu"] or {}))
    text = f"gpu {result.get('device')}: {'; '.join(parts)}; {_hbm_text(result.get('hbm') or {})}"
    # "wrong data" is already told by the mismatch; a crash, a timeout or bad output is not
    other = [e for e in (result.get("error") or "").split("; ") if e and not e.endswith(": wrong data")]
    return text + (f" [{'; '.join(other)}]" if other else "")
