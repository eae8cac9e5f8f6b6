"""``bin/gpu_check`` (csrc/health/gpu_check.hip) and its wrapper ``gpu/health.py``.

Inputs are integers in [-2, 2], so every sum the GEMM forms is an integer below 2^24 and
fp32 is exact: each comparison is ``np.array_equal`` against float64, no tolerance.
"""
import json
import subprocess
import sys

import numpy as np
import pytest


def _run(args):
    from nexus_supervisor_amd._build import binary

    p = subprocess.run([binary("gpu_check")] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1])


def _bf16_bits(a):
    return (a.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,poison", [
    (32, 32, 16, None),      # one MFMA, the rest of the tile zero-filled: operand / accumulator lane layout
    (128, 128, 64, None),    # one full tile, one K step: wave quadrants, LDS padding
    (128, 128, 192, None),   # three K steps: double-buffer reuse, odd step count
    (160, 96, 80, None),     # partial tile in M, N under a tile, short last K step: zero-fill, bounds
    (256, 384, 128, None),   # several tiles both ways, not square: tile indices, checksum stripes
    (160, 96, 80, (37, 5)),  # the detector: one element off by one
    (160, 96, 80, (159, 95)),  # ... the last element, in the partial tile
])
def test_gemm_is_exact_and_the_checksums_locate_a_wrong_element(tmp_path, m, n, k, poison):
    rng = np.random.default_rng(20240607)
    a, b = rng.integers(-2, 3, (m, k)), rng.integers(-2, 3, (n, k))
    _bf16_bits(a).tofile(tmp_path / "a.bin")
    _bf16_bits(b).tofile(tmp_path / "b.bin")
    args = ["gemm", "--m", m, "--n", n, "--k", k, "--seconds", 0, "--a", tmp_path / "a.bin", "--b", tmp_path / "b.bin",
            "--c-out", tmp_path / "c.bin"] + (["--poison", "%d,%d" % poison] if poison else [])
    rc, rec = _run(args)
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    c = np.fromfile(tmp_path / "c.bin", dtype=np.float32).reshape(m, n)
    if poison is None:
        assert (rc, rec["ok"], rec["mismatches"]) == (0, True, []), rec
        assert np.array_equal(c, ref)
    else:
        i, j = poison
        assert (rc, rec["ok"]) == (1, False), rec
        tile = (i // 128) * ((n + 127) // 128) + j // 128
        assert rec["mismatches"] == [{"kind": "element", "i": i, "j": j, "delta": 1, "tile": tile}], rec
        ref[i, j] += 1
        assert np.array_equal(c, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [None, (0, 0x1), (-1, 0x80000000)])
@pytest.mark.parametrize("size", [16 << 20, (16 << 20) + 48])
def test_hbm_sweep_is_clean_and_finds_one_flipped_bit(size, flip):
    mib = repr(size / 2**20)
    if flip is None:
        rc, rec = _run(["hbm", "--mib", mib, "--passes", 3])
        assert (rc, rec["ok"], rec["bytes"], rec["mismatch_count"]) == (0, True, size, 0), rec
        return
    word, mask = flip[0] % (size // 4), flip[1]
    rc, rec = _run(["hbm", "--mib", mib, "--flip", "%d:%#x" % (word, mask)])
    assert (rc, rec["ok"], rec["mismatch_count"]) == (1, False, 1), rec
    (m,) = rec["mismatches"]
    assert (m["offset"], m["xor"], m["expected"] ^ m["got"]) == (4 * word, mask, mask), rec


@pytest.mark.gpu
def test_check_gpu_on_the_device():
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    result = check_gpu(gemm=(256, 256, 128), seconds=0, hbm_mib=16)
    assert result["ok"] and result["error"] is None, result
    assert summarize(result) == "gpu 0: gemm clean; hbm clean"


def test_check_gpu_over_a_fake_binary(tmp_path):
    """A child that reports wrong data, then one that hangs: killed at the timeout, second step not run."""
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    bad = {"check": "gemm", "ok": False, "m": 256, "n": 256, "k": 128, "passes": 1, "mismatch_count": 2,
           "mismatches": [{"kind": "element", "i": 37, "j": 101, "delta": 1, "tile": 0}], "tflops": 1.0}
    clean = {"check": "hbm", "ok": True, "bytes": 16, "passes": 2, "mismatch_count": 0, "mismatches": [], "gbps": 1.0}
    fake, log = tmp_path / "fake_gpu_check", tmp_path / "log"
    script = (f"#!{sys.executable}\nimport sys, time\nopen({str(log)!r}, 'a').write(sys.argv[1] + '\\n')\n"
              "if HANG: time.sleep(60)\n"
              f"print('noise')\nprint({json.dumps(bad)!r} if sys.argv[1] == 'gemm' else {json.dumps(clean)!r})\n"
              "sys.exit(sys.argv[1] == 'gemm')\n")
    fake.write_text(script.replace("HANG", "False"))
    fake.chmod(0o755)

    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake))
    assert not result["ok"] and result["gemm"]["exit"] == 1 and result["hbm"]["ok"], result
    assert result["error"] == "gemm: wrong data" and log.read_text() == "gemm\nhbm\n"
    assert summarize(result) == "gpu 3: gemm mismatch at C[37,101] (+1) in tile 0; hbm clean"

    fake.write_text(script.replace("HANG", "True"))
    log.unlink()
    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, timeout=1.0, binary=str(fake))
    assert not result["ok"] and "gemm: timeout" in result["error"], result
    assert result["hbm"] == {"skipped": True} and log.read_text() == "gemm\n"
    assert "hbm not run" in summarize(result) and "timeout" in summarize(result)
