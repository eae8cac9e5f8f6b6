"""``gpu_check gemm --dtype mxfp8|mxfp4`` (csrc/health/gpu_check.hip) and ``check_gpu(dtypes=...)``.

Elements are small integers (mxfp8) or halves (mxfp4) and scales are x1 or x2, so every sum the
GEMM forms is a multiple of 1/4 below 2^24 quarter-units and fp32 is exact: each comparison is
``np.array_equal`` against float64, no tolerance.
"""
import json
import subprocess
import sys

import numpy as np
import pytest

# element code -> value: the E4M3 bytes of -2 .. 2, the E2M1 codes of 0 .. 2 in halves with sign in bit 3
TABLES = {"mxfp8": {0x00: 0.0, 0x38: 1.0, 0x40: 2.0, 0xB8: -1.0, 0xC0: -2.0},
          "mxfp4": {0: 0.0, 1: 0.5, 2: 1.0, 3: 1.5, 4: 2.0, 9: -0.5, 10: -1.0, 11: -1.5, 12: -2.0}}


def _run(args):
    from nexus_supervisor_amd._build import binary

    p = subprocess.run([binary("gpu_check")] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,poison", [
    (32, 32, 64, None),      # one instruction: operand byte/nibble order, scale lane/byte/opsel, accumulator layout
    (128, 128, 256, None),   # one full tile, two fp8 K steps, one fp4: wave quadrants, swizzle, scale reuse in a step
    (128, 128, 640, None),   # five fp8 steps; three fp4 steps, the last half full: double buffer, scale fill past K
    (160, 96, 192, None),    # partial tile in M, N under a tile, short last step: zero-fill, bounds of both loads
    (256, 384, 512, None),   # several tiles both ways, not square: tile indices, stripes, scale row stride
    (160, 96, 192, (37, 5)),  # the detector: one element off by one
    (160, 96, 192, (159, 95)),  # ... the last element, in the partial tile
])
@pytest.mark.parametrize("dtype", ["mxfp8", "mxfp4"])
def test_mx_gemm_is_exact_and_the_checksums_locate_a_wrong_element(tmp_path, dtype, m, n, k, poison):
    rng = np.random.default_rng(20250211)
    codes = np.array(sorted(TABLES[dtype]), dtype=np.uint8)
    values = np.zeros(256)
    values[codes] = [TABLES[dtype][c] for c in codes]
    args = ["gemm", "--dtype", dtype, "--m", m, "--n", n, "--k", k, "--seconds", 0, "--c-out", tmp_path / "c.bin"]
    ops = []
    for name, rows in (("a", m), ("b", n)):
        x, s = rng.choice(codes, (rows, k)), rng.integers(127, 129, (rows, k // 32), dtype=np.uint8)
        (x if dtype == "mxfp8" else x[:, 0::2] | (x[:, 1::2] << 4)).tofile(tmp_path / f"{name}.bin")
        s.tofile(tmp_path / f"s{name}.bin")
        args += [f"--{name}", tmp_path / f"{name}.bin", f"--s{name}", tmp_path / f"s{name}.bin"]
        ops.append(values[x] * np.repeat(2.0 ** (s.astype(np.float64) - 127), 32, axis=1))
    rc, rec = _run(args + (["--poison", "%d,%d" % poison] if poison else []))
    ref = ops[0] @ ops[1].T
    c = np.fromfile(tmp_path / "c.bin", dtype=np.float32).reshape(m, n)
    assert rec["dtype"] == dtype, rec
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
def test_check_gpu_all_formats_on_the_device():
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    result = check_gpu(gemm=(256, 256, 128), seconds=0, hbm_mib=16, dtypes=("bf16", "mxfp8", "mxfp4"))
    assert result["ok"] and result["error"] is None, result
    assert summarize(result) == "gpu 0: gemm clean; gemm mxfp8 clean; gemm mxfp4 clean; hbm clean"


def test_check_gpu_dtypes_over_a_fake_binary(tmp_path):
    """A binary whose mxfp4 child alone reports wrong data; the default ``dtypes`` starts what it always did."""
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    bad = {"check": "gemm", "dtype": "mxfp4", "ok": False, "m": 256, "n": 256, "k": 128, "passes": 1, "mismatch_count": 2,
           "mismatches": [{"kind": "element", "i": 37, "j": 101, "delta": 1, "tile": 0}], "tflops": 1.0}
    fake, log = tmp_path / "fake_gpu_check", tmp_path / "log"
    fake.write_text(f"#!{sys.executable}\nimport json, sys\n"
                    "what = ' '.join([sys.argv[1]] + sys.argv[2:4] * (sys.argv[2] == '--dtype'))\n"
                    f"open({str(log)!r}, 'a').write(what + '\\n')\n"
                    f"wrong = 'mxfp4' in what\nprint({json.dumps(bad)!r} if wrong else json.dumps({{'ok': True}}))\n"
                    "sys.exit(wrong)\n")
    fake.chmod(0o755)

    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake), dtypes=("bf16", "mxfp8", "mxfp4"))
    assert log.read_text() == "gemm\ngemm --dtype mxfp8\ngemm --dtype mxfp4\nhbm\n"
    assert not result["ok"] and result["gemm_mxfp4"]["exit"] == 1 and result["error"] == "gemm_mxfp4: wrong data", result
    assert result["gemm"]["ok"] and result["gemm_mxfp8"]["ok"] and result["hbm"]["ok"], result
    assert summarize(result) == ("gpu 3: gemm clean; gemm mxfp8 clean; gemm mxfp4 mismatch at C[37,101] (+1) in tile 0; "
                                 "hbm clean")

    log.unlink()
    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake))
    assert result["ok"] and log.read_text() == "gemm\nhbm\n" and "gemm_mxfp4" not in result
    assert summarize(result) == "gpu 3: gemm clean; hbm clean"
