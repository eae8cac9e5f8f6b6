"""``gpu_check gemm --dtype int8`` (csrc/health/gpu_check.hip) and ``check_gpu(dtypes=(..., "int8"))``.

int8 x int8 products accumulated in int32 are exact for any data while |C| <= 2^14 * K <= 2^30, so
the inputs are random over all 256 byte values and each comparison is ``np.array_equal`` against
int64, no tolerance.
"""
import json
import subprocess
import sys

import numpy as np
import pytest


def _run(args):
    from nexus_supervisor_amd._build import binary

    return subprocess.run([binary("gpu_check")] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,poison,low", [
    (32, 32, 32, None, False),         # one instruction: operand and accumulator lane layout, on random bytes
    (128, 256, 64, None, False),       # one full workgroup tile, one stage: wave blocks, 2x4 block order, LDS swizzle
    (128, 256, 160, None, False),      # three stages, the last half full: double-buffer reuse, zero-fill past K
    (160, 288, 96, None, False),       # partial tile in M, one-and-a-bit in N: load and store bounds, wn stripe mapping
    (256, 768, 64, None, False),       # several workgroup tiles both ways: tile indices, stripe numbering
    (160, 288, 96, (37, 5), False),    # the detector: one element off by one
    (160, 288, 96, (159, 287), False),  # ... the last element, in the partial tile and a workgroup's second column stripe
    (128, 32, 65536, None, True),      # the cap, every byte -128: elements 2^30, checksums 2^37, the largest allowed
])
def test_int8_gemm_is_exact_and_the_checksums_locate_a_wrong_element(tmp_path, m, n, k, poison, low):
    rng = np.random.default_rng(20251126)
    a, b = (np.full((rows, k), -128, np.int8) if low else rng.integers(-128, 128, (rows, k), np.int8) for rows in (m, n))
    a.tofile(tmp_path / "a.bin")
    b.tofile(tmp_path / "b.bin")
    p = _run(["gemm", "--dtype", "int8", "--m", m, "--n", n, "--k", k, "--seconds", 0, "--a", tmp_path / "a.bin",
              "--b", tmp_path / "b.bin", "--c-out", tmp_path / "c.bin"] + (["--poison", "%d,%d" % poison] if poison else []))
    rc, rec = p.returncode, json.loads(p.stdout.strip().splitlines()[-1])
    ref = a.astype(np.int64) @ b.astype(np.int64).T
    c = np.fromfile(tmp_path / "c.bin", dtype=np.int32).reshape(m, n)
    assert rec["dtype"] == "int8", rec
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


@pytest.mark.parametrize("m,k,short", [(32, 65568, False), (32, 48, False), (40, 32, False), (32, 32, True)])
def test_int8_gemm_refuses_what_the_exactness_argument_does_not_cover(tmp_path, m, k, short):
    """Exit 2 before the device is opened: K over the cap, K and M off their multiples, an --a file one byte short."""
    args = ["gemm", "--dtype", "int8", "--m", m, "--n", 32, "--k", k, "--seconds", 0]
    if short:
        np.zeros(m * k - 1, np.int8).tofile(tmp_path / "a.bin")
        np.zeros(32 * k, np.int8).tofile(tmp_path / "b.bin")
        args += ["--a", tmp_path / "a.bin", "--b", tmp_path / "b.bin"]
    p = _run(args)
    assert p.returncode == 2 and "(int8)" in p.stderr.splitlines()[0], p.stderr


@pytest.mark.gpu
def test_check_gpu_with_int8_on_the_device():
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    result = check_gpu(gemm=(256, 256, 128), seconds=0, hbm_mib=16, dtypes=("bf16", "int8"))
    assert result["ok"] and result["error"] is None, result
    assert summarize(result) == "gpu 0: gemm clean; gemm int8 clean; hbm clean"


def test_check_gpu_int8_over_a_fake_binary(tmp_path):
    """A binary whose int8 child alone reports wrong data; the default ``dtypes`` starts what it always did."""
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    bad = {"check": "gemm", "dtype": "int8", "ok": False, "m": 256, "n": 256, "k": 128, "passes": 1, "mismatch_count": 2,
           "mismatches": [{"kind": "element", "i": 37, "j": 101, "delta": 1, "tile": 0}], "tflops": 1.0}
    fake, log = tmp_path / "fake_gpu_check", tmp_path / "log"
    fake.write_text(f"#!{sys.executable}\nimport json, sys\n"
                    "what = ' '.join([sys.argv[1]] + sys.argv[2:4] * (sys.argv[2] == '--dtype'))\n"
                    f"open({str(log)!r}, 'a').write(what + '\\n')\n"
                    f"wrong = 'int8' in what\nprint({json.dumps(bad)!r} if wrong else json.dumps({{'ok': True}}))\n"
                    "sys.exit(wrong)\n")
    fake.chmod(0o755)

    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake), dtypes=("bf16", "fp64", "int8"))
    assert log.read_text() == "gemm\ngemm --dtype fp64\ngemm --dtype int8\nhbm\n"
    assert not result["ok"] and result["gemm_int8"]["exit"] == 1 and result["error"] == "gemm_int8: wrong data", result
    assert summarize(result) == ("gpu 3: gemm clean; gemm fp64 clean; gemm int8 mismatch at C[37,101] (+1) in tile 0; "
                                 "hbm clean")

    log.unlink()
    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake))
    assert result["ok"] and log.read_text() == "gemm\nhbm\n" and "gemm_int8" not in result
