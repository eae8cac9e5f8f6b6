"""``gpu_check gemm --dtype fp64`` (csrc/health/gpu_check.hip) and ``check_gpu(dtypes=(..., "fp64"))``.

Elements are integers of magnitude <= 65535, so a product is below 2^32 and every sum the GEMM or
its checksums form is an integer below 2^52 for K <= 8192: FP64 is exact in any order and each
comparison is ``np.array_equal`` against int64, no tolerance.
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
@pytest.mark.parametrize("m,n,k,poison,top", [
    (16, 16, 4, None, False),        # one instruction: operand and accumulator lane layout
    (128, 128, 32, None, False),     # one full tile, two K steps: wave quadrants, block order within a wave, LDS swizzle
    (128, 128, 100, None, False),    # seven K steps of 16, the last a quarter full: double-buffer reuse, zero-fill past K
    (144, 80, 36, None, False),      # partial tile in M, N under a tile: bounds of both loads and of the checksum stores
    (256, 384, 64, None, False),     # several tiles both ways, not square: tile indices, stripes
    (144, 80, 36, (37, 5), False),   # the detector: one element off by one
    (144, 80, 36, (143, 79), False),  # ... the last element, in the partial tile
    (128, 128, 8192, None, True),  # the cap, every element +65535: the largest checksum the argument allows, < 2^52
])
def test_fp64_gemm_is_exact_and_the_checksums_locate_a_wrong_element(tmp_path, m, n, k, poison, top):
    rng = np.random.default_rng(20250711)
    a, b = (np.full((rows, k), 65535) if top else rng.integers(-65535, 65536, (rows, k)) for rows in (m, n))
    a.astype(np.float64).tofile(tmp_path / "a.bin")
    b.astype(np.float64).tofile(tmp_path / "b.bin")
    p = _run(["gemm", "--dtype", "fp64", "--m", m, "--n", n, "--k", k, "--seconds", 0, "--a", tmp_path / "a.bin",
              "--b", tmp_path / "b.bin", "--c-out", tmp_path / "c.bin"] + (["--poison", "%d,%d" % poison] if poison else []))
    rc, rec = p.returncode, json.loads(p.stdout.strip().splitlines()[-1])
    ref = a.astype(np.int64) @ b.astype(np.int64).T
    c = np.fromfile(tmp_path / "c.bin", dtype=np.float64).reshape(m, n)
    assert rec["dtype"] == "fp64", rec
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


@pytest.mark.parametrize("m,k,bad", [(16, 8196, None), (16, 6, None), (24, 4, None), (16, 4, 65536.0), (16, 4, 0.5)])
def test_fp64_gemm_refuses_what_the_exactness_argument_does_not_cover(tmp_path, m, k, bad):
    """Exit 2 before the device is opened: K over the cap, K and M off their multiples, an element too large, a fraction."""
    args = ["gemm", "--dtype", "fp64", "--m", m, "--n", 16, "--k", k, "--seconds", 0]
    if bad is not None:
        a = np.ones((m, k))
        a[3, 1] = bad
        a.tofile(tmp_path / "a.bin")
        np.ones((16, k)).tofile(tmp_path / "b.bin")
        args += ["--a", tmp_path / "a.bin", "--b", tmp_path / "b.bin"]
    assert _run(args).returncode == 2


@pytest.mark.gpu
def test_check_gpu_with_fp64_on_the_device():
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    result = check_gpu(gemm=(256, 256, 128), seconds=0, hbm_mib=16, dtypes=("bf16", "fp64"))
    assert result["ok"] and result["error"] is None, result
    assert summarize(result) == "gpu 0: gemm clean; gemm fp64 clean; hbm clean"


def test_check_gpu_fp64_over_a_fake_binary(tmp_path):
    """A binary whose fp64 child alone reports wrong data; the default ``dtypes`` starts what it always did."""
    from nexus_supervisor_amd.gpu.health import MX_K_CAP, check_gpu, summarize

    bad = {"check": "gemm", "dtype": "fp64", "ok": False, "m": 256, "n": 256, "k": 128, "passes": 1, "mismatch_count": 2,
           "mismatches": [{"kind": "element", "i": 37, "j": 101, "delta": 1, "tile": 0}], "tflops": 1.0}
    fake, log = tmp_path / "fake_gpu_check", tmp_path / "log"
    fake.write_text(f"#!{sys.executable}\nimport json, sys\n"
                    "what = ' '.join([sys.argv[1]] + sys.argv[2:4] * (sys.argv[2] == '--dtype'))\n"
                    f"open({str(log)!r}, 'a').write(what + '\\n')\n"
                    f"wrong = 'fp64' in what\nprint({json.dumps(bad)!r} if wrong else json.dumps({{'ok': True}}))\n"
                    "sys.exit(wrong)\n")
    fake.chmod(0o755)

    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake), dtypes=("bf16", "mxfp8", "fp64"))
    assert log.read_text() == "gemm\ngemm --dtype mxfp8\ngemm --dtype fp64\nhbm\n"
    assert not result["ok"] and result["gemm_fp64"]["exit"] == 1 and result["error"] == "gemm_fp64: wrong data", result
    assert summarize(result) == ("gpu 3: gemm clean; gemm mxfp8 clean; gemm fp64 mismatch at C[37,101] (+1) in tile 0; "
                                 "hbm clean")
    assert MX_K_CAP == {"mxfp8": 8192, "mxfp4": 2048}

    log.unlink()
    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake))
    assert result["ok"] and log.read_text() == "gemm\nhbm\n" and "gemm_fp64" not in result
