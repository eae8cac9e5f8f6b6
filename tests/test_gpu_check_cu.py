"""``gpu_check cu`` (csrc/health/gpu_check.hip) and ``check_gpu(cu=True)``.

Both sides of the check are exact (LDS words against a hash, accumulators against integer dot
products), so every assertion is an equality.  ``covered == cus`` is also the test of the hardware-ID
decode: dropped bits can never reach ``cus`` distinct CUs and garbage bits overshoot it.
"""
import json
import subprocess
import sys

import pytest


def _run(args):
    from nexus_supervisor_amd._build import binary

    p = subprocess.run([binary("gpu_check"), "cu"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    return p.returncode, json.loads((p.stdout.strip().splitlines() or ["null"])[-1])


@pytest.fixture(scope="module")
def cus():
    return _run(["--k", 16, "--reps", 1, "--passes", 1])[1]["cus"]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [
    ["--k", 16, "--reps", 1, "--passes", 1],  # one instruction per wave: operand and accumulator lane layout
    ["--k", 48],                              # an odd number of steps
    ["--k", 304],                             # the cap: the last operand chunk of every row
    [],                                       # defaults
])
def test_every_cu_and_simd_is_reached_and_clean(args):
    rc, rec = _run(args)
    print(rec)
    assert (rc, rec["ok"], rec["bad"]) == (0, True, []), rec
    assert rec["covered"] == rec["cus"] and rec["simds"] == 4 * rec["cus"] and rec["rounds"] <= 8, rec
    assert rec["lds_bytes"] == 163840 and rec["k"] == (args[1] if args else 304), rec


@pytest.mark.gpu
@pytest.mark.parametrize("last,word,mask", [(False, 0, 0x1), (True, 40959, 0x80000000)])
def test_a_flipped_lds_word_is_found_and_placed(cus, last, word, mask):
    wg = cus - 1 if last else 0
    rc, rec = _run(["--flip", f"{wg}:{word}:{mask}"])
    assert (rc, rec["ok"], len(rec["bad"])) == (1, False, 1), rec
    bad = rec["bad"][0]
    assert bad["wg"] == wg and bad["round"] == 0 and "mfma" not in bad, rec
    lds = bad["lds"]
    assert (lds["count"], lds["offset"], lds["xor"]) == (1, 4 * word, mask) and lds["expected"] ^ lds["got"] == mask, rec


@pytest.mark.gpu
@pytest.mark.parametrize("last,i,j", [(False, 0, 0), (True, 31, 31)])
def test_a_wrong_accumulator_element_is_found_and_placed(cus, last, i, j):
    wg, wave = (cus - 1, 15) if last else (0, 0)
    rc, rec = _run(["--poison", f"{wg}:{wave}:{i},{j}"])
    assert (rc, rec["ok"], len(rec["bad"])) == (1, False, 1), rec
    bad = rec["bad"][0]
    assert bad["wg"] == wg and "lds" not in bad, rec
    simd = bad["mfma"]["simd"]
    assert simd in range(4) and bad["mfma"] == {"count": 1, "simd": simd, "i": i, "j": j, "delta": 1}, rec


@pytest.mark.parametrize("args", [["--k", 24], ["--k", 320], ["--rounds", 0], ["--flip", "0:40960:1"],
                                  ["--poison", "0:0:32,0"], ["--poison", "0:0:0,32"]])
def test_cu_refuses_bad_arguments_before_the_device_is_opened(args):
    from nexus_supervisor_amd._build import binary

    p = subprocess.run([binary("gpu_check"), "cu"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2, p.stderr  # a HIP call that failed would be exit 3


@pytest.mark.gpu
def test_check_gpu_with_cu_on_the_device():
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    result = check_gpu(gemm=(256, 256, 128), seconds=0, hbm_mib=16, cu=True)
    assert result["ok"] and result["error"] is None, result
    assert summarize(result) == "gpu 0: gemm clean; cu clean; hbm clean"


BAD = {"xcc": 3, "se": 1, "sh": 0, "cu": 7, "wg": 99, "round": 0}
LDS = {"count": 1, "offset": 4096, "expected": 6, "got": 7, "xor": 1}
MFMA = {"count": 1, "simd": 2, "i": 5, "j": 17, "delta": 1}


@pytest.mark.parametrize("rec,text", [
    ({"bad_count": 1, "bad": [{**BAD, "lds": LDS}]}, "cu xcc 3 se 1 cu 7: lds 1 bad word at byte 4096 (xor 0x00000001)"),
    ({"bad_count": 3, "bad": [{**BAD, "mfma": MFMA}, BAD, BAD]},
     "cu xcc 3 se 1 cu 7: matrix unit simd 2 wrong at [5,17] (+1) and 2 more"),
    ({"error": "coverage", "covered": 255, "bad": []}, "cu reached 255 of 256 CUs"),
    ("hang", "cu failed"),
])
def test_check_gpu_cu_over_a_fake_binary(tmp_path, rec, text):
    """A binary whose cu child alone reports wrong data, or hangs: then nothing more is started on the device."""
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    hang = rec == "hang"
    full = {"check": "cu", "ok": False, "cus": 256, "covered": 256, "simds": 1024, "rounds": 1, **({} if hang else rec)}
    fake, log = tmp_path / "fake_gpu_check", tmp_path / "log"
    fake.write_text(f"#!{sys.executable}\nimport json, sys, time\nopen({str(log)!r}, 'a').write(sys.argv[1] + '\\n')\n"
                    f"wrong = sys.argv[1] == 'cu'\nif wrong and {hang}: time.sleep(60)\n"
                    f"print({json.dumps(full)!r} if wrong else json.dumps({{'ok': True}}))\nsys.exit(wrong)\n")
    fake.chmod(0o755)

    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake), cu=True, timeout=1.0 if hang else 60)
    assert not result["ok"] and list(result)[2:5] == ["gemm", "cu", "hbm"], result
    if hang:
        assert log.read_text() == "gemm\ncu\n" and result["hbm"] == {"skipped": True}, result
        assert summarize(result) == f"gpu 3: gemm clean; {text}; hbm not run [cu: timeout after 1s (killed)]"
    else:
        assert log.read_text() == "gemm\ncu\nhbm\n" and result["error"] == "cu: wrong data", result
        assert summarize(result) == f"gpu 3: gemm clean; {text}; hbm clean"
