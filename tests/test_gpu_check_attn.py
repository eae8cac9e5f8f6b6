"""``gpu_check attn`` (csrc/health/gpu_check.hip) and ``check_gpu(attn=True)``.

Scores are integers of magnitude <= 6 and the softmax is base 2, so every probability is a power of
two and every sum a multiple of 2^-12 that float64 (and, within the caps, fp32) holds exactly: each
comparison is ``np.array_equal`` against plain numpy, no tolerance.
"""
import json
import subprocess
import sys

import numpy as np
import pytest


def _run(args):
    from nexus_supervisor_amd._build import binary

    return subprocess.run([binary("gpu_check"), "attn"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


@pytest.mark.gpu
@pytest.mark.parametrize("h,s,d,causal,poison,crafted", [
    (1, 64, 64, False, None, False),          # one key tile: lane layouts, the permuted-key PV step, the l <-> l + 32 exchange
    (1, 128, 128, False, None, False),        # d = 128, two key tiles: double-buffer reuse, one rescale
    (2, 192, 64, False, None, False),         # a partial query block and a second head: row guards, head strides
    (1, 192, 64, True, None, False),          # causal: a skipped tile, the masked diagonal tile, row 0 with a single key
    (1, 2048, 64, False, None, True),         # the cap: O' reaches 2 (1984 + 64 * 2^-12), every row rescales by 2^-12
    (2, 192, 64, False, (1, 191, 63), False),  # the detector: the last element, one unit of 2^-12 off
    (2, 192, 64, False, (0, 0, 0), False),     # ... and the first
])
def test_attention_is_exact_and_a_wrong_element_is_named(tmp_path, h, s, d, causal, poison, crafted):
    rng = np.random.default_rng(20261126)
    k, v, q = rng.integers(-2, 3, (h, s, d)), rng.integers(-2, 3, (h, s, d)), np.zeros((h, s, d), np.int64)
    for row in q.reshape(-1, d):  # three +-1 per row, summed where they collide: sum |q| <= 3
        np.add.at(row, rng.integers(0, d, 3), rng.choice([-1, 1], 3))
    if crafted:  # scores -6 in the first key tile and +6 after it, V all 2
        q[:], k[:], v[:] = 0, 0, 2
        q[:, :, 5], k[:, :64, 5], k[:, 64:, 5] = 3, -2, 2
    for name, x in (("q", q), ("k", k), ("v", v)):  # raw bf16: the upper half of the float32
        (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tofile(tmp_path / name)
    p = _run(["--heads", h, "--seq", s, "--d", d, "--seconds", 0, "--q", tmp_path / "q", "--k", tmp_path / "k", "--v", tmp_path / "v",
              "--o-out", tmp_path / "o.bin", "--ml-out", tmp_path / "ml.bin"] + (["--causal"] if causal else [])
             + (["--poison", "%d,%d,%d" % poison] if poison else []))
    rc, rec = p.returncode, json.loads(p.stdout.strip().splitlines()[-1])
    sc = (q @ k.transpose(0, 2, 1)).astype(np.float64)
    if causal:
        sc[:, np.triu_indices(s, 1)[0], np.triu_indices(s, 1)[1]] = -np.inf
    m = sc.max(axis=2)
    pr = 2.0 ** (sc - m[:, :, None])
    ref, ml = pr @ v, np.stack([m, pr.sum(axis=2)], axis=2)
    if crafted:
        assert ref.max() == 2 * (1984 + 64 * 2.0 ** -12)
    o = np.fromfile(tmp_path / "o.bin", dtype=np.float32).reshape(h, s, d)
    assert np.array_equal(np.fromfile(tmp_path / "ml.bin", dtype=np.float32).reshape(h, s, 2), ml)
    assert (rec["check"], rec["heads"], rec["seq"], rec["d"], rec["causal"]) == ("attn", h, s, d, causal), rec
    if poison is None:
        assert (rc, rec["ok"], rec["mismatches"]) == (0, True, []), rec
    else:
        assert (rc, rec["ok"]) == (1, False), rec
        assert rec["mismatches"] == [{"kind": "o", "head": poison[0], "i": poison[1], "c": poison[2], "delta": 1}], rec
        ref[poison] += 2.0 ** -12
    assert np.array_equal(o, ref)


@pytest.mark.parametrize("s,d,short,q_sum,k_max", [
    (96, 64, False, 0, 0), (2112, 64, False, 0, 0), (64, 32, False, 0, 0),  # S off its multiple, S over the cap, d
    (64, 64, True, 0, 0), (64, 64, False, 4, 0), (64, 64, False, 0, 3),     # a --q file one element short, a Q row of 4, a K of 3
])
def test_attention_refuses_what_the_exactness_argument_does_not_cover(tmp_path, s, d, short, q_sum, k_max):
    """Exit 2 before the device is opened."""
    args = ["--heads", 1, "--seq", s, "--d", d, "--seconds", 0]
    if short or q_sum or k_max:
        q, k = np.zeros(s * d - short, np.float32), np.zeros(s * d, np.float32)
        q[:2], k[0] = q_sum / 2, k_max
        for name, x in (("q", q), ("k", k), ("v", np.zeros(s * d, np.float32))):
            (x.view(np.uint32) >> 16).astype(np.uint16).tofile(tmp_path / name)
        args += ["--q", tmp_path / "q", "--k", tmp_path / "k", "--v", tmp_path / "v"]
    p = _run(args)
    assert p.returncode == 2 and "(attn)" in p.stderr.splitlines()[0], p.stderr


@pytest.mark.gpu
def test_check_gpu_with_attention_on_the_device():
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    result = check_gpu(gemm=(256, 256, 128), seconds=0, hbm_mib=16, attn=True)
    assert result["ok"] and result["error"] is None, result
    assert summarize(result) == "gpu 0: gemm clean; attn clean; hbm clean"


def test_check_gpu_attention_over_a_fake_binary(tmp_path):
    """A binary whose attn child alone reports wrong data; with ``attn`` left alone nothing new is started."""
    from nexus_supervisor_amd.gpu.health import check_gpu, summarize

    bad = {"check": "attn", "ok": False, "heads": 64, "seq": 2048, "d": 128, "causal": False, "passes": 1, "mismatch_count": 3,
           "mismatches": [{"kind": "o", "head": 3, "i": 37, "c": 5, "delta": 1}], "tflops": 1.0}
    fake, log = tmp_path / "fake_gpu_check", tmp_path / "log"
    fake.write_text(f"#!{sys.executable}\nimport json, sys\n"
                    f"open({str(log)!r}, 'a').write(sys.argv[1] + '\\n')\n"
                    f"wrong = sys.argv[1] == 'attn'\nprint({json.dumps(bad)!r} if wrong else json.dumps({{'ok': True}}))\n"
                    "sys.exit(wrong)\n")
    fake.chmod(0o755)

    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake), cu=True, attn=True)
    assert log.read_text() == "gemm\nattn\ncu\nhbm\n"
    assert not result["ok"] and result["attn"]["exit"] == 1 and result["error"] == "attn: wrong data", result
    assert summarize(result) == "gpu 3: gemm clean; attn mismatch at head 3 O[37,5] (+1 x 2^-12) and 2 more; cu clean; hbm clean"
    result["attn"]["mismatches"][0].update(kind="l")
    assert "attn mismatch at head 3 l[37] (+1 x 2^-12)" in summarize(result)

    log.unlink()
    result = check_gpu(3, gemm=(256, 256, 128), seconds=0, hbm_mib=16, binary=str(fake))
    assert result["ok"] and log.read_text() == "gemm\nhbm\n" and "attn" not in result
