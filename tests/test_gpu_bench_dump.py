"""GPU: a plain bench.py run with --dump-outputs — the arrays it writes are
the index the timed path left in device memory (compared byte for byte with
the oracle's index of the same corpus), and the line of a plain run carries
the headline figures and none of the --full legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ii_ctypes
from conftest import REPO
from oracle_py import oracle_index

pytestmark = pytest.mark.gpu
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def test_plain_run_dumps_the_index_of_the_last_timed_step(tmp_path):
    # small enough for the whole text to be dumped (< 8 MiB), large enough for several 32 KiB chunks per file
    nb, nf, vocab, seed = 6_000_000, 37, 30_000, 11
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bytes", str(nb), "--files", str(nf), "--vocab", str(vocab), "--seed", str(seed),
                        "--dump-outputs", out], cwd=REPO, capture_output=True, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = json.loads([x for x in r.stdout.decode().splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert abs(line["value"] - nb / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * line["value"]
    # a plain run runs none of the legs behind --full
    assert line["verified"] is None and line["cpu_baseline"] is None and line["io"] is None and line["e2e"] is None

    text, off = ii_ctypes.zipf_corpus(nb, nf, vocab, seed, threads=8)
    exp = oracle_index(text, off, list(range(nf)), threads=8)
    whole = b"".join(exp[l] for l in LETTERS)
    assert sorted(os.listdir(out)) == ["counts.npy", "letter_byte_sums.npy", "letter_offsets.npy", "text_sample.npy"]
    arr = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    ends = np.cumsum([0] + [len(exp[l]) for l in LETTERS])
    assert arr["letter_offsets"].tolist() == ends.tolist()
    sums = [float(np.frombuffer(exp[l], np.uint8).sum(dtype=np.int64)) for l in LETTERS]
    assert arr["letter_byte_sums"].tolist() == sums
    assert len(whole) <= 8 << 20 and arr["text_sample"].astype(np.uint8).tobytes() == whole
    assert arr["counts"][1] == whole.count(b"\n") and arr["counts"][3] == len(whole)
    assert arr["counts"].tolist() == [line["counts"][k] for k in ("tokens", "words", "pairs", "out_bytes")]
