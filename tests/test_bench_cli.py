"""bench.py's command line without a GPU: what a plain run leaves out, what
--full keeps, and the fixed sample --dump-outputs takes of a large text."""
import sys

import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_does_the_timed_steps_only(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    # nothing after the timed loop: no verification, no CPU baseline, no file-reader / end-to-end legs
    assert a.no_verify and a.cpu_baseline == "none" and a.io_bytes == 0


def test_full_keeps_the_legs_and_their_switches(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.full and not a.no_verify and a.cpu_baseline == "quick" and a.io_bytes == 2e9
    a = parse(monkeypatch, "--full", "--no-cpu-baseline", "--io-bytes", "0", "--no-verify", "--dump-outputs", "d")
    assert a.no_verify and a.cpu_baseline == "none" and a.io_bytes == 0 and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        parse(monkeypatch, *argv)


@pytest.mark.parametrize("total", [bench.DUMP_WHOLE + 1, 3 * bench.DUMP_WHOLE + 12345, 5_000_000_000])
def test_sample_blocks_are_fixed_and_in_bounds(total):
    s = bench.sample_starts(total)
    assert s == bench.sample_starts(total)  # seeded: the same blocks for the same text size
    assert len(s) == bench.DUMP_BLOCKS and s == sorted(s)
    assert s[0] == 0 and s[-1] == total - bench.DUMP_BLOCK
    assert all(0 <= x <= total - bench.DUMP_BLOCK for x in s)
    # the float32 sample and the three small arrays stay far below 64 MB
    assert 4 * bench.DUMP_BLOCKS * bench.DUMP_BLOCK + 8 * (27 + 26 + 4) < 64_000_000


@pytest.mark.parametrize("total", [1, 4096, bench.DUMP_WHOLE])
def test_small_text_is_dumped_whole(total):
    assert bench.sample_starts(total) == [0]
    assert 4 * bench.DUMP_WHOLE < 64_000_000
