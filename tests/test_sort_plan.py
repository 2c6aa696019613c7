"""CPU: the token sort's plan (csrc/ii_sortplan.h plan_token_sort) through its
host-only driver (tools/sortplan_check.cpp, built with ASan + UBSan).  The
expected values are worked out by hand from the rules ("The token
sort's plan") and the shapes DESIGN records, not from the code:
  m = max(7, W + F - 32, II_PACKED_M), packable iff m <= 11 and 2 <= W - m <= 16;
  the record set iff nfiles > 0 and T < 16384 nfiles, unless II_S0_DEDUP forces one;
  the first pass writes id0s iff the ids are not affine, the record set dedups,
  II_S0_FMAP allows it (unset: from 65536 files) and the key packs with the id0s' bits.
"""
import os
import subprocess

import pytest

from conftest import PKG

# (name, "T nfiles id_bound affine W keys [knobs]", (m, F, wide, hashd, id source))
CASES = [
    # config3: 72 files of 1.4e5 tokens each, ids 0..71
    ("config3-like", "1600000000 72 72 1 21 wid", (7, 7, 0, 0, "Affine")),
    # configs[4] rank 7: bitlen(439992) = 19, 23 + 19 - 32 = 10; 1.7e9 < 16384 * 439993 = 7.2e9
    ("rank7, K3 gathers", "1700000000 439993 1000000 0 23 wid II_S0_FMAP=0", (10, 19, 1, 1, "GatherInK3")),
    # bitlen(999999) = 20, 23 + 20 - 32 = 11, L = 12
    ("rank7, knob unset", "1700000000 439993 1000000 0 23 wid", (11, 20, 1, 1, "MappedInSort0")),
    # 21 + 20 - 32 = 9, L = 12; 4e6 < 16384 * 9000
    ("forced map", "4000000 9000 1000000 0 21 wid II_S0_FMAP=1", (9, 20, 1, 1, "MappedInSort0")),
    # bitlen(8999) = 14, 21 + 14 - 32 = 3 -> 7, L = 14
    ("map off", "4000000 9000 1000000 0 21 wid II_S0_FMAP=0", (7, 14, 0, 1, "GatherInK3")),
    ("9000 files, knob unset", "4000000 9000 1000000 0 21 wid", (7, 14, 0, 1, "GatherInK3")),
    # bitlen(2^31 - 1) = 31, 21 + 31 - 32 = 20 > 11: the id map is refused, the indices stay
    ("id map refused", "4000000 9000 2147483648 0 21 wid II_S0_FMAP=1", (7, 14, 0, 1, "GatherInK3")),
    ("bitmap forced, map asked", "4000000 9000 1000000 0 21 wid II_S0_DEDUP=bitmap II_S0_FMAP=1",
     (7, 14, 0, 0, "GatherInK3")),
    # bitlen(1999999) = 21, 23 + 21 - 32 = 12 > 11
    ("key too wide", "40000000000 2000000 2000000 1 23 wid", (0, 21, 0, 0, "Affine")),
    # m = 7 leaves L = 1 < 2
    ("too few low bits", "1000000 2 2 1 8 lexid", (0, 1, 0, 0, "Affine")),
    # m = 7 leaves L = 17 > 16
    ("too many low bits", "1000000000 100 100 1 24 wid", (0, 7, 0, 0, "Affine")),
    ("II_PACKED_M=9", "1000000000 1000 1000 1 21 wid II_PACKED_M=9", (9, 10, 1, 0, "Affine")),
    ("II_PACKED_M=11", "1000000000 1000 1000 1 21 wid II_PACKED_M=11", (11, 10, 1, 0, "Affine")),
    # L = 21 - 12 = 9 would do, but m > 11
    ("II_PACKED_M=12", "1000000000 1000 1000 1 21 wid II_PACKED_M=12", (0, 10, 0, 0, "Affine")),
    ("II_PACKED_SORT=0", "1600000000 72 72 1 21 wid II_PACKED_SORT=0", (0, 7, 0, 0, "Affine")),
    # the u64 form has no record set and maps no ids, whatever the knobs ask
    ("u64 form, set and map asked", "4000000 9000 1000000 0 21 wid II_PACKED_SORT=0 II_S0_DEDUP=set II_S0_FMAP=1",
     (0, 14, 0, 0, "GatherInK3")),
    # 7e6 > 16384 * 40: the bitmap by size; bitlen(39) = 6
    ("40 files by size", "7000000 40 40 1 21 wid", (7, 6, 0, 0, "Affine")),
    ("II_S0_DEDUP=set", "7000000 40 40 1 21 wid II_S0_DEDUP=set", (7, 6, 0, 1, "Affine")),
    # 600 files of 5e5 tokens: the record set by itself; ids sampled from [0, 10^6) and the map forced
    ("600 files", "500000 600 1000000 0 17 wid", (7, 10, 0, 1, "GatherInK3")),
    ("600 files, map", "500000 600 1000000 0 17 wid II_S0_FMAP=1", (7, 20, 0, 1, "MappedInSort0")),
    ("600 files, map, m = 11", "500000 600 1000000 0 17 wid II_S0_FMAP=1 II_PACKED_M=11",
     (11, 20, 1, 1, "MappedInSort0")),
    ("nfiles=0", "1000 0 0 1 10 wid", (7, 1, 0, 0, "Affine")),
]


@pytest.fixture(scope="module")
def planned():
    subprocess.run(["make", "-C", PKG, "sortplan_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([os.path.join(PKG, "sortplan_check")], input="".join(c[1] + "\n" for c in CASES).encode(),
                       capture_output=True, env=env, timeout=60)
    err = r.stderr.decode(errors="replace")
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert marker not in err, err[-3000:]
    assert r.returncode == 0, err
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(CASES), lines
    return dict(zip((c[0] for c in CASES), lines))


@pytest.mark.parametrize("name,line,want", CASES, ids=[c[0] for c in CASES])
def test_plan(planned, name, line, want):
    assert planned[name] == "%d %d %d %d %s" % want, line
