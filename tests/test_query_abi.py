"""CPU: the query entry points of include/ii.h exist, ii_clean_term restates
the reference's cleaning loop (main.c:105-111), and the argument checks that
need no device."""
import ctypes
import random

import pytest

import ii_ctypes
from conftest import CASES, load_case

C_WHITESPACE = b" \t\n\v\f\r"


def ref_clean(raw):
    """main.c:102-111 for one token: fscanf("%s") ends it at whitespace, the
    loop at a NUL or at MAX_WORD - 1 kept letters."""
    out = bytearray()
    for ch in raw:
        if ch == 0 or ch in C_WHITESPACE or len(out) >= 299:
            break
        if 65 <= ch <= 90:
            out.append(ch + 32)
        elif 97 <= ch <= 122:
            out.append(ch)
    return bytes(out)


FIXED = [b"Hello,", b"h-E-l.L0o", b"123", b"", b"a" * 299, b"b" * 300, b"Cd" * 200, b"ab\0cd", b"ab cd",
         b"\x80 \xc3\xa9 \xff", b"\x80\xc3\xa9\xff", b"x\ty", b"\nq", b"Z"]


@pytest.mark.parametrize("raw", FIXED, ids=[repr(r[:12]) + str(len(r)) for r in FIXED])
def test_clean_term_fixed(raw):
    assert ii_ctypes.clean_term(raw) == ref_clean(raw)


def test_clean_term_lengths():
    assert len(ii_ctypes.clean_term(b"a" * 299)) == 299
    assert len(ii_ctypes.clean_term(b"a" * 300)) == 299
    assert len(ii_ctypes.clean_term(b"a" * 400)) == 299
    assert ii_ctypes.clean_term(b"Hello,") == b"hello"
    assert ii_ctypes.clean_term(b"123") == b""


def test_clean_term_writes_terminator_and_length():
    L = ii_ctypes.lib()
    out = ctypes.create_string_buffer(b"\xaa" * 300, 300)
    n = L.ii_clean_term(b"Ab-c\0zz", 7, out)
    assert n == 3 and out.raw[:4] == b"abc\0"
    n = L.ii_clean_term(b"q" * 400, 400, out)
    assert n == 299 and out.raw[299] == 0
    n = L.ii_clean_term(b"abcdef", 2, out)  # reading stops at n
    assert n == 2 and out.raw[:3] == b"ab\0"


def test_clean_term_random():
    rng = random.Random(20260)
    alphabet = bytes(range(256)) + b"abcXYZ  \t\n--''" * 8  # every byte value, biased to letters and separators
    for _ in range(2000):
        raw = bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 3, 8, 20, 40, 350])))
        assert ii_ctypes.clean_term(raw) == ref_clean(raw), raw


@pytest.mark.parametrize("case", CASES)
def test_clean_term_yields_the_golden_vocabulary(case):
    _, files, expected = load_case(case)
    words = set()
    for data in files.values():
        for tok in data.split():  # bytes.split(): the C locale's whitespace
            w = ii_ctypes.clean_term(tok)
            if w:
                words.add(w)
    golden = set()
    for text in expected.values():
        golden.update(line.split(b":", 1)[0] for line in text.splitlines() if line)
    assert words == golden


def test_null_context_is_an_argument_error():
    L = ii_ctypes.lib()
    off = (ctypes.c_uint32 * 2)(0, 1)
    df = (ctypes.c_uint32 * 1)()
    assert L.ii_lookup(None, b"a", off, 1, df) == -1
    first = (ctypes.c_uint32 * 2)(0, 1)
    roff = ctypes.POINTER(ctypes.c_uint64)()
    rids = ctypes.POINTER(ctypes.c_uint32)()
    assert L.ii_query(None, b"a", off, first, 1, 0, ctypes.byref(roff), ctypes.byref(rids)) == -1
    assert L.ii_query(None, None, None, None, 0, 0, None, None) == -1
    po, pi = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.ii_query_device(None, ctypes.byref(po), ctypes.byref(pi)) == -1
    assert L.ii_get_query_stats(None, None) == -1


def test_binding_constants_match_the_header():
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "ii.h")).read()
    assert int(re.search(r"#define II_MAX_QUERY_TERMS (\d+)", src).group(1)) == ii_ctypes.MAX_QUERY_TERMS
    assert int(re.search(r"#define II_MAX_WORD (\d+)", src).group(1)) == ii_ctypes.MAX_WORD
    assert re.search(r"II_Q_AND = 0, II_Q_OR = 1", src)
    assert (ii_ctypes.Q_AND, ii_ctypes.Q_OR) == (0, 1)
    # ii_query_stats: three u32, padding, two u64, three doubles
    assert ctypes.sizeof(ii_ctypes.QueryStats) == 56
