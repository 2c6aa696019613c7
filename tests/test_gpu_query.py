"""GPU: term lookups and boolean queries on the device-resident index
(ii_lookup / ii_query) against the reference's golden outputs and the oracle,
parsed into {word: [ids]} and combined with Python sets.  No expectation
comes from the library."""
import itertools
import os
import random
import re

import numpy as np
import pytest

import ii_ctypes
from conftest import CASES, PKG, case_arrays
from oracle_py import oracle_index
from test_query_abi import ref_clean

pytestmark = pytest.mark.gpu
LETTERS = "abcdefghijklmnopqrstuvwxyz"


@pytest.fixture(scope="module")
def idx():
    ix = ii_ctypes.Index(0)
    yield ix
    ix.close()


def parse_index(letters):
    """{letter: text of <letter>.txt} -> {word: [printed ids, ascending]}"""
    out = {}
    for text in letters.values():
        for line in text.splitlines():
            if line:
                w, ids = line.split(b":", 1)
                out[w] = [int(x) for x in ids.strip(b"[]").split()]
    return out


_GOLDEN = {}


def golden(case):
    """(text, off, ids, expected letters, {word: ids}) of a golden case, parsed once."""
    if case not in _GOLDEN:
        text, off, ids, expected = case_arrays(case)
        _GOLDEN[case] = (text, off, ids, expected, parse_index(expected))
    return _GOLDEN[case]


def mutations(rng, words, index, n):
    """Seeded near-misses that are not in the vocabulary: a letter appended,
    the last letter dropped, one letter changed."""
    out = []
    for w in rng.sample(words, min(n, len(words))):
        for m in (w + bytes([rng.randrange(97, 123)]), w[:-1],
                  w[:(k := rng.randrange(len(w)))] + bytes([rng.randrange(97, 123)]) + w[k + 1:]):
            if m and m not in index and len(m) <= 299:
                out.append(m)
    return out


def expect(index, terms, op):
    sets = [set(index.get(ref_clean(t), ())) for t in terms]
    if not sets:
        return []
    return sorted(set.intersection(*sets) if op == "and" else set.union(*sets))


def check_queries(ix, index, queries):
    for op in ("and", "or"):
        got = ix.query(queries, op)
        assert len(got) == len(queries)
        for q, g in zip(queries, got):
            assert g.dtype == np.uint32
            assert g.tolist() == expect(index, q, op), (op, q)
        st = ix.query_stats()
        assert st.queries == len(queries) and st.terms == sum(len(q) for q in queries)
        assert st.ids_out == sum(len(g) for g in got)


def check_index(ix, index, seed, nqueries=300, own=None):
    """lookup of every word and of near-misses, then seeded queries of 1-4 terms.
    own(word) (optional): the words this context answers for; the others must read as absent."""
    rng = random.Random(seed)
    words = sorted(index)
    mine = [w for w in words if own is None or own(w)]
    theirs = {w for w in words if own is not None and not own(w)}
    local = {w: index[w] for w in mine}
    assert ix.lookup(mine) == [len(index[w]) for w in mine]
    if theirs:
        other = sorted(theirs)
        assert ix.lookup(other) == [0] * len(other)
    miss = mutations(rng, mine, index, 200) if mine else [b"zzzzqq"]
    assert ix.lookup(miss) == [0] * len(miss)
    if not mine:
        check_queries(ix, local, [[b"zzzzqq"], []])
        return
    # terms by rank of df, so that conjunctions are not all empty; some absent, some repeated
    by_df = sorted(mine, key=lambda w: (-len(index[w]), w))
    pool = sorted(theirs) + miss

    def term():
        r = rng.random()
        if r < 0.08 and pool:
            return rng.choice(pool)
        return by_df[min(len(by_df) - 1, int(rng.paretovariate(0.6)) - 1)] if r < 0.7 else rng.choice(by_df)

    queries = []
    for _ in range(nqueries):
        q = [term() for _ in range(rng.randint(1, 4))]
        if rng.random() < 0.05:
            q.append(q[0])
            q = q[:4]
        queries.append(q)
    check_queries(ix, local, queries)


# ---------------------------------------------------------------- goldens
@pytest.mark.parametrize("case", CASES)
def test_goldens(idx, case):
    text, off, ids, expected, index = golden(case)
    idx.map_host(text, off, ids)
    idx.reduce()
    before = idx.letters()
    assert before == expected
    check_index(idx, index, seed=CASES.index(case))
    assert idx.letters() == expected  # a query leaves the formatted index alone
    p, loff = idx.device_text()
    assert loff[26] == sum(len(v) for v in expected.values())


# ---------------------------------------------------------------- every pair form
def oracle_dict(text, off, ids):
    return parse_index(oracle_index(text, off, ids))


@pytest.mark.parametrize("case", ["config2", "edge"])
def test_after_reduce_local_alone(idx, case):
    # u64 pairs (key << 32 | id0), no formatted text
    text, off, ids, expected, index = golden(case)
    idx.map_host(text, off, ids)
    idx.reduce_local()
    assert idx.stats().pair_bytes == 8
    check_index(idx, index, seed=11)
    idx.reduce()  # ... and the reduce that follows formats the same index
    assert idx.letters() == expected
    check_index(idx, index, seed=12, nqueries=50)


@pytest.mark.parametrize("case", ["config2", "edge"])
def test_lexid_sort_keys(idx, case, monkeypatch):
    monkeypatch.setenv("II_SORT_KEYS", "lexid")
    text, off, ids, expected, index = golden(case)
    idx.map_host(text, off, ids)
    idx.reduce()
    check_index(idx, index, seed=13)
    assert idx.letters() == expected


@pytest.mark.parametrize("case", ["config2", "edge"])
def test_non_consecutive_ids(idx, case):
    text, off, ids, _, _ = golden(case)
    ids2 = [3 * f + 5 for f in ids]
    idx.map_host(text, off, ids2)
    idx.reduce()
    check_index(idx, oracle_dict(text, off, ids2), seed=14)


@pytest.mark.parametrize("case", ["config2", "edge"])
def test_id_above_2_31_keeps_u64_pairs(idx, case):
    text, off, ids, _, _ = golden(case)
    ids2 = list(ids)
    ids2[-1] = (1 << 31) + 7
    idx.map_host(text, off, ids2)
    idx.reduce()
    assert idx.stats().pair_bytes == 8
    exp = oracle_index(text, off, ids2)
    assert idx.letters() == exp
    check_index(idx, parse_index(exp), seed=15)


def test_export_plan_and_reduce_after_a_query(idx):
    # what follows a query works as it would have without it
    text, off, ids, expected, index = golden("config2")
    with ii_ctypes.Index(0) as plain:
        plain.map_host(text, off, ids)
        plain.reduce()
        want = plain.export_plan(3)
    idx.map_host(text, off, ids)
    idx.reduce()
    check_index(idx, index, seed=16, nqueries=50)
    assert idx.export_plan(3) == want  # (maps again: the pairs are u64 now)
    assert idx.stats().pair_bytes == 8
    check_index(idx, index, seed=17, nqueries=50)
    idx.reduce()
    assert idx.letters() == expected
    check_index(idx, index, seed=18, nqueries=50)


# ---------------------------------------------------------------- long words
P12 = b"abcdefghijkl"                       # 12 letters, indexed itself
P12_ALONE = b"qrstuvwxyzab"                  # 12 letters, no longer word shares them
P12_ONLY_LONGER = b"mnopqrstuvwx"            # not indexed; two longer words start with it
W24 = b"zyxwvutsrqponmlkjihgfedc"            # 24 letters
LONG_WORDS = [P12, P12 + b"m", P12 + b"nop", P12_ALONE, P12_ONLY_LONGER + b"aa", P12_ONLY_LONGER + b"bb",
              W24, W24 + b"a", W24 + b"b", b"k" * 299, b"y" * 350, b"hello"]


def long_corpus():
    rng = random.Random(5)
    raw = {P12 + b"nop": b"Abc-defGHIJ.kl9nOp!", b"hello": b"HeLLo,", W24 + b"b": W24.upper() + b"--B;"}
    files = []
    for f in range(23):
        toks = [raw.get(w, w) if rng.random() < 0.5 else w for w in LONG_WORDS if rng.random() < 0.45]
        toks += [b"filler", b"h-e-l-l-o"] if f % 4 == 0 else [b"filler"]
        rng.shuffle(toks)
        files.append(b" ".join(toks) + b"\n")
    # (every word at least once, in the last file, in raw form where it has one)
    files.append(b"\t".join(raw.get(w, w) for w in LONG_WORDS) + b"\n")
    text, off = b"", [0]
    for d in files:
        text += d
        off.append(len(text))
    return text, off, list(range(len(files)))


def test_long_words(idx):
    text, off, ids = long_corpus()
    index = oracle_dict(text, off, ids)
    for w in LONG_WORDS:
        assert w[:299] in index, w[:20]
    assert P12_ONLY_LONGER not in index
    idx.map_host(text, off, ids)
    idx.reduce()
    terms = LONG_WORDS + [
        P12 + b"z",                    # 13 letters, absent; its 12-letter prefix is a word, and longer words share it
        P12 + b"mm", P12 + b"no", P12 + b"nopq", P12 + b"a",
        P12_ALONE + b"c",              # 13 letters, absent; no indexed word is longer than its prefix
        P12_ONLY_LONGER,               # the bare prefix when only longer words exist
        P12_ONLY_LONGER + b"a", P12_ONLY_LONGER + b"ab", P12_ONLY_LONGER + b"bbb",
        W24 + b"c", W24[:23], W24 + b"aa",
        b"k" * 298, b"k" * 300, b"y" * 299, b"y" * 298, b"K-" * 299,
        b"HeLLo,", b"h-e-l-l-o", b"123", b"", b"Abc-defGHIJ.kl9nOp!", b"filler",
    ]
    assert idx.lookup(terms) == [len(index.get(ref_clean(t), ())) for t in terms]
    assert idx.lookup([b"HeLLo,"])[0] > 0 and idx.lookup([b"y" * 350])[0] > 0
    rng = random.Random(6)
    queries = [[a, b] for a, b in itertools.combinations(LONG_WORDS, 2)]
    queries += [[rng.choice(terms) for _ in range(rng.randint(1, 4))] for _ in range(150)]
    queries += [[b"123"], [b"123", b"hello"], [b"hello", b"123"], [b"h-e-l-l-o", b"HeLLo,"]]
    check_queries(idx, index, queries)


# ---------------------------------------------------------------- tile boundaries
def kquery_tile():
    """kQueryTile of csrc/ii_query.h: the driver postings of one work item."""
    src = open(os.path.join(PKG, "csrc", "ii_query.h")).read()
    return int(re.search(r"constexpr uint32_t kQueryTile = (\d+);", src).group(1))


def pairs_and_triples(words):
    return [list(c) for n in (2, 3) for c in itertools.combinations(words, n)]


def test_tile_boundaries_small_tile(idx, monkeypatch):
    monkeypatch.setenv("II_QUERY_TILE", "64")
    n = 64 * 3 + 1
    files = []
    for f in range(n):
        w = [b"all"]
        if f % 2 == 0:
            w.append(b"second")
        if f % 3 == 0:
            w.append(b"third")
        if f == 0:
            w.append(b"first")
        if f == n - 1:
            w.append(b"last")
        for pos, name in ((63, b"atsixthree"), (64, b"atsixfour"), (65, b"atsixfive")):
            if f == pos:
                w.append(name)
        files.append(b" ".join(w) + b"\n")
    text, off = b"".join(files), [0]
    for d in files:
        off.append(off[-1] + len(d))
    ids = list(range(n))
    index = oracle_dict(text, off, ids)
    words = [b"all", b"second", b"third", b"first", b"last", b"atsixthree", b"atsixfour", b"atsixfive"]
    assert sorted(index) == sorted(words)
    for form in ("reduce", "reduce_local"):
        idx.map_host(text, off, ids)
        getattr(idx, form)()
        assert idx.lookup(words) == [len(index[w]) for w in words]
        check_queries(idx, index, pairs_and_triples(words) + [[w] for w in words])


def test_tile_boundaries_default_tile(idx, monkeypatch):
    monkeypatch.delenv("II_QUERY_TILE", raising=False)
    tile = kquery_tile()
    assert tile == 2048  # kQueryTile, csrc/ii_query.h
    n = 2 * tile + 3
    rng = random.Random(9)
    vocab = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]
    files = [b" ".join(rng.sample(vocab, 3)) + b"\n" for _ in range(n)]
    files[0] = b"alpha beta edgefirst\n"
    files[tile - 1] = b"alpha beta tileend\n"
    files[tile] = b"alpha beta tilestart\n"
    files[n - 1] = b"alpha beta edgelast\n"
    text, off = b"".join(files), [0]
    for d in files:
        off.append(off[-1] + len(d))
    ids = list(range(n))
    index = oracle_dict(text, off, ids)
    words = vocab + [b"edgefirst", b"tileend", b"tilestart", b"edgelast"]
    assert max(len(v) for v in index.values()) > tile  # some list spans more than one tile
    idx.map_host(text, off, ids)
    idx.reduce()
    assert idx.lookup(words) == [len(index[w]) for w in words]
    check_queries(idx, index, pairs_and_triples(words))


# ---------------------------------------------------------------- limits and state
def test_limits(idx):
    text, off, ids, expected, index = golden("config2")
    idx.map_host(text, off, ids)
    idx.reduce()
    by_df = sorted(index, key=lambda w: (-len(index[w]), w))
    full = by_df[:ii_ctypes.MAX_QUERY_TERMS]
    assert len(full) == 16
    check_queries(idx, index, [full, full[::-1], [full[0]] * 16, []])
    for op in ("and", "or"):
        with pytest.raises(ii_ctypes.IIError) as e:
            idx.query([full + [by_df[16]]], op)
        assert e.value.code == -1
        with pytest.raises(ii_ctypes.IIError) as e:
            idx.query([[full[0]], full + [full[0]], [full[1]]], op)
        assert e.value.code == -1
        assert idx.query([], op) == []
        assert [g.tolist() for g in idx.query([[], [], []], op)] == [[], [], []]
    with pytest.raises(ii_ctypes.IIError) as e:
        idx.query([[full[0]]], 2)  # unknown op
    assert e.value.code == -1
    assert idx.lookup([]) == []
    # the refused calls left the index as it was
    check_queries(idx, index, [[full[0], full[1]]])
    assert idx.letters() == expected


class DeviceArray:
    """n elements at a device pointer, for torch.as_tensor."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def test_device_result_matches_host_result(idx):
    import torch
    text, off, ids, expected, index = golden("zipf_small")
    idx.map_host(text, off, ids)
    idx.reduce()
    by_df = sorted(index, key=lambda w: (-len(index[w]), w))
    queries = [[by_df[i], by_df[i + 1]] for i in range(40)] + [[], [b"nosuchwordqq"]]
    for op in ("and", "or"):
        assert idx.query(queries, op, to_host=False) is None
        po, pi = idx.query_device()
        exp = [expect(index, q, op) for q in queries]
        n = sum(len(e) for e in exp)
        assert idx.query_stats().ids_out == n
        assert po and pi
        o = torch.as_tensor(DeviceArray(po, len(queries) + 1, "<i8"), device="cuda").cpu().tolist()
        flat = torch.as_tensor(DeviceArray(pi, n, "<i4"), device="cuda").cpu().tolist() if n else []
        assert o[0] == 0 and o[-1] == n
        assert [flat[o[q]:o[q + 1]] for q in range(len(queries))] == exp


def test_state_errors():
    with ii_ctypes.Index(0) as ix:
        for call in (lambda: ix.query([[b"a"]]), lambda: ix.lookup([b"a"]), lambda: ix.query([]),
                     lambda: ix.query_device(), lambda: ix.query_stats()):
            with pytest.raises(ii_ctypes.IIError) as e:
                call()
            assert e.value.code == -5
        text, off, ids, _, index = golden("tiny360")
        ix.map_host(text, off, ids)
        with pytest.raises(ii_ctypes.IIError) as e:
            ix.query([[b"a"]])
        assert e.value.code == -5
        ix.reduce()
        w = sorted(index)[0]
        assert ix.query([[w]])[0].tolist() == index[w]
        ix.map_host(text, off, ids)  # a fresh map: the partial index is gone
        for call in (lambda: ix.query([[w]]), lambda: ix.lookup([w])):
            with pytest.raises(ii_ctypes.IIError) as e:
                call()
            assert e.value.code == -5


@pytest.mark.parametrize("corpus", [(b"", [0], []), (b"12 34 -- \n!!\n", [0, 9, 13], [0, 1])])
def test_empty_index_answers_empty(idx, corpus):
    text, off, ids = corpus
    idx.map_host(text, off, ids)
    idx.reduce()
    assert idx.lookup([b"a", b"hello", b""]) == [0, 0, 0]
    for op in ("and", "or"):
        assert [g.tolist() for g in idx.query([[b"a"], [b"a", b"b"], []], op)] == [[], [], []]
    assert idx.query_stats().ids_out == 0


# ---------------------------------------------------------------- owner after an exchange
def test_owner_after_exchange():
    import ii_dist
    text, off, ids, expected, index = golden("config2")
    G = 2
    n = len(ids)
    sizes = [off[i + 1] - off[i] for i in range(n)]
    order, sb, se = ii_ctypes.partition(sizes, G)
    idxs = []
    try:
        for g in range(G):
            fids = sorted(order[sb[g]:se[g]])
            t, o = bytearray(), [0]
            for f in fids:
                t += text[off[f]:off[f + 1]]
                o.append(len(t))
            ix = ii_ctypes.Index(0)
            idxs.append(ix)
            ix.map_host(bytes(t), o, fids)
        los, his = ii_dist.logical_shards_reduce(idxs, n)
        for g, ix in enumerate(idxs):
            lo, hi = los[g], his[g]
            assert (lo, hi) == ii_ctypes.reducer_letters(g, G)
            check_index(ix, index, seed=20 + g, own=lambda w: lo <= w[0] - 97 < hi)
            got = ix.letters()
            for l in range(26):
                assert got[LETTERS[l]] == (expected[LETTERS[l]] if lo <= l < hi else b"")
    finally:
        for ix in idxs:
            ix.close()


def test_owner_after_import_without_reduce():
    # ii_import alone leaves a partial index that answers queries
    import torch
    text, off, ids, expected, index = golden("edge")
    with ii_ctypes.Index(0) as src, ii_ctypes.Index(0) as own:
        src.map_host(text, off, ids)
        sizes = src.export_plan_ranges([0], [26])
        buf = torch.empty(max(sizes[0], 8), dtype=torch.uint8, device="cuda")
        src.export(1, buf.data_ptr(), [0])
        torch.cuda.synchronize()
        own.import_(1, buf.data_ptr(), [0], len(ids))
        check_index(own, index, seed=31)
        own.reduce()
        assert own.letters() == expected
        check_index(own, index, seed=32, nqueries=50)
