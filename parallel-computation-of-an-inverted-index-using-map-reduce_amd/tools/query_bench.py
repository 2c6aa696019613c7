#!/usr/bin/env python3
"""Throughput of boolean term queries on the device-resident index (ii_query).

Indexes a Zipf corpus (zipf_corpus, 1 GB by default), draws two- and three-term
AND queries and OR queries by Zipf rank from the indexed vocabulary, runs them
on the GPU and reports queries/s, postings read/s and ii_query_stats.  The
same queries are timed on the host with numpy.intersect1d / union1d over
posting arrays parsed from the letter texts (the CPU baseline), and a 1 %
sample of the GPU results is checked against that baseline before anything is
printed.  One JSON line on stdout.  Not part of bench.py.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(PKG, "bindings"))
import ii_ctypes  # noqa: E402


def vocabulary(letters):
    """-> (words, df, spans): every indexed word, its df and the (letter,
    begin, end) of its id list inside the letter's text."""
    words, df, spans = [], [], []
    for l, text in letters.items():
        pos = 0
        for line in text.split(b"\n"):
            if line:
                k = line.index(b":")
                words.append(line[:k])
                df.append(line.count(b" ", k) + 1)
                spans.append((l, pos + k + 2, pos + len(line) - 1))
            pos += len(line) + 1
    return words, np.asarray(df, dtype=np.int64), spans


def draw(rng, order, n, lo, hi):
    """n queries of lo..hi terms; a term is the word of Zipf rank r (by df), P(r) ~ 1 / r."""
    V = len(order)
    out = []
    sizes = rng.integers(lo, hi + 1, size=n)
    ranks = np.minimum(V - 1, np.floor(V ** rng.random(int(sizes.sum()))).astype(np.int64) - 1)
    k = 0
    for s in sizes:
        out.append([int(order[r]) for r in ranks[k:k + s]])
        k += s
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--files", type=int, default=10_000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--and-queries", type=int, default=100_000)
    ap.add_argument("--or-queries", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=float, default=0.01, help="share of the GPU results checked against the baseline")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    text, off = ii_ctypes.zipf_corpus(a.bytes, a.files, a.vocab, a.seed, threads=min(16, os.cpu_count() or 4))
    ix = ii_ctypes.Index(a.device)
    ix.map_host(text, off, np.arange(a.files, dtype=np.uint32))
    ix.reduce()
    st = ix.stats()
    letters = ix.letters()
    del text
    words, df, spans = vocabulary(letters)
    assert len(words) == st.words
    order = np.lexsort((np.arange(len(words)), -df))  # Zipf rank -> word index
    rng = np.random.default_rng(a.seed)
    sets = {"and": draw(rng, order, a.and_queries, 2, 3), "or": draw(rng, order, a.or_queries, 2, 3)}

    cache = {}

    def postings(w):
        if w not in cache:
            l, b, e = spans[w]
            cache[w] = np.array(letters[l][b:e].split(), dtype=np.uint32)
        return cache[w]

    result = {"tool": "query_bench", "corpus": {"bytes": a.bytes, "files": a.files, "vocab": a.vocab, "seed": a.seed},
              "index": {"words": int(st.words), "pairs": int(st.pairs), "pair_bytes": int(st.pair_bytes)},
              "libii_sha256_16": hashlib.sha256(open(os.path.join(PKG, "libii.so"), "rb").read()).hexdigest()[:16],
              "box": box_name(a.device), "tile": os.environ.get("II_QUERY_TILE", "default")}
    for op, queries in sets.items():
        if not queries:
            continue
        terms = [[words[w] for w in q] for q in queries]
        # GPU: the result left on the device (ms_total is the host wall time inside ii_query) ...
        runs = []
        for _ in range(1 + a.repeats):  # (the first call grows the buffers)
            ix.query(terms, op, to_host=False)
            runs.append(ix.query_stats().as_dict())
        runs = sorted(runs[1:], key=lambda s: s["ms_total"])
        med = runs[len(runs) // 2]
        # ... and once with the ids copied to the host, for the check
        got = ix.query(terms, op)
        host = ix.query_stats().as_dict()
        # CPU baseline: posting arrays parsed beforehand, the combine timed
        arrays = [[postings(w) for w in q] for q in queries]
        comb = np.intersect1d if op == "and" else np.union1d
        t0 = time.perf_counter()
        base = []
        for arrs in arrays:
            r = arrs[0]
            for x in arrs[1:]:
                r = comb(r, x)  # (ids of one list are unique)
            base.append(r)
        cpu_s = time.perf_counter() - t0
        step = max(1, int(round(1 / a.sample))) if a.sample > 0 else len(queries) + 1
        checked = 0
        for q in range(0, len(queries), step):
            if not np.array_equal(got[q], np.unique(base[q])):
                raise SystemExit("query_bench: %s query %d differs from the numpy baseline" % (op, q))
            checked += 1
        n = len(queries)
        result[op] = {
            "queries": n, "checked": checked,
            "gpu_queries_per_s": n / (med["ms_total"] * 1e-3),
            "gpu_postings_read_per_s": med["postings_read"] / (med["ms_total"] * 1e-3),
            "gpu_queries_per_s_with_host_copy": n / (host["ms_total"] * 1e-3),
            "cpu_queries_per_s": n / cpu_s, "cpu_s": cpu_s,
            "stats": med, "stats_with_host_copy": host,
        }
    ix.close()
    print(json.dumps(result))


def box_name(device):
    try:
        import torch
        return torch.cuda.get_device_name(device)
    except Exception:
        return "unknown"


if __name__ == "__main__":
    main()
