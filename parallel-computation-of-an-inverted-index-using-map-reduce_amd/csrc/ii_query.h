// Boolean term queries on the device-resident partial index (ii_lookup /
// ii_query, include/ii.h).  The kernels read the dictionary (dkey, lrep, llen),
// the posting ranges (pstart / pstop by lexicographic id) and the postings
// (uniq, either pair form) and write only the query's own buffers.
//
// One ii_query call:
//   k_query_lookup   term -> lexicographic id, posting start, df
//   k_query_plan     query -> driver list (AND) / distinct lists (OR), the
//                    bound of its candidate segment and its work items
//   (two scans: segment offsets, work-item offsets; the totals go to the host)
//   k_query_and / k_query_or   one wave per work item writes the candidates of
//                    its tile into the query's segment, in result order: the
//                    printed id (id0 + 1) where the candidate survives, 0
//                    where it does not
//   (one scan compacts the survivors of all segments: OpQueryCompact)
//   k_query_off      result offsets of every query
// No kernel waits on another workgroup, and every loop is bounded by an
// argument (list lengths, V, nbytes) or by a constant.
#pragma once

#include "ii_kernels.h"

namespace ii {

constexpr uint32_t kQueryTile = 2048;     // driver postings per work item (II_QUERY_TILE shrinks it: tests)
constexpr uint32_t kQueryMaxTerms = 16;   // II_MAX_QUERY_TERMS
constexpr uint32_t kQueryNone = 0xFFFFFFFFu;
constexpr uint32_t kQueryPad = 64;        // a query's candidate segment starts at a multiple of it (k_query_off)
enum : int { QT_BOUND = 0, QT_ITEMS, QT_POSTINGS, QT_FOUND, QT_OUT, QT_NUM };  // the query's device totals

// id0 of posting p of either pair form: compact u32 pairs carry kPairFirst on
// a word's first posting, u64 pairs are key << 32 | id0.
template <bool k32>
__device__ __forceinline__ uint32_t posting_id(const void* __restrict__ uniq, uint64_t p) {
    if (k32) return reinterpret_cast<const uint32_t*>(uniq)[p] & ~kPairFirst;
    return (uint32_t) reinterpret_cast<const uint64_t*>(uniq)[p];
}

// First posting of [lo, hi) whose id is >= x (kUpper: > x).  At most 64 halvings of a u64 range.
template <bool k32, bool kUpper>
__device__ __forceinline__ uint64_t posting_bound(const void* __restrict__ uniq, uint64_t lo, uint64_t hi, uint32_t x) {
    for (int it = 0; it < 64 && lo < hi; it++) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint32_t y = posting_id<k32>(uniq, mid);
        if (kUpper ? y <= x : y < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Letters [12, ...) of a cleaned term (tlen > 12 letters 'a'..'z') against
// the indexed word whose occurrence starts at text[pos] and that has wlen
// letters (llen): strcmp order of the cleaned words, < 0 / 0 / > 0.  The
// occurrence is raw text: non-letters are skipped and case is folded as
// read_word does; the walk ends at nbytes, at the word's terminator or after
// wlen letters, whichever comes first.
__device__ __forceinline__ int term_vs_word(const uint8_t* __restrict__ term, uint32_t tlen,
                                            const uint8_t* __restrict__ text, uint64_t nbytes, uint64_t pos,
                                            uint32_t wlen) {
    uint32_t n = 0;
    for (uint64_t g = pos; g < nbytes && n < wlen; g++) {
        const uint32_t c = text[g];
        if (c == 0u || is_ws(c)) break;
        const uint32_t lc = letter_of(c);
        if (lc < 26u) {
            if (n >= 12u) {
                if (n >= tlen) return -1;  // the term is a proper prefix of the word
                const uint32_t tc = (uint32_t)term[n] - 0x61u;
                if (tc != lc) return tc < lc ? -1 : 1;
            }
            n++;
        }
    }
    return tlen > n ? 1 : 0;
}

// Term t (cleaned letters arena[toff[t], toff[t + 1])) -> its lexicographic
// id (kQueryNone: absent), first posting and df.  The first 12 letters are
// packed as read_word / word_chunk pack them (5 bits per letter, 1..26, from
// bit 59 down) and searched in dkey: the key itself for a term of at most 12
// letters, key | 1 for a longer one.  Words that share a 12-letter prefix and
// are longer than it form a run of equal keys, ordered by their remaining
// letters (dict_lex): the run is binary-searched with term_vs_word, not
// scanned, so a lookup costs O(log V) word comparisons whatever the run's length.
__global__ __launch_bounds__(kBlock) void k_query_lookup(const uint8_t* __restrict__ text, uint64_t nbytes,
                                                         const uint64_t* __restrict__ dkey,
                                                         const uint64_t* __restrict__ lrep,
                                                         const uint32_t* __restrict__ llen,
                                                         const uint64_t* __restrict__ pstart,
                                                         const uint64_t* __restrict__ pstop, uint32_t V,
                                                         const uint8_t* __restrict__ arena,
                                                         const uint32_t* __restrict__ toff, uint32_t nterms,
                                                         uint32_t* __restrict__ t_lex, uint64_t* __restrict__ t_ps,
                                                         uint32_t* __restrict__ t_df, uint64_t* __restrict__ qtot) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nterms) return;
    const uint32_t a = toff[t], tlen = toff[t + 1] - a;
    const uint8_t* term = arena + a;
    uint32_t lex = kQueryNone;
    if (tlen > 0 && V > 0) {
        uint64_t key = 0;
        for (uint32_t n = 0; n < 12u && n < tlen; n++) key |= (uint64_t)((uint32_t)term[n] - 0x60u) << (59 - 5 * n);
        const uint64_t want = tlen > 12u ? key | 1ull : key;
        uint32_t lo = 0, hi = V;
        for (int it = 0; it < 32 && lo < hi; it++) {  // first key >= want
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (dkey[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        if (lo < V && dkey[lo] == want) {
            if (tlen <= 12u) {
                lex = lo;  // (words of at most 12 letters have distinct keys)
            } else {
                uint32_t rl = lo, rh = V;
                for (int it = 0; it < 32 && rl < rh; it++) {  // end of the run of equal keys
                    const uint32_t mid = rl + ((rh - rl) >> 1);
                    if (dkey[mid] <= want) rl = mid + 1;
                    else rh = mid;
                }
                rh = rl;
                rl = lo;
                for (int it = 0; it < 32 && rl < rh; it++) {
                    const uint32_t mid = rl + ((rh - rl) >> 1);
                    const int c = term_vs_word(term, tlen, text, nbytes, lrep[mid], llen[mid]);
                    if (c == 0) {
                        lex = mid;
                        break;
                    }
                    if (c < 0) rh = mid;
                    else rl = mid + 1;
                }
            }
        }
    }
    uint64_t ps = 0;
    uint32_t df = 0;
    if (lex != kQueryNone) {
        ps = pstart[lex];
        df = (uint32_t)(pstop[lex] - ps);
    }
    // terms found: one add per wave (the first lane that found one adds the wave's count)
    const uint64_t fm = __ballot(lex != kQueryNone);
    if (lex != kQueryNone && lanes_below(fm) == 0)
        atomicAdd((unsigned long long*)&qtot[QT_FOUND], (unsigned long long)__popcll(fm));
    t_lex[t] = lex;
    t_ps[t] = ps;
    t_df[t] = df;
}

// Query q -> the lists it reads (t_use: the df of a term as this query uses
// it), the length of its candidate segment and its work items.
//   AND: the driver is the found term with the smallest df; any absent term
//        (or no term) empties the query.  Candidates = the driver's postings.
//   OR:  a term whose word an earlier term of the query already names is
//        dropped (t_use = 0).  Candidates = all postings of the distinct lists.
// q_bound[q] = candidates rounded up to kQueryPad; q_tiles[q] = work items:
// every list that is walked is cut into tiles of 1 << tile_log2 postings.
__global__ __launch_bounds__(kBlock) void k_query_plan(const uint32_t* __restrict__ query_first, uint32_t nq, int op_or,
                                                       const uint32_t* __restrict__ t_lex,
                                                       const uint32_t* __restrict__ t_df, uint32_t* __restrict__ t_use,
                                                       uint32_t* __restrict__ q_drv, uint64_t* __restrict__ q_bound,
                                                       uint64_t* __restrict__ q_tiles, int tile_log2,
                                                       uint64_t* __restrict__ qtot) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool live = q < nq;  // (no early return: the wave sums its candidates below)
    const uint32_t t0 = live ? query_first[q] : 0u;
    const uint32_t nt = live ? min(query_first[q + 1] - t0, kQueryMaxTerms) : 0u;  // (the host refused longer queries)
    const uint64_t tmask = (1ull << tile_log2) - 1ull;
    uint64_t cand = 0, tiles = 0;
    uint32_t drv = kQueryNone;
    if (op_or) {
        for (uint32_t j = 0; j < nt; j++) {
            uint32_t use = t_df[t0 + j];
            for (uint32_t k = 0; k < j; k++)
                if (t_lex[t0 + k] == t_lex[t0 + j]) use = 0;
            t_use[t0 + j] = use;
            cand += use;
            tiles += ((uint64_t)use + tmask) >> tile_log2;
        }
    } else {
        uint32_t best = 0;
        bool all = nt > 0;
        for (uint32_t j = 0; j < nt; j++) {
            const uint32_t df = t_df[t0 + j];
            t_use[t0 + j] = df;
            if (df == 0) all = false;
            else if (drv == kQueryNone || df < best) {
                drv = t0 + j;
                best = df;
            }
        }
        if (!all) drv = kQueryNone;
        else {
            cand = best;
            tiles = ((uint64_t)best + tmask) >> tile_log2;
        }
    }
    if (live) {
        q_drv[q] = drv;
        q_bound[q] = (cand + (kQueryPad - 1)) & ~(uint64_t)(kQueryPad - 1);
        q_tiles[q] = tiles;
    }
    const uint64_t wcand = wave_sum(cand);  // one add per wave
    if (lane_id() == 0 && wcand) atomicAdd((unsigned long long*)&qtot[QT_POSTINGS], (unsigned long long)wcand);
}

// The query of work item `item`: istart[q] <= item < istart[q + 1] (istart =
// the exclusive scan of q_tiles over nq queries; item < the scan's total).
__device__ __forceinline__ uint32_t query_of_item(const uint64_t* __restrict__ istart, uint32_t nq, uint64_t item) {
    uint32_t lo = 0, hi = nq;  // first q with istart[q] > item
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (istart[mid] <= item) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// The lists of one query, staged per wave in LDS: lane j < nt fills entry j,
// every lane reads all of them.
struct QueryLists {
    uint64_t ps[kQueryMaxTerms];   // first posting of list j
    uint64_t lo[kQueryMaxTerms];   // window of list j for the tile's id range: [lo, hi)
    uint64_t hi[kQueryMaxTerms];
    uint32_t use[kQueryMaxTerms];  // its length as the query uses it
};

// AND, one wave per work item = (query, tile of the driver list).  The lanes
// load the tile's candidates 64 at a time (consecutive postings: coalesced);
// lane j narrows list j once to the postings between the tile's first and
// last id; each candidate is then binary-searched in every other list's
// window.  The candidate's slot in the query's segment receives id0 + 1, or 0
// when some list lacks it; the last tile also clears the segment's padding.
// The survivors keep the driver's order because every slot is written in
// place; OpQueryCompact removes the zeros of all segments in one scan.
template <bool k32>
__global__ __launch_bounds__(kBlock) void k_query_and(const void* __restrict__ uniq,
                                                      const uint32_t* __restrict__ query_first,
                                                      const uint64_t* __restrict__ t_ps,
                                                      const uint32_t* __restrict__ t_use,
                                                      const uint32_t* __restrict__ q_drv,
                                                      const uint64_t* __restrict__ istart,
                                                      const uint64_t* __restrict__ boff, uint32_t nq, uint64_t nitems,
                                                      int tile_log2, uint32_t* __restrict__ cand) {
    __shared__ QueryLists s_l[kWG];
    const uint64_t item = wave_chunk();
    if (item >= nitems) return;  // (wave-uniform)
    QueryLists& L = s_l[threadIdx.x >> 6];
    const uint32_t lane = lane_id();
    const uint32_t q = query_of_item(istart, nq, item);
    const uint32_t t0 = query_first[q];
    const uint32_t nt = min(query_first[q + 1] - t0, kQueryMaxTerms);
    const uint32_t d = q_drv[q];  // (a query with work items has a driver)
    const uint64_t dps = t_ps[d];
    const uint64_t ddf = t_use[d];
    const uint64_t e0 = (item - istart[q]) << tile_log2;
    const uint64_t e1 = e0 + ((uint64_t)1 << tile_log2) < ddf ? e0 + ((uint64_t)1 << tile_log2) : ddf;
    const uint32_t first = posting_id<k32>(uniq, dps + e0), last = posting_id<k32>(uniq, dps + e1 - 1);
    if (lane < nt) {
        const uint64_t ps = t_ps[t0 + lane], n = t_use[t0 + lane];
        L.ps[lane] = ps;
        L.use[lane] = (uint32_t)n;
        L.lo[lane] = posting_bound<k32, false>(uniq, ps, ps + n, first);
        L.hi[lane] = posting_bound<k32, true>(uniq, ps, ps + n, last);
    }
    wave_sync();
    // the last tile writes up to the segment's padded end (e0 is a multiple of 64)
    const uint64_t e_end = e1 == ddf ? (ddf + (kQueryPad - 1)) & ~(uint64_t)(kQueryPad - 1) : e1;
    uint32_t* seg = cand + boff[q];
    for (uint64_t r = e0; r < e_end; r += 64) {
        const uint64_t e = r + lane;
        uint32_t out = 0;
        if (e < e1) {
            const uint32_t x = posting_id<k32>(uniq, dps + e);
            bool ok = true;
            for (uint32_t j = 0; j < nt && ok; j++) {
                if (t0 + j == d) continue;
                const uint64_t p = posting_bound<k32, false>(uniq, L.lo[j], L.hi[j], x);
                ok = p < L.hi[j] && posting_id<k32>(uniq, p) == x;
            }
            if (ok) out = x + 1u;  // (id0 = UINT32_MAX has no printed u32 id: left out, ii.h)
        }
        if (e < e_end) seg[e] = out;
    }
}

// OR, one wave per work item = (query, list i, tile of list i).  Element x of
// list i is kept iff no list j < i holds x, and its slot in the query's
// segment is its rank in the merge of all lists with ties broken by list
// index:  sum_j |{y in L_j : y < x}| + |{j < i : x in L_j}|.  Dropped elements
// write nothing: the segment was cleared before the launch.  Lane j narrows
// list j to the tile's id range once, so the per-element searches run in
// windows of about a tile's span.
template <bool k32>
__global__ __launch_bounds__(kBlock) void k_query_or(const void* __restrict__ uniq,
                                                     const uint32_t* __restrict__ query_first,
                                                     const uint64_t* __restrict__ t_ps,
                                                     const uint32_t* __restrict__ t_use,
                                                     const uint64_t* __restrict__ istart,
                                                     const uint64_t* __restrict__ boff, uint32_t nq, uint64_t nitems,
                                                     int tile_log2, uint32_t* __restrict__ cand) {
    __shared__ QueryLists s_l[kWG];
    const uint64_t item = wave_chunk();
    if (item >= nitems) return;  // (wave-uniform)
    QueryLists& L = s_l[threadIdx.x >> 6];
    const uint32_t lane = lane_id();
    const uint32_t q = query_of_item(istart, nq, item);
    const uint32_t t0 = query_first[q];
    const uint32_t nt = min(query_first[q + 1] - t0, kQueryMaxTerms);
    if (lane < nt) {
        L.ps[lane] = t_ps[t0 + lane];
        L.use[lane] = t_use[t0 + lane];
    }
    wave_sync();
    // the list and the tile of this item: the query's items are its lists' tiles, list after list
    const uint64_t tmask = (1ull << tile_log2) - 1ull;
    uint64_t tix = item - istart[q];
    uint32_t i = 0;
    for (; i + 1 < nt; i++) {
        const uint64_t nt_i = ((uint64_t)L.use[i] + tmask) >> tile_log2;
        if (tix < nt_i) break;
        tix -= nt_i;
    }
    const uint64_t ips = L.ps[i], idf = L.use[i];
    const uint64_t e0 = tix << tile_log2;
    if (e0 >= idf) return;  // (cannot happen: the plan counted these tiles)
    const uint64_t e1 = e0 + ((uint64_t)1 << tile_log2) < idf ? e0 + ((uint64_t)1 << tile_log2) : idf;
    const uint32_t first = posting_id<k32>(uniq, ips + e0), last = posting_id<k32>(uniq, ips + e1 - 1);
    if (lane < nt) {
        const uint64_t ps = L.ps[lane], n = L.use[lane];
        L.lo[lane] = posting_bound<k32, false>(uniq, ps, ps + n, first);
        L.hi[lane] = posting_bound<k32, true>(uniq, ps, ps + n, last);
    }
    wave_sync();
    uint32_t* seg = cand + boff[q];
    for (uint64_t r = e0; r < e1; r += 64) {
        const uint64_t e = r + lane;
        if (e >= e1) continue;
        const uint32_t x = posting_id<k32>(uniq, ips + e);
        uint64_t rank = e;  // the postings of list i below x
        bool keep = true;
        for (uint32_t j = 0; j < nt; j++) {
            if (j == i) continue;
            const uint64_t p = posting_bound<k32, false>(uniq, L.lo[j], L.hi[j], x);
            rank += p - L.ps[j];
            if (j < i && p < L.hi[j] && posting_id<k32>(uniq, p) == x) {
                keep = false;
                break;
            }
        }
        if (keep && x != 0xFFFFFFFFu) seg[rank] = x + 1u;
    }
}

// Compaction of the candidate segments: ids[k] = the k-th non-zero candidate;
// gex[i / kQueryPad] = the survivors before candidate i at every multiple of
// kQueryPad, which is where every query's segment starts.
struct OpQueryCompact {
    const uint32_t* cand;
    uint32_t* ids;
    uint64_t* gex;
    __device__ uint64_t value(uint64_t i) const { return cand[i] != 0u; }
    __device__ void emit(uint64_t i, uint64_t ex, uint64_t v) const {
        if (v) ids[ex] = cand[i];
        if ((i & (kQueryPad - 1)) == 0) gex[i / kQueryPad] = ex;
    }
};

// res_off[q] = survivors before query q's segment (q <= nq; the last entry
// and every query whose segment starts at the end of the candidates: all of them).
__global__ __launch_bounds__(kBlock) void k_query_off(const uint64_t* __restrict__ boff, uint32_t nq,
                                                      const uint64_t* __restrict__ gex,
                                                      const uint64_t* __restrict__ qtot,
                                                      uint64_t* __restrict__ res_off) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q > nq) return;
    const uint64_t B = qtot[QT_BOUND];
    const uint64_t b = q < nq ? boff[q] : B;
    res_off[q] = b < B ? gex[b / kQueryPad] : qtot[QT_OUT];
}

}  // namespace ii
