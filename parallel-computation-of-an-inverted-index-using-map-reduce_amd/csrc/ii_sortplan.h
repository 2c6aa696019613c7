// ii_sortplan.h — the form of local_reduce's token sort, decided once: the packed form's top digit (or the u64
// LSD form), the first pass's dedup and where K1's shard-local file indices become id0s.  The first pass and K3
// both take their arguments from the one TokenSortPlan, so they cannot disagree.  Plain integers only — no HIP —
// so tools/sortplan_check.cpp builds it into a host program (tests/test_sort_plan.py); ii_api.hip asserts that
// the digit widths restated here are the kernels'.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

constexpr int kPlanRadixBits = 8;    // kRadixBits: an LSD digit
constexpr int kPlanMsdMaxBits = 11;  // kMsdMaxBits: the packed form's top digit, at most
// the record set dedups when the files average fewer tokens than this (configs[4]'s small-file shares: 3.9·10^3),
// the epoch bitmap otherwise (config3: 1.4·10^5 per file, more distinct pairs per file than the set holds)
constexpr uint64_t kHashDedupTokens = 16384;
constexpr uint32_t kS0FmapFiles = 65536;  // files from which the first pass maps file indices to id0s (a 256 KiB fmap)

static inline int bitlen(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

struct SortKnobs {  // the token sort's knobs, parsed from the environment's strings (null: unset)
    bool packed = true;  // II_PACKED_SORT=0: always the u64 form (test_packed_sort_forms_vs_oracle)
    int packed_m = 0;    // II_PACKED_M=<m>: at least m top bits, so that small inputs reach the wide split
    int dedup = 0;       // II_S0_DEDUP=set|bitmap (test and A/B knob) -> 1 | 2: forces the first pass's dedup; 0: by size
    int fmap = -1;       // II_S0_FMAP=0|1 (test and A/B knob): whether the first pass may write id0s; -1: by file count
};
static inline SortKnobs parse_sort_knobs(const char* packed, const char* packed_m, const char* dedup, const char* fmap) {
    SortKnobs k;
    k.packed = !(packed && !strcmp(packed, "0"));
    k.packed_m = packed_m ? atoi(packed_m) : 0;
    k.dedup = dedup && !strcmp(dedup, "set") ? 1 : dedup && !strcmp(dedup, "bitmap") ? 2 : 0;
    k.fmap = fmap ? strcmp(fmap, "0") != 0 : -1;
    return k;
}

struct SortPlanIn {
    uint64_t T;         // K1 records
    uint32_t nfiles;    // mapped files: the records carry indices below it
    uint32_t id_bound;  // 1 + the largest id0
    bool fid_affine;    // id0 = index + fid_off
    int W;              // key bits
    bool wid;           // word-id keys (lexid keys otherwise)
    SortKnobs knobs;
};
enum class IdSource {  // where a record's shard-local file index becomes an id0
    Affine,            // K3 adds fid_off
    GatherInK3,        // K3 reads fid[index]
    MappedInSort0,     // the first pass (its record-set form) writes id0s: K3 gathers nothing
};
struct TokenSortPlan {
    int W = 0, F = 0;    // key bits; id bits of the sorted records (file indices, or id0s when MappedInSort0)
    int m = 0;           // the packed form's top digit; 0: the u64 LSD form
    bool wid = false;
    bool wide = false;   // m > kRadixBits (k_sort0_compact<.., kWideD>, k_msd_scatter)
    bool hashd = false;  // the first pass dedups by the record set (kHashD), not the epoch bitmap; packed form only
    IdSource ids = IdSource::Affine;
};

// Packed token sort (ii_prims.h): the top digit m of a W-bit key when the other W - m key bits and the
// F id bits fit a u32 and leave two LSD passes of <= kRadixBits bits each; 0 = not packable.
static inline int packed_top_digit(int W, int F, const SortKnobs& k) {
    const int m = std::max({7, W + F - 32, k.packed_m}), L = W - m;
    return (k.packed && m <= kPlanMsdMaxBits && L >= 2 && L <= 2 * kPlanRadixBits) ? m : 0;
}

// 0, or -1 for a plan whose parts contradict each other (never launched).
static inline int plan_token_sort(const SortPlanIn& in, TokenSortPlan* p) {
    const SortKnobs& k = in.knobs;
    const bool set = k.dedup == 1 || (k.dedup == 0 && in.nfiles && in.T < kHashDedupTokens * (uint64_t)in.nfiles);
    *p = TokenSortPlan{};
    p->W = in.W;
    p->wid = in.wid;
    p->F = std::max(1, bitlen(in.nfiles ? in.nfiles - 1 : 0));
    p->ids = in.fid_affine ? IdSource::Affine : IdSource::GatherInK3;
    // many small files with non-consecutive ids (a size-sorted ii_partition share): the first pass writes id0s (F =
    // their bits) when the packed form still holds them — K3's gather of fid[index] missed L1 on nearly every pair
    const int Fg = std::max(1, bitlen(in.id_bound ? in.id_bound - 1 : 0));
    if (!in.fid_affine && in.id_bound && set && (k.fmap < 0 ? in.nfiles >= kS0FmapFiles : k.fmap != 0) &&
        packed_top_digit(in.W, Fg, k)) {
        p->F = Fg;
        p->ids = IdSource::MappedInSort0;
    }
    p->m = packed_top_digit(in.W, p->F, k);
    p->wide = p->m > kPlanRadixBits;
    p->hashd = p->m && set;
    return p->ids == IdSource::MappedInSort0 && !p->hashd ? -1 : 0;
}
