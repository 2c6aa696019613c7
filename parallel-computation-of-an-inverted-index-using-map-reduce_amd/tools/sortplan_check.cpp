// sortplan_check.cpp — host-only driver of the token sort's plan
// (csrc/ii_sortplan.h), built under ASan + UBSan (make sortplan_check;
// tests/test_sort_plan.py).  One case per line of stdin:
//   T nfiles id_bound affine W wid|lexid [II_PACKED_SORT=.. II_PACKED_M=.. II_S0_DEDUP=.. II_S0_FMAP=..]
// and per case one line of stdout:
//   m F wide hashd Affine|GatherInK3|MappedInSort0      (or "error")
#include <stdio.h>

#include <sstream>
#include <string>

#include "../csrc/ii_sortplan.h"

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream is(line);
        SortPlanIn in{};
        int affine = 0;
        std::string keys, tok;
        if (!(is >> in.T >> in.nfiles >> in.id_bound >> affine >> in.W >> keys)) continue;  // (blank line)
        in.fid_affine = affine != 0;
        in.wid = keys == "wid";
        std::string packed, packed_m, dedup, fmap;
        bool has[4] = {false, false, false, false};
        while (is >> tok) {
            const size_t eq = tok.find('=');
            const std::string name = tok.substr(0, eq), val = eq == std::string::npos ? "" : tok.substr(eq + 1);
            if (name == "II_PACKED_SORT") packed = val, has[0] = true;
            else if (name == "II_PACKED_M") packed_m = val, has[1] = true;
            else if (name == "II_S0_DEDUP") dedup = val, has[2] = true;
            else if (name == "II_S0_FMAP") fmap = val, has[3] = true;
            else return 2;
        }
        in.knobs = parse_sort_knobs(has[0] ? packed.c_str() : nullptr, has[1] ? packed_m.c_str() : nullptr,
                                    has[2] ? dedup.c_str() : nullptr, has[3] ? fmap.c_str() : nullptr);
        TokenSortPlan p;
        if (plan_token_sort(in, &p)) {
            puts("error");
            continue;
        }
        printf("%d %d %d %d %s\n", p.m, p.F, (int)p.wide, (int)p.hashd,
               p.ids == IdSource::Affine ? "Affine" : p.ids == IdSource::GatherInK3 ? "GatherInK3" : "MappedInSort0");
    }
    return 0;
}
