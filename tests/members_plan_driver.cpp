// The stand-alone driver of tests/test_members_plan.py: rp_members_plan.h's knob reader, fold
// plan, checksum pool and string mode, without HIP. One row a line of standard input:
//     k cap names damp ranged id_lo id_hi pw_on pw_same_stream need [NAME=VALUE ...]
// Every Membership.update knob is unset, the row's are set (NAME= sets the empty string), and one
// line comes out: what members_knobs(), fold_plan(), ck_pool() and string_mode() say.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "rp_members_plan.h"

static const char* const kKnobs[] = {"RP_MEMBERS_SORTED_FOLD", "RP_MEMBERS_BUCKET_FOLD", "RP_MEMBERS_FUSE",
                                     "RP_MEMBERS_SIDE_BUILD",  "RP_MEMBERS_CK_BYTES",    "RP_MEMBERS_GROUP_SLOTS",
                                     "RP_BK_REC8",             "RP_BK_DIRECT",           "RP_BK_SGRID",
                                     "RP_BK_PROF_PRINT"};

static const char* name(rp::FoldPath p) {
    switch (p) {
    case rp::FoldPath::Empty: return "empty";
    case rp::FoldPath::Bucket: return "bucket";
    case rp::FoldPath::Grouped: return "grouped";
    case rp::FoldPath::Sorted: return "sorted";
    }
    return "?";
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t k, cap, id_lo, id_hi;
        uint64_t names, need;
        int damp, ranged, pw_on, pw_same;
        if (!(in >> k >> cap >> names >> damp >> ranged >> id_lo >> id_hi >> pw_on >> pw_same >> need)) return 2;
        for (const char* v : kKnobs) unsetenv(v);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) return 2;
            setenv(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str(), 1);
        }
        const rp::MemberKnobs kn = rp::members_knobs();
        const rp::FoldPlan p = rp::fold_plan(kn, k, cap, names, damp != 0, ranged != 0, id_lo, id_hi, pw_on != 0, pw_same != 0);
        const rp::CkPool pool = rp::ck_pool(need, kn);
        printf("path=%s nb=%u b_lo=%u b_hi=%u ntiles=%u sgrid=%u rec8=%d direct=%d gather=%d fuse=%d bits=%d nparts=%u "
               "drain=%d nslots=%u group_slots=%u ngroups=%u mode_ov=%d mode_plain=%d prof=%d\n",
               name(p.path), p.nb, p.b_lo, p.b_hi, p.ntiles, p.sgrid, p.rec8, p.direct, p.gather, p.fuse, p.bits, p.nparts,
               p.drain, pool.nslots, pool.group_slots, pool.ngroups, rp::string_mode(kn, true), rp::string_mode(kn, false),
               kn.prof_print);
    }
    return 0;
}
