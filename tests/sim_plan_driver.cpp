// The stand-alone driver of tests/test_sim_plan.py: rp_sim_plan.h's knob reader and refresh
// plan, without HIP. One row a line of standard input:
//     NL G cus nd [NAME=VALUE ...]
// Every simulator knob is unset, the row's are set, and one line comes out: what sim_knobs(),
// ck_plan_begin / ck_plan_finish (with nd as the dirty count, used only when the plan asks for
// it), d1_ck_kernel and early_ck_kernel say.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "rp_sim_plan.h"

static const char* const kKnobs[] = {"RP_SIM_CK",         "RP_SIM_CK_ABLATE",   "RP_SIM_TWINS",  "RP_SIM_TWIN_VERIFY",
                                     "RP_SIM_PASS1",      "RP_SIM_CK_SORT",     "RP_SIM_CK_SORT_PC", "RP_SIM_PC32_PER_CU",
                                     "RP_SIM_D1_CK",      "RP_SIM_D1_BLOCKCK",  "RP_SIM_D1_VPG", "RP_SIM_EARLY"};

static const char* name(rp::CkKernel k) {
    switch (k) {
    case rp::CkKernel::None: return "none";
    case rp::CkKernel::Lanes: return "lanes";
    case rp::CkKernel::Pc7: return "pc<7>";
    case rp::CkKernel::Pc3: return "pc<3>";
    case rp::CkKernel::Pc32: return "pc<3,2>";
    case rp::CkKernel::Pair32: return "pair<6,2,32>";
    case rp::CkKernel::Pair16: return "pair<6,2,16>";
    case rp::CkKernel::Pair8: return "pair<6,2,8>";
    }
    return "?";
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t NL, G, cus, nd;
        if (!(in >> NL >> G >> cus >> nd)) return 2;
        for (const char* k : kKnobs) unsetenv(k);
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) return 2;
            setenv(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str(), 1);
        }
        const rp::SimKnobs k = rp::sim_knobs();
        const rp::CkPlan b = rp::ck_plan_begin(k, NL, G, cus);
        const rp::CkPlan p = rp::ck_plan_finish(b, b.need_nd ? nd : 0);
        if (p.twins != b.twins || p.list != b.list) return 3;  // finish keeps what begin promised
        printf("kernel=%s twins=%d list=%d nd_read=%d sort=%d radix=%d key=%d pass1=%d ablate=%u verify=%d d1=%s early=%d "
               "early_kernel=%s\n",
               name(p.kernel), p.twins, p.list, b.need_nd, p.sort, p.radix, p.key_flag, p.pass1, k.ck_ablate,
               k.twin_verify, name(rp::d1_ck_kernel(k)), k.early, name(rp::early_ck_kernel(NL, cus)));
    }
    return 0;
}
