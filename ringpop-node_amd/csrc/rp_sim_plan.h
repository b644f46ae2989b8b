// rp_sim_plan.h — the gossip simulator's checksum refresh as a decision: its environment
// variables (SimKnobs) and the rule that turns them, the shard's size and the dirty count into the
// kernels to launch (CkPlan). No HIP and no launch here, so that a plain C++ compiler builds it
// alone (tests/sim_plan_driver.cpp); rp_sim.hip's Sim::refresh_checksums() and stage 2 execute it.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace rp {

// RP_SIM_CK's values. Other: any other text, the empty one too; it behaves as `pc`.
enum class CkKnob : uint8_t { Unset, Lanes, Pc, Pc3, Pc32, Pair, Other };
// A 0|1 override of a choice the plan otherwise makes itself.
enum class Tri : int8_t { Unset = -1, Off = 0, On = 1 };
// RP_SIM_D1_CK
enum class D1Ck : uint8_t { Pair, Pc, BlockCk };

// The chain kernels (one checksum chain a lane) that launch_ck of rp_sim.hip can start.
enum class CkKernel : uint8_t {
    None,    // no launch (D1 with blockck: a workgroup per sender inside k_phase_d1)
    Lanes,   // k_ck_lanes: one wave per 64 views, no producers
    Pc7,     // k_ck_pc<7>: a chain wave + 7 producer waves per 64 views
    Pc3,     // k_ck_pc<3>
    Pc32,    // k_ck_pc<3, 2>: 3 producers x 2 chunks per epoch, 41 KB of LDS, 3 groups on a CU
    Pair32,  // k_ck_pair<6, 2, 32>: the lane-pair chains, 32 views per workgroup
    Pair16,  // k_ck_pair<6, 2, 16>
    Pair8,   // k_ck_pair<6, 2, 8>
};

// Every environment variable of the checksum refresh and of stage 2's sender and early refreshes
// (A/B and diagnostics; none is API). sim_knobs() is their only reader. A handle reads them when
// it is created and again at stage 0 of every round, and keeps the value: the tests change them
// between simulators of one process. Which kernels a value selects: ck_plan_* below.
// (The capacity knobs of a simulator's creation, RP_SIM_CAP and its kin, are read there.)
struct SimKnobs {
    // RP_SIM_CK=lanes|pc|pc3|pc32|pair: the refresh's chain kernel (unset: by size and dirty count)
    CkKnob ck;
    // RP_SIM_CK_ABLATE: timing ablation of k_ck_lanes, SimDev::ck_ablate (results wrong; default 0)
    uint32_t ck_ablate;
    // RP_SIM_TWINS=0|1: the twin-view pass off | on, by the first character (unset or empty: on
    // when the lane path is chosen by size, else off)
    Tri twins;
    // RP_SIM_TWIN_VERIFY=1: k_twin_fp recomputes every fingerprint from the rows, a check of vfp
    // (on unless unset, empty or starting with '0')
    bool twin_verify;
    // RP_SIM_PASS1=0|1: k_pass1 ahead of the chains off | on, by the first character (unset or
    // empty: on except on the lane path)
    Tri pass1;
    // RP_SIM_CK_SORT: order of the views to hash, 3 = by length delta (vdt), 1 = by this round's
    // shifts from a pass-1 launch, 0 = list order (unset or empty: 3)
    int ck_sort;
    // RP_SIM_CK_SORT_PC=1: that order on the producer/consumer paths too; any other text: not
    // (unset or empty: when the handle is one shard of several)
    Tri ck_sort_pc;
    // RP_SIM_PC32_PER_CU: the automatic lane path takes k_ck_pc<3, 2> while the dirty views fill at
    // most this many 64-view groups a CU (unset or empty: 3)
    uint32_t pc32_per_cu;
    // RP_SIM_D1_CK=pc|blockck: the D1 senders' checksums by k_ck_pc<7> | by a workgroup per sender
    // inside D1 (else k_ck_pair); RP_SIM_D1_BLOCKCK set at all: blockck, unless RP_SIM_D1_CK=pc
    D1Ck d1_ck;
    // RP_SIM_D1_VPG=16: k_ck_pair's views per workgroup for the D1 senders (anything else: 8)
    int d1_vpg;
    // RP_SIM_EARLY=1: the early refresh of stage 2 on a side stream (on only for a first character
    // '1'; off by default)
    bool early;
};

inline SimKnobs sim_knobs() {
    const auto text = [](const char* name) {  // set and not empty, else null
        const char* e = getenv(name);
        return e && *e ? e : nullptr;
    };
    const auto tri = [](const char* e, bool on) { return !e ? Tri::Unset : on ? Tri::On : Tri::Off; };
    SimKnobs k;
    const char* m = getenv("RP_SIM_CK");
    k.ck = !m                    ? CkKnob::Unset
           : !strcmp(m, "lanes") ? CkKnob::Lanes
           : !strcmp(m, "pc")    ? CkKnob::Pc
           : !strcmp(m, "pc3")   ? CkKnob::Pc3
           : !strcmp(m, "pc32")  ? CkKnob::Pc32
           : !strcmp(m, "pair")  ? CkKnob::Pair
                                 : CkKnob::Other;
    const char* e = text("RP_SIM_CK_ABLATE");
    k.ck_ablate = e ? (uint32_t)atoi(e) : 0u;
    e = text("RP_SIM_TWINS");
    k.twins = tri(e, e && *e != '0');
    e = text("RP_SIM_TWIN_VERIFY");
    k.twin_verify = e && *e != '0';
    e = text("RP_SIM_PASS1");
    k.pass1 = tri(e, e && *e != '0');
    e = text("RP_SIM_CK_SORT");
    k.ck_sort = e ? atoi(e) : 3;
    e = text("RP_SIM_CK_SORT_PC");
    k.ck_sort_pc = tri(e, e && *e == '1');
    e = text("RP_SIM_PC32_PER_CU");
    k.pc32_per_cu = e ? (uint32_t)atoi(e) : 3u;
    e = getenv("RP_SIM_D1_CK");
    k.d1_ck = e && !strcmp(e, "pc")                                          ? D1Ck::Pc
              : (e && !strcmp(e, "blockck")) || getenv("RP_SIM_D1_BLOCKCK") ? D1Ck::BlockCk
                                                                             : D1Ck::Pair;
    e = text("RP_SIM_D1_VPG");
    k.d1_vpg = e && atoi(e) == 16 ? 16 : 8;
    e = getenv("RP_SIM_EARLY");
    k.early = e && *e == '1';
    return k;
}

// One chain per lane on every path. With no more 64-node groups than CUs (a shard, C4) each group
// gets a whole CU: its chain wave plus producer waves (k_ck_pc, ~130 cycles per chunk). With more
// groups than CUs the machine is issue-bound on the chunks' multiplies, and one wave per group
// without producers (k_ck_lanes) does less work.
inline bool ck_groups_fit(uint32_t NL, uint32_t cus) { return (NL + 63) / 64 <= cus; }

// What one refresh of NL local views launches. ck_plan_begin fills the first three fields, which
// are known before anything runs; ck_plan_finish fills the rest, from the dirty count when need_nd
// says so (a host wait: only the paths that use the count's value pay for it).
struct CkPlan {
    bool twins;    // k_twin_fp and k_twin_check mark dirty views with equal content clean; k_twin_copy
                   // at the end gives each its representative's checksum
    bool list;     // k_dirty_list compacts the views left to hash, so that waves hold only real
                   // chains (a wave runs as long as its longest lane); else every view, in place
    bool need_nd;  // the list's count comes back to the host before ck_plan_finish
    CkKernel kernel;
    bool pass1;    // k_pass1 ahead of the chains; else each lane walks its own view's pass 1
    bool sort;     // k_ck_sort_keys over the list, and the chains run over its sorted copy
    bool radix;    // the radix sort between them (more than one dirty view)
    int key_flag;  // k_ck_sort_keys' from_vdt
    // the inputs that ck_plan_finish still needs
    SimKnobs k;
    uint32_t G, cus;
    bool pc;      // a producer/consumer (or pair) kernel by knob or by size, not the lane path
    bool auto32;  // the lane path chosen by size: k_ck_pc<3, 2> or k_ck_lanes by the dirty count
};

inline CkPlan ck_plan_finish(CkPlan p, uint32_t nd) {
    const SimKnobs& k = p.k;
    const bool pair = k.ck == CkKnob::Pair;
    // pc32 puts 3 groups on a CU. On the lane path it takes the rounds whose compacted dirty views
    // fill at most 3 groups per CU (C5 on one GPU: median round 64 against 68 ms); the peak
    // rounds, where nearly every view is dirty and the machine is issue-bound, stay on k_ck_lanes
    // (pc32 there: 111 against 96 ms). Choosing reads the dirty count back (one small copy per
    // round). A/B: RP_SIM_PC32_PER_CU.
    const bool use32 = k.ck == CkKnob::Pc32 || (p.auto32 && (nd + 63) / 64 <= k.pc32_per_cu * p.cus);
    const bool lanes_path = !use32 && !p.pc;
    // The lane path's order (round 6): the views to hash sorted by their string's length delta
    // (vdt, kept by block_apply), so that a wave's 64 lanes reach their deviated pieces in the
    // same chunk groups: the fixup path runs for a whole wave when any lane needs it, and in C5's
    // peak refreshes list order put a fixup in 10-13 % of wave-groups against 3-4 % sorted
    // (-DRP_CKL_STAT, profiles/r06/r06ab, r06ac); C5 p95 round 78 -> 68 ms (r06ae).
    // RP_SIM_CK_SORT: 3 (default) that order, 1 = by this round's shifts from a pass-1 launch
    // (slower: the launch), 0 = list order.
    // The same order on the producer/consumer paths when this handle is one shard of several
    // (each rank of a sharded C5 refreshes on them): C5 in 8 shards on one GPU 147.7 -> 142.6 ms
    // per round; C4 on one GPU (not sharded) 2.41 -> 2.46, so not there (profiles/r06/r06ah,
    // r06ai). RP_SIM_CK_SORT_PC=0|1 overrides; it builds the list where the twins did not.
    const bool sort_pc = !lanes_path && !pair && k.ck_sort == 3 &&
                         (k.ck_sort_pc != Tri::Unset ? k.ck_sort_pc == Tri::On : p.G > 1);
    p.list = p.twins || sort_pc;
    p.sort = (lanes_path || sort_pc) && p.list && k.ck_sort > 0;
    p.radix = p.sort && nd > 1;
    p.key_flag = k.ck_sort == 3 ? 1 : 0;
    // Pass 1 of every view to hash, a wave per view, ahead of the producer/consumer kernels, whose
    // chain wave otherwise walks its 64 views' bitmaps and deviated members before any chunk is
    // produced (C5: k_ck_pc<3, 2> 375 -> 324 ms over a run for 13 ms of k_pass1). k_ck_lanes
    // hides its own lane walks behind other waves: there k_pass1 costs more than it saves (153
    // against 49 ms), so it stays in the kernel (RP_SIM_PASS1=0|1 overrides). The order by this
    // round's shifts needs it; the pair kernel never takes it.
    p.pass1 = !pair && ((p.sort && k.ck_sort == 1) || (k.pass1 != Tri::Unset ? k.pass1 == Tri::On : !lanes_path));
    p.kernel = pair                          ? CkKernel::Pair32
               : use32                       ? CkKernel::Pc32
               : p.pc && k.ck != CkKnob::Pc3 ? CkKernel::Pc7
               : p.pc                        ? CkKernel::Pc3
                                             : CkKernel::Lanes;
    return p;
}

inline CkPlan ck_plan_begin(const SimKnobs& k, uint32_t NL, uint32_t G, uint32_t cus) {
    CkPlan p{};
    p.k = k;
    p.G = G;
    p.cus = cus;
    p.pc = k.ck != CkKnob::Unset ? k.ck != CkKnob::Lanes : ck_groups_fit(NL, cus);
    // twins pay on the lane path (C5 on one GPU: 76.7 vs 78.2 ms per round, 31 % fewer chains); at
    // a shard's size (C4, the producer/consumer path) the two passes cost about what they save
    // (3.25 vs 3.14 ms), so RP_SIM_TWINS=1 forces them there
    p.twins = k.twins != Tri::Unset ? k.twins == Tri::On : !p.pc;
    p.auto32 = k.ck == CkKnob::Unset && !p.pc && p.twins;
    // Only auto32 makes the plan depend on the count's value, and then the twins build the list
    // whatever it is; so whether the list is built and sorted is ck_plan_finish's answer for any
    // count. A sorted list needs its count on the host for the radix sort's size.
    const CkPlan f = ck_plan_finish(p, 0);
    p.list = f.list;
    p.need_nd = p.auto32 || f.sort;
    return p;
}

// The D1 senders' checksums (their ping-req bodies carry them), over the list of senders, as
// side-by-side chains before k_phase_d1, so that its workgroups find their views clean.
inline CkKernel d1_ck_kernel(const SimKnobs& k) {
    return k.d1_ck == D1Ck::Pc        ? CkKernel::Pc7
           : k.d1_ck == D1Ck::BlockCk ? CkKernel::None
           : k.d1_vpg == 16           ? CkKernel::Pair16
                                      : CkKernel::Pair8;
}

// The early refresh (RP_SIM_EARLY=1), on the side stream: the size rule alone.
inline CkKernel early_ck_kernel(uint32_t NL, uint32_t cus) {
    return ck_groups_fit(NL, cus) ? CkKernel::Pc7 : CkKernel::Lanes;
}

}  // namespace rp
