// rp_members_plan.h — Membership.update's host dispatch as a decision: its environment variables
// (MemberKnobs) and the rules that turn them and a batch's sizes into the fold path to launch
// (FoldPlan), the checksum slot pool (CkPool) and where a batch's checksum string is written
// (string_mode). No HIP and no launch here, so that a plain C++ compiler builds it alone
// (tests/members_plan_driver.cpp); rp_members.hip's Members::update_dev() and checksum_dev()
// execute it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace rp {

// The bucket path's sizes that the rule needs (its kernels' other constants: rp_members.hip).
#ifndef RP_BK_BITS
#define RP_BK_BITS 12
#endif
#ifndef RP_BK_TILE
#define RP_BK_TILE 4096
#endif
constexpr uint32_t kBkBits = RP_BK_BITS, kBk = 1u << kBkBits;  // ids per bucket (4,096: 64 KB of rows)
constexpr uint32_t kBkTile = RP_BK_TILE;                       // changes per scatter tile
constexpr uint32_t kBkMin = 1u << 19;                          // changes from which a batch takes the bucket path
constexpr uint32_t kBkMaxBuckets = 2048;                       // (LDS of the scatter tiles): 8M ids
// The checksum slot pool's limits: slots, slots hashed by one launch, groups in flight.
constexpr uint32_t kMaxSlots = 1024, kGroupSlots = 512, kMaxGroups = 4;

// Every environment variable of Membership.update and its checksum (A/B and diagnostics; none is
// API). members_knobs() is their only reader. A handle reads them when it is created and again at
// the top of every update, set and checksum call, and keeps the value: the tests change them
// between the batches of one handle.
struct MemberKnobs {
    // RP_MEMBERS_SORTED_FOLD=1: radix sort + k_fold for every batch (on unless unset, empty or starting with '0')
    bool sorted_fold;
    // RP_MEMBERS_BUCKET_FOLD=0|1: the bucket path off | on, by the first character (-1, unset or empty: from kBkMin changes)
    int bucket_fold;
    // RP_MEMBERS_FUSE=1: k_link_fold for a grid resident at once; C3 fold 0.098-0.102 against 0.021 ms, batch 115-119 against 39 us (r04s)
    bool fuse;
    // RP_MEMBERS_SIDE_BUILD=0|1: the string inline | on a build stream (0.0410 -> 0.0369 ms per C3 batch, r06e); anything else: 2, deferred
    int side_build;
    // RP_MEMBERS_CK_BYTES: the slot pool's bytes (6 GiB: 0.0384 -> 0.0311 ms per C3 batch against 2 GiB, r06j; 1 GiB: 51.4 against 45.2 us, r04e)
    uint64_t ck_bytes;
    // RP_MEMBERS_GROUP_SLOTS: strings hashed by one launch (512; groups of 64 gave 0.86 against 1.00-1.07 G updates/s)
    uint32_t group_slots;
    // RP_BK_REC8=0: 12-B scatter records always (off only for exactly "0")
    bool rec8;
    // RP_BK_DIRECT=0: k_bk_fold keeps its 2-bit map and k_bk_gather runs (off only for exactly "0")
    bool direct;
    // RP_BK_SGRID: workgroups of the scatter, each looping over tiles (0, unset or no positive number: one tile each)
    uint32_t sgrid;
    // RP_BK_PROF_PRINT set at all: k_bk_fold's cycle counters on stderr (-DRP_BK_PROF builds only)
    bool prof_print;
};

inline MemberKnobs members_knobs() {
    const auto first = [](const char* name) {  // the first character; 0 when unset or empty
        const char* e = getenv(name);
        return e ? *e : '\0';
    };
    const auto not_zero = [](const char* name) {  // off only for exactly "0"
        const char* e = getenv(name);
        return !(e && e[0] == '0' && e[1] == '\0');
    };
    const auto pos = [](const char* name, uint64_t dflt) {  // a positive decimal, else dflt
        const char* e = getenv(name);
        if (!e || !*e) return dflt;
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        return (end && *end == 0 && v > 0) ? (uint64_t)v : dflt;
    };
    MemberKnobs k;
    char c = first("RP_MEMBERS_SORTED_FOLD");
    k.sorted_fold = c && c != '0';
    c = first("RP_MEMBERS_BUCKET_FOLD");
    k.bucket_fold = !c ? -1 : c != '0';
    k.fuse = first("RP_MEMBERS_FUSE") == '1';
    c = first("RP_MEMBERS_SIDE_BUILD");
    k.side_build = c == '0' || c == '1' ? c - '0' : 2;
    k.ck_bytes = pos("RP_MEMBERS_CK_BYTES", 6ull << 30);
    k.group_slots = (uint32_t)pos("RP_MEMBERS_GROUP_SLOTS", kGroupSlots);
    k.rec8 = not_zero("RP_BK_REC8");
    k.direct = not_zero("RP_BK_DIRECT");
    k.sgrid = (uint32_t)pos("RP_BK_SGRID", 0);
    k.prof_print = getenv("RP_BK_PROF_PRINT") != nullptr;
    return k;
}

// The key bits the radix sort of a batch's ids covers: whole bytes that hold every interned id.
inline int sort_bits(uint64_t names) {
    int bits = 8;
    while (bits < 32 && (1ull << bits) < names) bits += 8;
    return bits;
}

enum class FoldPath : uint8_t {
    Empty,    // nothing to fold: no changes, or a range past the table
    Bucket,   // k_bk_scatter + k_bk_fold (+ k_bk_gather): large batches, and every ranged one
    Grouped,  // k_link + k_fold_fast, or k_link_fold when fusing
    Sorted,   // radix sort + k_fold
};

// What one batch of k changes launches on a table of cap ids.
struct FoldPlan {
    FoldPath path;
    uint32_t nb, b_lo, b_hi;  // the table's buckets, and the ones this batch folds: [b_lo, b_hi)
    uint32_t ntiles;          // scatter tiles of kBkTile changes
    uint32_t sgrid;           // the scatter's workgroups, each looping over tiles; 0: one tile each
    bool rec8;                // the scatter may store 8-B records (and the per-tile bases they need)
    bool direct;              // k_bk_fold writes the applied flags itself
    bool gather;              // else k_bk_gather writes them from its map (when the caller asks for flags)
    bool fuse;                // k_link_fold is wanted; the host still asks whether its grid is resident at once
    int bits;                 // the radix sort's key bits
    uint32_t nparts;          // partial applied counts for the overflow step to sum: buckets, or k_link's workgroups
    bool drain;               // a deferred checksum string is written by its own launch first
};

// Whether a batch may take the bucket path: no damp scoring (k_bk_fold does not score), no sorted
// fold, a table of at most kBkMaxBuckets buckets, a batch index that leaves the record's two status
// bits free.
inline bool bucket_can(const MemberKnobs& kn, uint32_t k, uint32_t nb, bool damp_on) {
    return !damp_on && nb <= kBkMaxBuckets && k < (1u << 29) && !kn.sorted_fold;
}

// A ranged batch (rp_members_update_range_dev) folds only whole buckets and so needs the bucket
// path: where it cannot take it the plan names the path a whole-table batch would take, and the
// caller refuses. pw_on: a deferred string is pending; pw_same_stream: on this batch's stream.
inline FoldPlan fold_plan(const MemberKnobs& kn, uint32_t k, uint32_t cap, uint64_t names, bool damp_on, bool ranged,
                          uint32_t id_lo, uint32_t id_hi, bool pw_on, bool pw_same_stream) {
    FoldPlan p{};
    p.nb = (uint32_t)(((uint64_t)cap + kBk - 1) / kBk);
    p.b_lo = ranged ? std::min(p.nb, id_lo / kBk) : 0u;
    p.b_hi = ranged ? (uint32_t)std::min<uint64_t>(p.nb, ((uint64_t)id_hi + kBk - 1) / kBk) : p.nb;
    const bool can = bucket_can(kn, k, p.nb, damp_on);
    const bool bucket = can && (ranged || (kn.bucket_fold >= 0 ? kn.bucket_fold != 0 : k >= kBkMin));
    const bool empty = ranged ? can && (!k || p.b_lo >= p.b_hi) : !k;
    p.path = empty             ? FoldPath::Empty
             : bucket          ? FoldPath::Bucket
             : kn.sorted_fold  ? FoldPath::Sorted
                               : FoldPath::Grouped;
    if (!k) return p;  // an empty batch launches nothing and leaves a deferred string pending
    // only the grouped fold's launch (k_fold_fast_mck) carries a deferred string
    p.drain = pw_on && (ranged || !pw_same_stream || p.path != FoldPath::Grouped || kn.fuse);
    if (p.path == FoldPath::Bucket) {
        p.ntiles = (k + kBkTile - 1) / kBkTile;
        p.sgrid = kn.sgrid && kn.sgrid < p.ntiles ? kn.sgrid : 0u;
        p.rec8 = kn.rec8;
        p.direct = ranged || kn.direct;  // a ranged batch has no map of the other ranks' buckets
        p.gather = !p.direct;
        p.nparts = p.nb;
    } else if (p.path == FoldPath::Grouped) {
        p.nparts = (k + 255) / 256;
        p.fuse = kn.fuse;
    } else if (p.path == FoldPath::Sorted) {
        p.bits = sort_bits(names);
    }
    return p;
}

// The checksum slot pool for strings of `need` bytes: what fits the budget, in groups of at most
// half the slots, so that one group's chains run while the next group's strings are built.
struct CkPool {
    uint32_t nslots, group_slots, ngroups;
};
inline CkPool ck_pool(uint64_t need, const MemberKnobs& kn) {
    CkPool p;
    p.nslots = (uint32_t)std::min<uint64_t>(kMaxSlots, std::max<uint64_t>(1, kn.ck_bytes / need));
    p.group_slots = std::max<uint32_t>(1, std::min<uint32_t>(kn.group_slots, p.nslots / 2));
    p.ngroups = std::max<uint32_t>(1, std::min<uint32_t>(kMaxGroups, p.nslots / p.group_slots));
    return p;
}

// Where a checksum string is written (Members::checksum_dev): 2 deferred into the next batch's
// fold launch, 1 on the build stream, 0 inline. Only an update batch's string, whose length launch
// carries the overflow step and takes the row snapshot, can leave the caller's stream.
inline int string_mode(const MemberKnobs& kn, bool has_overflow_args) { return has_overflow_args ? kn.side_build : 0; }

}  // namespace rp
