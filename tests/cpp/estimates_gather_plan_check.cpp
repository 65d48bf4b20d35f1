// The rules of the resident-estimates gather (rpvg_amd/csrc/estimates_gather_plan.hpp) on the host: gatherModel on a hand-written case
// of both forms with every output array written out, every refusal with the smallest offending (part, unit) reported when two are
// planted.  Every array lives on the heap exactly as long as the part's sizes say, so an index used before it is checked trips the
// address sanitizer.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "estimates_gather_plan.hpp"

using namespace rpvg_gather;
using rpvg_hip_detail::kNoBad;
using rpvg_hip_detail::offenderOf;
using rpvg_hip_detail::offenderWord;
using rpvg_hip_detail::word64;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {

constexpr uint32_t NO = kNoMember;

struct OwnedPart {
    uint32_t width = 0;
    std::vector<uint32_t> unit_cluster, set_count, set_first, set_second, set_size, set_member;
    std::vector<uint64_t> subset_off, path_off;
    std::vector<double> cluster_noise_count, set_posterior, set_abundance;
    uint64_t num_slots = 0;  // what the part says (path_off may be broken on purpose)
    HostPart host() const {
        HostPart h;
        h.part.num_units = static_cast<uint32_t>(unit_cluster.size());
        h.part.width = width;
        h.part.num_subsets = path_off.size() - 1;
        h.part.num_slots = num_slots;
        h.part.subset_off = subset_off.data();
        h.part.path_off = path_off.data();
        h.part.set_count = set_count.data();
        h.part.cluster_noise_count = cluster_noise_count.data();
        h.part.set_posterior = set_posterior.data();
        h.part.set_first = set_first.data();
        h.part.set_second = set_second.data();
        h.part.set_size = set_size.data();
        h.part.set_member = set_member.data();
        h.part.set_abundance = set_abundance.data();
        h.unit_cluster = unit_cluster.data();
        return h;
    }
};

struct Case {
    std::vector<uint64_t> cluster_path_off{0, 3, 5, 9, 10};  // clusters of 3, 2, 4 and 1 paths
    std::vector<double> total{10.0, 20.0, 30.0, 40.0};
    OwnedPart a, b;
    Case() {
        // part 0, the diploid form: unit 0 is cluster 2 (two subsets, five slots, three sets), unit 1 is cluster 0 (no subset)
        a.width = 0;
        a.unit_cluster = {2, 0};
        a.subset_off = {0, 2, 2};
        a.path_off = {0, 2, 5};
        a.num_slots = 5;
        a.set_count = {3, 0};
        a.cluster_noise_count = {7.0, 8.0};
        a.set_first = {1, 0, 3, 9, 9};
        a.set_second = {NO, 2, 3, 9, 9};
        a.set_posterior = {0.5, 0.25, 0.125, -1.0, -1.0};
        a.set_abundance = {1.5, 99.0, 2.5, 3.5, 4.5, 5.5, -1.0, -1.0, -1.0, -1.0};
        // part 1, width 3: unit 0 is cluster 3 (one subset, four slots, two sets: one member, then three times path 0)
        b.width = 3;
        b.unit_cluster = {3};
        b.subset_off = {0, 1};
        b.path_off = {0, 4};
        b.num_slots = 4;
        b.set_count = {2};
        b.cluster_noise_count = {0.75};
        b.set_size = {1, 3, 7, 7};
        b.set_member = {0, NO, NO, 0, 0, 0, 5, 5, 5, 5, 5, 5};
        b.set_posterior = {0.0625, 0.03125, -1.0, -1.0};
        b.set_abundance = {6.5, 0.0, 0.0, 7.5, 8.5, 9.5, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0};
    }
    word64 run(FlatArrays & out) const {
        const HostPart parts[2] = {a.host(), b.host()};
        return gatherModel(4, cluster_path_off.data(), total.data(), parts, 2, out);
    }
};

void expectRefusal(const Case & c, const uint64_t g, const int why) {
    FlatArrays out;
    const word64 bad = c.run(out);
    CHECK(bad != kNoBad);
    const auto o = offenderOf(bad, kBadMember);
    if (o.second_kind || o.index != g || o.why != why) {
        std::printf("offender (%llu, %d), expected (%llu, %d)\n", static_cast<unsigned long long>(o.index), o.why, static_cast<unsigned long long>(g), why);
        std::exit(1);
    }
    CHECK(out.set_off.empty() && out.noise_count.empty());
}

void handCase() {
    const Case c;
    FlatArrays out;
    CHECK(c.run(out) == kNoBad);
    // cluster 0: a unit without subsets (no sets, its total as noise); cluster 1: in no unit; cluster 2: part 0's unit 0; cluster 3: part 1's
    CHECK((out.set_off == std::vector<uint64_t>{0, 0, 0, 3, 5}));
    CHECK((out.member_off == std::vector<uint64_t>{0, 1, 3, 5, 6, 9}));
    CHECK((out.members == std::vector<uint32_t>{1, 0, 2, 3, 3, 0, 0, 0, 0}));
    CHECK((out.posteriors == std::vector<double>{0.5, 0.25, 0.125, 0.0625, 0.03125}));
    CHECK((out.abund_off == std::vector<uint64_t>{0, 0, 0, 5, 9}));
    CHECK((out.abundances == std::vector<double>{1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5}));
    CHECK((out.noise_count == std::vector<double>{10.0, 20.0, 7.0, 0.75}));
    for (size_t k = 0; k + 1 < out.set_off.size(); ++k) CHECK(out.abund_off[k] == out.member_off[out.set_off[k]]);

    // no part at all, and no cluster at all
    FlatArrays none;
    CHECK(gatherModel(4, c.cluster_path_off.data(), c.total.data(), nullptr, 0, none) == kNoBad);
    CHECK((none.set_off == std::vector<uint64_t>{0, 0, 0, 0, 0}) && none.members.empty() && (none.noise_count == c.total));
    CHECK((none.member_off == std::vector<uint64_t>{0}));
    const uint64_t zero = 0;
    CHECK(gatherModel(0, &zero, nullptr, nullptr, 0, none) == kNoBad);
    CHECK((none.set_off == std::vector<uint64_t>{0}) && (none.abund_off == std::vector<uint64_t>{0}) && none.noise_count.empty());
}

void slotRules() {
    CHECK(cellsPerSlot(0) == 2 && cellsPerSlot(1) == 1 && cellsPerSlot(8) == 8 && maxSetSize(0) == 2 && maxSetSize(3) == 3);
    const Case c;
    const HostPart a = c.a.host(), b = c.b.host();
    CHECK(slotSize(a.part, 0) == 1 && slotSize(a.part, 1) == 2 && slotMember(a.part, 1, 1) == 2 && slotAbundance(a.part, 2, 1) == 5.5);
    CHECK(slotSize(b.part, 1) == 3 && slotMember(b.part, 0, 0) == 0 && slotAbundance(b.part, 1, 2) == 9.5);
    uint32_t n = 0;
    CHECK(slotOffence(a.part, 1, 4, &n) == 0 && n == 2);
    CHECK(slotOffence(a.part, 1, 2, &n) == kBadMember);  // member 2 of a cluster of two paths
    CHECK(slotOffence(b.part, 2, 9, &n) == kBadSetSize);
    CHECK(unitNoise(a.part, 0, 30.0) == 7.0 && unitNoise(a.part, 1, 10.0) == 10.0);
}

void refusals() {
    {   // unit_cluster >= K
        Case c;
        c.b.unit_cluster[0] = 4;
        expectRefusal(c, 2, kBadUnitCluster);
        c.a.unit_cluster[1] = 77;  // ... and a smaller offender
        expectRefusal(c, 1, kBadUnitCluster);
    }
    {   // a cluster listed by two units: the first of them is named
        Case c;
        c.b.unit_cluster[0] = 0;
        expectRefusal(c, 1, kBadDuplicate);
        c.b.unit_cluster[0] = 2;
        expectRefusal(c, 0, kBadDuplicate);
    }
    {   // subset_off
        Case c;
        c.a.subset_off = {0, 3, 2};  // beyond S, and decreasing
        expectRefusal(c, 0, kBadSubsetOff);
        c.a.subset_off = {0, 2, 1};  // does not end at S: unit 1
        expectRefusal(c, 1, kBadSubsetOff);
        c.a.subset_off = {1, 2, 2};  // does not begin at 0
        expectRefusal(c, 0, kBadSubsetOff);
    }
    {   // path_off
        Case c;
        c.a.path_off = {0, 6, 5};
        expectRefusal(c, 0, kBadPathOff);
        c.a.path_off = {0, 2, 4};  // does not end at L
        expectRefusal(c, 0, kBadPathOff);
        Case d;
        d.b.path_off = {1, 4};
        expectRefusal(d, 2, kBadPathOff);
    }
    {   // set_count beyond the unit's slots; a unit without subsets has none
        Case c;
        c.a.set_count[0] = 6;
        expectRefusal(c, 0, kBadSetCount);
        Case d;
        d.a.set_count[1] = 1;
        expectRefusal(d, 1, kBadSetCount);
        d.a.set_count[0] = 6;  // two planted: the smaller unit
        expectRefusal(d, 0, kBadSetCount);
    }
    {   // set sizes
        Case c;
        c.b.set_size[1] = 4;
        expectRefusal(c, 2, kBadSetSize);
        c.b.set_size[1] = 0;
        expectRefusal(c, 2, kBadSetSize);
        c.b.set_size[1] = 3;
        c.b.set_size[3] = 0;  // beyond set_count: not looked at
        FlatArrays out;
        CHECK(c.run(out) == kNoBad);
    }
    {   // members
        Case c;
        c.a.set_second[1] = 4;  // cluster 2 has four paths
        expectRefusal(c, 0, kBadMember);
        Case d;
        d.b.set_member[4] = 1;  // cluster 3 has one
        expectRefusal(d, 2, kBadMember);
        d.b.set_size[0] = 9;    // a bad size anywhere in the unit comes first
        expectRefusal(d, 2, kBadSetSize);
        d.a.set_first[2] = 4;   // two units offend: the smaller one
        expectRefusal(d, 0, kBadMember);
        Case e;
        e.b.set_member[1] = 0;  // a cell beyond the set's size is never a member
        e.b.set_member[2] = 1;
        FlatArrays out;
        CHECK(e.run(out) == kNoBad);
    }
    {   // width
        Case c;
        c.b.width = 9;
        FlatArrays out;
        const word64 bad = c.run(out);
        const auto o = offenderOf(bad, kBadWidth);
        CHECK(bad != kNoBad && o.second_kind && o.index == 1 && o.why == kBadWidth);
    }
    {   // a reason for every offence, in the reporting order
        for (int why = kBadUnitCluster; why <= kBadMember; ++why) CHECK(reasonOf(why)[0] != 0);
        CHECK(reasonOf(0)[0] == 0 && reasonOf(kBadMember + 1)[0] == 0);
        CHECK(offenderWord(3, kBadMember) < offenderWord(4, kBadUnitCluster) && offenderWord(3, kBadDuplicate) < offenderWord(3, kBadSubsetOff));
    }
}

}  // namespace

int main() {
    slotRules();
    handCase();
    refusals();
    std::printf("ok\n");
    return 0;
}
