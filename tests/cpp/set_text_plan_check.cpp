// The set rows of rpvg_amd/csrc/set_text_plan.hpp on the CPU: both kinds at ploidy 1, 2, 3 and 8 against rows built with snprintf, the
// lengths of the measure pass against the bytes of the write pass, and the write kernel's wavefront (writeSetsKernel, set_text.hip)
// walked lane by lane — the name slots into the staging block, the block leaving when it is full, the number cells as one step,
// flushPlan — with a counter behind every byte of the text: every byte of a row is stored exactly once and no byte outside it is
// touched, at every residue of the row's start modulo 4.  Names of 0 to 4000 bytes: longer than one step, several of them in a row.
// Prints "ok".
#define RPVG_NUMBER_TEXT_CHECKED 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "set_text_plan.hpp"

using namespace rpvg_set_text;
using rpvg_table_text::FlushPlan;
using rpvg_table_text::flushPlan;

namespace {

void require(const bool condition, const char * what) {
    if (!condition) {
        std::printf("failed: %s\n", what);
        std::exit(1);
    }
}

std::string g(const double v, const int precision) {
    char text[64];
    std::snprintf(text, sizeof(text), "%.*g", precision, v);
    return text;
}

// the write kernel's row loop with the 64 lanes one after the other; stores[i]: how often byte i of the text was stored
void waveWrite(const SetRows & t, const uint64_t s, const uint64_t begin, const uint64_t end, std::vector<char> & text, std::vector<int> & stores) {
    if (begin >= end) return;
    std::vector<char> stage((kStageBytes + 15) & ~15, '?');
    const SetRow row = setRow(t, s);
    uint64_t base = begin & ~3ull;
    uint32_t lo = static_cast<uint32_t>(begin & 3u), hi = lo;
    const auto flush = [&](const bool last) {
        require(hi <= static_cast<uint32_t>(kStageBytes), "a step fits the staging block");
        const FlushPlan p = flushPlan(lo, hi);
        const auto store = [&](const uint32_t i) {
            require(i >= lo && i < hi, "a stored byte is a filled byte of the block");
            text[base + i] = stage[i];
            stores[base + i] += 1;
        };
        for (uint32_t i = lo; i < p.head_end; ++i) store(i);
        for (uint32_t w = p.first_word; w < p.end_word; ++w) {
            require((base + 4 * w) % 4 == 0, "a word store is aligned");
            for (uint32_t b = 0; b < 4; ++b) store(4 * w + b);
        }
        require(hi - p.tail_begin <= 3 || (lo > 0 && hi < 4), "at most three bytes are left behind the words");
        if (last) {
            for (uint32_t i = p.tail_begin; i < hi; ++i) store(i);
            return;
        }
        std::vector<char> carried(stage.begin() + p.tail_begin, stage.begin() + hi);
        for (size_t i = 0; i < carried.size(); ++i) stage[p.next_lo + i] = carried[i];
        base += p.advance;
        lo = p.next_lo;
        hi = p.next_hi;
    };
    for (uint32_t j = 0; j < t.ploidy; ++j) {
        const NameSlot slot = nameSlot(t, row, j);
        const uint64_t bytes = slotBytes(slot);
        uint64_t done = 0;
        while (done < bytes) {
            const uint32_t piece = pieceOf(bytes - done, hi);
            if (piece == 0) {
                flush(false);
                require(hi < 4, "a full block leaves but for a ragged word");
                continue;
            }
            for (uint32_t lane = 0; lane < 64; ++lane) {
                for (uint32_t i = lane; i < piece; i += 64) stage[hi + i] = slotByte(t, slot, done + i);
            }
            hi += piece;
            done += piece;
        }
    }
    if (numbersNeedFlush(t, hi)) flush(false);
    const uint32_t cells = numberCells(t);
    require(cells <= 64, "the number cells are one step");
    uint32_t total = 0;
    for (uint32_t lane = 0; lane < cells; ++lane) {
        const Cell cell = cellOf(t, row, lane);
        const uint32_t bytes = cellText<false>(cell, t.precision, nullptr);
        require(bytes <= static_cast<uint32_t>(kMaxCellBytes), "a cell fits its share of the block");
        require(hi + total + bytes <= static_cast<uint32_t>(kStageBytes), "the number cells fit the block");
        require(cellText<true>(cell, t.precision, stage.data() + hi + total) == bytes, "a cell is as long as it was measured");
        total += bytes;
    }
    hi += total;
    flush(true);
}

void checkDescriptor(const SetRows & t, const std::vector<std::string> & want_rows, const char * what) {
    std::vector<uint64_t> row_off(t.num_sets + 1, 0);
    uint64_t exact = 0;
    for (uint64_t s = 0; s < t.num_sets; ++s) {
        const uint64_t bytes = rowBytes(t, s, &exact);
        if (bytes != want_rows[s].size()) {
            std::printf("%s: set %llu measures %llu bytes, the reference row has %zu\n", what, static_cast<unsigned long long>(s), static_cast<unsigned long long>(bytes), want_rows[s].size());
            std::exit(1);
        }
        row_off[s + 1] = row_off[s] + bytes;
        std::string got(bytes + 2, '#');
        require(rowWrite(t, s, &got[1]) == bytes && got[0] == '#' && got[bytes + 1] == '#', "rowWrite writes the measured bytes and no other");
        if (got.substr(1, bytes) != want_rows[s]) {
            std::printf("%s: set %llu is \"%s\", the reference row \"%s\"\n", what, static_cast<unsigned long long>(s), got.substr(1, bytes).c_str(), want_rows[s].c_str());
            std::exit(1);
        }
    }
    for (uint64_t shift = 0; shift < 4; ++shift) {
        const uint64_t total = row_off[t.num_sets];
        std::vector<char> text(64 + shift + total + 64 + 8, '#');
        std::vector<int> stores(text.size(), 0);
        for (uint64_t s = 0; s < t.num_sets; ++s) waveWrite(t, s, 64 + shift + row_off[s], 64 + shift + row_off[s + 1], text, stores);
        std::string want;
        for (const auto & row : want_rows) want += row;
        for (uint64_t i = 0; i < text.size(); ++i) {
            const bool inside = i >= 64 + shift && i < 64 + shift + total;
            if (stores[i] != (inside ? 1 : 0) || (inside && text[i] != want[i - 64 - shift])) {
                std::printf("%s: byte %llu of the text at alignment %llu was stored %d times\n", what, static_cast<unsigned long long>(i), static_cast<unsigned long long>(shift), stores[i]);
                std::exit(1);
            }
        }
    }
}

}  // namespace

int main() {
    std::vector<uint64_t> pow10(rpvg_number_text::kPow10Words);
    rpvg_number_text::buildPow10Table(pow10.data(), nullptr);

    // three clusters of 4, 0 and 5 paths; names of 0, 1, 3, 4, 26, 27, 255, 1700 and 4000 bytes (the last two longer than the block)
    const std::vector<std::string> names = {"", "a", "abc", "abcd", std::string(26, 'x'), std::string(27, 'y'), std::string(255, 'z'), std::string(1700, 'n'), std::string(4000, 'm')};
    const std::vector<uint64_t> cluster_path_off = {0, 4, 4, 9};
    const std::vector<uint32_t> cluster_id = {1, 77, 4000000000u};
    std::vector<uint64_t> name_off = {0};
    std::string name_bytes;
    for (const auto & name : names) {
        name_bytes += name;
        name_off.push_back(name_bytes.size());
    }
    const double quiet_nan = std::nan("");
    const std::vector<double> hard = {123456785.0, 123456795.0, 99999999.5, -0.0, 5e-324, 1e-5, -1.2345678901234567e-308, 10000000.5, 10000001.5, 0.1, 1e22, 3.0,
                                      std::numeric_limits<double>::infinity(), 0.0, 1.0 / 3.0};

    for (const uint32_t ploidy : {1u, 2u, 3u, 8u}) {
        // the sets: every size 1 .. ploidy in both clusters that have paths, members unsorted and repeated, the long names together
        std::vector<uint64_t> set_off = {0}, member_off = {0}, abund_off = {5};  // (five abundances of nobody in front: the base is not 0)
        std::vector<uint32_t> members;
        std::vector<double> posteriors, abundances = {-1, -2, -3, -4, -5}, member_tpm;
        std::vector<uint32_t> cluster_of_set;
        uint64_t salt = ploidy;
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t paths = static_cast<uint32_t>(cluster_path_off[k + 1] - cluster_path_off[k]);
            for (uint32_t n = 1; paths > 0 && n <= ploidy; ++n) {
                for (uint32_t variant = 0; variant < 3; ++variant) {
                    for (uint32_t j = 0; j < n; ++j) {
                        const uint32_t member = variant == 0 ? (paths - 1 - (j * 3 + n) % paths) : (variant == 1 ? paths - 1 : (j % 2 == 0 ? 1 : 0));
                        members.push_back(member);
                        salt += 1;
                        abundances.push_back(hard[salt % hard.size()] * (salt % 3 == 0 ? 1.0 : 0.5 + static_cast<double>(salt)));
                        member_tpm.push_back(hard[(salt * 5) % hard.size()]);
                    }
                    member_off.push_back(members.size());
                    posteriors.push_back(hard[(salt * 7) % hard.size()]);
                    cluster_of_set.push_back(k);
                }
            }
            set_off.push_back(posteriors.size());
            abund_off.push_back(abundances.size());
        }
        const uint64_t S = posteriors.size();
        posteriors[0] = quiet_nan;       // printed
        posteriors[S - 1] = -quiet_nan;  // printed
        posteriors[1] = 0.25;            // == min_posterior below: printed
        posteriors[2] = std::nextafter(0.25, 0.0);  // dropped
        for (const int precision : {8, 17, 1}) {
            for (const bool joint : {true, false}) {
                for (const double min_posterior : {0.25, 0.0}) {
                    SetRows t = {};
                    t.num_sets = S;
                    t.num_clusters = 3;
                    t.ploidy = ploidy;
                    t.joint = joint;
                    t.name_off = name_off.data();
                    t.name_bytes = name_bytes.data();
                    t.cluster_path_off = cluster_path_off.data();
                    t.cluster_id = cluster_id.data();
                    t.set_off = set_off.data();
                    t.member_off = member_off.data();
                    t.members = members.data();
                    t.posteriors = posteriors.data();
                    t.abund_off = joint ? abund_off.data() : nullptr;
                    t.abundances = joint ? abundances.data() : nullptr;
                    t.member_tpm = joint ? member_tpm.data() : nullptr;
                    t.min_posterior = min_posterior;
                    t.precision = precision;
                    t.pow10 = pow10.data();
                    require(descriptorBad(t) == nullptr, "the descriptor is accepted");
                    require(numCells(t) == ploidy + 2 + (joint ? 2 * ploidy : 0), "the cells of a row");
                    std::vector<std::string> want;
                    uint64_t printed_rows = 0;
                    for (uint64_t s = 0; s < S; ++s) {
                        std::string row;
                        require(clusterOf(t, s) == cluster_of_set[s], "the cluster of a set");
                        if (!(posteriors[s] < min_posterior)) {
                            const uint32_t k = cluster_of_set[s];
                            const uint64_t m0 = member_off[s], m1 = member_off[s + 1];
                            for (uint64_t m = m0; m < m1; ++m) row += names[cluster_path_off[k] + members[m]] + "\t";
                            for (uint64_t j = m1 - m0; j < ploidy; ++j) row += ".\t";
                            row += std::to_string(cluster_id[k]) + "\t" + g(posteriors[s], precision);
                            if (joint) {
                                for (uint64_t m = m0; m < m1; ++m) row += "\t" + g(abundances[abund_off[k] + m - member_off[set_off[k]]], precision) + "\t" + g(member_tpm[m], precision);
                                for (uint64_t j = m1 - m0; j < ploidy; ++j) row += "\t0\t0";
                            }
                            row += "\n";
                            printed_rows += 1;
                        }
                        want.push_back(row);
                    }
                    require(want[1].size() > 0 && (min_posterior == 0.0 ? want[2].size() > 0 : want[2].empty()), "the filter at min_posterior and one below it");
                    require(want[0].find("nan") != std::string::npos && want[S - 1].find("-nan") != std::string::npos, "a NaN posterior is printed");
                    require(printed_rows >= 3, "rows are printed");
                    checkDescriptor(t, want, joint ? "joint" : "posterior");
                }
            }
        }
    }

    SetRows bad = {};
    bad.precision = 8;
    bad.ploidy = 0;
    require(descriptorBad(bad) != nullptr, "ploidy 0 is refused");
    bad.ploidy = 9;
    require(descriptorBad(bad) != nullptr, "ploidy 9 is refused");
    bad.ploidy = 8;
    require(descriptorBad(bad) == nullptr, "an empty descriptor is accepted");
    bad.precision = 0;
    require(descriptorBad(bad) != nullptr, "precision 0 is refused");
    bad.precision = 18;
    require(descriptorBad(bad) != nullptr, "precision 18 is refused");
    bad.precision = 17;
    bad.num_sets = 1;
    require(descriptorBad(bad) != nullptr, "sets without clusters are refused");
    std::printf("ok\n");
    return 0;
}
