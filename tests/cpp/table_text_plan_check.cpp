// The row descriptor of rpvg_amd/csrc/table_text_plan.hpp on the CPU: the three files as three descriptors against rows built with
// snprintf, the lengths of the measure pass against the bytes of the write pass, and the write kernel's wavefront walked lane by lane
// (the staging block, flushPlan) with a counter behind every byte of the text: every byte of a row is stored exactly once and no
// byte outside it is touched, for every alignment of the row's start.  Prints "ok".
#define RPVG_NUMBER_TEXT_CHECKED 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "table_text_plan.hpp"

using namespace rpvg_table_text;

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

struct Arrays {
    std::vector<uint64_t> name_off, cluster_path_off, abund_off, member_base;
    std::string name_bytes;
    std::vector<uint32_t> cluster_id, length;
    std::vector<double> eff, abundances, member_tpm, prob, count, tpm, samples;
    std::vector<uint8_t> listed;
    std::vector<uint64_t> pow10;
};

// the write kernel's row loop with the 64 lanes one after the other; stores[i]: how often byte i of the text was stored
void waveWrite(const TextRows & t, const uint64_t r, const uint64_t begin, const uint64_t end, std::vector<char> & text, std::vector<int> & stores) {
    if (begin >= end) return;
    std::vector<char> stage((kStageBytes + 15) & ~15, '?');
    const uint64_t k = clusterOf(t, r), cells = numCells(t), name = nameBytes(t, r);
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
        require(p.advance % 4 == 0 && p.next_hi - p.next_lo == hi - p.tail_begin, "the carried bytes keep their number and their alignment");
        base += p.advance;
        lo = p.next_lo;
        hi = p.next_hi;
    };
    const uint64_t piece_bytes = static_cast<uint64_t>(kStepCells) * kMaxCellBytes;
    for (uint64_t done = 0; done < name; done += piece_bytes) {
        const uint32_t piece = static_cast<uint32_t>(name - done < piece_bytes ? name - done : piece_bytes);
        for (uint32_t i = 0; i < piece; ++i) stage[hi + i] = t.name_bytes[t.name_off[r] + done + i];
        hi += piece;
        flush(false);
    }
    for (uint64_t c0 = 0; c0 < cells; c0 += kStepCells) {
        uint32_t total = 0;
        for (uint64_t c = c0; c < cells && c < c0 + kStepCells; ++c) {
            const Cell cell = cellOf(t, r, k, c);
            const uint32_t bytes = cellText<false>(cell, t.precision, nullptr);
            require(bytes <= static_cast<uint32_t>(kMaxCellBytes), "a cell fits its share of the block");
            require(cellText<true>(cell, t.precision, stage.data() + hi + total) == bytes, "a cell is as long as it was measured");
            total += bytes;
        }
        hi += total;
        flush(c0 + kStepCells >= cells);
    }
}

void checkDescriptor(const TextRows & t, const std::vector<std::string> & want_rows, const char * what) {
    std::vector<uint64_t> row_off(t.num_rows + 1, 0);
    uint64_t exact = 0;
    for (uint64_t r = 0; r < t.num_rows; ++r) {
        const uint64_t bytes = rowBytes(t, r, &exact);
        if (bytes != want_rows[r].size()) {
            std::printf("%s: row %llu measures %llu bytes, the reference row has %zu\n", what, static_cast<unsigned long long>(r), static_cast<unsigned long long>(bytes), want_rows[r].size());
            std::exit(1);
        }
        row_off[r + 1] = row_off[r] + bytes;
        std::string got(bytes + 2, '#');
        require(rowWrite(t, r, &got[1]) == bytes && got[0] == '#' && got[bytes + 1] == '#', "rowWrite writes the measured bytes and no other");
        if (got.substr(1, bytes) != want_rows[r]) {
            std::printf("%s: row %llu is \"%s\", the reference row \"%s\"\n", what, static_cast<unsigned long long>(r), got.substr(1, bytes).c_str(), want_rows[r].c_str());
            std::exit(1);
        }
    }
    // the wavefront's walk at every alignment of the text's start, guards of 64 bytes around it
    for (uint64_t shift = 0; shift < 4; ++shift) {
        const uint64_t total = row_off[t.num_rows];
        std::vector<char> text(64 + shift + total + 64 + 8, '#');
        std::vector<int> stores(text.size(), 0);
        for (uint64_t r = 0; r < t.num_rows; ++r) waveWrite(t, r, 64 + shift + row_off[r], 64 + shift + row_off[r + 1], text, stores);
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
    Arrays a;
    a.pow10.resize(rpvg_number_text::kPow10Words);
    rpvg_number_text::buildPow10Table(a.pow10.data(), nullptr);

    // three clusters of 3, 0 and 2 paths; names of 0, 1, 3, 4 and 1700 bytes (the last longer than a step of the block)
    const std::vector<std::string> names = {"", "a", "abc", "abcd", std::string(1700, 'n')};
    a.cluster_path_off = {0, 3, 3, 5};
    a.cluster_id = {1, 4000000000u, 30};
    a.length = {0, 9, 10, 4294967295u, 1234};
    a.name_off = {0};
    for (const auto & name : names) {
        a.name_bytes += name;
        a.name_off.push_back(a.name_bytes.size());
    }
    const uint64_t P = names.size();
    const std::vector<double> hard = {123456785.0, 123456795.0, 99999999.5, -0.0, 5e-324, 1e-5, -1.2345678901234567e-308, 10000000.5, 10000001.5, 0.1, 1e22, 3.0};
    for (const int precision : {8, 17, 1}) {
        for (const uint64_t N : {1ull, 2ull, 62ull, 63ull, 64ull, 65ull, 130ull}) {
            a.samples.assign(P * N, 0.0);
            for (uint64_t i = 0; i < P * N; ++i) a.samples[i] = hard[(i * 7 + N) % hard.size()] * (i % 3 == 0 ? 1.0 : 0.5 + static_cast<double>(i));
            a.listed = {1, 0, 1, 1, 1};
            TextRows t = {};
            t.num_rows = P;
            t.num_clusters = 3;
            t.name_off = a.name_off.data();
            t.name_bytes = a.name_bytes.data();
            t.cluster_path_off = a.cluster_path_off.data();
            t.cluster_id = a.cluster_id.data();
            t.run_length = N;
            t.run = a.samples.data();
            t.run_stride = N;
            t.filter = a.listed.data();
            t.precision = precision;
            t.pow10 = a.pow10.data();
            require(descriptorBad(t) == nullptr, "the Gibbs descriptor is accepted");
            require(measuredByWavefront(t) == (N + 1 > kNarrowCells), "the measure route");
            std::vector<std::string> want;
            for (uint64_t r = 0; r < P; ++r) {
                std::string row;
                if (a.listed[r]) {
                    row = names[r] + "\t" + std::to_string(a.cluster_id[r < 3 ? 0 : 2]);
                    for (uint64_t s = 0; s < N; ++s) row += "\t" + g(a.samples[r * N + s], precision);
                    row += "\n";
                }
                want.push_back(row);
            }
            checkDescriptor(t, want, "gibbs");
        }
        // the estimates files: set i = {i}, the abundances and the members of cluster k from abund_off[k] and member_base[k]
        a.eff = {812.25, 1e-7, 0.0, 123456.78, 99999999.5};
        a.abund_off = {2, 5, 5, 7};  // (two abundances of nobody in front: the base is not the path offset)
        a.abundances = {-1.0, -2.0, 1.5, 0.0, 2.5e-10, 1e100, 7.0};
        a.member_base = {1, 4, 4};
        a.member_tpm = {-3.0, 250000.0, 0.0, 1.0 / 3.0, 1e6, 5e-324};
        a.prob = {1.0, 1.0 / 3.0, 0.0, 0.5, 1e-300};
        a.count = {12.0, 99999999.5, 0.0, 1e15, 2.5};
        a.tpm = {1e6, 0.125, 0.0, 123456785.0, 1e-5};
        TextRows t = {};
        t.num_rows = P;
        t.num_clusters = 3;
        t.name_off = a.name_off.data();
        t.name_bytes = a.name_bytes.data();
        t.cluster_path_off = a.cluster_path_off.data();
        t.cluster_id = a.cluster_id.data();
        t.second_u32 = a.length.data();
        t.precision = precision;
        t.pow10 = a.pow10.data();
        t.num_fixed = 3;
        t.fixed[0] = DoubleColumn{a.eff.data(), nullptr};
        t.fixed[1] = DoubleColumn{a.abundances.data(), a.abund_off.data()};
        t.fixed[2] = DoubleColumn{a.member_tpm.data(), a.member_base.data()};
        require(descriptorBad(t) == nullptr && !measuredByWavefront(t), "the per-path descriptor");
        std::vector<std::string> want;
        for (uint64_t r = 0; r < P; ++r) {
            const uint64_t k = r < 3 ? 0 : 2, local = r - a.cluster_path_off[k];
            want.push_back(names[r] + "\t" + std::to_string(a.cluster_id[k]) + "\t" + std::to_string(a.length[r]) + "\t" + g(a.eff[r], precision) + "\t" +
                           g(a.abundances[a.abund_off[k] + local], precision) + "\t" + g(a.member_tpm[a.member_base[k] + local], precision) + "\n");
        }
        checkDescriptor(t, want, "per path");
        t.num_fixed = 4;
        t.fixed[1] = DoubleColumn{a.prob.data(), nullptr};
        t.fixed[2] = DoubleColumn{a.count.data(), nullptr};
        t.fixed[3] = DoubleColumn{a.tpm.data(), nullptr};
        require(descriptorBad(t) == nullptr && !measuredByWavefront(t), "the haplotype descriptor");
        want.clear();
        for (uint64_t r = 0; r < P; ++r) {
            want.push_back(names[r] + "\t" + std::to_string(a.cluster_id[r < 3 ? 0 : 2]) + "\t" + std::to_string(a.length[r]) + "\t" + g(a.eff[r], precision) + "\t" +
                           g(a.prob[r], precision) + "\t" + g(a.count[r], precision) + "\t" + g(a.tpm[r], precision) + "\n");
        }
        checkDescriptor(t, want, "haplotype");
    }

    TextRows bad = {};
    bad.precision = 0;
    require(descriptorBad(bad) != nullptr, "precision 0 is refused");
    bad.precision = 18;
    require(descriptorBad(bad) != nullptr, "precision 18 is refused");
    bad.precision = 8;
    require(descriptorBad(bad) == nullptr, "an empty descriptor is accepted");
    bad.num_fixed = kMaxFixedColumns + 1;
    require(descriptorBad(bad) != nullptr, "too many fixed columns are refused");
    bad.num_fixed = 0;
    bad.run_length = 5;
    bad.run_stride = 4;
    require(descriptorBad(bad) != nullptr, "a run longer than its stride is refused");
    bad.run_stride = 5;
    bad.num_rows = 1;
    require(descriptorBad(bad) != nullptr, "rows without clusters are refused");

    // flushPlan over every (lo, hi): what leaves and what stays is a partition of [lo, hi)
    for (uint32_t lo = 0; lo < 4; ++lo) {
        for (uint32_t hi = lo; hi <= static_cast<uint32_t>(kStageBytes); ++hi) {
            const FlushPlan p = flushPlan(lo, hi);
            require(p.head_end >= lo && p.head_end <= 4 && (p.head_end == lo || p.head_end == 4), "the head ends at the first word's end");
            require(p.tail_begin <= hi && p.next_hi - p.next_lo == hi - p.tail_begin && p.next_hi < 4, "fewer than four bytes stay");
            const uint32_t left = (p.head_end > lo ? p.head_end - lo : 0) + 4 * (p.end_word - p.first_word) + (hi - p.tail_begin);
            require(left == hi - lo, "head, words and tail make up the block");
        }
    }
    std::printf("ok\n");
    return 0;
}
