// The dump rows of rpvg_amd/csrc/rows_text_plan.hpp on the CPU: rowBytes and rowWrite against lines built with snprintf, bare and
// ranked, at 8, 12 and 17 digits; and the kernels' wavefront (blockWalk, the very code measureRowsKernel and writeRowsKernel run)
// walked lane by lane — the measure pass into cell_len, the exclusive sum, the write pass through the staging block and flushPlan —
// with a counter behind every byte of the text: every byte is stored exactly once and no byte outside the text is touched, at every
// residue of the text's start modulo 4 (and, the lines being ragged, of the lines' starts).  Names of 0 to 4000 bytes, a row of 1000
// indices, rows whose cells end inside, at and just behind a step of 64 cells, 64 cells of the longest kind (a full block), skipped
// clusters first, last and adjacent.  formatU64 against snprintf("%llu") at every digit count.  Prints "ok".
#define RPVG_NUMBER_TEXT_CHECKED 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rows_text_plan.hpp"

using namespace rpvg_rows_text;
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

// the 64 lanes one after the other
struct CpuWave {
    std::vector<uint64_t> * cell_len;
    std::vector<char> * text;
    std::vector<int> * stores;
    std::vector<char> stage_block = std::vector<char>((kStageBytes + 15) & ~15, '?');
    char * stage = stage_block.data();
    uint64_t base = 0, exact = 0;
    uint32_t lo = 0, hi = 0;
    uint64_t flushes = 0;
    uint32_t laneBegin() const { return 0; }
    uint32_t laneEnd() const { return kBlockCells; }
    void length(const uint64_t c, const uint64_t bytes) {
        require((*cell_len)[c] == ~0ull, "a cell is measured once");
        (*cell_len)[c] = bytes;
    }
    void open(const uint64_t begin) {
        base = begin & ~3ull;
        lo = hi = static_cast<uint32_t>(begin & 3u);
    }
    void flush(const bool last) {
        require(hi <= static_cast<uint32_t>(kStageBytes), "a step fits the staging block");
        flushes += 1;
        const FlushPlan p = flushPlan(lo, hi);
        const auto store = [&](const uint32_t i) {
            require(i >= lo && i < hi, "a stored byte is a filled byte of the block");
            (*text)[base + i] = stage[i];
            (*stores)[base + i] += 1;
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
        std::vector<char> carried(stage + p.tail_begin, stage + hi);
        for (size_t i = 0; i < carried.size(); ++i) stage[p.next_lo + i] = carried[i];
        base += p.advance;
        lo = p.next_lo;
        hi = p.next_hi;
    }
};

struct Case {
    std::vector<uint64_t> cro = {0}, cpo = {0}, rgo = {0}, gio = {0}, name_off = {0}, lists, index;
    std::vector<uint32_t> count, idx, length;
    std::vector<double> noise, prob, eff;
    std::string name_bytes;
    std::vector<std::string> names;
    void path(const std::string & name, const uint32_t len, const double e) {
        names.push_back(name);
        name_bytes += name;
        name_off.push_back(name_bytes.size());
        length.push_back(len);
        eff.push_back(e);
    }
    void row(const uint32_t c, const double n, const std::vector<std::pair<double, std::vector<uint32_t>>> & groups) {
        count.push_back(c);
        noise.push_back(n);
        for (const auto & group : groups) {
            prob.push_back(group.first);
            idx.insert(idx.end(), group.second.begin(), group.second.end());
            gio.push_back(idx.size());
        }
        rgo.push_back(prob.size());
    }
    void endCluster(const uint64_t a, const uint64_t b) {
        cro.push_back(count.size());
        cpo.push_back(length.size());
        lists.push_back(a);
        index.push_back(b);
    }
};

uint64_t checkCase(const Case & c, const bool ranked, const int digits, const uint64_t * pow10, const char * what) {
    DumpRows t = {};
    t.num_clusters = static_cast<uint32_t>(c.cro.size() - 1);
    t.num_rows = c.count.size();
    t.num_groups = c.prob.size();
    t.num_entries = c.idx.size();
    t.num_paths = c.length.size();
    t.cluster_row_off = c.cro.data();
    t.cluster_path_off = c.cpo.data();
    t.row_count = c.count.data();
    t.row_noise = c.noise.data();
    t.row_grp_off = c.rgo.data();
    t.grp_prob = c.prob.data();
    t.grp_idx_off = c.gio.data();
    t.path_idx = c.idx.data();
    t.name_off = c.name_off.data();
    t.name_bytes = c.name_bytes.data();
    t.path_length = c.length.data();
    t.path_effective_length = c.eff.data();
    t.num_align_lists = ranked ? c.lists.data() : nullptr;
    t.cluster_index = ranked ? c.index.data() : nullptr;
    t.digits = digits;
    t.pow10 = pow10;
    require(descriptorBad(t) == nullptr, "the descriptor is accepted");

    // the lines with snprintf
    std::vector<std::string> want;
    for (uint32_t k = 0; k < t.num_clusters; ++k) {
        const bool printed = c.cro[k + 1] > c.cro[k] && c.cpo[k + 1] > c.cpo[k];
        std::string marker = ranked ? "# " + std::to_string(c.lists[k]) + " " + std::to_string(c.index[k]) + "\n" : "#\n", paths;
        for (uint64_t p = c.cpo[k]; p < c.cpo[k + 1]; ++p) paths += (p > c.cpo[k] ? " " : "") + c.names[p] + "," + std::to_string(c.length[p]) + "," + g(c.eff[p], 8);
        paths += "\n";
        want.push_back(printed ? marker : "");
        want.push_back(printed ? paths : "");
        for (uint64_t r = c.cro[k]; r < c.cro[k + 1]; ++r) {
            std::string row = std::to_string(c.count[r]) + " " + g(c.noise[r], digits);
            for (uint64_t gr = c.rgo[r]; gr < c.rgo[r + 1]; ++gr) {
                row += " " + g(c.prob[gr], digits) + ":";
                for (uint64_t m = c.gio[gr]; m < c.gio[gr + 1]; ++m) row += (m > c.gio[gr] ? "," : "") + std::to_string(c.idx[m]);
            }
            want.push_back(printed ? row + "\n" : "");
        }
    }
    const uint64_t L = numLines(t), C = numCells(t);
    require(want.size() == L, "2 K + R lines");

    // rowBytes and rowWrite
    std::vector<uint64_t> row_off(L + 1, 0);
    uint64_t exact = 0;
    std::string all;
    for (uint64_t j = 0; j < L; ++j) {
        const uint64_t bytes = rowBytes(t, j, &exact);
        if (bytes != want[j].size()) {
            std::printf("%s: line %llu measures %llu bytes, the reference line has %zu\n", what, static_cast<unsigned long long>(j), static_cast<unsigned long long>(bytes), want[j].size());
            std::exit(1);
        }
        row_off[j + 1] = row_off[j] + bytes;
        std::string got(bytes + 2, '@');
        require(rowWrite(t, j, &got[1]) == bytes && got[0] == '@' && got[bytes + 1] == '@', "rowWrite writes the measured bytes and no other");
        if (got.substr(1, bytes) != want[j]) {
            std::printf("%s: line %llu is \"%s\", the reference line \"%s\"\n", what, static_cast<unsigned long long>(j), got.substr(1, bytes).c_str(), want[j].c_str());
            std::exit(1);
        }
        all += want[j];
    }

    // the kernels' walk: the index, the measure pass, the scan, the line offsets, the write pass
    std::vector<uint64_t> row_cell(t.num_rows + 1), cluster_cell(t.num_clusters + 1);
    for (uint64_t r = 0; r <= t.num_rows; ++r) row_cell[r] = rowCell(t, r);
    for (uint64_t k = 0; k <= t.num_clusters; ++k) cluster_cell[k] = clusterCell(t, k);
    for (uint64_t r = 0; r < t.num_rows; ++r) require(row_cell[r] < row_cell[r + 1], "rowCell increases");
    for (uint64_t k = 0; k < t.num_clusters; ++k) require(cluster_cell[k] < cluster_cell[k + 1], "clusterCell increases");
    require(cluster_cell[t.num_clusters] == C, "the cells of the file");
    t.row_cell = row_cell.data();
    t.cluster_cell = cluster_cell.data();
    std::vector<uint64_t> cell_len(C + 1, ~0ull), cell_off(C + 1, 0);
    CpuWave measure;
    measure.cell_len = &cell_len;
    for (uint64_t c0 = 0; c0 < C; c0 += kBlockCells) blockWalk<false>(t, nullptr, c0, measure);
    for (uint64_t i = 0; i < C; ++i) {
        require(cell_len[i] != ~0ull, "every cell is measured");
        cell_off[i + 1] = cell_off[i] + cell_len[i];
    }
    require(measure.exact == exact, "the walk counts the exact cells of the lines");
    for (uint64_t j = 0; j <= L; ++j) {
        if (cell_off[lineCell(t, j)] != row_off[j]) {
            std::printf("%s: line %llu starts at %llu by its first cell, at %llu by the lines\n", what, static_cast<unsigned long long>(j), static_cast<unsigned long long>(cell_off[lineCell(t, j)]), static_cast<unsigned long long>(row_off[j]));
            std::exit(1);
        }
    }
    const uint64_t total = row_off[L];
    uint64_t flushes = 0;
    for (uint64_t shift = 0; shift < 4; ++shift) {
        std::vector<char> text(64 + shift + total + 64 + 8, '@');
        std::vector<int> stores(text.size(), 0);
        std::vector<uint64_t> shifted(cell_off);
        for (auto & off : shifted) off += 64 + shift;
        CpuWave write;
        write.text = &text;
        write.stores = &stores;
        uint64_t blocks = 0;
        for (uint64_t c0 = 0; c0 < C; c0 += kBlockCells) {
            blockWalk<true>(t, shifted.data(), c0, write);
            blocks += shifted[c0] != shifted[c0 + kBlockCells < C ? c0 + kBlockCells : C] ? 1 : 0;
        }
        require(write.flushes >= blocks, "a block with bytes flushes");
        flushes = write.flushes - blocks;  // beyond the one at the end of a block
        for (uint64_t i = 0; i < text.size(); ++i) {
            const bool inside = i >= 64 + shift && i < 64 + shift + total;
            if (stores[i] != (inside ? 1 : 0) || (inside && text[i] != all[i - 64 - shift])) {
                std::printf("%s: byte %llu of the text at alignment %llu was stored %d times\n", what, static_cast<unsigned long long>(i), static_cast<unsigned long long>(shift), stores[i]);
                std::exit(1);
            }
        }
    }
    return flushes;
}

}  // namespace

int main() {
    std::vector<uint64_t> pow10(rpvg_number_text::kPow10Words);
    rpvg_number_text::buildPow10Table(pow10.data(), nullptr);

    // formatU64 at every digit count: 10^n - 1, 10^n, 10^n + 1 and the largest
    std::vector<uint64_t> integers = {0, 1, 9, 0xffffffffull, 0x100000000ull, ~0ull};
    uint64_t power = 1;
    for (int n = 0; n <= 19; ++n) {
        integers.push_back(power - 1);
        integers.push_back(power);
        integers.push_back(power + 1);
        integers.push_back(power * 7 / 3);
        if (n < 19) power *= 10;
    }
    bool digit_counts[21] = {};
    for (const uint64_t x : integers) {
        char want[32], got[32];
        const int n = std::snprintf(want, sizeof(want), "%llu", static_cast<unsigned long long>(x));
        std::memset(got, '@', sizeof(got));
        require(rpvg_number_text::decimalDigits64(x) == n && rpvg_number_text::formatU64(x, got + 1) == n, "formatU64 returns the digits of %llu");
        require(std::memcmp(got + 1, want, n) == 0 && got[0] == '@' && got[n + 1] == '@', "formatU64 writes what %llu writes and no other byte");
        digit_counts[n] = true;
    }
    for (int n = 1; n <= 20; ++n) require(digit_counts[n], "every digit count of a u64 is checked");

    const double quiet_nan = std::nan("");
    const std::vector<double> hard = {123456785.0, 123456795.0, 99999999.5, -0.0, 5e-324, 1e-5, -1.2345678901234567e-308, 10000000.5, 1.99999995, 0.1, 1e22, 3.0,
                                      std::numeric_limits<double>::infinity(), 0.0, 1.0 / 3.0, quiet_nan, -quiet_nan, 1.0, 0.5};
    uint64_t salt = 0;
    const auto next = [&] { return hard[salt++ % hard.size()]; };

    Case c;
    // cluster 0: skipped (rows, no paths)
    c.row(3, 0.5, {});
    c.endCluster(0, ~0ull);
    // cluster 1: names of 0 .. 4000 bytes; rows without groups, of an empty group, of one and three members, of 1000 indices
    for (const size_t n : {size_t(0), size_t(1), size_t(3), size_t(4), size_t(5), size_t(26), size_t(27), size_t(255), size_t(1700), size_t(4000)}) c.path(std::string(n, static_cast<char>('a' + n % 26)), static_cast<uint32_t>(n * 1000003u), next());
    c.row(0, next(), {});
    c.row(9, next(), {{next(), {}}});
    c.row(10, next(), {{next(), {7}}});
    c.row(4294967295u, next(), {{next(), {0, 9, 4}}, {next(), {}}, {next(), {1}}});
    {
        std::vector<uint32_t> thousand(1000);
        for (uint32_t i = 0; i < 1000; ++i) thousand[i] = (i * 7u) % 10u;
        c.row(1, next(), {{next(), thousand}, {next(), {2, 3}}});
    }
    c.endCluster(18446744073709551615ull, 12);
    // clusters 2, 3: skipped (paths, no rows; neither)
    c.path("lonely", 5, 1.5);
    c.endCluster(1, 2);
    c.endCluster(3, 4);
    // cluster 4: rows of 2 .. 70 and 129 cells, so that lines end inside, at and just behind every step of 64 cells
    for (int p = 0; p < 3; ++p) c.path("p" + std::to_string(p), 100 + p, next());
    for (uint32_t cells = 2; cells <= 70; ++cells) {
        std::vector<std::pair<double, std::vector<uint32_t>>> groups;
        uint32_t left = cells - 2;
        while (left > 0) {
            const uint32_t size = (left - 1) % 5 == 0 ? left - 1 : (left - 1) % 5;
            groups.push_back({next(), std::vector<uint32_t>(size, cells % 3)});
            left -= 1 + size;
        }
        c.row(cells, next(), groups);
    }
    c.row(129, 0.25, {{0.5, std::vector<uint32_t>(126, 2)}});
    c.endCluster(5, 6);
    // cluster 5: one path, 70 rows of two cells, the longest there are, and 70 groups without members in one row
    c.path("x", 1, -1.2345678901234567e-308);
    for (int i = 0; i < 70; ++i) c.row(4294967295u, -1.2345678901234567e-308, {});
    {
        std::vector<std::pair<double, std::vector<uint32_t>>> groups(70, {-1.2345678901234567e-308, {}});
        c.row(4000000000u, -1.2345678901234567e-308, groups);
    }
    // (63 cells of 26 bytes and the last of a row, 27, are the most 64 cells hold: 64 such rows, 69 cells apart, end at every residue of 64)
    for (int i = 0; i < 64; ++i) {
        c.row(1, 0.5, {{0.5, {}}});
        c.row(1, 0.5, std::vector<std::pair<double, std::vector<uint32_t>>>(64, {-1.2345678901234567e-308, {}}));
    }
    c.endCluster(7, 8);
    // cluster 6: skipped, last
    c.path("tail", 9, 2.0);
    c.endCluster(9, 10);

    for (const bool ranked : {false, true}) {
        for (const int digits : {8, 12, 17}) {
            const uint64_t flushes = checkCase(c, ranked, digits, pow10.data(), ranked ? "ranked" : "bare");
            require(flushes >= 3, "a name of 1700 bytes and one of 4000 are three full blocks");
        }
    }

    // every cluster skipped, and a single cluster of one path and one row
    Case none;
    none.row(1, 0.5, {});
    none.endCluster(0, 0);
    none.path("a", 1, 1.0);
    none.endCluster(0, 0);
    checkCase(none, true, 8, pow10.data(), "all skipped");
    Case one;
    one.path("a", 1, 1.0);
    one.row(1, 0.5, {{0.5, {0}}});
    one.endCluster(4, 2);
    checkCase(one, false, 8, pow10.data(), "one");

    DumpRows bad = {};
    bad.digits = 8;
    require(descriptorBad(bad) == nullptr, "an empty descriptor is accepted");
    bad.digits = 7;
    require(descriptorBad(bad) != nullptr, "7 digits are refused");
    bad.digits = 18;
    require(descriptorBad(bad) != nullptr, "18 digits are refused");
    bad.digits = 17;
    bad.num_rows = 1;
    require(descriptorBad(bad) != nullptr, "rows without clusters are refused");
    bad.num_clusters = 1;
    require(descriptorBad(bad) == nullptr, "a row in a cluster is accepted");
    bad.num_align_lists = pow10.data();
    require(descriptorBad(bad) != nullptr, "one rank-key array without the other is refused");
    bad.cluster_index = pow10.data();
    bad.num_rows = 0x7ffffffdull;
    require(descriptorBad(bad) != nullptr, "2^31 - 1 lines are refused");
    bad.num_rows = 0;
    bad.num_entries = 0x7ffffffcull;
    require(descriptorBad(bad) != nullptr, "2^31 - 1 cells are refused");
    bad.num_entries = 0x7ffffffbull;
    require(descriptorBad(bad) == nullptr, "2^31 - 2 cells are accepted");
    require(probPrecisionDigits(1e-8) == 8 && probPrecisionDigits(0.5) == 8 && probPrecisionDigits(1e-12) == 12 && probPrecisionDigits(1e-17) == 17, "the digits of a precision");
    require(probPrecisionBad(1e-8) == nullptr && probPrecisionBad(0.0) && probPrecisionBad(1.0) && probPrecisionBad(1e-18) && probPrecisionBad(quiet_nan) && probPrecisionBad(-1.0), "the precisions that are refused");
    std::printf("ok\n");
    return 0;
}
