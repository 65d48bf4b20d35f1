// The functions of rpvg_amd/csrc/rows_parse_plan.hpp over serial scans, under the sanitizers (tests/test_rows_parse_plan.py builds and
// runs this with RPVG_NUMBER_TEXT_CHECKED): every array has exactly the size the kernels give it, and the text lies in a heap block of
// exactly its length, so a load or a store one past an end is an error here and not a fault on the GPU.  Reads texts from the file
// argv[1] (each: a decimal length, '\n', the bytes) and prints one line per text:
//   "ok K P R G M name_bytes exact"   or   "refused <1-based line> <reason code>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "rows_parse_plan.hpp"

namespace pp = rpvg_rows_parse;
using rpvg_hip_detail::word64;

namespace {

struct Sink {
    word64 bad = rpvg_hip_detail::kNoBad;
    uint64_t name_bytes = 0, exact = 0;
    void report(const uint32_t line_start, const int why) { bad = std::min(bad, rpvg_hip_detail::offenderWord(line_start, why)); }
    void nameBytes(const uint32_t n) { name_bytes += n; }
    void exactToken() { exact += 1; }
};

// a block of exactly n elements (n = 0: no block at all)
template <typename T>
std::unique_ptr<T[]> exactly(const uint64_t n) {
    return std::unique_ptr<T[]>(n ? new T[n]() : nullptr);
}

void run(const char * text, const uint32_t n, const uint64_t * pow10) {
    std::unique_ptr<uint32_t[]> scans[9];
    for (auto & scan : scans) scan = exactly<uint32_t>(static_cast<uint64_t>(n) + 1);
    for (uint32_t i = 0; i < n; ++i) pp::rawFlags(text, i, scans[0].get(), scans[1].get(), scans[2].get(), scans[3].get());
    for (int a = 0; a < 4; ++a) {
        for (uint32_t i = 1; i < n; ++i) scans[a][i] = std::max(scans[a][i], scans[a][i - 1]);
    }
    const pp::Scanned x = {text, n, scans[0].get(), scans[1].get(), scans[2].get(), scans[3].get()};
    for (uint32_t i = 0; i < n; ++i) pp::countFlags(x, i, scans[4].get(), scans[5].get(), scans[6].get(), scans[7].get(), scans[8].get());
    uint64_t totals[5];
    for (int a = 4; a < 9; ++a) {
        uint32_t sum = 0;
        for (uint32_t i = 0; i <= n; ++i) {
            const uint32_t flag = scans[a][i];
            scans[a][i] = sum;
            sum += flag;
        }
        totals[a - 4] = scans[a][n];
    }
    const pp::Counted c = {scans[4].get(), scans[5].get(), scans[6].get(), scans[7].get(), scans[8].get()};
    const uint64_t K = totals[0], P = totals[1], R = totals[2], G = totals[3], M = totals[4];
    auto cluster_row_off = exactly<uint64_t>(K + 1), cluster_path_off = exactly<uint64_t>(K + 1), lists = exactly<uint64_t>(K), index = exactly<uint64_t>(K);
    auto name_off = exactly<uint64_t>(P + 1), row_grp_off = exactly<uint64_t>(R + 1), text_idx_off = exactly<uint64_t>(G + 1), grp_idx_off = exactly<uint64_t>(G + 1), source = exactly<uint64_t>(G);
    auto has_rank = exactly<uint8_t>(K);
    auto cluster_id = exactly<uint32_t>(K), name_src = exactly<uint32_t>(P), path_length = exactly<uint32_t>(P), row_count = exactly<uint32_t>(R), text_idx = exactly<uint32_t>(M),
         path_idx = exactly<uint32_t>(M), row_unsorted = exactly<uint32_t>(R), row_line = exactly<uint32_t>(R);
    auto eff = exactly<double>(P), row_noise = exactly<double>(R), text_prob = exactly<double>(G), grp_prob = exactly<double>(G);
    pp::Parsed o = {};
    o.K = K;
    o.P = P;
    o.R = R;
    o.G = G;
    o.M = M;
    o.cluster_row_off = cluster_row_off.get();
    o.cluster_path_off = cluster_path_off.get();
    o.has_rank_key = has_rank.get();
    o.num_align_lists = lists.get();
    o.cluster_index = index.get();
    o.cluster_id = cluster_id.get();
    o.name_len = name_off.get();
    o.name_src = name_src.get();
    o.path_length = path_length.get();
    o.path_effective_length = eff.get();
    o.row_count = row_count.get();
    o.row_noise = row_noise.get();
    o.row_grp_off = row_grp_off.get();
    o.row_line = row_line.get();
    o.text_prob = text_prob.get();
    o.text_idx_off = text_idx_off.get();
    o.text_idx = text_idx.get();
    o.pow10 = pow10;
    for (uint32_t i = 0; i < n; ++i) pp::markerByte(x, c, o, i);
    Sink sink;
    for (uint32_t i = 0; i < n; ++i) pp::fillByte(x, c, o, i, sink);
    const auto refused = [&]() {
        if (sink.bad == rpvg_hip_detail::kNoBad) return false;
        const auto offender = rpvg_hip_detail::offenderOf(sink.bad, pp::kWhyLast);
        uint64_t line = 1;
        for (uint64_t i = 0; i < offender.index; ++i) line += text[i] == '\n';
        std::printf("refused %llu %d\n", static_cast<unsigned long long>(line), offender.why);
        return true;
    };
    if (refused()) return;
    if (n) {
        const pp::Groups q = {R, G, M, row_grp_off.get(), text_prob.get(), text_idx_off.get(), text_idx.get(), row_unsorted.get(), source.get(), grp_idx_off.get()};
        grp_idx_off[G] = M;
        for (uint64_t g = 0; g < G; ++g) pp::orderGroup(q, g, [&](const uint64_t r) { row_unsorted[r] = 1; });
        for (uint64_t r = 0; r < R; ++r) pp::sortRow(q, r, [&](const uint64_t row) { sink.report(row_line[row], pp::kWhyUnsortedRow); });
        if (refused()) return;
        for (uint64_t j = 0; j < std::max(G, M); ++j) pp::placeEntry(q, j, grp_prob.get(), path_idx.get());
        uint64_t sum = 0;
        for (uint64_t p = 0; p <= P; ++p) {
            const uint64_t length = name_off[p];
            name_off[p] = sum;
            sum += length;
        }
        if (sum != sink.name_bytes) {
            std::printf("FAILED the names' bytes\n");
            return;
        }
        auto names = exactly<char>(sum);
        for (uint64_t b = 0; b < sum; ++b) names[b] = pp::nameByte(text, name_off.get(), name_src.get(), P, b);
    }
    std::printf("ok %llu %llu %llu %llu %llu %llu %llu\n", static_cast<unsigned long long>(K), static_cast<unsigned long long>(P), static_cast<unsigned long long>(R),
                static_cast<unsigned long long>(G), static_cast<unsigned long long>(M), static_cast<unsigned long long>(sink.name_bytes), static_cast<unsigned long long>(sink.exact));
}

}  // namespace

int main(int argc, char ** argv) {
    if (argc < 2) return 2;
    std::FILE * file = std::fopen(argv[1], "rb");
    if (!file) return 2;
    std::vector<uint64_t> pow10(rpvg_number_text::kPow10Words);
    rpvg_number_text::buildPow10Table(pow10.data(), nullptr);
    unsigned long long length = 0;
    while (std::fscanf(file, "%llu", &length) == 1) {
        if (std::fgetc(file) != '\n') return 2;
        auto text = exactly<char>(length);
        if (length && std::fread(text.get(), 1, length, file) != length) return 2;
        run(text.get(), static_cast<uint32_t>(length), pow10.data());
    }
    std::fclose(file);
    return 0;
}
